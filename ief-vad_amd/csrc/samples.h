// Score samples of one forward (include/iefvad.h, iefvad_forward_samples): Monte Carlo over the heads' own Gaussians.  The reference
// collapses each modality's N(mu_m, exp(lv_m)) to its mean before the fusion (imf_vad.py:130-144) and never samples, so these
// semantics are this library's own ("parity unpinned", as for the row noise of common.h).  For sample s, modality m, snippet id r,
// column c:
//   seed_s = seed + s 0x9E3779B97F4A7C15 (mod 2^64)            eps = gauss_pair(seed_s, r, m, c >> 1)     (common.h, unchanged)
//   sd_m   = scale exp(0.5 lv_m) / sqrt(f)                       f = the Student-t factor (nu + 1) / nu, or 1: sd_m^2 = scale^2 / w_m,
//                                                                the variance the fusion itself assigns to modality m
//   mu~_m  = mu_m + eps sd_m
//   z0_s   = fuse_weights(w_i, w_e, mu~_i, mu~_e, epsilon)       the call's own precisions, sampled means (rowops.h)
// followed by the unchanged refinement and classifier.  Literal fp32, every product and sum rounded on its own, no clamps: inf and
// NaN behave as the expression does; scale = 0 gives eps 0 = 0 and mu + 0 = mu exactly for finite logvars.
//
// iefvad_sample_states_kernel reads the four head tensors of a pass's row set ONCE per group of up to IEF_MAX_VARIANTS samples and
// writes the group's z0 into the stacked state [G][nrows][D] fp32 (and its bf16 copy where the bf16 launch-per-projection route reads
// one, as VariantArgs::zb); the refinement and the scorer then run on the stacked state as one row set of G nrows rows (iefvad.hip,
// pass_samples).  The row-kernel idiom of rowops.h / variants.h: one wavefront per row, lane l owns columns 4 l + 256 j, 16-byte loads
// and stores, no LDS, no atomics.  HBM traffic per row and group: 4 D 4 bytes read, G D 4 (+ G D 2) written.
//
// Rows: the row set of ONE pass, walked as iefvad_step_probe_kernel walks it.  With a chunk table, chunk c owns row-set rows
// enc_row .. enc_row + valid - 1, which are packed rows src_row .. of the pass; without one (a dense pass, or the compacted set) slab s
// stands for rows 256 s .. and the map is the identity.  The snippet id of a row is ids[packed row of the pass], or -- ids NULL -- its
// row in the CALL, row0 + packed row of the pass: the id the row noise uses, so a snippet gets the same draws on the dense and the
// valid-row route, in any batch composition and in any micro-batch pass; both routes go through sample_row below.  The rows of the set
// that stand for no snippet (a chunk's pad row, the rows that round the set up to whole tiles: workgroup gridDim.x - 1 with a chunk
// table) get zeros in every sample, so the stacked set holds no stale bits; their logits are never copied out.
//
// iefvad_samples_reduce_kernel runs behind the pass's last group: per valid row of the pass it reads the S logits of the call's
// [S, stride] result in index order and writes the mean and the population standard deviation (ddof = 0) of their sigmoids, two passes
// (mean, then squared deviations about it), fp32, one thread per row: no atomics, the same call gives the same bits.
// A group's logits reach the [S, stride] result through iefvad_variants_out_kernel (variants.h) at the group's first sample.
#pragma once
#include "common.h"
#include "rowops.h"
#include "variants.h"

#define IEF_MAX_SAMPLES 64
#define SAMPLE_SLICES 8

struct SampleArgs {
    const float* mu_i; const float* lv_i; const float* mu_e; const float* lv_e;   // [nrows, D]
    float* z;                   // [count][nrows][D]
    __bf16* zb;                 // the same as bf16 (nullable)
    const RaggedChunk* chunks;  // nullable: slabs of 256 rows
    const int* ids;             // [packed rows of the pass] snippet ids, nullable
    long long row0;             // row of the CALL that the pass's first packed row is
    int nrows, valid_rows;      // rows of the set; packed rows of the pass
    int used_rows;              // with a chunk table: rows of the set that belong to chunks
    int chunk_rows;             // with a chunk table: 256 = whole chunks in the set, 0 = row-compressed (valid rows + one pad row)
    int count;
    unsigned long long seed[IEF_MAX_VARIANTS];      // seed_s of the group's samples
    float factor, eps, scale;
};

// the group's z0 of one row (all lanes of the wave); id: the snippet id
template <int D>
__device__ __forceinline__ void sample_row(const SampleArgs& a, size_t row, unsigned id, int lane) {
    constexpr int NJ = D / 256;
    const size_t base = row * D + 4 * lane;
    const size_t vstride = (size_t)a.nrows * D;
    const float root_f = sqrtf(a.factor);
    f32x4 mi[NJ], me[NJ], wi[NJ], we[NJ], si[NJ], se[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const size_t o = base + 256 * j;
        mi[j] = *(const f32x4*)(a.mu_i + o);
        me[j] = *(const f32x4*)(a.mu_e + o);
        const f32x4 li = *(const f32x4*)(a.lv_i + o), le = *(const f32x4*)(a.lv_e + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            wi[j][e] = __fmul_rn(a.factor, expf(-li[e]));
            we[j][e] = __fmul_rn(a.factor, expf(-le[e]));
            si[j][e] = __fmul_rn(a.scale, expf(__fmul_rn(0.5f, li[e]))) / root_f;
            se[j][e] = __fmul_rn(a.scale, expf(__fmul_rn(0.5f, le[e]))) / root_f;
        }
    }
    for (int v = 0; v < a.count; ++v) {
        const unsigned long long seed = a.seed[v];          // wave-uniform
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int q = (4 * lane + 256 * j) >> 1;
            float ei[4], ee[4];
            gauss_pair(seed, id, 0, q, ei[0], ei[1]);
            gauss_pair(seed, id, 0, q + 1, ei[2], ei[3]);
            gauss_pair(seed, id, 1, q, ee[0], ee[1]);
            gauss_pair(seed, id, 1, q + 1, ee[2], ee[3]);
            f32x4 z;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ti = __fadd_rn(mi[j][e], __fmul_rn(ei[e], si[j][e]));
                const float te = __fadd_rn(me[j][e], __fmul_rn(ee[e], se[j][e]));
                float ni, ne, ze;
                fuse_weights(wi[j][e], we[j][e], ti, te, a.eps, ni, ne, ze);
                z[e] = ze;
            }
            *(f32x4*)(a.z + v * vstride + base + 256 * j) = z;
            if (a.zb) *(bf16x4_t*)(a.zb + v * vstride + base + 256 * j) = to_bf16x4(z);
        }
    }
}

// a row of the set that stands for no snippet: zeros in every sample of the group
template <int D>
__device__ __forceinline__ void sample_row_zero(const SampleArgs& a, size_t row, int lane) {
    constexpr int NJ = D / 256;
    const size_t base = row * D + 4 * lane;
    const size_t vstride = (size_t)a.nrows * D;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int v = 0; v < a.count; ++v)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            *(f32x4*)(a.z + v * vstride + base + 256 * j) = zero;
            if (a.zb) *(bf16x4_t*)(a.zb + v * vstride + base + 256 * j) = to_bf16x4(zero);
        }
}

// grid (chunk or slab [+ 1 with a chunk table: the rows behind the last chunk], slice)
template <int D>
__global__ __launch_bounds__(256) void iefvad_sample_states_kernel(SampleArgs a) {
    int begin, src, nr, nvalid;                                      // row-set row, packed row of the pass, rows, sampled rows: workgroup-uniform
    if (a.chunks) {
        if (blockIdx.x + 1 < gridDim.x) {
            const RaggedChunk c = a.chunks[blockIdx.x];
            begin = c.enc_row; src = c.src_row; nvalid = c.valid; nr = a.chunk_rows ? a.chunk_rows : ragged_rows(c.valid);
        } else {
            begin = a.used_rows; src = 0; nvalid = 0; nr = a.nrows - a.used_rows;
        }
    } else {
        begin = src = blockIdx.x * 256;
        nr = a.nrows - begin < 256 ? a.nrows - begin : 256;
        nvalid = a.valid_rows - begin < nr ? a.valid_rows - begin : nr;
    }
    const int lane = threadIdx.x & 63;
    for (int r = ROW_WAVES * blockIdx.y + (threadIdx.x >> 6); r < nr; r += ROW_WAVES * gridDim.y) {
        const size_t row = (size_t)begin + r;
        if (r < nvalid)
            sample_row<D>(a, row, a.ids ? (unsigned)a.ids[src + r] : (unsigned)(a.row0 + src + r), lane);
        else
            sample_row_zero<D>(a, row, lane);
    }
}

// grid (chunk or slab): thread r of the workgroup owns packed row `out + r` of the pass, column row0 + out + r of the call
__global__ __launch_bounds__(256) void iefvad_samples_reduce_kernel(const float* __restrict__ logits, long long stride, int count,
                                                                     const RaggedChunk* __restrict__ chunks, int valid_rows, long long row0,
                                                                     float* __restrict__ mean_out, float* __restrict__ std_out) {
    int out, nr;
    if (chunks) {
        const RaggedChunk c = chunks[blockIdx.x];
        out = c.src_row; nr = c.valid;
    } else {
        out = blockIdx.x * 256;
        nr = valid_rows - out < 256 ? valid_rows - out : 256;
    }
    const int r = threadIdx.x;
    if (r >= nr) return;
    const long long col = row0 + out + r;
    float sum = 0.f;
    for (int s = 0; s < count; ++s) sum += 1.f / (1.f + expf(-logits[(long long)s * stride + col]));
    const float mean = sum / (float)count;
    float dev = 0.f;
    for (int s = 0; s < count; ++s) {
        const float d = 1.f / (1.f + expf(-logits[(long long)s * stride + col])) - mean;
        dev += d * d;
    }
    mean_out[col] = mean;
    std_out[col] = sqrtf(dev / (float)count);
}

// Fusion ablations of one forward (include/iefvad.h, iefvad_forward_variants): the precision-weighted fusion (imf_vad.py:130-144)
//   w_i = f exp(-lv_i), w_e = f exp(-lv_e), den = w_i + w_e + eps, z0 = (w_i / den) mu_i + (w_e / den) mu_e
// with one substitution per variant, each followed by the unchanged refinement and classifier:
//   IEFVAD_VARIANT_FUSED  none (the call's own z0: a self-check)
//   IEFVAD_VARIANT_IMAGE  w_e := 0        z0 = w_i / (w_i + eps) mu_i + 0 mu_e
//   IEFVAD_VARIANT_EVENT  w_i := 0
//   IEFVAD_VARIANT_EQUAL  lv_i := lv_e := 0, so w_i = w_e = f exp(-0) = f
// The substituted precisions go through fuse_weights (rowops.h), the second half of the fusion kernel's own fuse_elem: the same
// __fmul_rn / __fadd_rn forms in the same order, 0 mu and eps included, so NaN and inf behave as the substituted reference expression
// does; the unsubstituted variant goes through fuse_elem itself and has the bits of the call's z0 (see the kernel).
//
// iefvad_fusion_variants_kernel reads the four head tensors of a pass's row set ONCE and writes the z0 of every asked-for variant
// into a stacked state [V][nrows][D] fp32 (and its bf16 copy where the bf16 launch-per-projection route reads one).  The refinement
// and the scorer then run on the stacked state as one row set of V nrows rows (iefvad.hip, pass_variants).  The row-kernel idiom of
// rowops.h: one wavefront per row, lane l owns columns 4 l + 256 j, 16-byte loads and stores, no LDS, no atomics.  HBM traffic per
// row: 4 D 4 bytes read, V D 4 (+ V D 2) written.
//
// iefvad_variants_out_kernel copies the stacked logits [V][nrows] of a pass to the call's [V, stride] result: the row map of
// iefvad_rows_out_kernel / iefvad_step_probe_kernel (chunk table, or 256-row slabs of the first valid_rows rows); pad rows are never
// written.  Output column = row0 + packed row of the pass.
#pragma once
#include "common.h"
#include "rowops.h"

#define IEF_MAX_VARIANTS 4

struct VariantArgs {
    const float* mu_i; const float* lv_i; const float* mu_e; const float* lv_e;   // [nrows, D]
    float* z;                   // [count][nrows][D]
    __bf16* zb;                 // the same as bf16 (nullable)
    int nrows, count;
    int kind[IEF_MAX_VARIANTS]; // IEFVAD_VARIANT_*
    float factor, eps;
};

template <int D>
__global__ __launch_bounds__(256) void iefvad_fusion_variants_kernel(VariantArgs a) {
    constexpr int NJ = D / 256;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (row >= a.nrows) return;
    const size_t base = (size_t)row * D + 4 * lane;
    const size_t vstride = (size_t)a.nrows * D;
    // The unsubstituted z0 goes through fuse_elem ITSELF, as one expression from the logvars on: the compiler contracts parts of that
    // expression (w_i + w_e becomes one fused multiply-add of f and exp(-lv_i) onto w_e), and only the same expression gives the
    // "fused" variant the bits of the call's z0.  The substitutions leave nothing to contract there: w + 0 and f + f are exact.
    f32x4 mi[NJ], me[NJ], wi[NJ], we[NJ], zf[NJ];
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
            float ni, ne, ze;
            fuse_elem(mi[j][e], li[e], me[j][e], le[e], a.factor, a.eps, ni, ne, ze);
            zf[j][e] = ze;
        }
    }
    const float w_equal = __fmul_rn(a.factor, expf(-0.f));
    for (int v = 0; v < a.count; ++v) {
        const int kind = a.kind[v];          // wave-uniform
        float* zp = a.z + v * vstride + base;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            f32x4 z = zf[j];
            if (kind != IEFVAD_VARIANT_FUSED) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pi = kind == IEFVAD_VARIANT_EVENT ? 0.f : kind == IEFVAD_VARIANT_EQUAL ? w_equal : wi[j][e];
                    const float pe = kind == IEFVAD_VARIANT_IMAGE ? 0.f : kind == IEFVAD_VARIANT_EQUAL ? w_equal : we[j][e];
                    float ni, ne, ze;
                    fuse_weights(pi, pe, mi[j][e], me[j][e], a.eps, ni, ne, ze);
                    z[e] = ze;
                }
            }
            *(f32x4*)(zp + 256 * j) = z;
            if (a.zb) *(bf16x4_t*)(a.zb + v * vstride + base + 256 * j) = to_bf16x4(z);
        }
    }
}

// grid (chunk or slab, variant)
__global__ __launch_bounds__(256) void iefvad_variants_out_kernel(const float* __restrict__ src, int nrows, const RaggedChunk* __restrict__ chunks,
                                                                   int valid_rows, float* __restrict__ dst, long long stride, long long row0) {
    int begin, out, nr;                                              // row-set row, packed row of the pass, rows: workgroup-uniform
    if (chunks) {
        const RaggedChunk c = chunks[blockIdx.x];
        begin = c.enc_row; out = c.src_row; nr = c.valid;
    } else {
        begin = out = blockIdx.x * 256;
        nr = valid_rows - begin < 256 ? valid_rows - begin : 256;
    }
    const int r = threadIdx.x;
    if (r < nr) dst[(long long)blockIdx.y * stride + row0 + out + r] = src[(size_t)blockIdx.y * nrows + begin + r];
}

// Row-wise (one wavefront per 768-wide snippet row) stages of the forward: LayerNorm, the
// precision-weighted fusion, the scorer and the input cast.  All are HBM-bound streaming passes:
// 16-byte coalesced loads (lane l owns columns 4l + 256 j, j = 0..2) and 64-lane shuffle reductions.
// The kernels are templates on the row width D (768, or 512 for ViT-B/16 features: j = 0..1); the per-lane sums run over
// j in ascending order, so the 768 instances keep the summation trees they always had, e.g. (v0 + v1) + v2.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>
#include "common.h"

#define ROW_WAVES 4   // rows per 256-thread block

typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bf16x4_t to_bf16x4(f32x4 v) {
    bf16x4_t w;
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = (__bf16)v[e];      // v_cvt_pk_bf16_f32: round-to-nearest-even, NaN stays NaN
    return w;
}

// ---- LayerNorm(768), eps inside the sqrt, biased variance; optionally a second LayerNorm applied to
// the result (the "whitening" LN that directly follows the last encoder LN, imf_vad.py:116-117,122-123).
struct LnArgs {
    const float* x[2];       // [N, 768] input (already x + attn_out from the out_proj epilogue)
    float* y[2];             // [N, 768] fp32 output (nullable)
    __bf16* yb[2];           // [N, 768] bf16 copy of the output (nullable): A operand of the next bf16 projection
    const float* g1[2];      // first LN weight/bias
    const float* b1[2];
    const float* g2[2];      // second LN (nullable: skip)
    const float* b2[2];
    int nrows;
    float eps;
    float* amax[2];          // fp16x3 mode: running max |y| of the output tensor (nullable)
};

// The per-row arithmetic is written on 4-vectors (hipcc maps them to v_pk_add / v_pk_mul / v_pk_fma_f32: two fp32 lanes per
// instruction): a LayerNorm epilogue of a row-block kernel is VALU-issue bound (~1,300 scalar instructions per wave and 64-row
// block at two waves per SIMD), not memory bound.  ln_row and ln_rows perform the SAME operations per row in the same order, so the
// stand-alone kernel and every fused epilogue agree bit for bit.
__device__ __forceinline__ float ln_hsum(f32x4 t) { return (t[0] + t[1]) + (t[2] + t[3]); }
// ((v0 + v1) + v2) ...: the lane's sum over its NJ column groups, left to right
template <int NJ>
__device__ __forceinline__ f32x4 row_vsum(const f32x4 (&v)[NJ]) {
    f32x4 s = v[0];
#pragma unroll
    for (int j = 1; j < NJ; ++j) s = s + v[j];
    return s;
}

// centre the row in place and return 1 / sqrt(var + eps): THE statistics of a LayerNorm row -- ln_row and the backward kernel
// (backward.h: iefvad_layernorm_bwd_kernel recomputes instead of storing them) share these operations, so both see the same bits
template <int NJ>
__device__ __forceinline__ float ln_center_rstd(f32x4 (&v)[NJ], float eps) {
    const float mean = wave_sum(ln_hsum(row_vsum(v))) * (1.0f / (256 * NJ));
    const f32x4 m4 = {mean, mean, mean, mean};
#pragma unroll
    for (int j = 0; j < NJ; ++j) v[j] = v[j] - m4;
    f32x4 sq = v[0] * v[0];
#pragma unroll
    for (int j = 1; j < NJ; ++j) sq = v[j] * v[j] + sq;
    const float var = wave_sum(ln_hsum(sq)) * (1.0f / (256 * NJ));
    return 1.0f / sqrtf(var + eps);
}

template <int NJ>
__device__ __forceinline__ void ln_row(f32x4 (&v)[NJ], const float* g, const float* b, int lane, float eps) {
    const float rstd = ln_center_rstd(v, eps);
    const f32x4 r4 = {rstd, rstd, rstd, rstd};
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const f32x4 gv = *(const f32x4*)(g + 4 * lane + 256 * j);
        const f32x4 bv = *(const f32x4*)(b + 4 * lane + 256 * j);
        v[j] = (v[j] * r4) * gv + bv;
    }
}

// ln_row on R rows of one wave at a time: the same operations per row in the same order, with the R independent reduction
// chains interleaved.  For callers with few resident waves (outproj_ln_*chain_bf16.h: two per SIMD).
template <int R>
__device__ __forceinline__ void ln_rows(f32x4 (&v)[R][3], const float* g, const float* b, int lane, float eps) {
    float s[R];
#pragma unroll
    for (int r = 0; r < R; ++r) s[r] = ln_hsum((v[r][0] + v[r][1]) + v[r][2]);
#pragma unroll
    for (int r = 0; r < R; ++r) s[r] = wave_sum(s[r]);      // R independent DPP chains: the scheduler interleaves them
    float ss[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float mean = s[r] * (1.0f / IEF_D);
        const f32x4 m4 = {mean, mean, mean, mean};
#pragma unroll
        for (int j = 0; j < 3; ++j) v[r][j] = v[r][j] - m4;
        f32x4 sq = v[r][0] * v[r][0];
        sq = v[r][1] * v[r][1] + sq;
        sq = v[r][2] * v[r][2] + sq;
        ss[r] = ln_hsum(sq);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) ss[r] = wave_sum(ss[r]);
    f32x4 gv[3], bv[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        gv[j] = *(const f32x4*)(g + 4 * lane + 256 * j);
        bv[j] = *(const f32x4*)(b + 4 * lane + 256 * j);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float var = ss[r] * (1.0f / IEF_D);
        const float rstd = 1.0f / sqrtf(var + eps);
        const f32x4 r4 = {rstd, rstd, rstd, rstd};
#pragma unroll
        for (int j = 0; j < 3; ++j) v[r][j] = (v[r][j] * r4) * gv[j] + bv[j];
    }
}

template <int D>
__global__ __launch_bounds__(256) void iefvad_layernorm_kernel(LnArgs a) {
    constexpr int NJ = D / 256;
    const int mod = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (row >= a.nrows) return;
    const float* xp = a.x[mod] + (size_t)row * D + 4 * lane;
    f32x4 v[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) v[j] = *(const f32x4*)(xp + 256 * j);
    ln_row(v, a.g1[mod], a.b1[mod], lane, a.eps);
    if (a.g2[mod] != nullptr) ln_row(v, a.g2[mod], a.b2[mod], lane, a.eps);
    if (a.y[mod]) {
        float* yp = a.y[mod] + (size_t)row * D + 4 * lane;
#pragma unroll
        for (int j = 0; j < NJ; ++j) *(f32x4*)(yp + 256 * j) = v[j];
    }
    if (a.yb[mod]) {
        __bf16* yb = a.yb[mod] + (size_t)row * D + 4 * lane;
#pragma unroll
        for (int j = 0; j < NJ; ++j) *(bf16x4_t*)(yb + 256 * j) = to_bf16x4(v[j]);
    }
    if (a.amax[mod]) {
        float m = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) m = amax_fold(m, v[j][e]);
        amax_store_part(a.amax[mod], row / IEF_T, row % IEF_T, wave_max(m), lane);
    }
}

// ---- Student-t / Gaussian precision weights + normalised inverse-variance fusion
// (/root/reference/model/imf_vad.py:130-144):
//   w_m = factor * exp(-logvar_m) ; den = w_i + w_e + eps ; n_m = w_m / den ; z = n_i*mu_i + n_e*mu_e
// The literal formula is kept (including its inf/inf = NaN behaviour for logvar < -88.7).
// one element of the fusion; the literal operation order of the reference (shared with the heads row-block kernels)
// the weight-combination half: from the two precisions on (shared with the ablation kernel of variants.h, which substitutes into wi / we)
__device__ __forceinline__ void fuse_weights(float wi, float we, float mi, float me, float eps, float& ni, float& ne, float& z) {
    const float den = __fadd_rn(__fadd_rn(wi, we), eps);
    ni = wi / den;
    ne = we / den;
    z = __fadd_rn(__fmul_rn(ni, mi), __fmul_rn(ne, me));
}
__device__ __forceinline__ void fuse_elem(float mi, float li, float me, float le, float factor, float eps,
                                          float& ni, float& ne, float& z) {
    const float wi = __fmul_rn(factor, expf(-li));
    const float we = __fmul_rn(factor, expf(-le));
    fuse_weights(wi, we, mi, me, eps, ni, ne, z);
}

struct FusionArgs {
    const float* mu_i; const float* lv_i; const float* mu_e; const float* lv_e;   // [N, 768]
    float* n_i; float* n_e;     // [N, 768], nullable
    float* z;                   // [N, 768]
    __bf16* zb;                 // [N, 768] bf16 copy of z (nullable)
    float* n_i_mean; float* n_e_mean;   // [N], nullable: mean over D (test.py:131-136)
    int nrows;
    float factor, eps;
    float* z_amax;              // fp16x3 mode: running max |z| (nullable)
};

template <int D>
__global__ __launch_bounds__(256) void iefvad_fusion_kernel(FusionArgs a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (row >= a.nrows) return;
    const size_t base = (size_t)row * D + 4 * lane;
    float si = 0.f, se = 0.f, zm = 0.f;
#pragma unroll
    for (int j = 0; j < D / 256; ++j) {
        const size_t o = base + 256 * j;
        const f32x4 mi = *(const f32x4*)(a.mu_i + o), li = *(const f32x4*)(a.lv_i + o);
        const f32x4 me = *(const f32x4*)(a.mu_e + o), le = *(const f32x4*)(a.lv_e + o);
        f32x4 ni, ne, z;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float nie, nee, ze;
            fuse_elem(mi[e], li[e], me[e], le[e], a.factor, a.eps, nie, nee, ze);
            ni[e] = nie; ne[e] = nee; z[e] = ze;
            si += ni[e];
            se += ne[e];
            zm = amax_fold(zm, z[e]);
        }
        if (a.n_i) *(f32x4*)(a.n_i + o) = ni;
        if (a.n_e) *(f32x4*)(a.n_e + o) = ne;
        *(f32x4*)(a.z + o) = z;
        if (a.zb) *(bf16x4_t*)(a.zb + o) = to_bf16x4(z);
    }
    if (a.z_amax) amax_store_part(a.z_amax, row / IEF_T, row % IEF_T, wave_max(zm), lane);
    if (a.n_i_mean || a.n_e_mean) {
        si = wave_sum(si) * (1.0f / D);
        se = wave_sum(se) * (1.0f / D);
        if (lane == 0) {
            if (a.n_i_mean) a.n_i_mean[row] = si;
            if (a.n_e_mean) a.n_e_mean[row] = se;
        }
    }
}

// ---- scorer: logits = z . w_c + b_c  (classifier = Linear(768, 1), imf_vad.py:107,150)
template <int D>
__global__ __launch_bounds__(256) void iefvad_scorer_kernel(const float* z, const float* w, const float* b,
                                                             float* logits, int nrows) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (row >= nrows) return;
    const float* zp = z + (size_t)row * D + 4 * lane;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < D / 256; ++j) {
        const f32x4 zv = *(const f32x4*)(zp + 256 * j);
        const f32x4 wv = *(const f32x4*)(w + 4 * lane + 256 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) s += zv[e] * wv[e];
    }
    s = wave_sum(s);
    if (lane == 0) logits[row] = s + b[0];
}

// ---- scorer with the last refinement projection folded in (bf16x6 inference, iefvad.hip forward_pass):
//   logits = c . z_K + b_c,  z_K = z_{K-1} - lambda (W2 h + b2)
//          = c . z_{K-1} + v . h + s0,   v = -lambda W2^T c,  s0 = b_c - lambda (c . b2)      (fold[0 .. D-1] = v, fold[D] = s0)
// c . z_{K-1} is taken exactly as iefvad_scorer_kernel takes c . z; v . h arrives as NPART per-column-tile partial sums per row from the
// EPI_BIAS_RELU_DOT epilogue (gemm_bf16.h) and is added in ascending tile order, then s0.
template <int D, int NPART>
__global__ __launch_bounds__(256) void iefvad_scorer_fold_kernel(const float* z, const float* w, const float* part, const float* fold,
                                                                  float* logits, int nrows) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (row >= nrows) return;
    const float* zp = z + (size_t)row * D + 4 * lane;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < D / 256; ++j) {
        const f32x4 zv = *(const f32x4*)(zp + 256 * j);
        const f32x4 wv = *(const f32x4*)(w + 4 * lane + 256 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) s += zv[e] * wv[e];
    }
    s = wave_sum(s);
    if (lane == 0) {
        const float* pp = part + (size_t)row * NPART;
#pragma unroll
        for (int t = 0; t < NPART; ++t) s += pp[t];
        logits[row] = s + fold[D];
    }
}

// v and s0 of the folded scorer, once per iefvad_set_weights (a training step sets the weights every step, so this is a few
// microseconds, not a 768-long dependent chain per thread): fp64 throughout, rounded once to fp32.  A workgroup takes 16 elements;
// thread (seg = t >> 4, jj = t & 15) sums n = 48 seg .. 48 seg + 47 in ascending order, thread (0, jj) then adds the 16 segment sums
// in ascending order -- a fixed order that no launch parameter changes.  Block b < D / 16: v[16 b + jj]; block D / 16: s0.  D = 768.
// blockIdx.y = refinement block: its W2 / b2 lie step_stride floats behind the previous block's (the arena order of iefvad_set_weights),
// its vector fold_stride floats behind the previous one -- every block's vector in one launch, each computed as a launch of its own would.
#define FOLD_SEGS 16
__global__ __launch_bounds__(256) void iefvad_scorer_fold_weights_kernel(const float* __restrict__ w2, const float* __restrict__ b2,
                                                                         const float* __restrict__ c, const float* __restrict__ bc,
                                                                         float lambda, float* __restrict__ fold, int D, size_t step_stride,
                                                                         int fold_stride) {
    w2 += blockIdx.y * step_stride;
    b2 += blockIdx.y * step_stride;
    fold += (size_t)blockIdx.y * fold_stride;
    __shared__ double part[FOLD_SEGS][16];
    const int seg = threadIdx.x >> 4, jj = threadIdx.x & 15;
    const int len = D / FOLD_SEGS, n0 = seg * len;
    const bool is_s0 = (int)blockIdx.x == D / 16;
    double s = 0.0;
    if (!is_s0) {
        const int j = blockIdx.x * 16 + jj;
        for (int n = n0; n < n0 + len; ++n) s = __builtin_fma((double)c[n], (double)w2[(size_t)n * D + j], s);
    } else if (jj == 0) {
        for (int n = n0; n < n0 + len; ++n) s = __builtin_fma((double)c[n], (double)b2[n], s);
    }
    part[seg][jj] = s;
    __syncthreads();
    if (seg != 0 || (is_s0 && jj != 0)) return;
    double t = 0.0;
    for (int g = 0; g < FOLD_SEGS; ++g) t += part[g][jj];
    if (!is_s0) fold[blockIdx.x * 16 + jj] = (float)(-(double)lambda * t);
    else fold[D] = (float)((double)bc[0] - (double)lambda * t);
}

// ---- input cast: the reference's `.to(torch.float)` (imf_vad.py:41-42) for fp16 / bf16 feature files, and
// the bf16 operand copies of the bf16-projection mode.  Two sources per launch (blockIdx.y), fp32 and/or
// bf16 destinations (nullable).
template <typename T>
__global__ __launch_bounds__(256) void iefvad_cast_kernel(const T* in0, const T* in1, float* out0, float* out1,
                                                          __bf16* ob0, __bf16* ob1, size_t n) {
    const T* in = blockIdx.y ? in1 : in0;
    float* out = blockIdx.y ? out1 : out0;
    __bf16* ob = blockIdx.y ? ob1 : ob0;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx * 4 < n; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t o = idx * 4;   // n is a multiple of 4
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (float)in[o + e];
        if (out) *(f32x4*)(out + o) = v;
        if (ob) *(bf16x4_t*)(ob + o) = to_bf16x4(v);
    }
}

// The same cast with a per-ROW scale folded in (iefvad_forward_scaled: the robustness sweep's attenuated time steps,
// /root/reference/test2.py:71-77 `x[:, idx] = x[:, idx] * 0.01`): the product is formed in fp32 and, for fp16 / bf16 sources, rounded
// to the source type before the widening -- torch multiplies a half tensor in fp32 and stores a half tensor, and the model then
// widens it (imf_vad.py:41-42).  A NULL scale vector, or a scale of exactly 1, leaves the row's bits alone.
// NOISE = RowNoise (iefvad_forward_perturbed with an amplitude vector): behind the scale, row r gets nz.amp[m][r] * eps added
// (add_row_noise4, common.h; amplitude 0: bits alone); its noise id is nz.id[r], or nz.row0 + r.  The mode is a parameter pack
// (row_noise_of, common.h): without it the kernel is, name and code, the one it was.
template <typename T, int D, typename... NOISE>
__global__ __launch_bounds__(256) void iefvad_cast_scaled_kernel(const T* in0, const T* in1, float* out0, float* out1, __bf16* ob0, __bf16* ob1,
                                                                 size_t n, const float* s0, const float* s1, NOISE... noise) {
    constexpr bool NZ = sizeof...(NOISE) == 1;
    static_assert(sizeof...(NOISE) <= 1, "the noise mode is one RowNoise");
    const RowNoise nz = row_noise_of(noise...);
    const T* in = blockIdx.y ? in1 : in0;
    float* out = blockIdx.y ? out1 : out0;
    __bf16* ob = blockIdx.y ? ob1 : ob0;
    const float* sc = blockIdx.y ? s1 : s0;
    const float* na = NZ ? nz.amp[blockIdx.y] : nullptr;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx * 4 < n; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t o = idx * 4;   // n is a multiple of 4, and so is the row length: the four elements share a row
        const float f = sc ? sc[o / D] : 1.0f;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = (float)in[o + e];
            if (f != 1.0f) {
                // the fp32 product must exist as such before it is narrowed: left to itself hipcc folds fpext -> fmul -> fptrunc into
                // v_fma_mixlo_f16, which rounds the exact product ONCE to fp16 -- torch rounds it to fp32 first (opmath) and then to
                // fp16, and once in a few million elements the two disagree (found by tests/test_gpu_config2.py, round 5)
                float prod = v[e] * f;
                asm volatile("" : "+v"(prod));
                v[e] = (float)(T)prod;
            }
        }
        if (NZ && na) {
            const size_t r = o / D;
            const float a = na[r];
            if (a != 0.0f) add_row_noise4<T>(v, a, nz.seed, nz.id ? (unsigned)nz.id[r] : (unsigned)(nz.row0 + (long long)r), blockIdx.y, (int)(o - r * D));
        }
        if (out) *(f32x4*)(out + o) = v;
        if (ob) *(bf16x4_t*)(ob + o) = to_bf16x4(v);
    }
}

// The perturbation of one input row on its own (iefvad_perturb_rows: the unit entry the fused loads above are tested against): the
// NaN rule if `fix_all`, the row scale, the row noise -- the steps and roundings of the two kernels above and of the chunker's
// (ragged.h) -- with the result written in the source type.  A row that no step touches keeps its bits, NaN payloads included.
// blockIdx.y = modality; a modality without a source or a destination is skipped.
template <typename T, int D>
__global__ __launch_bounds__(256) void iefvad_perturb_rows_kernel(const T* in0, const T* in1, T* out0, T* out1, size_t n, const float* s0,
                                                                  const float* s1, int fix_all, RowNoise nz, float big) {
    const int m = blockIdx.y;
    const T* in = m ? in1 : in0;
    T* out = m ? out1 : out0;
    if (!in || !out) return;
    const float* sc = m ? s1 : s0;
    const float* na = nz.amp[m];
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx * 4 < n; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t o = idx * 4, r = o / D;
        const float f = sc ? sc[r] : 1.0f;
        const float a = na ? na[r] : 0.0f;
        T raw[4];
        f32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            raw[e] = in[o + e];
            w[e] = (float)raw[e];
            if (fix_all) {
                const float x = w[e];
                w[e] = (x != x) ? 0.f : (x > big ? big : (x < -big ? -big : x));     // torch.nan_to_num(nan=0.0)
            }
            if (f != 1.0f) {
                float prod = w[e] * f;
                asm volatile("" : "+v"(prod));
                w[e] = (float)(T)prod;
            }
        }
        if (a != 0.0f) add_row_noise4<T>(w, a, nz.seed, nz.id ? (unsigned)nz.id[r] : (unsigned)(nz.row0 + (long long)r), m, (int)(o - r * D));
        const bool touched = fix_all || f != 1.0f || a != 0.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e) out[o + e] = touched ? (T)w[e] : raw[e];
    }
}

// ---- running max |x| of two tensors (blockIdx.y): the raw inputs of the first projection in fp16x3 mode
__global__ __launch_bounds__(256) void iefvad_amax_kernel(const float* in0, const float* in1, float* out0, float* out1, size_t n) {
    const float* in = blockIdx.y ? in1 : in0;
    float* out = blockIdx.y ? out1 : out0;
    float m = 0.f;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx * 4 < n; idx += (size_t)gridDim.x * blockDim.x) {
        const f32x4 v = *(const f32x4*)(in + idx * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) m = amax_fold(m, v[e]);
    }
    amax_publish(out, wave_max(m), threadIdx.x & 63);
}

// ---- per-chunk max |x| of the raw inputs (fp16x3 mode): one workgroup per (chunk, modality), no atomics
// Zeroes the per-chunk running-max words of a micro-batch: tensor blockIdx.y's first `words` floats (its chunks x IEF_AMAX_PARTS), the
// tensors `stride` floats apart.  A kernel, not hipMemsetAsync: in a captured graph the zeroing has to be a kernel node in the chain of
// the producers and consumers of these words (test_reloaded_model_equals_fresh_model[fp16x3-6] differed from run to run on the replayed
// graph with a memset node here, TRIED.md).
__global__ __launch_bounds__(256) void iefvad_amax_zero_kernel(float* am, size_t stride, unsigned words) {
    const unsigned i = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i < words) *(f32x4*)(am + blockIdx.y * stride + i) = f32x4{0.f, 0.f, 0.f, 0.f};
}

__global__ __launch_bounds__(256) void iefvad_amax_chunk_kernel(const float* in0, const float* in1, float* out0, float* out1) {
    __shared__ float part[4];
    const float* in = (blockIdx.y ? in1 : in0) + (size_t)blockIdx.x * IEF_T * IEF_D;
    float* out = blockIdx.y ? out1 : out0;
    float m = 0.f;
    for (int i = threadIdx.x * 4; i < IEF_T * IEF_D; i += 256 * 4) {
        const f32x4 v = *(const f32x4*)(in + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) m = amax_fold(m, v[e]);
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) out[(size_t)blockIdx.x * IEF_AMAX_PARTS] = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}

// Epilogue of the two-half bf16x6 split kernel (gemm_split_wide.h), one specialisation per epilogue kind.
//
// gemm_wave_epilogue (gemm_bf16.h) serves every 128 x 256 / 128 x 128 kernel of the library and tests the runtime `epi`, the nullable
// output pointers and `amax_out` inside its unrolled row loops; hipcc does not unswitch them, so each of a wave's 32 row pairs became a
// basic-block chain of its own: one LDS read, a full lgkmcnt wait, about nine scalar compare-and-branch steps, one store with a fresh
// 64-bit multiply-add for its address (DESIGN.md 4.4 has the instruction counts).  Here the kind is a template parameter (one kernel
// per kind, chosen on the host: gemm_split_wide.h), and a specialisation holds no test of `epi` or of a pointer:
//   - bf16x6 only: fp32 results, no bf16 copy, no running maximum, accumulator scale 1;
//   - the arithmetic per element and its order are gemm_wave_epilogue's (the small tiling still runs that function and is what
//     tests/test_gpu_gemm_split_epilogue.py compares against, bit for bit);
//   - the [32][GB2_EPI_LD] park image per wave, its map and the row-wise 16-byte non-temporal stores are kept;
//   - every load is requested before the first store: both halves' bias (and dot) vectors at entry, half 0's residual rows before its
//     park, half 1's right after it (half 0's accumulators are dead by then).  vmcnt counts loads and stores in one in-order queue on
//     gfx9, so a load behind a store waits for that store's acknowledgement;
//   - a half's 16 LDS reads go out in batches of GSE_BATCH with the batch's arithmetic and stores behind it;
//   - a row's address is a wave-uniform 64-bit row base plus one 32-bit lane offset (the global_store saddr form: no vector address
//     arithmetic per row).
#pragma once
#include "gemm_bf16.h"

#define GSE_BATCH 4          // LDS reads in flight per batch (rows rq + 2 u of 4 consecutive u)

// EPI: the kind; STORE_H: EPI_BIAS_RELU_DOT also stores h to C (every other kind stores C always).
// The wave owns rows m0 + 32 uwave .. + 31 and columns n0 .. n0 + 255 as two halves of 128: acc16[half][16-row tile][16-column tile].
template <int EPI, bool STORE_H>
__device__ __forceinline__ void gemm_split_wide_epilogue(const GemmBArgs& args, const GemmBProblem& P, float* smem, int m0, int n0,
                                                         int uwave, int lane, f32x4 (&acc16)[2][2][8]) {
    constexpr bool RESID = EPI == EPI_BIAS_RESID || EPI == EPI_REFINE || EPI == EPI_GATE;
    constexpr bool DOTK = EPI == EPI_BIAS_RELU_DOT;
    constexpr bool STORE = !DOTK || STORE_H;
    constexpr float cscale = 1.0f;                     // (the fp16x3 arithmetic, which scales its accumulators, has the narrow tiling only)
    const int r16 = lane & 15, q16 = lane >> 4;        // accumulator map: column r16, rows 4 q16 + r of a 16 x 16 tile
    const int rq = lane >> 5, cq = lane & 31;          // row-wise map: columns 4 cq .. 4 cq + 3 of rows rq + 2 u, u = 0..15
    const int ldc = args.ldc;
    const float alpha = args.alpha;
    const int mw = m0 + uwave * 32;                    // the wave's first row (wave-uniform)
    float* E = smem + uwave * (32 * GB2_EPI_LD);       // 16.9 KB per wave in the dead ring
    float* Ew = E + 4 * q16 * GB2_EPI_LD + r16;
    const float* Er = E + rq * GB2_EPI_LD + 4 * cq;
    const unsigned loff = (unsigned)(rq * ldc + 4 * cq) * 4u;           // bytes from a row pair's base to the lane's 16 bytes
    const size_t rstep = (size_t)ldc * 8;                               // bytes between row pairs

    f32x4 bv[2], dv[2], scale[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ncol = n0 + 128 * h + 4 * cq;
        bv[h] = *(const f32x4*)(P.bias + ncol);
        if constexpr (DOTK) dv[h] = *(const f32x4*)(P.R + ncol);
        if constexpr (EPI == EPI_QKV) {
            const float s = ncol < args.qcols ? alpha : 1.f;           // qcols is a multiple of 8: one answer per lane
            scale[h] = f32x4{s, s, s, s};
        }
    }
    f32x4 res[2][16];
    auto load_resid = [&](int h) {
        const char* rb = (const char*)P.R + ((size_t)mw * ldc + n0 + 128 * h) * 4;
#pragma unroll
        for (int u = 0; u < 16; ++u) res[h][u] = *(const f32x4*)(rb + u * rstep + loff);
    };
    auto park = [&](int h) {
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int b = 0; b < 8; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) Ew[(x * 16 + r) * GB2_EPI_LD + b * 16] = acc16[h][x][b][r];
    };
    auto rows = [&](int h) {
        const int nb = n0 + 128 * h;                   // the half's first column (wave-uniform)
        char* cb = nullptr;
        if constexpr (STORE) {
            // heads: columns below ldc go to C, the others to C2, decided per 128-column half (ldc % 128 == 0)
            const bool second = EPI == EPI_HEADS && nb >= ldc;
            cb = (char*)(second ? P.C2 : P.C) + ((size_t)mw * ldc + (second ? nb - ldc : nb)) * 4;
        }
        const int ntile = args.N / 128;
        char* pb = nullptr;
        if constexpr (DOTK) pb = (char*)(P.C2 + (size_t)mw * ntile + nb / 128);
        const unsigned poff = (unsigned)(rq * ntile) * 4u;
#pragma unroll
        for (int u0 = 0; u0 < 16; u0 += GSE_BATCH) {
            f32x4 vv[GSE_BATCH];
#pragma unroll
            for (int j = 0; j < GSE_BATCH; ++j) vv[j] = *(const f32x4*)(Er + 2 * (u0 + j) * GB2_EPI_LD);
#pragma unroll
            for (int j = 0; j < GSE_BATCH; ++j) {
                const int u = u0 + j;
                f32x4 v = vv[j];
                v = v * cscale + bv[h];
                if constexpr (EPI == EPI_QKV) v = v * scale[h];
                if constexpr (EPI == EPI_BIAS_RELU || DOTK) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (v[e] < 0.f) ? 0.f : v[e];          // NaN stays NaN
                }
                if constexpr (EPI == EPI_BIAS_RESID) v = v + res[h][u];
                if constexpr (EPI == EPI_REFINE) v = res[h][u] - alpha * v;
                if constexpr (EPI == EPI_GATE) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = res[h][u][e] > 0.f ? alpha * v[e] : 0.f;
                }
                if constexpr (STORE) GB2_STORE((f32x4*)(cb + u * rstep + loff), v);
                if constexpr (DOTK) {
                    float d = v[0] * dv[h][0];
                    d += v[1] * dv[h][1];
                    d += v[2] * dv[h][2];
                    d += v[3] * dv[h][3];
                    // the 32 lanes of the row (one half of the wave): wave_sum's first five steps; lanes 16..31 / 48..63 end with the sum
                    d += dpp_take<0xB1, 0xF>(d, d);          // quad_perm [1,0,3,2]
                    d += dpp_take<0x4E, 0xF>(d, d);          // quad_perm [2,3,0,1]
                    d += dpp_take<0x141, 0xF>(d, d);         // row_half_mirror
                    d += dpp_take<0x140, 0xF>(d, d);         // row_mirror
                    d += dpp_take<0x142, 0xA>(0.f, d);       // row_bcast:15 into rows 1 and 3
                    if (cq == 16) *(float*)(pb + (size_t)u * (2 * ntile * 4) + poff) = d;
                }
            }
            __builtin_amdgcn_sched_barrier(0);         // the next batch's reads stay behind this batch's stores
        }
    };

    if constexpr (RESID) load_resid(0);
    park(0);
    if constexpr (RESID) load_resid(1);                // (half 0's accumulators are dead: the registers exist)
    if constexpr (DOTK) {
        // The partial sums are stored under an exec branch, and across a branch hipcc cannot count the stores in vmcnt: half 1's first
        // use of its vectors would wait with vmcnt(0), that is for half 0's stores.  Have the vectors arrive before the first store.
        asm volatile("" : "+v"(bv[1]), "+v"(dv[1]));
    }
    rows(0);
    park(1);                                           // the image is private to the wave, whose LDS accesses stay in program order
    rows(1);
}

// The bf16x6 split GEMM (gemm_split.h) on a 128 x 256 block tile taken as TWO COLUMN HALVES of 128: iefvad_gemm_split_n128x2_kernel.
//
// gemm_split.h's NA = 2 configuration fetches, stages and splits every A element once per 128-column tile (6 times at N = 768, 18
// times at N = 2304), and the kernel is bound by the energy per MFMA, of which the in-register split and the operand stream are
// the measured extras (profiles/r05_gemm_split_nosplit_nodma_bounds.log).  This body keeps that configuration's shape on the CU --
// 4 waves of 32 rows, the 80 KB ring (two workgroups per CU), two W slots of 3 planes x 128 rows, one barrier per 96 MFMAs of a
// wave -- and lets a wave own 32 x 256: the W ring cycles over half-tiles it = 2 kt + hh (columns n0 + 128 hh .. of k-tile kt),
// while A is staged, read and split ONCE per k-tile for both halves.  Per MFMA: half the split VALU and A staging, 20 % fewer
// LDS-DMA instructions, 7 % fewer LDS reads; each A panel crosses the fabric for half as many column groups.  32 accumulators,
// 214-226 VGPRs by epilogue kind (one kernel per kind, at the end of this file), no AGPRs, no scratch, two waves per SIMD.  Each output element sums its k-tiles in ascending order and the six
// products of a k-tile in gemm_split.h's order, so the results are that kernel's BIT FOR BIT (tests/test_gpu_gemm_split_wide.py),
// and plan_gemm_split (launch_rules.h) chooses between the two by grid size alone.
// Measured against the 128 x 128 kernel in one lease: 0.93 of its time from 4,000 workgroups on (235 against 218
// TFLOP/s-equivalent at M = 262,144, N = 768), a tie at two rounds of the chip's 512 workgroup slots, 6-15 % slower at one round
// and below (profiles/split_wide_gemm_tune.log); in-kernel stamps at M = 65,536, N = 768: 3042 cycles per 96 MFMAs and wave at
// 1.77 GHz against 3381 at 1.73 GHz (profiles/split_wide_bench_ab.log).
// The body is a copy of gemm_split_body's with the half-tile loop worked in, NOT a third parameter of that template: hipcc's
// register allocation and scalar code of the existing instantiations changed when they were compiled from a generalised body
// (DESIGN.md 4.4), and those kernels, fp16x3's among them, are to stay the code they were.  NA, NH and F16 are constants here; the expressions that
// test them are kept as they are in gemm_split_body, so that the two bodies can be read side by side.
#pragma once
#include <type_traits>
#include "gemm_split.h"
#include "gemm_split_epilogue.h"

#ifndef GS_WIDE_SPREAD     // 1 = half h splits A half-fragments 2h, 2h+1 of the next k-tile; 0 = the first half splits all four
#define GS_WIDE_SPREAD 1   // (within noise of each other, profiles/split_wide_gemm_tune.log)
#endif
#undef GS_DIAG_STAMP

// EPI, STORE_H: the epilogue kind of the kernel and, for the dot kind, whether h is stored (gemm_split_epilogue.h)
template <int EPI, bool STORE_H>
__device__ __forceinline__ void gemm_split_wide_body(const GemmBArgs& args, float* smem) {
    constexpr int NA = 2, NH = 2;                      // 16-row tiles per wave, column halves per block
    constexpr bool F16 = false;                        // (the fp16x3 arithmetic has the narrow tiling only)
    constexpr int NP = F16 ? 2 : 3;                    // planes per operand
    constexpr int NT = F16 ? 3 : 6;                    // products per multiply-add
    constexpr int BN = GS_BN_OF(NA);                   // columns per W slot
    constexpr int BNB = BN * NH;                       // columns per block tile
    constexpr int W_PLANE = BN * 16;                   // 4-byte units: BN rows x 64 B
    constexpr int W_SLOT = NP * W_PLANE;
    constexpr int W_BASE = 2 * GS_A_SLOT;
    constexpr int WROWS = BN / 4;                      // W rows staged per wave and plane
    constexpr int NM = NT * NA;                        // MFMAs per step (24 / 12)
#ifdef GB2_CLOCK_DIAG
    const unsigned long long dg_entry = __builtin_amdgcn_s_memtime();
#endif
    const GemmBProblem& P = args.p[blockIdx.z];
    // Tile map.  xcd_remap gives each XCD a contiguous range of `bid`; the workgroups resident on an XCD at one time are
    // consecutive bids.  Column tiles are taken in groups of PN: inside a group the order is (row panel, column tile of
    // the group), so the resident set is (64 / PN) row panels x PN column tiles: each A panel is fetched once for its PN
    // co-running blocks and the group's W planes (PN x 590 KB at K = 768) stay in the 4 MB L2 instead of being re-read
    // from the Infinity Cache by every panel (N = 2304 with all 18 column tiles in flight: 10.6 MB of W planes per panel,
    // profiles/r01_gemm_split_hbm_traffic.json).  A is re-read once per group (N / (128 PN) times per launch).
    const int ntn = args.N / BNB;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    int tm, tn;
    {
        constexpr int PN = GS_PN / NH;                 // NH = 2: three wide tiles hold the W planes of six narrow ones
        const int pn = (PN > 0 && ntn % PN == 0) ? PN : ntn;
        const int ntm = args.M / GS_BM;
        const int grp = bid / (ntm * pn), rem = bid - grp * (ntm * pn);
        tm = rem / pn;
        tn = grp * pn + (rem - tm * pn);
    }
    const int m0 = tm * GS_BM, n0 = tn * BNB;
#ifdef GS_EXPERIMENT_A_ALIAS      // tools/gemm_tune_split_alias: every row panel reads one of GS_EXPERIMENT_A_ALIAS panels (A L2-resident)
    const int m0a = (tm % GS_EXPERIMENT_A_ALIAS) * GS_BM;
#else
    const int m0a = m0;
#endif
    const int K = args.K, lda = args.lda;
    const int wplane = args.wplane;                    // bytes between the planes of W
    float ascale = 1.0f, cscale = 1.0f;                // fp16x3: operand scale of A, inverse of both scales
    if constexpr (F16) {
        if (P.amaxA && P.amaxW) {
            const int ea = 13 - amax_exponent(amax_read_chunk(P.amaxA, m0 / IEF_T)), ew = 13 - amax_exponent(amax_read(P.amaxW));
            ascale = __builtin_ldexpf(1.0f, ea);
            cscale = __builtin_ldexpf(1.0f, -ea - ew);
        }
    }

    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int wrow0 = NA == 4 ? (wave >> 1) * 64 : wave * 32;      // origin of the wave tile inside the block tile
    const int wcol0 = NA == 4 ? (wave & 1) * 128 : 0;
    const int r16 = lane & 15, q16 = lane >> 4;
    const int uwave = __builtin_amdgcn_readfirstlane(wave);

    // ---- staging (LDS-DMA, lane-linear 1 KB images; the swizzle is applied to the SOURCE chunk) ----
    // A: one instruction = 8 rows x 128 B; wave w, instruction j -> rows 32 w + 8 j + (lane >> 3), chunk lane & 7
    // W: one instruction = 16 rows x 64 B; wave w, plane p, instruction j -> rows WROWS w + 16 j + (lane >> 2), chunk lane & 3
    const int nrecA = (int)((GS_BM - 1) * lda + K) * 4, nrecW = (NP - 1) * wplane + (int)((BNB - 1) * K + K) * 2;
    const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)P.A + (size_t)m0a * lda * 4), 0, nrecA, 0x00020000);
    const auto rsW = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)P.W + (size_t)n0 * K * 2), 0, nrecW, 0x00020000);
    const int arow = lane >> 3, achk = lane & 7;
    int voA[2];                                        // row bit 3 = j & 1 enters the swizzle
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) voA[jj] = arow * lda * 4 + ((achk ^ (((arow >> 1) & 1) | (jj << 2))) << 4);
    const int wrow = lane >> 2, wchk = lane & 3;
    const int voW = wrow * K * 2 + ((wchk ^ ((0xD2 >> (2 * ((wrow >> 2) & 3))) & 3)) << 4);
#define GLDS16(rs, vo, so, lp) \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(lp), 16, vo, so, 0, 0)
    auto stage_a = [&](int tile, int slot) {
        float* Ad = smem + slot * GS_A_SLOT + uwave * 32 * 32;
#pragma unroll
        for (int j = 0; j < 4; ++j) GLDS16(rsA, voA[j & 1], ((uwave * 32 + j * 8) * lda + tile * GS_BK) * 4, Ad + j * 8 * 32);
    };
    auto stage_w = [&](int tile, int slot) {
        float* Wd = smem + W_BASE + slot * W_SLOT + uwave * WROWS * 16;
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int j = 0; j < WROWS / 16; ++j)
                GLDS16(rsW, voW, p * wplane + ((uwave * WROWS + j * 16) * K + tile * GS_BK) * 2, Wd + p * W_PLANE + j * 16 * 16);
    };

    // ---- fragment addresses (4-byte units) ----
    const int swa = (r16 >> 1) & 5;
    const int a_lo = (wrow0 + r16) * 32 + (((2 * q16) ^ swa) << 2);
    const int a_hi = (wrow0 + r16) * 32 + (((2 * q16 + 1) ^ swa) << 2);
    const int b_of = (wcol0 + r16) * 16 + ((q16 ^ ((0xD2 >> (2 * ((r16 >> 2) & 3))) & 3)) << 2);

    f32x4 acc16[NH][NA][8];
#pragma unroll
    for (int hh = 0; hh < NH; ++hh)
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int b = 0; b < 8; ++b) acc16[hh][a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    u32x4 ap[NA][NP], an[NA][NP];                      // planes of the A fragments: current k-tile / next k-tile
    auto mfma_row = [&](int hh, int b, int pa, const u32x4& wv) {
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            if constexpr (F16)
                acc16[hh][a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, ap[a][pa]),
                                                                         __builtin_bit_cast(f16x8, wv), acc16[hh][a][b], 0, 0, 0);
            else
                acc16[hh][a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ap[a][pa]),
                                                                          __builtin_bit_cast(bf16x8, wv), acc16[hh][a][b], 0, 0, 0);
        }
    };
    // half `hf` (k = 8q + 4 (hf & 1) .. + 3) of row-tile (hf >> 1) of the NEXT k-tile: fp32 fragment -> three planes
    auto split_half = [&](int hf, const f32x4& v) {
        Split4 sp;
        if constexpr (F16) {
#pragma unroll
            for (int e = 0; e < 4; ++e) sp.r[e] = v[e] * ascale;       // scalar multiplies: v_pk_mul_f32 is slow beside MFMAs
        } else {
            sp.r = v;
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            unsigned d0, d1;
            if constexpr (F16) sp.plane_f16(d0, d1, p < NP - 1); else sp.plane(d0, d1, p < NP - 1);
            an[hf >> 1][p][2 * (hf & 1)] = d0;
            an[hf >> 1][p][2 * (hf & 1) + 1] = d1;
        }
    };
#define GS_FENCE() __builtin_amdgcn_sched_barrier(0)
#define GS_PIPE(mask) __builtin_amdgcn_sched_group_barrier(mask, 1, 0)

    const int nk = K / GS_BK;
    stage_a(0, 0);
    stage_a(1, 1);
    stage_w(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    GB2_BARRIER();
#pragma unroll
    for (int hf = 0; hf < 2 * NA; ++hf)                // k-tile 0 is split up front (exposed once per block)
        split_half(hf, *(const f32x4*)(smem + (hf >> 1) * 16 * 32 + ((hf & 1) ? a_hi : a_lo)));
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int p = 0; p < NP; ++p) ap[a][p] = an[a][p];
#ifdef GB2_CLOCK_DIAG
    const unsigned long long dg_c0 = __builtin_amdgcn_s_memtime(), dg_r0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long dg_last = dg_c0, dg_acc[3] = {0, 0, 0};   // cycles in: MFMA body | vmcnt + lgkmcnt wait | barrier
#define GS_DIAG_STAMP(i) { const unsigned long long now = __builtin_amdgcn_s_memtime(); dg_acc[i] += now - dg_last; dg_last = now; }
#else
#define GS_DIAG_STAMP(i)
#endif

    // One k-tile per iteration: W of slot (kt & 1) against the planes in `ap`; the fp32 A fragments of k-tile kt+1 (slot
    // (kt+1) & 1) are read and split into `an` on the way.  Step B of 8 is the 6 NA MFMAs of column-tile B (six terms x
    // NA row-tiles) with the other work of the step issued BETWEEN them:
    //   NA = 4: steps 0..5 split one half-fragment each (22 VALU), step 6 two (44); NA = 2: steps 0..3 one each;
    //   step 7 moves `an` into `ap` (12 NA v_mov);
    //   the wave's LDS-DMA instructions (A of k-tile kt+2, then W of k-tile kt+1) go out 4 per step in steps 0..3
    //   (NA = 4) / 2 per step in steps 0..4 (NA = 2): issued back to back they fill the vector-memory queue and stall
    //   the wave's MFMA stream;
    //   every step reads the W fragments (and the fp32 A half) of the next step.
    // sched_group_barrier pins that interleaving (hipcc otherwise lumps the VALU work in front of the MFMAs).  On the
    // last k-tile the split works on stale LDS data that is never used, and the DMA descriptors have zero records.
    //
    // NH = 2: the iteration is run once per column half hh (a constant expression inside `half_tile`, as the sched_group_barrier
    // counts need), on half-tile it = kt NH + hh: W of slot (it & 1) into acc16[hh], W of half-tile it + 1 by DMA into the other
    // slot (6 instructions), vmcnt(0) / lgkmcnt(0) / barrier after every half -- once per 96 MFMAs, as with NH = 1.  The A side
    // runs once per k-tile: A of k-tile kt+2 goes out in half 0, the four half-fragments of k-tile kt+1 are split two per half
    // (GS_WIDE_SPREAD; else all in half 0), and `an` moves into `ap` at the end of the last half.
    for (int kt = 0; kt < nk; ++kt) {
      auto half_tile = [&](auto hh_c) __attribute__((always_inline)) {
        constexpr int HH = decltype(hh_c)::value;
        const int it = kt * NH + HH, it1 = it + 1;
        const auto rW = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)P.W + (size_t)n0 * K * 2), 0,
                                                          (it1 < nk * NH) ? nrecW : 0, 0x00020000);
        const auto rA = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)P.A + (size_t)m0a * lda * 4), 0,
                                                          (kt + 2 < nk) ? nrecA : 0, 0x00020000);
        float* Wd = smem + W_BASE + (it1 & 1) * W_SLOT + uwave * WROWS * 16;
        float* Ad = smem + (kt & 1) * GS_A_SLOT + uwave * 32 * 32;
        const int kW = (it1 % NH) * BN * K * 2 + (it1 / NH) * GS_BK * 2, kA = (kt + 2) * GS_BK * 4;
        auto dma = [&](int d) {                        // d = 0..3: A, d = 4..: W (plane-major)
            if (GS_EXP_NODMA) return;
            if (d < 4) {
                GLDS16(rA, voA[d & 1], (uwave * 32 + d * 8) * lda * 4 + kA, Ad + d * 8 * 32);
            } else {
                const int p = (d - 4) / (WROWS / 16), j = (d - 4) % (WROWS / 16);      /* d - 4 < NP WROWS / 16 */
                GLDS16(rW, voW, p * wplane + (uwave * WROWS + j * 16) * K * 2 + kW, Wd + p * W_PLANE + j * 16 * 16);
            }
        };
        const float* Wv = smem + W_BASE + (it & 1) * W_SLOT + b_of;
        const float* Av = smem + ((kt + 1) & 1) * GS_A_SLOT;
        auto a_half = [&](int hf) { return *(const f32x4*)(Av + (hf >> 1) * 16 * 32 + ((hf & 1) ? a_hi : a_lo)); };
        // (B and g are literals below, HH a constant expression: sched_group_barrier takes integer constant expressions only)
#define GS_NSPLIT(B) (NA == 4 ? ((B) < 6 ? 1 : (B) == 6 ? 2 : 0) : NH == 2 ? (GS_WIDE_SPREAD ? ((B) < 2 ? 1 : 0) : (HH == 0 && (B) < 4 ? 1 : 0)) \
                                                                           : ((B) < 4 ? 1 : 0))   /* half-fragments split in step B */
#define GS_HF(B) (NH == 2 && GS_WIDE_SPREAD ? 2 * HH + (B) : (B))                            /* the half-fragment step B splits */
#define GS_NAREAD(B) ((B) < 7 ? GS_NSPLIT((B) + 1) : 0)                                      /* fp32 A reads for step B+1 */
#define GS_NREAD(B) (((B) < 7 ? NP : 0) + GS_NAREAD(B))
#define GS_NDMA(B) (NA == 4 ? ((B) < 4 ? (F16 ? 3 : 4) : 0) : (F16 ? ((B) < 4 ? 2 : 0) : HH > 0 ? ((B) < 3 ? 2 : 0) : ((B) < 5 ? 2 : 0)))
#define GS_DMA0 (HH > 0 ? 4 : 0)                                                             /* later halves: the W instructions only */
#define GS_NVALU(B) ((B) == 7 ? (HH == NH - 1 ? 4 * NP * NA : 0) : GS_EXP_NOSPLIT ? 0 : (F16 ? 12 : 22) * GS_NSPLIT(B))
        u32x4 w[NP];
        f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int p = 0; p < NP; ++p) w[p] = *(const u32x4*)(Wv + p * W_PLANE);
        if (GS_NSPLIT(0) > 0) v0 = a_half(GS_HF(0));
        GS_FENCE();
#define GS_VSLOT(B, g) (((g) + 1) * GS_NVALU(B) / NM - (g) * GS_NVALU(B) / NM)
#define GS_SLOT(B, g)                                                                                           \
        if ((g) < NM) {                                                                                         \
            GS_PIPE(0x008);                                                                                     \
            if (GS_VSLOT(B, g) > 0) __builtin_amdgcn_sched_group_barrier(0x002, GS_VSLOT(B, g) > 0 ? GS_VSLOT(B, g) : 1, 0); \
            if (GS_NDMA(B) > 0 && !GS_EXP_NODMA && (g) % (NM / 4) == 2 && (g) / (NM / 4) < GS_NDMA(B)) GS_PIPE(0x020); \
        }
#define GS_STEP(B)                                                                                              \
        {                                                                                                       \
            u32x4 wn[NP];                                                                                       \
            f32x4 vn0 = {0.f, 0.f, 0.f, 0.f}, vn1 = {0.f, 0.f, 0.f, 0.f};                                       \
            if ((B) < 7) {                                                                                      \
                _Pragma("unroll") for (int p = 0; p < NP; ++p) wn[p] = *(const u32x4*)(Wv + p * W_PLANE + ((B) + 1) * 16 * 16); \
                if (GS_NAREAD(B) == 1) vn0 = a_half(GS_HF((B) + 1));                                            \
                if (GS_NAREAD(B) == 2) { vn0 = a_half((B) + 1); vn1 = a_half((B) + 2); }                        \
            }                                                                                                   \
            if constexpr (!F16) {                                                                               \
                mfma_row(HH, B, NP - 1, w[0]);  /* a3 w1 */                                                     \
                mfma_row(HH, B, 0, w[NP - 1]);  /* a1 w3 */                                                     \
                mfma_row(HH, B, 1, w[1]);       /* a2 w2 */                                                     \
            }                                                                                                   \
            mfma_row(HH, B, 1, w[0]);  /* a2 w1 */                                                              \
            mfma_row(HH, B, 0, w[1]);  /* a1 w2 */                                                              \
            mfma_row(HH, B, 0, w[0]);  /* a1 w1 */                                                              \
            if (!GS_EXP_NOSPLIT) {                                                                              \
                if (GS_NSPLIT(B) >= 1) split_half(GS_HF(B), v0);                                                 \
                if (GS_NSPLIT(B) == 2) split_half((B) + 1, v1);                                                 \
            }                                                                                                   \
            if ((B) == 7 && HH == NH - 1) {                                                                     \
                _Pragma("unroll") for (int a = 0; a < NA; ++a)                                                  \
                    _Pragma("unroll") for (int p = 0; p < NP; ++p) ap[a][p] = an[a][p];                         \
            }                                                                                                   \
            _Pragma("unroll") for (int d = 0; d < GS_NDMA(B); ++d) dma(GS_DMA0 + GS_NDMA(B) * (B) + d);         \
            if (GS_NREAD(B) > 0) __builtin_amdgcn_sched_group_barrier(0x100, GS_NREAD(B) > 0 ? GS_NREAD(B) : 1, 0); \
            GS_SLOT(B, 0) GS_SLOT(B, 1) GS_SLOT(B, 2) GS_SLOT(B, 3) GS_SLOT(B, 4) GS_SLOT(B, 5)                 \
            GS_SLOT(B, 6) GS_SLOT(B, 7) GS_SLOT(B, 8) GS_SLOT(B, 9) GS_SLOT(B, 10) GS_SLOT(B, 11)               \
            GS_SLOT(B, 12) GS_SLOT(B, 13) GS_SLOT(B, 14) GS_SLOT(B, 15) GS_SLOT(B, 16) GS_SLOT(B, 17)           \
            GS_SLOT(B, 18) GS_SLOT(B, 19) GS_SLOT(B, 20) GS_SLOT(B, 21) GS_SLOT(B, 22) GS_SLOT(B, 23)           \
            GS_FENCE();                                                                                         \
            if ((B) < 7) {                                                                                      \
                _Pragma("unroll") for (int p = 0; p < NP; ++p) w[p] = wn[p];                                    \
                if (GS_NAREAD(B) >= 1) v0 = vn0;                                                                \
                if (GS_NAREAD(B) == 2) v1 = vn1;                                                                \
            }                                                                                                   \
        }
        GS_STEP(0) GS_STEP(1) GS_STEP(2) GS_STEP(3) GS_STEP(4) GS_STEP(5) GS_STEP(6) GS_STEP(7)
#undef GS_STEP
#undef GS_SLOT
#undef GS_VSLOT
#undef GS_NVALU
#undef GS_NDMA
#undef GS_DMA0
#undef GS_HF
#undef GS_NREAD
#undef GS_NAREAD
#undef GS_NSPLIT
        GS_DIAG_STAMP(0)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        GS_DIAG_STAMP(1)
        if (!GS_EXP_NOBAR) GB2_BARRIER();
        GS_DIAG_STAMP(2)
      };
      half_tile(std::integral_constant<int, 0>{});
      if constexpr (NH == 2) half_tile(std::integral_constant<int, 1>{});
    }
#ifdef GB2_CLOCK_DIAG
    if (threadIdx.x == 0 && P.C2) {   // diagnostic build only: in-kernel clock = d(s_memtime) / d(s_memrealtime) * 100 MHz
        unsigned long long* dg = (unsigned long long*)P.C2 + 2 * (blockIdx.x + gridDim.x * blockIdx.z);
        dg[0] = __builtin_amdgcn_s_memtime() - dg_c0;
        dg[1] = __builtin_amdgcn_s_memrealtime() - dg_r0;
        unsigned long long* dx = (unsigned long long*)P.C2 + 2 * gridDim.x * gridDim.z + 3 * (blockIdx.x + gridDim.x * blockIdx.z);
        dx[0] = dg_acc[0]; dx[1] = dg_acc[1]; dx[2] = dg_acc[2];
    }
    const unsigned long long dg_loop_end = __builtin_amdgcn_s_memtime();
#endif
#undef GS_PIPE
#undef GS_FENCE
#undef GLDS16
    // (the last tile ended with lgkmcnt(0) + barrier: the ring is dead, the epilogue image may overwrite it)
    // The epilogue is specialised per kind (gemm_split_epilogue.h).  Its lane index is laundered here so that hipcc cannot form the
    // epilogue's lane-dependent addresses above the k-loop, where they would cost the loop its registers.
    (void)cscale;                                      // (1 here: the specialised epilogue holds it as a constant)
    int elane = lane;
    asm volatile("" : "+v"(elane));
    gemm_split_wide_epilogue<EPI, STORE_H>(args, P, smem, m0, n0, uwave, elane, acc16);
#ifdef GB2_CLOCK_DIAG
    if (threadIdx.x == 0 && P.C2) {
        unsigned long long* dy = (unsigned long long*)P.C2 + 5 * gridDim.x * gridDim.z + 2 * (blockIdx.x + gridDim.x * blockIdx.z);
        dy[0] = dg_c0 - dg_entry;                                   // prologue: entry -> main loop
        dy[1] = __builtin_amdgcn_s_memtime() - dg_loop_end;         // epilogue (stores issued, not necessarily landed)
    }
#endif
}

// 128 x 256 as two column halves of 128, two workgroups per CU: one kernel per epilogue kind.  The kind is chosen on the host
// (gemm_split_wide_kernel), so a kernel's code holds one epilogue and hipcc allocates the k-loop's registers as it did for the
// single kernel (a switch inside one kernel moved the seven kinds' scalar and address work above the loop: 256 VGPRs and scratch).
// Every name begins with iefvad_gemm_split_n128x2_kernel, which is what the profile summaries select by.
typedef void (*GemmSplitWideKernel)(GemmBArgs);
#define GSW_KERNEL(suffix, EPI, STORE_H)                                                                      \
    __global__ __launch_bounds__(256, 2) void iefvad_gemm_split_n128x2_kernel##suffix(GemmBArgs args) {       \
        extern __shared__ __attribute__((aligned(16))) float smem[];                                          \
        gemm_split_wide_body<EPI, STORE_H>(args, smem);                                                       \
    }
GSW_KERNEL(, EPI_BIAS, true)
GSW_KERNEL(_qkv, EPI_QKV, true)
GSW_KERNEL(_relu, EPI_BIAS_RELU, true)
GSW_KERNEL(_resid, EPI_BIAS_RESID, true)
GSW_KERNEL(_refine, EPI_REFINE, true)
GSW_KERNEL(_heads, EPI_HEADS, true)
GSW_KERNEL(_gate, EPI_GATE, true)
GSW_KERNEL(_dot, EPI_BIAS_RELU_DOT, false)
GSW_KERNEL(_dot_h, EPI_BIAS_RELU_DOT, true)
#undef GSW_KERNEL

// every kernel above, for the callers that raise the dynamic-LDS limit
static const GemmSplitWideKernel kGemmSplitWideKernels[] = {
    iefvad_gemm_split_n128x2_kernel,        iefvad_gemm_split_n128x2_kernel_qkv,   iefvad_gemm_split_n128x2_kernel_relu,
    iefvad_gemm_split_n128x2_kernel_resid,  iefvad_gemm_split_n128x2_kernel_refine, iefvad_gemm_split_n128x2_kernel_heads,
    iefvad_gemm_split_n128x2_kernel_gate,   iefvad_gemm_split_n128x2_kernel_dot,   iefvad_gemm_split_n128x2_kernel_dot_h};

// The kernel of an epilogue kind; store_h: the dot kind also stores h (C is given).  nullptr: no such kind.
static inline GemmSplitWideKernel gemm_split_wide_kernel(int epi, bool store_h) {
    switch (epi) {
    case EPI_BIAS: return iefvad_gemm_split_n128x2_kernel;
    case EPI_QKV: return iefvad_gemm_split_n128x2_kernel_qkv;
    case EPI_BIAS_RELU: return iefvad_gemm_split_n128x2_kernel_relu;
    case EPI_BIAS_RESID: return iefvad_gemm_split_n128x2_kernel_resid;
    case EPI_REFINE: return iefvad_gemm_split_n128x2_kernel_refine;
    case EPI_HEADS: return iefvad_gemm_split_n128x2_kernel_heads;
    case EPI_GATE: return iefvad_gemm_split_n128x2_kernel_gate;
    case EPI_BIAS_RELU_DOT: return store_h ? iefvad_gemm_split_n128x2_kernel_dot_h : iefvad_gemm_split_n128x2_kernel_dot;
    default: return nullptr;
    }
}

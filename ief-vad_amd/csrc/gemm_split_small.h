// Small-M tiling of the bf16x6 split projection (gemm_split.h): the arithmetic of iefvad_gemm_split_n128_kernel, bit for bit, on a
// short per-wave MFMA chain.  It exists for the batch-invariant mode (iefvad_set_batch_invariant): a bf16x6 handle in that mode runs
// the split arithmetic at every row count, and on small grids the 128 x 128 tiling leaves most of the chip idle behind one wave's 96
// MFMAs per k-tile.  It takes a launch of up to kSplitSmallMaxWgs workgroups of the 128 x 128 tiling (launch_rules.h).  Measured
// (tools/batch_invariant_probe.py, profiles/batch_invariant_probe.log; K = 768, bias epilogue): 17.6 us against the 128 x 128 tiling's
// 29.2 us at M = 256, N = 768; 26.5 against 31.8 us at 480 workgroups (M = 1280, N = 1536); 44.9 against 31.6 us at 576, its second
// round.  It is bound by latency, not by MFMAs (0.73 us per k-tile at M = 256): an iteration waits for the LDS-DMA issued one k-tile
// earlier.  Tried and rejected (TRIED.md): a three-slot W ring, two k-tiles ahead, with the A fragments loaded straight into registers
// -- the same bits, 19.6 us, and from 257 workgroups on a second round (72 KB of LDS ran one workgroup per CU).
//
//   C[M,N] = epilogue( A[M,K] * W[N,K]^T + bias[N] ),  A fp32 (split in registers, Split4), W the three bf16 planes.
//
// Shape (chosen because the 32 x 128 block is one row band of the existing epilogue image, so the epilogue code can be shared):
//   block tile 32 x 128, four waves, wave w owns all 32 rows x columns 32 w .. 32 w + 31: 2 row tiles x 2 column tiles of
//   v_mfma_f32_16x16x32_bf16 x 6 products = 24 MFMAs per k-tile and wave (n128: 96), on four independent accumulators, so the six
//   dependent products of one accumulator are four issue slots apart.  Every wave splits its own copy of the 32 A rows (16 elements
//   per lane and k-tile, 88 VALU: duplicated four times per block, the price of not exchanging planes through LDS on a chain this short).
//   Grid (M / 32)(N / 128) x nz: 16 x the workgroups of the 128 x 128 tiling on M, so one chunk (M = 256, N = 768) is 48 workgroups.
// Why the bits are those of the n128 kernel: an output element is a sum over k-tiles of 32 in ascending order, and inside a k-tile
// over the six products a3 w1, a1 w3, a2 w2, a2 w1, a1 w2, a1 w1 into ONE accumulator, lane (r16, q16) supplying k = 8 q16 .. 8 q16 + 7
// -- the instruction, the k-to-lane assignment and the order are those of gemm_split_body.  The accumulators are parked in one
// [32][GB2_EPI_LD] LDS image shared by the four waves and gemm_wave_epilogue (NW = 4) runs over it: wave w takes rows rq + 2 u,
// u = 4 w .. 4 w + 3, with the SAME row-wise code (bias, ReLU, residual, refine, heads, the in-lane 4-column dot and its 32-lane
// DPP order, one partial per 128 columns at C2[row * (N / 128) + tile]) that the n128 kernel runs, not a copy of it.
// Ring: as in gemm_split.h, a one-tile-ahead double buffer filled by LDS-DMA, the A ring one k-tile ahead of the W ring (the fp32
// fragments of k-tile t+1 are read and split while the MFMAs of k-tile t run), one barrier per k-tile, the same swizzles:
//   A slot [32 rows][128 B fp32] = 4 KB, one 1 KB LDS-DMA instruction per wave (8 rows), chunk index XOR ((row >> 1) & 5);
//   W slot 3 planes x [128 rows][64 B] = 24 KB, six instructions per wave, chunk index XOR G[(row >> 2) & 3].
// The issue order is left to the compiler (no sched_group_barrier): 24 MFMAs leave too little to pin.
// Shapes: M % 32 == 0, N % 128 == 0, K % 64 == 0, K >= 64, nz in {1, 2} (plan_gemm_split_small).
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): see the figures at the kernel below.
// Training (train.h) keeps its own kernel rule and never launches this kernel.
#pragma once
#include "gemm_split.h"

#define GSS_BM 32
#define GSS_BN 128
#define GSS_A_SLOT (GSS_BM * 32)                       // 4-byte units: 32 rows x 128 B
#define GSS_W_PLANE (GSS_BN * 16)                      // 128 rows x 64 B
#define GSS_W_SLOT (3 * GSS_W_PLANE)
#define GSS_W_BASE (2 * GSS_A_SLOT)
#define GSS_LDS_BYTES ((2 * GSS_A_SLOT + 2 * GSS_W_SLOT) * 4)      // 57,344 B (the epilogue image, 16,896 B, reuses the ring)
static_assert(GSS_LDS_BYTES >= GSS_BM * GB2_EPI_LD * 4, "the epilogue image lives in the dead ring");
static_assert(GSS_BM == kSplitSmallBM && GSS_BN == kSplitBN, "launch_rules.h plans this tile");

// 70 VGPR + 0 AGPR, 41 SGPR, no scratch, no spills; LDS 57,344 B dynamic: two workgroups per CU by LDS (the 160 KB of a CU), i.e. two
// waves per SIMD, where the registers alone would allow seven.
__global__ __launch_bounds__(256, 2) void iefvad_gemm_split_small_kernel(GemmBArgs args) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const GemmBProblem& P = args.p[blockIdx.z];
    const int ntn = args.N / GSS_BN;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tm = bid / ntn, tn = bid - tm * ntn;
    const int m0 = tm * GSS_BM, n0 = tn * GSS_BN;
    const int K = args.K, lda = args.lda;
    const int wplane = args.wplane;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, q16 = lane >> 4;
    const int uwave = __builtin_amdgcn_readfirstlane(wave);

    // ---- staging (LDS-DMA, lane-linear 1 KB images; the swizzle is applied to the SOURCE chunk) ----
    // A: wave w -> rows 8 w + (lane >> 3), chunk lane & 7 (row bit 3 = w & 1 enters the swizzle)
    // W: wave w, plane p, instruction j -> rows 32 w + 16 j + (lane >> 2), chunk lane & 3
    const int nrecA = (int)((GSS_BM - 1) * lda + K) * 4, nrecW = 2 * wplane + (int)((GSS_BN - 1) * K + K) * 2;
    const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)P.A + (size_t)m0 * lda * 4), 0, nrecA, 0x00020000);
    const auto rsW = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)P.W + (size_t)n0 * K * 2), 0, nrecW, 0x00020000);
    const int arow = lane >> 3, achk = lane & 7;
    const int voA = arow * lda * 4 + ((achk ^ (((arow >> 1) & 1) | ((wave & 1) << 2))) << 4);
    const int wrow = lane >> 2, wchk = lane & 3;
    const int voW = wrow * K * 2 + ((wchk ^ ((0xD2 >> (2 * ((wrow >> 2) & 3))) & 3)) << 4);
#define GSS_GLDS16(rs, vo, so, lp) \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(lp), 16, vo, so, 0, 0)
    auto stage_a = [&](int tile, int slot) {
        GSS_GLDS16(rsA, voA, (uwave * 8 * lda + tile * GS_BK) * 4, smem + slot * GSS_A_SLOT + uwave * 8 * 32);
    };
    auto stage_w = [&](int tile, int slot) {
        float* Wd = smem + GSS_W_BASE + slot * GSS_W_SLOT + uwave * 32 * 16;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                GSS_GLDS16(rsW, voW, p * wplane + ((uwave * 32 + j * 16) * K + tile * GS_BK) * 2, Wd + p * GSS_W_PLANE + j * 16 * 16);
    };

    // ---- fragment addresses (4-byte units) ----
    const int swa = (r16 >> 1) & 5;
    const int a_lo = r16 * 32 + (((2 * q16) ^ swa) << 2);
    const int a_hi = r16 * 32 + (((2 * q16 + 1) ^ swa) << 2);
    const int b_of = (wave * 32 + r16) * 16 + ((q16 ^ ((0xD2 >> (2 * ((r16 >> 2) & 3))) & 3)) << 2);

    f32x4 acc16[2][8];                                 // [row tile][column tile]: column tiles 0 and 1 are used (gemm_wave_epilogue's type)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc16[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    u32x4 ap[2][3];                                    // planes of the A fragments of the current k-tile
    // row tile x of the k-tile in A slot `slot`: fp32 fragment (k = 8 q16 .. 8 q16 + 7 of row r16) -> three planes
    auto split_tile = [&](int slot, int x, u32x4 (&dst)[3]) {
        const float* Av = smem + slot * GSS_A_SLOT + x * 16 * 32;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            Split4 sp;
            sp.r = *(const f32x4*)(Av + (hf ? a_hi : a_lo));
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                unsigned d0, d1;
                sp.plane(d0, d1, p < 2);
                dst[p][2 * hf] = d0;
                dst[p][2 * hf + 1] = d1;
            }
        }
    };

    const int nk = K / GS_BK;                          // >= 2
    stage_a(0, 0);
    stage_a(1, 1);
    stage_w(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    GB2_BARRIER();
    split_tile(0, 0, ap[0]);
    split_tile(0, 1, ap[1]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    GB2_BARRIER();                                     // every wave has read A slot 0: k-tile 2 may land there

    // One k-tile per iteration: W of slot (kt & 1) against the planes in `ap`; the fp32 A fragments of k-tile kt + 1 (A slot
    // (kt + 1) & 1) are read and split on the way.  LDS-DMA of this iteration: A of k-tile kt + 2 into A slot (kt & 1), whose
    // fragments every wave took before the last barrier; W of k-tile kt + 1 into W slot ((kt + 1) & 1), last read in iteration kt - 1.
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 2 < nk) stage_a(kt + 2, kt & 1);
        if (kt + 1 < nk) stage_w(kt + 1, (kt + 1) & 1);
        const float* Wv = smem + GSS_W_BASE + (kt & 1) * GSS_W_SLOT + b_of;
        u32x4 w[2][3];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int p = 0; p < 3; ++p) w[b][p] = *(const u32x4*)(Wv + p * GSS_W_PLANE + b * 16 * 16);
        auto mfma4 = [&](int pa, int pw) {             // one product on the four accumulators
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    acc16[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ap[a][pa]),
                                                                          __builtin_bit_cast(bf16x8, w[b][pw]), acc16[a][b], 0, 0, 0);
        };
        mfma4(2, 0);       // a3 w1
        mfma4(0, 2);       // a1 w3
        mfma4(1, 1);       // a2 w2
        mfma4(1, 0);       // a2 w1
        mfma4(0, 1);       // a1 w2
        mfma4(0, 0);       // a1 w1
        if (kt + 1 < nk) {
            u32x4 an[2][3];
            split_tile((kt + 1) & 1, 0, an[0]);
            split_tile((kt + 1) & 1, 1, an[1]);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int p = 0; p < 3; ++p) ap[a][p] = an[a][p];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        GB2_BARRIER();
    }
#undef GSS_GLDS16
    // (the last tile ended with lgkmcnt(0) + barrier: the ring is dead, the shared epilogue image may overwrite it)
    f32x16 unused[1][4];
    gemm_wave_epilogue<true, 1, true, 4>(args, P, smem, m0, n0, 0, 0, unused, acc16, 1.0f, nullptr);
}

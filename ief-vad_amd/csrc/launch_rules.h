// Kernel selection of libiefvad: which of the bit-identical kernels of a stage runs, and on what grid.  Host-only C++17 -- no HIP,
// no pointers, no handle -- so that tests/cabi/launch_rules.cpp (g++, no GPU) pins every threshold at its boundary
// (tests/test_launch_rules_cpu.py).  iefvad.hip asks for a plan, fills the argument block and launches what the plan names.
#pragma once
#include "../../include/iefvad.h"   // IEFVAD_COMPUTE_*

// ------------------------------------------------------------------------------------------------
// tile dimensions the rules read (the kernels' LDS byte sizes stay in the kernel headers)
// ------------------------------------------------------------------------------------------------
#define GEMM_BM 128                 // fp32 128 x 128 (gemm_f32.h); also the block tile of the bf16 v1 kernel
#define GEMM_BN 128
#define GEMM_BK 32
#define GEMS_BM 64                  // fp32 64 x 64
#define GEMS_BN 64
#define GEMT_BM 32                  // fp32 32 x 32
#define GEMT_BN 32
#define GEMMB_BK 64                 // bf16 elements per k-tile (128 bytes per row)
#define GB2_BM 128                  // bf16 ring, 128 x 256 (gemm_bf16.h); the fp32 128 x 256 kernel runs on the same ring
#define GB2_BN 256
#define GB2_BK 32                   // bf16 elements per k-tile
#define GB3_BM 256                  // bf16 ring, 256 x 256
#define GS_BM 128                   // split kernels (gemm_split.h): NA = 2: 128 x 128, NA = 4: 128 x 256
#define GS_BN_OF(NA) ((NA) == 4 ? 256 : 128)
#define IC_BM 64                    // rows per block of the bf16 row-block kernels: in_proj, out_proj + LayerNorm, heads, refinement
#define OC_BM 64
#define HC_BM 64
#define HC_THIRDS 3
#define RC_BM 64

// ------------------------------------------------------------------------------------------------
// environment switches, as create_impl reads them
// ------------------------------------------------------------------------------------------------
static const int kRowblockMinWgsDefault = 128;   // tools/rowblock_threshold_probe.py
static const int kChainMinBlocksDefault = 4;     // one chunk: 4 blocks take one block time, 2K launches more

struct LaunchPolicy {
    // IEFVAD_ROWBLOCK_OFF=<mask> at iefvad_create (A/B runs and the bit-identity tests): bf16 mode takes the stage off its row-block kernel
    //   1 in_proj -> ring GEMM (+ the stand-alone cast); 2 out_proj + LayerNorm -> ring GEMM + LayerNorm kernel;
    //   4 heads + fusion -> ring GEMM + fusion kernel; 8 refinement chain -> 2K projection launches + the scorer kernel
    bool no_inproj_chain, no_ln_fusion, no_heads_fusion, no_chain;
    int rowblock_min_wgs;  // bf16 mode: the row-block kernels take a projection from this many workgroups on (IEFVAD_ROWBLOCK_MIN_WGS overrides)
    int chain_min_blocks;  // bf16 mode: the refinement chain kernel takes a micro-batch from this many 64-row blocks on (IEFVAD_CHAIN_MIN_BLOCKS overrides)
    bool persist;          // bf16 mode: the persistent out_proj + LayerNorm, heads + fusion and attention kernels from two blocks per CU on (IEFVAD_PERSIST=0: off)
    int split_tile;        // IEFVAD_SPLIT_TILE=128 / 256: the bf16x6 projections on one tiling of the split kernel (unset: plan_gemm_split's rule)
    bool dense_encoder;    // IEFVAD_DENSE_ENCODER=1: whole-video passes run the encoder on whole 256-row chunks (pad rows computed), the tail on the gathered valid rows
    // iefvad_set_batch_invariant (not an environment switch; launch_policy leaves it false): a bf16x6 handle runs the split
    // arithmetic at EVERY row count, so its results do not depend on how the caller batches.  Below the split kernels'
    // crossover the projections run on the small tiling (plan_gemm_split_small, same bits as the 128 x 128 one).
    bool split_always;
};
// from the switches' numeric values (0 = unset): out-of-range values fall back to the defaults
static inline LaunchPolicy launch_policy(int rowblock_off, int rowblock_min_wgs, int chain_min_blocks, bool persist, int split_tile, bool dense_encoder) {
    LaunchPolicy p;
    p.no_inproj_chain = rowblock_off & 1; p.no_ln_fusion = rowblock_off & 2; p.no_heads_fusion = rowblock_off & 4; p.no_chain = rowblock_off & 8;
    p.rowblock_min_wgs = rowblock_min_wgs > 0 ? rowblock_min_wgs : kRowblockMinWgsDefault;
    p.chain_min_blocks = chain_min_blocks > 0 ? chain_min_blocks : kChainMinBlocksDefault;
    p.persist = persist;
    p.split_tile = (split_tile == 128 || split_tile == 256) ? split_tile : 0;
    p.dense_encoder = dense_encoder;
    p.split_always = false;
    return p;
}

// ------------------------------------------------------------------------------------------------
// projections: the launch is grid (wgs, 1, nz) of `kernel`, or refused for `reject`
// ------------------------------------------------------------------------------------------------
enum GemmKernel {
    GEMM_NONE = 0,
    GEMM_F32_TINY, GEMM_F32_SMALL, GEMM_F32_128, GEMM_F32_T256,          // iefvad_gemm_f32_{tiny, small, , t256}_kernel
    GEMM_BF16_V1, GEMM_BF16_PIPE, GEMM_BF16_W256,                        // iefvad_gemm_bf16_{v1, pipe, w256}_kernel
    GEMM_SPLIT_N128, GEMM_SPLIT_N128X2, GEMM_SPLIT_F16_N128              // iefvad_gemm_split_{n128, n128x2, f16_n128}_kernel
};
enum GemmReject { GEMM_OK = 0, GEMM_BAD_SHAPE, GEMM_BAD_TILE_N, GEMM_NO_WIDE_TILING, GEMM_BAD_DOT_EPILOGUE };
struct GemmPlan {
    GemmKernel kernel;
    int wgs;
    GemmReject reject;
};
static inline GemmPlan gemm_refused(GemmReject why) { return GemmPlan{GEMM_NONE, 0, why}; }

// Grid-size rules of the fp32 tilings, measured over B = 1 .. 256 chunks (profiles/r03_kernel_selection_thresholds.log): the 32x32
// kernel below 320 blocks of 64x64, the 128x256 one from 1536 blocks of 128x256 on, the 64x64 one below 1024 blocks of 128x128.
// They were {320, 256, 256} ("when the grid fills the chip") until measured: B = 48 forward 6.7 -> 5.5 ms.
static const int kF32TinyMaxBlocks64 = 320;
static const int kF32T256MinBlocks = 1536;
static const int kF32SmallMaxBlocks128 = 1024;

static inline GemmPlan plan_gemm_f32(int M, int N, int K, int nz) {
    if (M % GEMM_BM || N % GEMM_BN || K % GEMM_BK) return gemm_refused(GEMM_BAD_SHAPE);
    // Four tilings of the same contraction, bit-identical to each other (same k order per output element):
    //   128x256 / 3-slot ring (iefvad_gemm_f32_t256_kernel)  the throughput kernel, from 6 blocks per CU on (it wins 2 % at a full
    //                                                         micro-batch and loses 10-18 % between 1 and 4 blocks per CU);
    //   128x128 / double buffer (iefvad_gemm_f32_kernel)      mid-size grids or N not a multiple of 256;
    //   64x64 (iefvad_gemm_f32_small_kernel)                  up to 4 blocks of 128x128 per CU: 4x the blocks, a quarter of the MFMA chain;
    //   32x32 on 16x16x4 MFMAs (iefvad_gemm_f32_tiny_kernel)  the per-video pattern (B = 1 .. a few chunks): 16x the
    //                                                         blocks, a wave's chain is 3.2 us instead of 10 / 41 us.
    const int blocks128 = (M / GEMM_BM) * (N / GEMM_BN) * nz;
    const int blocks64 = (M / GEMS_BM) * (N / GEMS_BN) * nz;
    const bool t256_ok = (N % GB2_BN == 0) && (K % 16 == 0) && (K >= 32);
    const int blocks256 = t256_ok ? (M / GB2_BM) * (N / GB2_BN) * nz : 0;
    const bool tiny = blocks64 < kF32TinyMaxBlocks64 && K % 64 == 0;      // < 1.25 blocks of 64x64 per CU: the chain, not the chip, bounds it
    if (tiny) return GemmPlan{GEMM_F32_TINY, (M / GEMT_BM) * (N / GEMT_BN), GEMM_OK};
    if (blocks256 >= kF32T256MinBlocks) return GemmPlan{GEMM_F32_T256, (M / GB2_BM) * (N / GB2_BN), GEMM_OK};
    if (blocks128 < kF32SmallMaxBlocks128) return GemmPlan{GEMM_F32_SMALL, (M / GEMS_BM) * (N / GEMS_BN), GEMM_OK};
    return GemmPlan{GEMM_F32_128, (M / GEMM_BM) * (N / GEMM_BN), GEMM_OK};
}

static const int kBf16W256MinWgs = 256;      // one 256 x 256 workgroup per CU
static inline GemmPlan plan_gemm_bf16(int M, int N, int K, int nz, bool refine_epilogue) {
    if (N % GB2_BN == 0 && M % GB2_BM == 0 && K % GB2_BK == 0 && K >= 2 * GB2_BK) {
        // two bit-identical tilings: 256 x 256 / 8 waves / one workgroup per CU is 2-6 % faster with bias-type epilogues
        // (in_proj, out_proj, heads, the refinement's first projection), 128 x 256 / 4 waves / two per CU with the refinement
        // epilogue (residual read + two stores): tools/gemm_tune_bf16, profiles/r02_gemm_bf16_w256.log
        if (M % GB3_BM == 0 && !refine_epilogue && (M / GB3_BM) * (N / GB2_BN) * nz >= kBf16W256MinWgs)
            return GemmPlan{GEMM_BF16_W256, (M / GB3_BM) * (N / GB2_BN), GEMM_OK};
        return GemmPlan{GEMM_BF16_PIPE, (M / GB2_BM) * (N / GB2_BN), GEMM_OK};   // pinned issue order: +1..3 %, same bits
    }
    if (M % GEMM_BM || N % GEMM_BN || K % GEMMB_BK) return gemm_refused(GEMM_BAD_SHAPE);
    return GemmPlan{GEMM_BF16_V1, (M / GEMM_BM) * (N / GEMM_BN), GEMM_OK};
}

// BF16X6: the split kernel (128 x 128 tiles, two workgroups per CU; tools/gemm_tune_split: +5..8 % over the 128 x 256 /
// one-workgroup configuration, same bits) takes a micro-batch's projections from 72 workgroups of a 768-wide projection on
// (6 chunks: measured crossover, B = 24 forward 3.55 -> 1.97 ms; it was 512 workgroups, "fills the chip", until the end of
// round 3; profiles/r03_kernel_selection_thresholds.log); smaller problems run on the fp32 kernels (plan_gemm_f32)
static const int kSplitBN = GS_BN_OF(2);
static const int kSplitD = 768;         // the split (and bf16) arithmetics are built for D = 768 (IEF_D, common.h)
static const int kSplitMinWgs = 72;      // 6 chunks
static inline bool split_eligible(int M, int N, int K, int nz) {
    return M % GS_BM == 0 && N % kSplitBN == 0 && K % 64 == 0 && K >= 64 && (M / GS_BM) * (N / kSplitBN) * nz >= kSplitMinWgs;
}

// Two bit-identical tilings of the bf16x6 arithmetic (gemm_split.h): 128 x 128, and 128 x 256 as two column halves that share the
// A planes (half the split work and A staging per MFMA: 7 % less time at 262,144 rows).  The wide one takes a launch whose wide grid
// has at least kSplitWideMinWgs workgroups, the measured crossover (`tools/gemm_tune_split sweep` at N = 768, 1536 and 2304, bias and
// refine epilogues, profiles/split_wide_gemm_tune.log): from three rounds of the chip's 512 workgroup slots on it wins at all three
// widths (time ratio 0.93-0.98); at two rounds it ties (0.99-1.01), at one round and below the narrow grid's twice as many, half as
// long workgroups win by 6-15 %.  tile_n = 128 / 256 forces a tiling (the unit entry iefvad_gemm_split_unit, IEFVAD_SPLIT_TILE);
// the fp16x3 arithmetic has the narrow tiling only.
static const int kSplitWideMinWgs = 1536;     // 3 x 512
// dot_epilogue: EPI_BIAS_RELU_DOT; dot_operands: its vector (R) and its partial sums (C2) are both there
static inline GemmPlan plan_gemm_split(int M, int N, int K, int nz, bool f16, int tile_n, bool dot_epilogue = false, bool dot_operands = false) {
    if (M % GS_BM || N % kSplitBN || K % 64 || K < 64) return gemm_refused(GEMM_BAD_SHAPE);
    if (tile_n != 0 && tile_n != 128 && tile_n != 256) return gemm_refused(GEMM_BAD_TILE_N);
    if (tile_n == 256 && (f16 || N % 256)) return gemm_refused(GEMM_NO_WIDE_TILING);
    const bool wide = !f16 && N % 256 == 0 && (tile_n == 256 || (tile_n == 0 && (M / GS_BM) * (N / 256) * nz >= kSplitWideMinWgs));
    if (dot_epilogue && (f16 || nz != 1 || !dot_operands)) return gemm_refused(GEMM_BAD_DOT_EPILOGUE);
    return GemmPlan{wide ? GEMM_SPLIT_N128X2 : f16 ? GEMM_SPLIT_F16_N128 : GEMM_SPLIT_N128, (M / GS_BM) * (N / (wide ? 256 : kSplitBN)), GEMM_OK};
}
// The small tiling of the bf16x6 arithmetic (gemm_split_small.h): 32 x 128 workgroups of four waves, 24 MFMAs per k-tile and wave
// against the 128 x 128 tiling's 96, bit-identical to it.  In the batch-invariant mode (LaunchPolicy::split_always) it takes a
// projection while its own grid fits the chip's 512 workgroup slots (256 CUs x 2 by LDS) in ONE round, i.e. up to kSplitSmallMaxWgs =
// 128 workgroups of the 128 x 128 tiling, and plan_gemm_split takes the rest.  Measured (tools/batch_invariant_probe.py, K = 768, us per
// launch, medians of 5 outside each other's min - max; profiles/batch_invariant_probe.log): the small tiling wins at every grid up to
// 120 workgroups of 128 x 128 -- N = 768: 17.6 against 29.3 at 12, 24.4 against 31.6 at 96; N = 1536: 27.0 against 32.2 at 120;
// N = 2304: 27.1 against 32.1 at 108 -- and loses from 144 on, its second round (N = 1536: 45.2 against 31.6; N = 2304: 46.7 against
// 32.0).  That is above kSplitMinWgs = 72, the default mode's crossover between the 128 x 128 tiling and the short-chain fp32 kernels,
// which stays where it is: the default selection does not change.  Bits do not depend on the choice.  A plan of its own: GemmKernel /
// GemmReject keep their enumerators.
static const int kSplitSmallBM = 32;
static const int kSplitSmallMaxWgs = 128;     // in workgroups of the 128 x 128 tiling: 4 x as many of 32 x 128 = one round of 512 slots
struct GemmSmallPlan {
    bool ok;               // false: refused, `why` says which of the shape rules
    int wgs;               // grid (wgs, 1, nz)
    GemmReject why;        // GEMM_OK, GEMM_BAD_SHAPE or GEMM_BAD_DOT_EPILOGUE
};
static inline GemmSmallPlan plan_gemm_split_small(int M, int N, int K, int nz, bool dot_epilogue = false, bool dot_operands = false) {
    if (M <= 0 || N <= 0 || M % kSplitSmallBM || N % kSplitBN || K % 64 || K < 64 || nz < 1 || nz > 2) return GemmSmallPlan{false, 0, GEMM_BAD_SHAPE};
    if (dot_epilogue && (nz != 1 || !dot_operands)) return GemmSmallPlan{false, 0, GEMM_BAD_DOT_EPILOGUE};
    return GemmSmallPlan{true, (M / kSplitSmallBM) * (N / kSplitBN), GEMM_OK};
}
// batch-invariant mode: which split tiling a bf16x6 projection runs on
static inline bool split_small_preferred(int M, int N, int K, int nz) {
    if (M % GS_BM || N % kSplitBN || K % 64 || K < 64) return true;      // no 128 x 128 plan: the small plan accepts or refuses the shape
    return (M / GS_BM) * (N / kSplitBN) * nz <= kSplitSmallMaxWgs;
}

// IEFVAD_SPLIT_TILE is a preference: a projection the wide tiling cannot take (fp16x3, N % 256 != 0) runs on the narrow one
static inline int split_tile_for(int preferred, int N, bool f16) {
    return (f16 || (preferred == 256 && N % 256)) ? (f16 ? 0 : 128) : preferred;
}

// ------------------------------------------------------------------------------------------------
// bf16 stages: the one-block-per-workgroup kernel or its persistent variant (same bits), grid (gx, gy, gz)
// ------------------------------------------------------------------------------------------------
enum StageKernel {
    STAGE_OUTLN_CHAIN, STAGE_OUTLN_PCHAIN,                                             // iefvad_outproj_ln_{chain, pchain}_bf16_kernel
    STAGE_ATTN_BF16, STAGE_ATTN_BF16_ROWS, STAGE_ATTN_PBF16, STAGE_ATTN_PBF16_ROWS,    // iefvad_attention_{bf16, pbf16}[_rows]_kernel
    STAGE_HEADS_CHAIN, STAGE_HEADS_PCHAIN                                              // iefvad_heads_{chain, pchain}_bf16_kernel
};
struct StagePlan {
    StageKernel kernel;
    int gx, gy, gz;
};

// From two blocks per workgroup on: the persistent kernel, one workgroup per CU, the next block's image fetched during the LayerNorm
// epilogue (outproj_ln_pchain_bf16.h; same bits); IEFVAD_PERSIST=0 keeps the one-block-per-workgroup kernels (A/B).
// uniform_outputs: both modalities store the same set of results (fp32 rows, bf16 rows), and at least one
static inline StagePlan plan_outproj_ln(const LaunchPolicy& p, int num_cus, int rows, bool uniform_outputs) {
    const int gx = num_cus / 2;
    const int nblk = rows / OC_BM;
    if (p.persist && nblk >= 2 * gx && uniform_outputs) return StagePlan{STAGE_OUTLN_PCHAIN, gx, 2, 1};
    return StagePlan{STAGE_OUTLN_CHAIN, nblk, 2, 1};
}

// from two items per CU on: the persistent kernel (attention_pbf16.h: one 8-wave workgroup per CU, K / V staged once for
// both query halves by LDS-DMA, the next item's K in flight under the current item); bit-identical to the one-item kernel.
// nb: chunks per modality (8 heads each); rows_mode: the row-compressed chunks of a whole-video pass (`_rows` kernels)
static inline StagePlan plan_attention_bf16(const LaunchPolicy& p, int num_cus, int nb, bool rows_mode) {
    const int heads = 8;      // IEF_H (common.h)
    const int items = 2 * nb * heads;
    if (p.persist && items >= 2 * num_cus) return StagePlan{rows_mode ? STAGE_ATTN_PBF16_ROWS : STAGE_ATTN_PBF16, num_cus, 1, 1};
    return StagePlan{rows_mode ? STAGE_ATTN_BF16_ROWS : STAGE_ATTN_BF16, heads, 2, 2 * nb};
}

// from two blocks per workgroup on: the persistent kernel (heads_pchain_bf16.h: one workgroup per CU and column third, both
// images by LDS-DMA under the previous block's epilogue / the first part of phase 2; same bits); IEFVAD_PERSIST=0: A/B
static inline StagePlan plan_heads(const LaunchPolicy& p, int num_cus, int rows) {
    const int gx = num_cus / HC_THIRDS;
    if (p.persist && rows / HC_BM >= 2 * gx) return StagePlan{STAGE_HEADS_PCHAIN, gx, HC_THIRDS, 1};
    return StagePlan{STAGE_HEADS_CHAIN, rows / HC_BM, HC_THIRDS, 1};
}

// ------------------------------------------------------------------------------------------------
// per-pass flags: which family of kernels a micro-batch's stages run on
// ------------------------------------------------------------------------------------------------
// Of the encoder's row set (rows: whole chunks, or the row-compressed set of a whole-video pass)
struct PassFlags {
    bool ip_chain;            // bf16 mode, full grids: in_proj on the row-block kernel (inproj_chain_bf16.h); its first layer reads the fp32 rows
    bool need_xb0;            // bf16 mode also needs the bf16 copy of the inputs (unless ip_chain)
    bool splitmb, f16mb;      // the split kernels take this micro-batch's projections; ... in the fp16x3 arithmetic
    // out_proj + residual + LayerNorm(s) in one row-owning kernel (bf16 mode, full grids): 64-row blocks on the refinement chain's
    // structure (outproj_ln_chain_bf16.h); same bits as the GEMM + LayerNorm kernels
    bool ln_fused;
};
static inline PassFlags plan_pass(const LaunchPolicy& p, int compute, int rows) {
    const bool bf = compute == IEFVAD_COMPUTE_BF16;
    PassFlags f;
    f.ip_chain = bf && !p.no_inproj_chain && rows % IC_BM == 0 && (rows / IC_BM) * 2 >= p.rowblock_min_wgs;
    f.need_xb0 = bf && !f.ip_chain;
    f.splitmb = (compute == IEFVAD_COMPUTE_BF16X6 || compute == IEFVAD_COMPUTE_FP16X3) && split_eligible(rows, kSplitD, kSplitD, 1);
    if (p.split_always && compute == IEFVAD_COMPUTE_BF16X6) f.splitmb = true;      // batch-invariant: one arithmetic at every row count
    f.f16mb = f.splitmb && compute == IEFVAD_COMPUTE_FP16X3;
    f.ln_fused = bf && !p.no_ln_fusion && rows % OC_BM == 0 && (rows / OC_BM) * 2 >= p.rowblock_min_wgs;
    return f;
}

// Of everything behind the encoder, evaluated on the row count after compaction (a dense-encoder whole-video pass gathers its valid rows)
struct TailFlags {
    bool tail_split;          // the split kernels take the tail's projections
    // 2 + 3 in one kernel (bf16 mode, full grids): heads of both modalities + fusion on the row-block structure (heads_chain_bf16.h)
    bool heads_rows;
    // 4 + 5 in one kernel (bf16 mode): the K refinement steps and the scorer with the state on chip, refine_chain_bf16.h
    bool chain;
    bool fold;                // bf16x6 on the split kernels, K >= 1: the last step's second projection is folded into the scorer
};
// K: refinement steps; heads_packed / chain_packed: the handle holds the stage's weights in the row-block kernel's stream order
static inline TailFlags plan_tail(const LaunchPolicy& p, int compute, int rows, int K, bool splitmb, bool compacted, bool heads_packed, bool chain_packed) {
    const bool bf = compute == IEFVAD_COMPUTE_BF16;
    TailFlags f;
    f.tail_split = splitmb && (!compacted || split_eligible(rows, kSplitD, kSplitD, 1));   // bf16x6: a small compact set runs on the fp32 kernels
    if (p.split_always && compute == IEFVAD_COMPUTE_BF16X6) f.tail_split = true;           // batch-invariant: compacted or not, hence fold = (K >= 1)
    f.heads_rows = bf && !p.no_heads_fusion && heads_packed && rows % HC_BM == 0 && (rows / HC_BM) * HC_THIRDS >= p.rowblock_min_wgs;
    f.chain = bf && K > 0 && !p.no_chain && chain_packed && rows % RC_BM == 0 && rows / RC_BM >= p.chain_min_blocks;
    f.fold = f.tail_split && compute == IEFVAD_COMPUTE_BF16X6 && K >= 1;
    return f;
}

// Head-averaged attention weights of one encoder layer: what nn.MultiheadAttention(...)(x, x, x) returns second with
// need_weights=True (imf_vad.py:115,121 compute it on every call and discard it) -- mean over the 8 heads of
// softmax(Q_h K_h^T / sqrt(d_h)), [256, 256] fp32 per chunk and modality.  Opt-in (iefvad_forward_attn, iefvad_forward_videos_attn).
//
// The kernel reads the layer's fp32 q | k | v rows right behind the attention launch, while they are alive.  q is pre-scaled by
// log2(e)/sqrt(d_h) (EPI_QKV), so the softmax is exp2(s - max) as in attention_f32.h, and the score tile is formed the same way:
// S^T = K_h Q_h^T on v_mfma_f32_32x32x2_f32, lane = query, registers = keys, a query's row in the lane pair (q, q + 32).
//
// One workgroup = (query half, chunk, modality): 4 waves x 32 queries, and it walks the eight heads in index order.  A lane cannot
// hold 256 scores beside 256 running means (128 + 128 registers per lane, plus 48 of q), so every head takes two sweeps over its
// four 64-key K tiles, 16 score registers live:
//   sweep 1  running max and sum of the lane's 128 keys (rescaled when the max moves), merged over the lane pair at its end;
//   sweep 2  the scores again (d_h-deep products: cheap), p = exp2(s - max), mean += p * (1 / sum / 8).
// The tiles stream through the double-buffered LDS image of attention_f32.h (same staging map, same ATT_LDK_OF padding); the
// eight tile steps of a head alternate between the buffers, and the prefetch runs on into the next head.  Sums are formed as trees
// (16 registers -> 1), so a row's sum is 13 additions deep, not 128.  Fixed order, no atomics: the same call gives the same bits.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; `make resource-usage`), 2 waves / SIMD:
//   <RG, DH>      VGPRs  AGPRs  spills  scratch  LDS
//   <false, 96>   241    0      0       0        51200
//   <true,  96>   254    0      0       0        51200
//   <false, 64>   221    0      0       0        34816
//   <true,  64>   234    0      0       0        34816
// Three things keep it there (each one alone brings spills back): no branch inside the head loop, the score tiles fenced one by one
// with sched_barrier, and the K tile staged in two halves.
#pragma once
#include "attention_f32.h"
#include "common.h"

struct AttnMapArgs {
    const float* qkv[2];           // [N, 3 D] per modality: q | k | v, head h at columns h * DH
    float* out[2];                 // [rows, 256] per modality; nullptr: the modality is not computed
    int nchunks;                   // chunks per modality in this launch
    // whole-video passes: the pass's chunk table.  It decides what is written (rows < valid, at packed row src_row + r); the
    // row-mapped kernels also read through it (row r of the window = row min(r, valid) of the chunk's compressed rows).
    // nullptr: dense, chunk c writes rows c * 256 ..
    const RaggedChunk* chunks;
};

__device__ __forceinline__ float attn_maps_max16(const f32x16& s) {
    const float a0 = fmaxf(s[0], s[1]), a1 = fmaxf(s[2], s[3]), a2 = fmaxf(s[4], s[5]), a3 = fmaxf(s[6], s[7]);
    const float a4 = fmaxf(s[8], s[9]), a5 = fmaxf(s[10], s[11]), a6 = fmaxf(s[12], s[13]), a7 = fmaxf(s[14], s[15]);
    return fmaxf(fmaxf(fmaxf(a0, a1), fmaxf(a2, a3)), fmaxf(fmaxf(a4, a5), fmaxf(a6, a7)));
}

template <bool RG, int DH>
__device__ __forceinline__ void attention_maps_body(const AttnMapArgs& args, float* kv) {
    constexpr int D = IEF_H * DH;
    constexpr int LDK = ATT_LDK_OF(DH), TILE = ATT_TILE_OF(DH);
    constexpr int NS = DH / 8;                       // q registers (f32x4) per lane
    constexpr int NSTG = 2 * (DH / 32);              // staging pieces per thread
    const int qhalf = blockIdx.x, chunk = blockIdx.y % args.nchunks, mod = blockIdx.y / args.nchunks;
    if (!args.out[mod]) return;
    int row0 = chunk * IEF_T, last = IEF_T - 1, valid = IEF_T;
    size_t orow = (size_t)chunk * IEF_T;
    if (args.chunks) {
        const RaggedChunk c = args.chunks[chunk];
        valid = c.valid;
        orow = (size_t)c.src_row;
        if constexpr (RG) {
            row0 = c.enc_row;
            last = ragged_rows(c.valid) - 1;
        }
        if (qhalf * 128 >= valid) return;            // every query of this half is a pad row: nothing to write
    }
#define ATM_ROW(r) (RG ? ((r) < last ? (r) : last) : (r))
    const float* qkv = args.qkv[mod] + (size_t)row0 * (3 * D);

    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int q0 = qhalf * 128 + wave * 32;

    // attention_f32.h's staging map: thread t moves rows (t >> 3) + 32 hf, 4-float chunks (t & 7) + 8 j of a 64-key tile (hf: row half)
    const int srow0 = t >> 3, sch0 = t & 7;
    // uniform bases (they move on by DH floats per head) and 32-bit per-thread offsets within the chunk's rows (< 2^20 floats)
    const float* __restrict__ gsrc = qkv + D;        // the K column block
    const float* __restrict__ qsrc = qkv;
    const int goff = (RG ? 0 : srow0 * (3 * D)) + sch0 * 4;      // RG: the row is clamped per load
    const int qoff = ATM_ROW(q0 + i) * (3 * D) + 4 * h;
    float* ldst = kv + srow0 * LDK + sch0 * 4;
    // A tile is staged in two halves of 32 keys, each loaded in front of one of the step's two score tiles and written to the other
    // buffer behind it: NSTG / 2 staging registers (f32x4) instead of NSTG -- with all of them the DH = 96 kernels spill.
    f32x4 stg[NSTG / 2];
    // rows 32 hf .. of key tile kt (64 keys) of the current head (gsrc), `hd` floats further right
#define ATM_LOAD(hd, kt, hf)                                                                                  \
    _Pragma("unroll") for (int j = 0; j < NSTG / 2; ++j)                                                      \
        stg[j] = *(const f32x4*)(gsrc + (unsigned)(goff + (RG ? ATM_ROW((kt) * ATT_TK + 32 * (hf) + srow0)    \
                                                              : (kt) * ATT_TK + 32 * (hf)) * (3 * D) + (hd) + 32 * j));
#define ATM_WRITE(buf, hf)                                                                                    \
    _Pragma("unroll") for (int j = 0; j < NSTG / 2; ++j)                                                      \
        *(f32x4*)(ldst + (buf) * TILE + 32 * (hf) * LDK + 32 * j) = stg[j];

    ATM_LOAD(0, 0, 0)
    ATM_WRITE(0, 0)
    ATM_LOAD(0, 0, 1)
    ATM_WRITE(0, 1)
    __syncthreads();

    f32x16 mean[8];                                    // mean[kt][r]: key 32 kt + (r & 3) + 8 (r >> 2) + 4 h of query q0 + i
#pragma unroll
    for (int kt = 0; kt < 8; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) mean[kt][r] = 0.f;

#pragma unroll 1
    for (int head = 0; head < IEF_H; ++head) {
        // Q fragment: lane (i, h) holds Q[q0 + i][8 s + 4 h .. + 3] of this head (B operand of K Q^T)
        f32x4 q[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) q[s] = *(const f32x4*)(qsrc + (unsigned)(qoff + 8 * s));
        float m = -INFINITY, l = 0.f;                // sweep 1: running max and sum of this lane's 128 keys
        float c = 0.f;                               // sweep 2: 1 / (8 sum)
#pragma unroll
        for (int ti = 0; ti < 8; ++ti) {             // tile ti & 3 of K_h: 0..3 sweep 1, 4..7 sweep 2
            const float* T = kv + (ti & 1) * TILE;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                // Half u of the next tile; behind a head's last step that is tile 0 of the next head, DH floats to the right.  The last
                // head loads it too (the first columns of V in the same rows: in bounds, never used): a branch here would split the loop
                // body into blocks, and hipcc then sinks the exp2 / fma of all of sweep 2 behind the branch, with the eight score tiles
                // alive -- spills.
                if (ti + 1 < 8) { ATM_LOAD(0, (ti + 1) & 3, u) }
                else { ATM_LOAD(DH, 0, u) }
                __builtin_amdgcn_sched_barrier(0);   // keep the loads in front of the MFMAs (attention_f32.h)
                f32x16 st;
#pragma unroll
                for (int r = 0; r < 16; ++r) st[r] = 0.f;
                const float* kp = T + (u * 32 + i) * LDK + 4 * h;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const f32x4 ka = *(const f32x4*)(kp + 8 * s);
#pragma unroll
                    for (int e = 0; e < 4; ++e) st = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[e], q[s][e], st, 0, 0, 0);
                }
                if (ti < 4) {
                    const float mn = fmaxf(m, attn_maps_max16(st));
#pragma unroll
                    for (int r = 0; r < 16; ++r) st[r] = __builtin_amdgcn_exp2f(st[r] - mn);
#pragma unroll
                    for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
                        for (int r = 0; r < w; ++r) st[r] += st[r + w];
                    l = l * __builtin_amdgcn_exp2f(m - mn) + st[0];       // m = -inf at first: l = 0 * 0 + sum
                    m = mn;
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        mean[2 * (ti - 4) + u][r] = fmaf(__builtin_amdgcn_exp2f(st[r] - m), c, mean[2 * (ti - 4) + u][r]);
                }
                ATM_WRITE((ti + 1) & 1, u)           // the other buffer: its previous tile was released by the last barrier
                __builtin_amdgcn_sched_barrier(0);   // one score tile at a time
            }
            if (ti == 3) {
                // the pair's max and sum: each lane rescales its own sum, the sum of the two is commutative -- both lanes get the same bits
                // (no contraction: a fused l * e + other would round the two lanes' sums differently)
#pragma clang fp contract(off)
                const float mx = fmaxf(m, __shfl_xor(m, 32, 64));
                const float ls = l * __builtin_amdgcn_exp2f(m - mx);
                const float sum = ls + __shfl_xor(ls, 32, 64);
                m = mx;
                c = 0.125f / sum;
            }
            __syncthreads();
        }
        gsrc += DH;                                  // the next head's columns
        qsrc += DH;
    }
#undef ATM_LOAD
#undef ATM_WRITE
#undef ATM_ROW
    // store: the lane's keys come in runs of four (r & 3), run (kt, r >> 2) at key 32 kt + 8 (r >> 2) + 4 h
    const int qrow = q0 + i;
    if (qrow < valid) {
        float* o = args.out[mod] + (orow + (size_t)qrow) * IEF_T + 4 * h;
#pragma unroll
        for (int kt = 0; kt < 8; ++kt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v;
                v[0] = mean[kt][4 * g]; v[1] = mean[kt][4 * g + 1]; v[2] = mean[kt][4 * g + 2]; v[3] = mean[kt][4 * g + 3];
                *(f32x4*)(o + 32 * kt + 8 * g) = v;
            }
    }
}

template <bool RG, int DH>
__global__ __launch_bounds__(256, 2) void iefvad_attention_maps_kernel(AttnMapArgs args) {
    __shared__ __attribute__((aligned(16))) float kv[2 * ATT_TILE_OF(DH)];
    attention_maps_body<RG, DH>(args, kv);
}

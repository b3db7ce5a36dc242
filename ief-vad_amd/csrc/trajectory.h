// The refinement trajectory of one forward (include/iefvad.h, iefvad_forward_trajectory): per snippet and state z_k of the K-step
// iteration z_{k+1} = z_k - lambda (W2_k relu(W1_k z_k + b1_k) + b2_k)   (imf_vad.py:146-149)
//   logits_steps[k] = c . z_k + b_c          k = 0 .. steps      the score a model stopped after k steps gives (before the sigmoid)
//   delta_norm[k]   = ||z_{k+1} - z_k||_2    k = 0 .. steps - 1  = lambda ||r_k||: the iteration's convergence diagnostic
// The states pass through HBM anyway on the launch-per-projection routes (z is updated in place by EPI_REFINE), so one row pass
// between two steps reads them where they are; no projection kernel changes.  The previous state lives in a second [rows, D] buffer
// z_prev of the pass, which this kernel alone writes.
//
// The row-kernel idiom of rowops.h / similarity.h: one wavefront per row, 16-byte loads (lane l owns columns 4 l + 256 j), fp32
// sums, wave_sum reductions in their fixed order; no LDS, no atomics.  The score is taken exactly as iefvad_scorer_kernel takes it
// (same column ownership, same order of the lane's multiply-adds, same reduction, bias added last), so logits_steps[k] has the bits
// the plain scorer gives on z_k.
//
// One launch per state:
//   first != 0 (z = z_0):   logit_out <- c . z + b_c;                                   z_prev <- z  (store_prev)
//   first == 0 (z = z_k+1): delta_out <- ||z - z_prev||;  logit_out <- c . z + b_c;     z_prev <- z  (store_prev: not after the last step)
// logit_out / delta_out are the rows of the call's [steps + 1, stride] / [steps, stride] outputs that belong to this state (either
// may be null).  logits_src != nullptr: logit_out receives logits_src[row] instead -- where the folded scorer of the bf16x6
// arithmetic has already produced the call's logits from z_{K-1} and h, the last entry is that value, not a second evaluation.
//
// Rows: the row set of ONE pass, as iefvad_similarity_rowset_kernel walks it.  With a chunk table, chunk c owns row-set rows
// enc_row .. enc_row + valid - 1, which are packed rows src_row .. of the pass; with chunks == nullptr (a dense pass, or the compacted
// set) slab s stands for rows 256 s .. of the first valid_rows rows and the map is the identity.  Grid (chunk or slab, slice).  Pad
// rows are never read or written.  Output column = row0 + packed row of the pass.
// HBM traffic per row: D * 4 bytes read (+ D * 4 for z_prev after step 0) and D * 4 written while a later step follows.
#pragma once
#include "common.h"
#include "rowops.h"

#define TRAJ_SLICES 8
template <int D>
__global__ __launch_bounds__(256) void iefvad_step_probe_kernel(const float* __restrict__ z, float* __restrict__ z_prev, const float* __restrict__ w,
                                                                 const float* __restrict__ b, const float* __restrict__ logits_src,
                                                                 const RaggedChunk* __restrict__ chunks, int valid_rows,
                                                                 float* __restrict__ logit_out, float* __restrict__ delta_out, long long row0,
                                                                 int first, int store_prev) {
    constexpr int NJ = D / 256;
    int begin, dst, nr;                                              // row-set row, packed row of the pass, rows: workgroup-uniform
    if (chunks) {
        const RaggedChunk c = chunks[blockIdx.x];
        begin = c.enc_row; dst = c.src_row; nr = c.valid;
    } else {
        begin = dst = blockIdx.x * 256;
        nr = valid_rows - begin < 256 ? valid_rows - begin : 256;
    }
    const int lane = threadIdx.x & 63;
    const bool want_delta = !first && delta_out;
    for (int r = ROW_WAVES * blockIdx.y + (threadIdx.x >> 6); r < nr; r += ROW_WAVES * gridDim.y) {
        const size_t row = (size_t)begin + r;
        const float* zp = z + row * D + 4 * lane;
        float* pp = z_prev + row * D + 4 * lane;
        f32x4 zv[NJ];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            zv[j] = *(const f32x4*)(zp + 256 * j);
            const f32x4 wv = *(const f32x4*)(w + 4 * lane + 256 * j);
#pragma unroll
            for (int e = 0; e < 4; ++e) s += zv[j][e] * wv[e];
        }
        float d = 0.f;
        if (want_delta) {
            f32x4 g = zv[0] - *(const f32x4*)pp;
            f32x4 dd = g * g;
#pragma unroll
            for (int j = 1; j < NJ; ++j) {
                g = zv[j] - *(const f32x4*)(pp + 256 * j);
                dd = g * g + dd;
            }
            d = wave_sum(ln_hsum(dd));
        }
        s = wave_sum(s);
        if (store_prev)
#pragma unroll
            for (int j = 0; j < NJ; ++j) *(f32x4*)(pp + 256 * j) = zv[j];
        if (lane == 0) {
            const long long col = row0 + dst + r;
            if (logit_out) logit_out[col] = logits_src ? logits_src[row] : s + b[0];
            if (want_delta) delta_out[col] = sqrtf(d);
        }
    }
}

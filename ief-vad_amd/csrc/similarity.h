// The four per-snippet series of the reference's similarity plots (test.py:235-238, train/ucf_test.py:243-247):
//   cos_i = F.cosine_similarity(fused, image_mu)     dist_i = torch.norm(fused - image_mu)          (and the event pair likewise)
// reduced on the device from the three [rows, D] tensors the full-dict forward already writes -- 16 bytes per snippet leave the
// device instead of three D-wide rows.  The row-kernel idiom of rowops.h: one wavefront per OUTPUT row, ROW_WAVES rows per 256-thread
// block, 16-byte loads (lane l owns columns 4l + 256 j), wave_sum reductions.  No LDS, no atomics.
//
// Output row j reads source row s = src_rows ? src_rows[j] : j, so the `[0:len]` slice of every video of a padded batch (test.py:142)
// is one index vector and the x16 repeat of the plots is never formed on the device.  Entries of src_rows lie in [0, rows): a caller
// error otherwise -- such an entry is not read for, its four outputs are NaN.
//
// Seven fp32 sums per row, as seven independent reduction chains (the scheduler interleaves independent DPP chains, rowops.h ln_rows):
//   ff = sum f^2, ii = sum i^2, ee = sum e^2, fi = sum f i, fe = sum f e, di = sum (f - i)^2, de = sum (f - e)^2
// The squared distances are summed directly: ff + ii - 2 fi cancels where fused is close to a mean.
//   cos_i = fi / (max(sqrt(ff), 1e-8) * max(sqrt(ii), 1e-8))      torch's form: each factor divided by its own clamped norm
//   dist_i = sqrt(di)
// NaN propagates as in torch: a NaN in fused reaches all four values, a NaN in one mean only that modality's pair (fmaxf drops a NaN
// norm, the NaN numerator keeps it).  Sums are plain fp32: a row whose squared sums overflow fp32 (|x| beyond ~1e18) is outside the
// contract -- torch scales nothing either, but its sums differ in order and may overflow elsewhere.
//
// similarity_row_body holds the loads, the seven sums and the finishing arithmetic; both kernels below call it, so a row gives the same
// bits whichever kernel reduces it.
//
// iefvad_similarity_rowset_kernel (iefvad_forward_videos_similarity, include/iefvad.h) runs on the row set of ONE valid-row pass, where
// fused (= z_K), image_mu and event_mu sit in the pass's workspace in row-set order (ragged.h): chunk c of the pass's table owns
// row-set rows enc_row .. enc_row + valid - 1, which are packed rows src_row .. of the pass -- the map of iefvad_rows_out_kernel.  With
// chunks == nullptr (the compacted set: the tail already ran in packed order) slab s stands for rows 256 s .. of the first valid_rows
// rows and the map is the identity.  Grid (chunk or slab, slice): the waves of slice y take rows 4 y + wave, then every
// 4 gridDim.y-th, so a 256-row chunk is SIM_SLICES workgroups and not one workgroup's serial loop.  Pad rows and the rows that round
// the set up to whole tiles are never read.  The output is the [4, stride] layout of the whole CALL (stride = its packed row count);
// the pass writes columns row0 + packed row of the pass.
#pragma once
#include "common.h"
#include "rowops.h"

template <int D>
__device__ __forceinline__ void similarity_row_body(const float* __restrict__ fused, const float* __restrict__ image_mu,
                                                    const float* __restrict__ event_mu, size_t s, int lane, float* __restrict__ out,
                                                    long long stride, long long j) {
    constexpr int NJ = D / 256;
    const size_t base = s * D + 4 * lane;
    f32x4 f[NJ], im[NJ], ev[NJ];
#pragma unroll
    for (int c = 0; c < NJ; ++c) {
        f[c] = *(const f32x4*)(fused + base + 256 * c);
        im[c] = *(const f32x4*)(image_mu + base + 256 * c);
        ev[c] = *(const f32x4*)(event_mu + base + 256 * c);
    }
    f32x4 ff = f[0] * f[0], ii = im[0] * im[0], ee = ev[0] * ev[0], fi = f[0] * im[0], fe = f[0] * ev[0];
    f32x4 gi = f[0] - im[0], ge = f[0] - ev[0];
    f32x4 di = gi * gi, de = ge * ge;
#pragma unroll
    for (int c = 1; c < NJ; ++c) {
        ff = f[c] * f[c] + ff;
        ii = im[c] * im[c] + ii;
        ee = ev[c] * ev[c] + ee;
        fi = f[c] * im[c] + fi;
        fe = f[c] * ev[c] + fe;
        gi = f[c] - im[c];
        ge = f[c] - ev[c];
        di = gi * gi + di;
        de = ge * ge + de;
    }
    float r[7] = {ln_hsum(ff), ln_hsum(ii), ln_hsum(ee), ln_hsum(fi), ln_hsum(fe), ln_hsum(di), ln_hsum(de)};
#pragma unroll
    for (int q = 0; q < 7; ++q) r[q] = wave_sum(r[q]);
    if (lane == 0) {
        const float nf = fmaxf(sqrtf(r[0]), 1e-8f), ni = fmaxf(sqrtf(r[1]), 1e-8f), ne = fmaxf(sqrtf(r[2]), 1e-8f);
        out[j] = r[3] / (nf * ni);
        out[stride + j] = r[4] / (nf * ne);
        out[2 * stride + j] = sqrtf(r[5]);
        out[3 * stride + j] = sqrtf(r[6]);
    }
}

template <int D>
__global__ __launch_bounds__(256) void iefvad_similarity_rows_kernel(const float* __restrict__ fused, const float* __restrict__ image_mu,
                                                                      const float* __restrict__ event_mu, long long rows,
                                                                      const int* __restrict__ src_rows, long long nout, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long j = (long long)blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (j >= nout) return;
    const long long s = src_rows ? (long long)src_rows[j] : j;      // wave-uniform
    if (s < 0 || s >= rows) {
        if (lane == 0)
#pragma unroll
            for (int q = 0; q < 4; ++q) out[q * nout + j] = __builtin_nanf("");
        return;
    }
    similarity_row_body<D>(fused, image_mu, event_mu, (size_t)s, lane, out, nout, j);
}

#define SIM_SLICES 8
template <int D>
__global__ __launch_bounds__(256) void iefvad_similarity_rowset_kernel(const float* __restrict__ fused, const float* __restrict__ image_mu,
                                                                        const float* __restrict__ event_mu,
                                                                        const RaggedChunk* __restrict__ chunks, int valid_rows,
                                                                        float* __restrict__ out, long long stride, long long row0) {
    int first, dst, nr;                                              // row-set row, packed row of the pass, rows: workgroup-uniform
    if (chunks) {
        const RaggedChunk c = chunks[blockIdx.x];
        first = c.enc_row; dst = c.src_row; nr = c.valid;
    } else {
        first = dst = blockIdx.x * 256;
        nr = valid_rows - first < 256 ? valid_rows - first : 256;
    }
    const int lane = threadIdx.x & 63;
    for (int r = ROW_WAVES * blockIdx.y + (threadIdx.x >> 6); r < nr; r += ROW_WAVES * gridDim.y)
        similarity_row_body<D>(fused, image_mu, event_mu, (size_t)first + r, lane, out, stride, row0 + dst + r);
}

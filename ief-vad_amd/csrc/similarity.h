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
#pragma once
#include "common.h"
#include "rowops.h"

template <int D>
__global__ __launch_bounds__(256) void iefvad_similarity_rows_kernel(const float* __restrict__ fused, const float* __restrict__ image_mu,
                                                                      const float* __restrict__ event_mu, long long rows,
                                                                      const int* __restrict__ src_rows, long long nout, float* __restrict__ out) {
    constexpr int NJ = D / 256;
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
    const size_t base = (size_t)s * D + 4 * lane;
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
        out[nout + j] = r[4] / (nf * ne);
        out[2 * nout + j] = sqrtf(r[5]);
        out[3 * nout + j] = sqrtf(r[6]);
    }
}

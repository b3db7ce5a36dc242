// The training loader's window rule on the device (/root/reference/data/tools.py:65-97: process_feat -> uniform_extract / pad;
// the test_mode == False branch of data/dataset.py:41-43, :71-73, :117-119).
//
// A video of n feature rows becomes ONE [256, D] fp32 window:
//   n <= 256: the rows (widened to fp32), zero rows behind them; length n.
//   n >  256: 256 segments with boundaries r[i] = (i n) >> 8 (= np.linspace(0, n, 257, dtype=int32) for every n: i (n / 256) is exact
//             in fp64), every segment >= 1 row; output row i = np.mean(rows r[i] .. r[i+1]-1, axis 0); length 256.
// The mean is numpy's, bit for bit: an fp32 accumulator that starts at +0, the rows added in ascending order with one fp32 add each
// (fp16 rows widened first), then ONE correctly rounded fp32 division by float(count); an fp16 file's quotient is rounded to fp16
// (nearest even) and widened again (np.mean of fp16 returns fp16).  So a sum is never split, there is no tree and no atomic, no
// reciprocal multiply: parallelism comes from the nv * 256 * D destinations.  Non-finite values pass through as the arithmetic has it.
//
//   * iefvad_resample_rows_kernel: a lane owns 16 bytes of ONE output row (4 fp32 / 8 fp16 columns) and streams its segment; a
//     wave's loads cover contiguous runs of a source row.  IEF_RS_AHEAD source rows are requested before the first add of a trip:
//     the adds are a dependent chain, the loads are not.  Segment lengths differ by orders of magnitude BETWEEN videos (2 rows at
//     n = 300, 156 at n = 40,000), so the host sorts the table longest video first: the long chains start while the machine is
//     full and the short ones fill the tail.
//   * iefvad_gather_windows_kernel: one step's batch = B cached windows of the image and of the event set picked by an index
//     vector, plus their lengths, in one launch.
#pragma once
#include <hip/hip_fp16.h>
#include "common.h"

struct ResampleVideo {
    long long src_row;   // first row of the video in the packed input
    int n;               // its row count (>= 1)
    int out;             // index of its window in the output (the video's position in the caller's list)
};
static_assert(sizeof(ResampleVideo) == 16, "ResampleVideo is 16 bytes");

#define IEF_RS_AHEAD 8

template <typename T> struct ResampleVec;
template <> struct ResampleVec<float> {
    static constexpr int G = 4;
    typedef f32x4 raw;
    static __device__ __forceinline__ void widen(const raw& r, float* f) {
#pragma unroll
        for (int e = 0; e < 4; ++e) f[e] = r[e];
    }
    static __device__ __forceinline__ float round_result(float q) { return q; }
};
typedef _Float16 rs_f16x8 __attribute__((ext_vector_type(8)));
template <> struct ResampleVec<__half> {
    static constexpr int G = 8;
    typedef rs_f16x8 raw;
    static __device__ __forceinline__ void widen(const raw& r, float* f) {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = (float)r[e];
    }
    static __device__ __forceinline__ float round_result(float q) { return (float)(_Float16)q; }      // nearest even, as numpy's cast
};

// grid: (D / G column groups * 256 output rows / 256 threads) workgroups per video, the videos in table order.
template <typename T>
__global__ __launch_bounds__(256) void iefvad_resample_rows_kernel(const T* rows, const ResampleVideo* table, int D, float* out,
                                                                   int* out_lengths) {
    typedef ResampleVec<T> V;
    constexpr int G = V::G;
    const int groups = D / G;                               // 16-byte column groups of a row = workgroups per video
    const ResampleVideo vid = table[blockIdx.x / groups];
    const int item = (blockIdx.x % groups) * 256 + threadIdx.x;      // < 256 * groups
    const int orow = item / groups, col = (item % groups) * G;
    if (item == 0) out_lengths[vid.out] = vid.n < IEF_T ? vid.n : IEF_T;
    const T* src = rows + (size_t)vid.src_row * D + col;
    float* dst = out + ((size_t)vid.out * IEF_T + orow) * D + col;
    float acc[G];
#pragma unroll
    for (int e = 0; e < G; ++e) acc[e] = 0.f;
    if (vid.n <= IEF_T) {                                   // pad: copy / widen, zero fill
        if (orow < vid.n) V::widen(*(const typename V::raw*)(src + (size_t)orow * D), acc);
    } else {
        const long long r0 = ((long long)orow * vid.n) >> 8, r1 = ((long long)(orow + 1) * vid.n) >> 8;
        const int count = (int)(r1 - r0);                   // >= 1
        const T* p = src + (size_t)r0 * D;
        int k = 0;
        for (; k + IEF_RS_AHEAD <= count; k += IEF_RS_AHEAD) {
            typename V::raw v[IEF_RS_AHEAD];
#pragma unroll
            for (int u = 0; u < IEF_RS_AHEAD; ++u) v[u] = *(const typename V::raw*)(p + (size_t)(k + u) * D);
#pragma unroll
            for (int u = 0; u < IEF_RS_AHEAD; ++u) {
                float f[G];
                V::widen(v[u], f);
#pragma unroll
                for (int e = 0; e < G; ++e) acc[e] += f[e];
            }
        }
        if (k < count) {                                    // the last 1 .. AHEAD-1 rows: loads clamped to the segment, adds predicated
            typename V::raw v[IEF_RS_AHEAD - 1];
#pragma unroll
            for (int u = 0; u < IEF_RS_AHEAD - 1; ++u) {
                const int r = k + u < count ? k + u : count - 1;
                v[u] = *(const typename V::raw*)(p + (size_t)r * D);
            }
#pragma unroll
            for (int u = 0; u < IEF_RS_AHEAD - 1; ++u) {
                if (k + u < count) {
                    float f[G];
                    V::widen(v[u], f);
#pragma unroll
                    for (int e = 0; e < G; ++e) acc[e] += f[e];
                }
            }
        }
        const float c = (float)count;
#pragma unroll
        for (int e = 0; e < G; ++e) acc[e] = V::round_result(acc[e] / c);      // IEEE division: no reciprocal, no fast-math
    }
#pragma unroll
    for (int e = 0; e < G; e += 4) *(f32x4*)(dst + e) = f32x4{acc[e], acc[e + 1], acc[e + 2], acc[e + 3]};
}

// grid: (chunks per window, B, 2 sets); a workgroup copies IEF_GW_VEC 16-byte vectors per thread of window index[b] of one set,
// all loads issued before the first store.  An index outside [0, nset) (refused on the host) yields a zero window of length 0.
#define IEF_GW_VEC 4
__global__ __launch_bounds__(256) void iefvad_gather_windows_kernel(const float* img_set, const float* ev_set, const int* set_lengths,
                                                                    int nset, const int* index, int D, float* img_out, float* ev_out,
                                                                    int* len_out) {
    const int b = blockIdx.y, m = blockIdx.z;
    const int idx = index[b];
    const bool ok = idx >= 0 && idx < nset;
    if (m == 0 && blockIdx.x == 0 && threadIdx.x == 0) len_out[b] = ok ? set_lengths[idx] : 0;
    const int nvec = IEF_T * D / 4;                        // 16-byte vectors of a window
    const f32x4* src = (const f32x4*)((m ? ev_set : img_set) + (size_t)(ok ? idx : 0) * IEF_T * D);
    f32x4* dst = (f32x4*)((m ? ev_out : img_out) + (size_t)b * IEF_T * D);
    const int base = blockIdx.x * (256 * IEF_GW_VEC) + threadIdx.x;
    f32x4 v[IEF_GW_VEC];
#pragma unroll
    for (int u = 0; u < IEF_GW_VEC; ++u) {
        const int i = base + 256 * u;
        v[u] = (ok && i < nvec) ? src[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < IEF_GW_VEC; ++u) {
        const int i = base + 256 * u;
        if (i < nvec) dst[i] = v[u];
    }
}

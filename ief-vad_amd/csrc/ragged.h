// Whole videos in, scores of their snippets out: the reference's loader + test() prologue folded into the library
// (/root/reference/data/tools.py:100-114 process_split, /root/reference/test.py:76-121).
//
// The reference pads every video to whole 256-snippet chunks on the HOST (process_split), scans the padded tensor for NaN and
// copies it to the device (test.py:90-95), runs the model on all chunk rows and slices the padding away again (test.py:121).
// On ShanghaiTech / MSAD-sized lists 84 % of the chunk rows are padding, on UCF / XD-sized lists 35-40 %, and the host's two
// passes over them bound the evaluation loop.  Here the caller hands over ONLY the valid rows ([sum(len), 768], the videos
// concatenated in list order) and their lengths; on the device
//   * iefvad_nanflag_kernel finds, per video and modality, whether any element is NaN (the condition of test.py:90,93);
//   * iefvad_scatter_rows_kernel lays the rows out as zero-padded chunks (the chunker; the all-zero chunk of a
//     len % 256 == 0 video, whose rows test.py:121 slices away, is not built), applies torch.nan_to_num(nan=0.0) -- NaN -> 0,
//     +-inf -> the source dtype's max / min -- to the videos whose flag is set, widens to fp32 (imf_vad.py:41-42) and, in
//     bf16 mode, writes the bf16 operand copy as well;
//   * attention is over the full zero-padded window (imf_vad.py:115: unmasked by design), but the pad rows of a chunk are
//     identical in every layer, so the encoder's row set holds ONE of them per chunk (RaggedChunk, common.h): the projections
//     and LayerNorms run on valid + 1 rows per chunk, the attention kernels read row min(r, valid) for row r of the window
//     (attention_*.h, *_rows_kernel) -- every product and every sum of the dense computation, from fewer distinct rows;
//   * everything behind the encoder (imf_vad.py:125-150: heads, fusion, K refinement steps, scorer -- 56 % of the FLOPs, all
//     row-wise) runs on the same row set; iefvad_rows_out_kernel picks the valid rows' results (test.py:121).
//   fp16x3 (per-chunk operand scales) and IEFVAD_DENSE_ENCODER=1 keep whole chunks in the encoder;
//   iefvad_compact_rows_kernel then gathers the valid rows of the last LayerNorm's output for the tail.
// The robustness sweep (/root/reference/test2.py:35-123) runs on the same route through iefvad_forward_videos_scaled: the chunker's
// scaled instantiation applies the unconditional nan_to_num (test2.py:59-60) and a per-row scale (test2.py:70-77), and
// iefvad_colsum_rows_kernel / iefvad_colsum_finish_kernel reduce w_i / w_e over the valid rows to 768 sums per modality (test2.py:102-103).
// The reference's whole return dict (imf_vad.py:152-161) leaves the same route through iefvad_forward_videos_full / _host_full: the pass keeps
// the asked-for [rows, D] tensors of its row set and iefvad_rows_out_wide_kernel copies the valid rows to the caller's packed tensors.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>
#include "common.h"
#include "rowops.h"
#include "window_plan.h"

template <typename T> struct RaggedLimits;
template <> struct RaggedLimits<float> { static __device__ float max() { return 3.40282347e38f; } };
template <> struct RaggedLimits<__half> { static __device__ float max() { return 65504.f; } };
template <> struct RaggedLimits<__hip_bfloat16> { static __device__ float max() { return 3.38953139e38f; } };

// gridDim.z workgroups per (chunk, modality), each scanning every gridDim.z-th 4096-element tile (a pass of 60 - 130 chunks is
// 120 - 260 workgroups otherwise: a few per CU, each a chain of memory latencies): any NaN among the chunk's valid elements ->
// flags[2 video + modality] = 1.  The kernels here are templates on the row width D (768, or 512 for ViT-B/16 features).
#define IEF_RAGGED_SLICES 4
template <typename T, int D>
__global__ __launch_bounds__(256) void iefvad_nanflag_kernel(const T* img, const T* ev, const RaggedChunk* chunks, int* flags) {
    const RaggedChunk c = chunks[blockIdx.x];
    const T* src = (blockIdx.y ? ev : img) + (size_t)c.src_row * D;
    const int n = c.valid * D;                         // a multiple of D, hence of 4
    bool bad = false;
    for (int base = blockIdx.z * 4096 + threadIdx.x * 4; base < n; base += gridDim.z * 4096) {
        float v[16];                                   // four 16-byte (8-byte) loads in flight per lane
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * u + e] = (base + 1024 * u < n) ? (float)src[base + 1024 * u + e] : 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) bad |= (v[e] != v[e]);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) flags[2 * c.video + blockIdx.y] = 1;      // benign race: every writer stores 1
}

// gridDim.z workgroups per (chunk, modality), 16-row groups dealt round-robin: valid rows from the packed input (fixed up if the
// video's flag is set), zeros behind them (nrows = 256: whole chunks; nrows = 0: row-compressed, one zero row).
// SC (iefvad_forward_videos_scaled): `fix_all` replaces in every video (test2.py:59-60, no flag words), and packed row r of the pass
// is multiplied by sc0[r] / sc1[r] (nullable) AFTER the replacement (test2.py:70-77) with the semantics of
// iefvad_cast_scaled_kernel (rowops.h): fp32 product, rounded to T before the widening, a scale of exactly 1 leaves the bits
// alone.  Pad rows are the zeros written here, never scaled.  SC = false is the kernel of iefvad_forward_videos, unchanged.
// NOISE = RowNoise (iefvad_forward_videos_perturbed with an amplitude vector; a mode of SC): behind the scale, packed row r gets
// nz.amp[m][r] * eps added (add_row_noise4, common.h); an amplitude of exactly 0 leaves the bits alone.  The row's noise id is nz.id[r],
// or -- nz.id NULL -- its packed row in the CALL, nz.row0 + src_row + r: src_row is pass-relative.  The mode is a parameter pack
// (row_noise_of, common.h): without it the kernels are, name and code, the ones they were.
template <typename T, int D, bool SC = false, typename... NOISE>
__global__ __launch_bounds__(256) void iefvad_scatter_rows_kernel(const T* img, const T* ev, const RaggedChunk* chunks, const int* flags,
                                                                  float* out0, float* out1, __bf16* ob0, __bf16* ob1, int nrows,
                                                                  const float* sc0, const float* sc1, int fix_all, NOISE... noise) {
    constexpr bool NZ = sizeof...(NOISE) == 1;
    static_assert(sizeof...(NOISE) <= 1 && (SC || !NZ), "the noise mode is one RowNoise, on the scaled chunker");
    const RowNoise nz = row_noise_of(noise...);
    constexpr int NJ = D / 256;
    const RaggedChunk c = chunks[blockIdx.x];
    const int m = blockIdx.y;
    const T* src = (m ? ev : img) + (size_t)c.src_row * D;
    float* out = (m ? out1 : out0) + (size_t)c.enc_row * D;
    __bf16* ob = m ? ob1 : ob0;
    if (ob) ob += (size_t)c.enc_row * D;
    const bool fix = (SC && fix_all) || (flags && flags[2 * c.video + m] != 0);
    const float* sc = SC ? (m ? sc1 : sc0) : nullptr;
    if (sc) sc += c.src_row;
    const float* na = NZ ? nz.amp[m] : nullptr;
    if (na) na += c.src_row;
    const float big = RaggedLimits<T>::max();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nr = nrows ? nrows : ragged_rows(c.valid);
    // four rows of the wave per trip: all their loads are issued before the first store (a 40-row chunk is 2-3 trips of pure latency)
    for (int r0 = wave + 16 * blockIdx.z; r0 < nr; r0 += 16 * gridDim.z) {
        f32x4 v[4][NJ];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r0 + 4 * u;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int col = 4 * lane + 256 * j;
                v[u][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (r < c.valid) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[u][j][e] = (float)src[(size_t)r * D + col + e];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r0 + 4 * u;
            if (r >= nr) break;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int col = 4 * lane + 256 * j;
                f32x4 w = v[u][j];
                if (fix && r < c.valid) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float x = w[e];
                        w[e] = (x != x) ? 0.f : (x > big ? big : (x < -big ? -big : x));     // torch.nan_to_num(nan=0.0)
                    }
                }
                if (SC && sc && r < c.valid) {
                    const float f = sc[r];
                    if (f != 1.0f) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float prod = w[e] * f;
                            asm volatile("" : "+v"(prod));       // keep the fp32 product: no fpext -> fmul -> fptrunc fold (rowops.h)
                            w[e] = (float)(T)prod;
                        }
                    }
                }
                if (NZ && na && r < c.valid) {
                    const float a = na[r];
                    if (a != 0.0f)
                        add_row_noise4<T>(w, a, nz.seed, nz.id ? (unsigned)nz.id[c.src_row + r] : (unsigned)(nz.row0 + c.src_row + r), m, col);
                }
                *(f32x4*)(out + (size_t)r * D + col) = w;
                if (ob) *(bf16x4_t*)(ob + (size_t)r * D + col) = to_bf16x4(w);
            }
        }
    }
}

// one workgroup per (chunk, modality): the chunk's valid rows of x -> the compact row set (packed order)
struct CompactArgs {
    const float* x[2];      // [chunks * 256, 768] fp32, nullable
    float* xc[2];
    const __bf16* xb[2];    // the same in bf16, nullable
    __bf16* xcb[2];
    const RaggedChunk* chunks;
};
template <int D>
__global__ __launch_bounds__(256) void iefvad_compact_rows_kernel(CompactArgs a) {
    const RaggedChunk c = a.chunks[blockIdx.x];
    const int m = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < c.valid; r += 4) {
        const size_t s = ((size_t)c.enc_row + r) * D + 4 * lane, d = ((size_t)c.src_row + r) * D + 4 * lane;
        if (a.x[m]) {
#pragma unroll
            for (int j = 0; j < D / 256; ++j) *(f32x4*)(a.xc[m] + d + 256 * j) = *(const f32x4*)(a.x[m] + s + 256 * j);
        }
        if (a.xb[m]) {
#pragma unroll
            for (int j = 0; j < D / 256; ++j) *(bf16x4_t*)(a.xcb[m] + d + 256 * j) = *(const bf16x4_t*)(a.xb[m] + s + 256 * j);
        }
    }
}

// per-row results of a pass -> the caller's packed vectors.  chunks == nullptr: the rows are already in packed order (the tail
// ran on the compact row set): copy n values; else gather the valid rows of every chunk.
__global__ __launch_bounds__(256) void iefvad_rows_out_kernel(const float* s0, const float* s1, const float* s2, float* d0, float* d1,
                                                              float* d2, const RaggedChunk* chunks, int n) {
    if (!chunks) {
        const int i = blockIdx.x * 256 + threadIdx.x;
        if (i < n) {
            if (d0) d0[i] = s0[i];
            if (d1) d1[i] = s1[i];
            if (d2) d2[i] = s2[i];
        }
        return;
    }
    const RaggedChunk c = chunks[blockIdx.x];
    const int r = threadIdx.x;
    if (r < c.valid) {
        const size_t s = (size_t)c.enc_row + r, d = (size_t)c.src_row + r;
        if (d0) d0[d] = s0[s];
        if (d1) d1[d] = s1[s];
        if (d2) d2[d] = s2[s];
    }
}

// The D-wide counterpart (iefvad_forward_videos_full / _host_full): the valid rows of up to seven [rows, D] tensors of a pass's row set
// (z = fused, mu_i, mu_e, lv_i, lv_e, n_i, n_e where the tail left them) -> the caller's packed tensors, the row map of the kernel
// above: row-set row enc_row + r of chunk c -> packed row src_row + r of the pass (dst points at the pass's first packed row), r <
// valid; chunks == nullptr: the compacted set, identity over the first valid_rows rows in 256-row slabs.  The host lists only the
// tensors the caller asked for: gridDim.z workgroups per (chunk or slab, listed tensor), 16-row groups dealt round-robin as in the
// chunker (a 40-row chunk on one workgroup is three dependent trips of pure latency), one wavefront per row, 16 bytes per lane and
// 256-column group, four rows of the wave in flight.  Pad rows and tile-rounding rows are never read; no LDS, no atomics.
#define ROWS_OUT_WIDE_MAX 7
struct RowsOutWideArgs {
    const float* src[ROWS_OUT_WIDE_MAX];
    float* dst[ROWS_OUT_WIDE_MAX];
    const RaggedChunk* chunks;
    int valid_rows;
};
template <int D>
__global__ __launch_bounds__(256) void iefvad_rows_out_wide_kernel(RowsOutWideArgs a) {
    constexpr int NJ = D / 256;
    int first_s, first_d, nr;
    if (a.chunks) {
        const RaggedChunk c = a.chunks[blockIdx.x];
        first_s = c.enc_row; first_d = c.src_row; nr = c.valid;
    } else {
        first_s = first_d = blockIdx.x * 256;
        nr = a.valid_rows - first_s < 256 ? a.valid_rows - first_s : 256;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* src = a.src[blockIdx.y] + (size_t)first_s * D + 4 * lane;
    float* dst = a.dst[blockIdx.y] + (size_t)first_d * D + 4 * lane;
    for (int r0 = wave + 16 * blockIdx.z; r0 < nr; r0 += 16 * gridDim.z) {
        f32x4 v[4][NJ];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r0 + 4 * u;
            if (r < nr) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) v[u][j] = *(const f32x4*)(src + (size_t)r * D + 256 * j);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r0 + 4 * u;
            if (r >= nr) break;
#pragma unroll
            for (int j = 0; j < NJ; ++j) *(f32x4*)(dst + (size_t)r * D + 256 * j) = v[u][j];
        }
    }
}

// ---- column sums of the fusion weights over the VALID rows of a pass (iefvad_forward_videos_scaled, w_colsum): the 768 sums per
// modality behind the robustness sweep's w_img_change / w_ev_change (test2.py:86-87,102-103), without a [rows, D] tensor
// crossing the boundary.  One workgroup per (slab, modality): slab = chunk c of the table (rows enc_row .. enc_row + valid - 1
// of the tail's row set), or, chunks == nullptr (the compacted set: packed order), rows 256 slab .. of the first valid_rows rows.
// The scatter kernel's lane map: a lane owns columns 4 lane + 256 j, wave w takes rows w, w + 4, ... in ascending order into fp64
// registers; the four waves' sums meet in LDS and are added in wave order.  part[(slab * 2 + m) * D + col]: no atomics, the same
// bits on every run.
template <int D>
__global__ __launch_bounds__(256) void iefvad_colsum_rows_kernel(const float* n0, const float* n1, const RaggedChunk* chunks, int valid_rows,
                                                                 double* part) {
    constexpr int NJ = D / 256;
    __shared__ double lds[4][D];
    const int m = blockIdx.y;
    int first, nr;
    if (chunks) {
        const RaggedChunk c = chunks[blockIdx.x];
        first = c.enc_row; nr = c.valid;
    } else {
        first = blockIdx.x * 256;
        nr = valid_rows - first < 256 ? valid_rows - first : 256;
    }
    const float* src = (m ? n1 : n0) + (size_t)first * D;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[NJ][4];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[j][e] = 0.0;
    // four rows of the wave per trip, all their loads issued before the first add
    for (int r0 = wave; r0 < nr; r0 += 16) {
        f32x4 v[4][NJ];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r0 + 4 * u;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                v[u][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (r < nr) v[u][j] = *(const f32x4*)(src + (size_t)r * D + 4 * lane + 256 * j);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (r0 + 4 * u >= nr) break;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j][e] += (double)v[u][j][e];
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) lds[wave][4 * lane + 256 * j + e] = acc[j][e];
    __syncthreads();
    double* dst = part + ((size_t)blockIdx.x * 2 + m) * D;
    for (int col = threadIdx.x; col < D; col += 256) dst[col] = ((lds[0][col] + lds[1][col]) + lds[2][col]) + lds[3][col];
}

// the slab partials of a pass onto the call's running total: out[m][d] (the caller's w_colsum) is overwritten by the first pass of a
// call (first != 0) and carried by the later ones.  A workgroup takes 16 of the 2 D (modality, column) sums; thread (seg, jj) adds the
// slabs of its sixteenth of the index range in ascending order, thread (0, jj) then adds the 16 segment sums in ascending order -- an
// order fixed by nslabs alone (a 256-slab pass would otherwise be one chain of 256 dependent adds per thread on six workgroups).
#define COLSUM_SEGS 16
__global__ __launch_bounds__(256) void iefvad_colsum_finish_kernel(const double* part, int nslabs, int twoD, int first, double* out) {
    __shared__ double seg_sum[COLSUM_SEGS][16];
    const int seg = threadIdx.x >> 4, jj = threadIdx.x & 15;
    const int i = blockIdx.x * 16 + jj;                // m * D + d; twoD is a multiple of 16
    const int len = (nslabs + COLSUM_SEGS - 1) / COLSUM_SEGS;
    const int k1 = (seg + 1) * len < nslabs ? (seg + 1) * len : nslabs;
    double s = 0.0;
    for (int k = seg * len; k < k1; ++k) s += part[(size_t)k * twoD + i];
    seg_sum[seg][jj] = s;
    __syncthreads();
    if (seg != 0) return;
    double t = first ? 0.0 : out[i];
    for (int g = 0; g < COLSUM_SEGS; ++g) t += seg_sum[g][jj];
    out[i] = t;
}

// ---- the read-out rows of an online pass (iefvad_forward_videos_online, csrc/window_plan.h) behind the last LayerNorm: of window c,
// rows enc_row + skip .. + count of the encoder's row set -> rows dst .. of the pass's packed read-out order (OnlineRead), so that the
// row-wise tail runs on the rows that are read and on nothing else.  It takes the role iefvad_compact_rows_kernel has in the
// dense-encoder mode.  T = float (the f32 and bf16x6 arithmetics' rows) or __bf16 (the bf16 arithmetic's operand copy); the copy is
// of bits, in 16-byte lanes: a row is NV = D sizeof(T) / 16 of them, lane l owns l, l + 64, ...  gridDim.z workgroups per (window,
// modality), 16-row groups dealt round-robin, one wavefront per row, four rows of the wave in flight, as in
// iefvad_rows_out_wide_kernel; no LDS, no atomics.  Rows outside [skip, skip + count) are never read.
template <typename T>
struct ReadoutArgs {
    const T* src[2];        // the encoder's row set of the last layer, per modality
    T* dst[2];
    const RaggedChunk* chunks;
    const OnlineRead* reads;
};
template <typename T, int D>
__global__ __launch_bounds__(256) void iefvad_readout_rows_kernel(ReadoutArgs<T> a) {
    constexpr int NV = D * (int)sizeof(T) / 16, NJ = (NV + 63) / 64;
    static_assert(D * sizeof(T) % 16 == 0, "rows are whole 16-byte lanes");
    const RaggedChunk c = a.chunks[blockIdx.x];
    const OnlineRead rd = a.reads[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const f32x4* src = (const f32x4*)(a.src[blockIdx.y] + ((size_t)c.enc_row + rd.skip) * D) + lane;
    f32x4* dst = (f32x4*)(a.dst[blockIdx.y] + (size_t)rd.dst * D) + lane;
    const int nr = rd.count;
    for (int r0 = wave + 16 * blockIdx.z; r0 < nr; r0 += 16 * gridDim.z) {
        f32x4 v[4][NJ];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r0 + 4 * u;
            if (r < nr) {
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    if (lane + 64 * j < NV) v[u][j] = src[(size_t)r * NV + 64 * j];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r0 + 4 * u;
            if (r >= nr) break;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (lane + 64 * j < NV) dst[(size_t)r * NV + 64 * j] = v[u][j];
        }
    }
}

// iefvad_auc_ap: the metric tail of the evaluation loop on the device.
//
// The reference ends test() with sklearn on the host (/root/reference/test.py:158-159):
//     ROC1 = roc_auc_score(gt, np.repeat(ap1, 16));  AP1 = average_precision_score(gt, np.repeat(ap1, 16))
// -- a sort of 16 x n points (33.5 M at BASELINE config 4) for numbers that depend on n snippet scores and, per snippet, on HOW
// MANY of its 16 frames are anomalous.  Here: one LSD radix sort of n (score key, positives-of-the-snippet) pairs, one scan, one
// reduction over the tie groups; the x16 repeat is never materialised.
//
//   thresholds = the DISTINCT score values, in decreasing order (sklearn: _binary_clf_curve); a snippet contributes its `repeat`
//   frames at one threshold.  With, per tie group g, P_g / N_g positive / negative frames, tp_g / fp_g the cumulative counts up
//   to and including g, P / N the totals:
//       AUC = sum_g P_g (2 (N - fp_g) + N_g) / (2 P N)        (trapezoids of the ROC curve = Mann-Whitney with ties at 1/2)
//       AP  = sum_g (P_g / P) tp_g / (tp_g + fp_g)            (sklearn: -sum(diff(recall) * precision[:-1]))
//   The AUC numerator is an INTEGER (at most (n repeat)^2 / 2 < 2^63 for n repeat < 2^32 frames): it is accumulated exactly in 64-bit
//   integers, so the result does not depend on any summation order; AP terms are doubles reduced in a fixed order (per-block partials, one
//   final block).  Deterministic, no floating-point atomics.
//
// Kernels are HBM-bound integer / byte work on 8-byte pairs: coalesced tile loads, LDS histograms, wave-level ballots for the
// stable in-tile ranks (wave64: one 64-bit ballot per digit bit); nothing here is reshaped into a GEMM.
//
// iefvad_auc_ap_grouped: the same numbers for up to 64 disjoint groups of snippets in ONE pass over the data (the per-class loops of
// test.py:165-174 and the Ano-AUC of test.py:161).  The group byte travels in the pair's payload word above the positives count
// (key << 32 | group << 24 | positives, hence repeat < 2^24) and is the FIFTH radix digit, so the pairs end up ordered by (group, key);
// snippets of no group sort behind the last group.  Tie groups are runs of equal (key, group) -- the upper 40 bits -- so none spans two
// groups; the inclusive positives stay ONE global scan, a 65-entry table of per-group bases (first sorted index, positives before it)
// turns them into per-group counts.  A tile of sorted pairs holds a contiguous range of groups: it leaves one AP partial per group
// it touches, and one final block per group adds that group's partials in a fixed order.
#pragma once
#include "common.h"

#define MT_THREADS 256
#define MT_ITEMS 16
#define MT_TILE (MT_THREADS * MT_ITEMS)      // 4096 pairs per workgroup
#define MT_WAVES (MT_THREADS / 64)
#define MT_RADIX 256
#define MT_MAXG 64                            // groups per grouped call; digit MT_MAXG at most = "no group"
#define MT_POS_BITS 24                        // grouped pairs: positives in the low 24 bits, the group byte above them
#define MT_POS_MASK 0xFFFFFFu

struct MetricGroupTab {            // grouped call: per group (entry ngroups = the snippets of no group), in sorted order
    unsigned beg[MT_MAXG + 1];     // index of the group's first pair
    unsigned cnt[MT_MAXG + 1];     // its pairs
    unsigned tpb[MT_MAXG + 1];     // positive frames in front of it
    unsigned pos[MT_MAXG + 1];     // its positive frames
};

struct MetricWs {                  // carved out of the caller's workspace by metric_layout()
    unsigned long long* a;         // [n] pairs: key << 32 | positives
    unsigned long long* b;         // [n] the sort's other buffer; afterwards tp_incl (u32 [n]) | gstart (u32 [n])
    unsigned* hist;                // [MT_RADIX * tiles]
    unsigned* bsum;                // [tiles] positives per tile
    unsigned* bstart;              // [tiles] largest group-start index inside the tile (0 if none)
    double* ap_part;               // [tiles]
    unsigned long long* auc_num;   // [1] exact numerator
    unsigned* flags;               // [1] bit 0: a NaN score was seen
    unsigned* dtotal;              // [MT_RADIX] pairs per digit of the current sort pass
    MetricGroupTab* tab;           // grouped call only; there ap_part is [ngroups][tiles], auc_num [MT_MAXG] and flags a 64-bit NaN mask
};

// descending order of the scores = ascending order of the keys.  -0.0 is folded into +0.0 (equal as numbers, so one threshold).
__device__ __forceinline__ unsigned metric_key(float s) {
    unsigned u = __float_as_uint(s);
    if ((u << 1) == 0) u = 0;
    const unsigned asc = u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    return ~asc;
}

// positive frames of snippet i: any non-zero byte counts (gt is 0 / 1 in every list the reference ships)
__device__ __forceinline__ unsigned metric_positives(const unsigned char* gt, long long i, int repeat) {
    unsigned pos = 0;
    const unsigned char* g = gt + i * repeat;
    if (repeat == 16 && (((uintptr_t)gt) & 15) == 0) {          // the reference's 16 frames per snippet: one 16-byte load
        const uint4 v = *(const uint4*)g;
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int b = 0; b < 4; ++b) pos += ((w[k] >> (8 * b)) & 0xFFu) != 0;
    } else {
        for (int k = 0; k < repeat; ++k) pos += g[k] != 0;
    }
    return pos;
}

// pairs from scores + frame-level ground truth (the sort kernels take n and mask the tail of the last tile themselves: nothing is padded)
__global__ __launch_bounds__(MT_THREADS) void iefvad_metric_pairs_kernel(const float* scores, const unsigned char* gt, long long n, int repeat,
                                                                        unsigned long long* out, unsigned* flags) {
    const long long i = (long long)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= n) return;
    const float s = scores[i];
    const unsigned pos = metric_positives(gt, i, repeat);
    if (s != s) atomicOr(flags, 1u);
    out[i] = ((unsigned long long)metric_key(s) << 32) | pos;
}

// grouped: the group byte above the positives; every byte outside [0, ngroups) becomes digit `ngroups` (no group).  A NaN score marks
// its own group only.
__global__ __launch_bounds__(MT_THREADS) void iefvad_metric_pairs_grouped_kernel(const float* scores, const unsigned char* gt, const unsigned char* group,
                                                                                long long n, int repeat, int ngroups, unsigned long long* out,
                                                                                unsigned long long* nanmask) {
    const long long i = (long long)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= n) return;
    const float s = scores[i];
    const unsigned pos = metric_positives(gt, i, repeat);
    const unsigned g = min((unsigned)group[i], (unsigned)ngroups);
    if (s != s && g < (unsigned)ngroups) atomicOr(nanmask, 1ull << g);
    out[i] = ((unsigned long long)metric_key(s) << 32) | (g << MT_POS_BITS) | pos;
}

// ---- LSD radix sort on the key half, 8 bits per pass ---------------------------------------------------------------------------
// element order inside a tile: wave w owns items [w * 1024, (w + 1) * 1024) of the tile, round r of the wave is 64 consecutive items
__device__ __forceinline__ long long mt_index(long long tile0, int wave, int round, int lane) {
    return tile0 + (long long)wave * (MT_ITEMS * 64) + round * 64 + lane;
}

__global__ __launch_bounds__(MT_THREADS) void iefvad_metric_hist_kernel(const unsigned long long* in, long long n, int shift, unsigned* hist, int tiles) {
    __shared__ unsigned h[MT_RADIX];
    h[threadIdx.x] = 0;
    __syncthreads();
    const long long tile0 = (long long)blockIdx.x * MT_TILE;
#pragma unroll
    for (int it = 0; it < MT_ITEMS; ++it) {
        const long long i = tile0 + it * MT_THREADS + threadIdx.x;
        if (i < n) atomicAdd(&h[(unsigned)(in[i] >> shift) & 0xFFu], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];      // digit-major: a digit's tile counts are one contiguous row
}

// The digit-major table [256 digits][tiles] becomes output bases in two levels: one workgroup per DIGIT scans its row of tile counts
// in place (exclusive) and leaves the digit's total; the scatter kernel turns the 256 totals into digit bases itself (a 256-entry scan
// in LDS per workgroup).  (The first build scanned the whole 131 k-word table with ONE workgroup: 72 us per pass, half of the call.)
__global__ __launch_bounds__(256) void iefvad_metric_digit_scan_kernel(unsigned* hist, int tiles, unsigned* dtotal) {
    __shared__ unsigned wsum[4];
    __shared__ unsigned carry_s;
    unsigned* row = hist + (size_t)blockIdx.x * tiles;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < tiles; base += 1024) {
        const int i0 = base + 4 * threadIdx.x;
        unsigned v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (i0 + k < tiles) ? row[i0 + k] : 0u;
        const unsigned mine = v[0] + v[1] + v[2] + v[3];
        unsigned inc = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        unsigned wbase = carry_s;
        for (int w = 0; w < wave; ++w) wbase += wsum[w];
        unsigned run = wbase + inc - mine;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < tiles) row[i0 + k] = run;
            run += v[k];
        }
        __syncthreads();
        if (threadIdx.x == 255) carry_s = run;
        __syncthreads();
    }
    if (threadIdx.x == 0) dtotal[blockIdx.x] = carry_s;
}

__global__ __launch_bounds__(MT_THREADS) void iefvad_metric_scatter_kernel(const unsigned long long* in, unsigned long long* out, long long n, int shift,
                                                                          const unsigned* hist, int tiles, const unsigned* dtotal) {
    __shared__ unsigned wcount[MT_WAVES][MT_RADIX];        // per wave: first its digit counts, then its running output offsets
    __shared__ unsigned dwave[MT_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long tile0 = (long long)blockIdx.x * MT_TILE;
#pragma unroll
    for (int w = 0; w < MT_WAVES; ++w) wcount[w][threadIdx.x] = 0;
    __syncthreads();
    unsigned long long e[MT_ITEMS];
#pragma unroll
    for (int r = 0; r < MT_ITEMS; ++r) {
        const long long i = mt_index(tile0, wave, r, lane);
        e[r] = (i < n) ? in[i] : 0ull;
        if (i < n) atomicAdd(&wcount[wave][(unsigned)(e[r] >> shift) & 0xFFu], 1u);
    }
    __syncthreads();
    // digit bases: exclusive scan of the 256 digit totals (thread d = digit d)
    const unsigned dt = dtotal[threadIdx.x];
    unsigned dinc = dt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(dinc, d);
        if (lane >= d) dinc += o;
    }
    if (lane == 63) dwave[wave] = dinc;
    __syncthreads();
    unsigned dbase = dinc - dt;
    for (int w = 0; w < wave; ++w) dbase += dwave[w];
    {   // thread d: global base of digit d for this tile, then one running offset per wave (waves in order: stable)
        unsigned run = dbase + hist[(size_t)threadIdx.x * tiles + blockIdx.x];
#pragma unroll
        for (int w = 0; w < MT_WAVES; ++w) {
            const unsigned c = wcount[w][threadIdx.x];
            wcount[w][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
    volatile unsigned* off = wcount[wave];
    const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < MT_ITEMS; ++r) {
        const long long i = mt_index(tile0, wave, r, lane);
        const bool valid = i < n;
        const unsigned d = (unsigned)(e[r] >> shift) & 0xFFu;
        unsigned long long peers = __ballot(valid);        // lanes of this round holding the same digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long m = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        unsigned base = 0;
        const int leader = peers ? __ffsll((long long)peers) - 1 : 0;
        if (valid && lane == leader) {
            base = off[d];
            off[d] = base + (unsigned)__popcll(peers);
        }
        base = __shfl(base, leader);
        if (valid) out[(size_t)base + (unsigned)__popcll(peers & lt)] = e[r];
    }
}

// ---- behind the sort: inclusive positives and, per element, the first index of its tie group -------------------------------------
// what two pairs of one tie group share, and a pair's positives: the key / the whole payload, or, in the grouped format, key and group
// byte / the payload's low 24 bits
template <bool GROUPED> __device__ __forceinline__ unsigned long long mt_tie(unsigned long long p) { return GROUPED ? p >> MT_POS_BITS : p >> 32; }
template <bool GROUPED> __device__ __forceinline__ unsigned mt_pos(unsigned long long p) { return GROUPED ? (unsigned)p & MT_POS_MASK : (unsigned)p; }

template <bool GROUPED>
__global__ __launch_bounds__(MT_THREADS) void iefvad_metric_tile_sums_kernel(const unsigned long long* sorted, long long n, unsigned* bsum, unsigned* bstart) {
    __shared__ unsigned s_sum[MT_WAVES], s_start[MT_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i0 = (long long)blockIdx.x * MT_TILE + (long long)threadIdx.x * MT_ITEMS;
    unsigned sum = 0, start = 0;
    unsigned long long prev_key = (i0 > 0 && i0 - 1 < n) ? mt_tie<GROUPED>(sorted[i0 - 1]) : 0ull;
#pragma unroll
    for (int k = 0; k < MT_ITEMS; ++k) {
        const long long i = i0 + k;
        if (i < n) {
            const unsigned long long p = sorted[i];
            sum += mt_pos<GROUPED>(p);
            const unsigned long long key = mt_tie<GROUPED>(p);
            if (i == 0 || key != prev_key) start = (unsigned)i;
            prev_key = key;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sum += __shfl_xor(sum, d);
        start = max(start, (unsigned)__shfl_xor((int)start, d));
    }
    if (lane == 0) { s_sum[wave] = sum; s_start[wave] = start; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned a = 0, b = 0;
        for (int w = 0; w < MT_WAVES; ++w) { a += s_sum[w]; b = max(b, s_start[w]); }
        bsum[blockIdx.x] = a;
        bstart[blockIdx.x] = b;
    }
}

// one workgroup: bsum -> exclusive sums, bstart -> exclusive running maxima (a group start index grows with the tile, so "max" = "last")
__global__ __launch_bounds__(1024) void iefvad_metric_tile_scan_kernel(unsigned* bsum, unsigned* bstart, int tiles) {
    __shared__ unsigned ws[16], wm[16];
    __shared__ unsigned carry_sum, carry_max;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) { carry_sum = 0; carry_max = 0; }
    __syncthreads();
    for (int base = 0; base < tiles; base += 1024) {
        const int i = base + threadIdx.x;
        const unsigned v = i < tiles ? bsum[i] : 0u, m = i < tiles ? bstart[i] : 0u;
        unsigned inc = v, mx = m;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = __shfl_up(inc, d), om = __shfl_up(mx, d);
            if (lane >= d) { inc += o; mx = max(mx, om); }
        }
        if (lane == 63) { ws[wave] = inc; wm[wave] = mx; }
        __syncthreads();
        unsigned bs = carry_sum, bm = carry_max;
        for (int w = 0; w < wave; ++w) { bs += ws[w]; bm = max(bm, wm[w]); }
        const unsigned up = (unsigned)__shfl_up(mx, 1);          // every lane takes part in the shuffle
        if (i < tiles) { bsum[i] = bs + inc - v; bstart[i] = lane ? max(bm, up) : bm; }
        __syncthreads();
        if (threadIdx.x == 1023) { carry_sum = bs + inc; carry_max = max(bm, mx); }
        __syncthreads();
    }
}

template <bool GROUPED>
__global__ __launch_bounds__(MT_THREADS) void iefvad_metric_tile_apply_kernel(const unsigned long long* sorted, long long n, const unsigned* bsum,
                                                                             const unsigned* bstart, unsigned* tp_incl, unsigned* gstart) {
    __shared__ unsigned s_sum[MT_WAVES], s_start[MT_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i0 = (long long)blockIdx.x * MT_TILE + (long long)threadIdx.x * MT_ITEMS;
    unsigned pos[MT_ITEMS], st[MT_ITEMS];
    unsigned sum = 0, start = 0;
    unsigned long long prev_key = (i0 > 0 && i0 - 1 < n) ? mt_tie<GROUPED>(sorted[i0 - 1]) : 0ull;
#pragma unroll
    for (int k = 0; k < MT_ITEMS; ++k) {
        const long long i = i0 + k;
        pos[k] = 0; st[k] = 0;
        if (i < n) {
            const unsigned long long p = sorted[i];
            const unsigned long long key = mt_tie<GROUPED>(p);
            if (i == 0 || key != prev_key) start = (unsigned)i;
            prev_key = key;
            sum += mt_pos<GROUPED>(p);
            pos[k] = sum;          // inclusive within the thread
            st[k] = start;         // running maximum within the thread (0 = "none yet in this thread")
        }
    }
    unsigned inc = sum, mx = start;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d), om = __shfl_up(mx, d);
        if (lane >= d) { inc += o; mx = max(mx, om); }
    }
    if (lane == 63) { s_sum[wave] = inc; s_start[wave] = mx; }
    __syncthreads();
    unsigned bs = bsum[blockIdx.x], bm = bstart[blockIdx.x];
    for (int w = 0; w < wave; ++w) { bs += s_sum[w]; bm = max(bm, s_start[w]); }
    const unsigned up = (unsigned)__shfl_up(mx, 1);
    const unsigned excl_sum = bs + inc - sum, excl_max = lane ? max(bm, up) : bm;
#pragma unroll
    for (int k = 0; k < MT_ITEMS; ++k) {
        const long long i = i0 + k;
        if (i < n) {
            tp_incl[i] = excl_sum + pos[k];
            gstart[i] = max(excl_max, st[k]);
        }
    }
}

// every LAST element of a tie group adds its group's terms
__global__ __launch_bounds__(MT_THREADS) void iefvad_metric_groups_kernel(const unsigned long long* sorted, long long n, int repeat, const unsigned* tp_incl,
                                                                         const unsigned* gstart, unsigned long long* auc_num, double* ap_part) {
    __shared__ double s_ap[MT_WAVES];
    __shared__ unsigned long long s_auc[MT_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long P = tp_incl[n - 1];
    const unsigned long long N = (unsigned long long)n * repeat - P;
    unsigned long long auc = 0;
    double ap = 0.0;
    const long long tile0 = (long long)blockIdx.x * MT_TILE;
#pragma unroll 4
    for (int it = 0; it < MT_ITEMS; ++it) {
        const long long i = tile0 + it * MT_THREADS + threadIdx.x;
        if (i >= n) continue;
        const unsigned key = (unsigned)(sorted[i] >> 32);
        if (i + 1 < n && (unsigned)(sorted[i + 1] >> 32) == key) continue;        // not the end of its group
        const unsigned long long s = gstart[i];
        const unsigned long long tp = tp_incl[i], tp_prev = s ? tp_incl[s - 1] : 0ull;
        const unsigned long long Pg = tp - tp_prev;
        const unsigned long long Ng = (unsigned long long)repeat * (unsigned long long)(i - (long long)s + 1) - Pg;
        const unsigned long long seen = (unsigned long long)repeat * (unsigned long long)(i + 1);      // tp + fp
        const unsigned long long fp = seen - tp;
        auc += Pg * (2ull * (N - fp) + Ng);
        if (Pg) ap += (double)Pg * ((double)tp / (double)seen);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        auc += __shfl_xor(auc, d);
        ap += __shfl_xor(ap, d);
    }
    if (lane == 0) { s_auc[wave] = auc; s_ap[wave] = ap; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long a = 0;
        double p = 0.0;
        for (int w = 0; w < MT_WAVES; ++w) { a += s_auc[w]; p += s_ap[w]; }
        if (a) atomicAdd(auc_num, a);          // integers: exact in any order
        ap_part[blockIdx.x] = p;
    }
}

__global__ __launch_bounds__(256) void iefvad_metric_finish_kernel(const unsigned* tp_incl, long long n, int repeat, const unsigned long long* auc_num,
                                                                  const double* ap_part, int tiles, const unsigned* flags, double* auc, double* ap) {
    __shared__ double s[256];
    double p = 0.0;
    for (int i = threadIdx.x; i < tiles; i += 256) p += ap_part[i];          // fixed assignment, fixed tree below
    s[threadIdx.x] = p;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double P = (double)tp_incl[n - 1];
        const double N = (double)n * repeat - P;
        const double nan = __builtin_nan("");
        const bool bad = (*flags & 1u) != 0;
        // one class only: sklearn's roc_auc_score raises; here NaN.  No positive frame: average_precision_score gives 0.
        if (auc) *auc = (bad || P == 0.0 || N == 0.0) ? nan : (double)*auc_num / (2.0 * P * N);
        if (ap) *ap = bad ? nan : (P == 0.0 ? 0.0 : s[0] / P);
    }
}

// ---- grouped call: per-group bases, the reduction over tie groups per (tile, group), one final block per group --------------------
// The last sort pass leaves the pairs per group byte in dtotal; one small workgroup turns them and the global scan into the table.
__global__ __launch_bounds__(128) void iefvad_metric_group_table_kernel(const unsigned* dtotal, const unsigned* tp_incl, int ngroups, MetricGroupTab* tab) {
    __shared__ unsigned c[MT_MAXG + 1];
    const int g = threadIdx.x;
    if (g <= ngroups) c[g] = dtotal[g];
    __syncthreads();
    if (g > ngroups) return;
    unsigned beg = 0;
    for (int j = 0; j < g; ++j) beg += c[j];
    const unsigned end = beg + c[g];
    const unsigned tpb = beg ? tp_incl[beg - 1] : 0u;
    tab->beg[g] = beg;
    tab->cnt[g] = c[g];
    tab->tpb[g] = tpb;
    tab->pos[g] = (end ? tp_incl[end - 1] : 0u) - tpb;
}

// every LAST element of a tie group forms its terms with its group's counts.  A tile holds the groups [first pair's, last pair's]; the
// workgroup walks the tile once per group in it (tiles + ngroups walks in all, whatever the sizes) and reduces in a fixed order: items
// of a thread in order, xor tree, waves in order
__global__ __launch_bounds__(MT_THREADS) void iefvad_metric_groups_grouped_kernel(const unsigned long long* sorted, long long n, int repeat, int ngroups,
                                                                                 const unsigned* tp_incl, const unsigned* gstart, const MetricGroupTab* tab,
                                                                                 unsigned long long* auc_num, double* ap_part, int tiles) {
    __shared__ double s_ap[MT_WAVES];
    __shared__ unsigned long long s_auc[MT_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long tile0 = (long long)blockIdx.x * MT_TILE;
    const long long last = (tile0 + MT_TILE <= n ? tile0 + MT_TILE : n) - 1;
    const int g_lo = (int)((sorted[tile0] >> MT_POS_BITS) & 0xFFu);
    const int g_hi = min((int)((sorted[last] >> MT_POS_BITS) & 0xFFu), ngroups - 1);          // behind it: the snippets of no group
    for (int g = g_lo; g <= g_hi; ++g) {
        const unsigned long long beg = tab->beg[g], cnt = tab->cnt[g], tpb = tab->tpb[g];
        if (cnt == 0) continue;                                                              // nobody reads an empty group's partials
        const unsigned long long N = (unsigned long long)repeat * cnt - tab->pos[g];
        unsigned long long auc = 0;
        double ap = 0.0;
#pragma unroll 4
        for (int it = 0; it < MT_ITEMS; ++it) {
            const long long i = tile0 + it * MT_THREADS + threadIdx.x;
            if (i < (long long)beg || i >= (long long)(beg + cnt)) continue;                  // another group's pair, or behind the end
            const unsigned long long tie = sorted[i] >> MT_POS_BITS;
            if (i + 1 < n && (sorted[i + 1] >> MT_POS_BITS) == tie) continue;                // not the end of its tie group
            const unsigned long long s = gstart[i];                                          // >= beg: the group byte is part of `tie`
            const unsigned long long tp = tp_incl[i] - tpb, tp_prev = s > beg ? tp_incl[s - 1] - tpb : 0ull;
            const unsigned long long Pg = tp - tp_prev;
            const unsigned long long Ng = (unsigned long long)repeat * (unsigned long long)(i - (long long)s + 1) - Pg;
            const unsigned long long seen = (unsigned long long)repeat * ((unsigned long long)i - beg + 1);      // tp + fp inside the group
            const unsigned long long fp = seen - tp;
            auc += Pg * (2ull * (N - fp) + Ng);
            if (Pg) ap += (double)Pg * ((double)tp / (double)seen);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            auc += __shfl_xor(auc, d);
            ap += __shfl_xor(ap, d);
        }
        if (lane == 0) { s_auc[wave] = auc; s_ap[wave] = ap; }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long a = 0;
            double p = 0.0;
            for (int w = 0; w < MT_WAVES; ++w) { a += s_auc[w]; p += s_ap[w]; }
            if (a) atomicAdd(&auc_num[g], a);          // integers: exact in any order
            ap_part[(size_t)g * tiles + blockIdx.x] = p;
        }
        __syncthreads();
    }
}

// workgroup g: group g's results.  Its AP partials are those of the tiles its pairs lie in -- each of them wrote slot (g, tile).
__global__ __launch_bounds__(256) void iefvad_metric_finish_grouped_kernel(const MetricGroupTab* tab, int repeat, const unsigned long long* auc_num,
                                                                          const double* ap_part, int tiles, const unsigned long long* nanmask, double* auc,
                                                                          double* ap, long long* frames) {
    __shared__ double s[256];
    const int g = blockIdx.x;
    const unsigned beg = tab->beg[g], cnt = tab->cnt[g];
    double p = 0.0;
    if (cnt) {
        const int t0 = (int)(beg / MT_TILE), t1 = (int)((beg + (cnt - 1)) / MT_TILE);
        for (int i = t0 + threadIdx.x; i <= t1; i += 256) p += ap_part[(size_t)g * tiles + i];          // fixed assignment, fixed tree below
    }
    s[threadIdx.x] = p;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double P = (double)tab->pos[g];
        const double N = (double)cnt * repeat - P;
        const double nan = __builtin_nan("");
        const bool bad = cnt == 0 || ((*nanmask >> g) & 1ull) != 0;          // an empty group has no curve at all
        if (auc) auc[g] = (bad || P == 0.0 || N == 0.0) ? nan : (double)auc_num[g] / (2.0 * P * N);
        if (ap) ap[g] = bad ? nan : (P == 0.0 ? 0.0 : s[0] / P);
        if (frames) { frames[2 * g] = (long long)cnt * repeat; frames[2 * g + 1] = (long long)tab->pos[g]; }
    }
}

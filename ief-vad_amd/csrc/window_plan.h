// The trailing windows of an online call (iefvad_forward_videos_online, include/iefvad.h) and the cut of the call into passes.
// Host-only C++17 -- no HIP, no pointers into the device, no handle -- so that tests/online_plan.cpp (g++, no GPU) pins it against
// harness.online_windows (tests/test_online_cpu.py).  csrc/online.h fills its tables from here.
//
// A video of n snippets has windows j = 1 .. ceil(n / stride):
//   end_j = min(j stride, n)      start_j = max(0, end_j - history)      read0_j = (j - 1) stride
// Window j is the 256-row chunk of rows [start_j, end_j) and zero rows behind them; its results are read for snippets [read0_j, end_j)
// only, rows read0_j - start_j .. of the window.  Every snippet is read from exactly one window, and read0_j >= start_j because
// stride <= history.  The score of a snippet depends on no snippet at or beyond its window's end: the look-ahead is below `stride`.
#pragma once
#include <stdint.h>

static const int kWindowRows = 256;   // IEF_T

static inline bool online_params_ok(long long stride, long long history) { return 1 <= stride && stride <= history && history <= kWindowRows; }
static inline int online_video_windows(int n, int stride) { return (n + stride - 1) / stride; }

// window j (1-based) of a video of n snippets, in rows of the video
struct OnlineWindow { long long start, end, read0; int video; };
static inline OnlineWindow online_window(int n, int stride, int history, int j) {
    OnlineWindow w;
    w.end = (long long)j * stride < n ? (long long)j * stride : n;
    w.start = w.end - history > 0 ? w.end - history : 0;
    w.read0 = (long long)(j - 1) * stride;
    w.video = 0;
    return w;
}

// windows of a whole call; -1 if a length is not positive
static inline long long online_call_windows(const int32_t* lengths, int nvideos, int stride) {
    long long total = 0;
    for (int v = 0; v < nvideos; ++v) {
        if (lengths[v] <= 0) return -1;
        total += online_video_windows(lengths[v], stride);
    }
    return total;
}

// the call's windows in list order, in PACKED rows of the call (the videos' rows concatenated); `w` holds online_call_windows entries
static inline void online_fill_windows(const int32_t* lengths, int nvideos, int stride, int history, OnlineWindow* w) {
    long long base = 0, i = 0;
    for (int v = 0; v < nvideos; ++v) {
        const int n = lengths[v], nw = online_video_windows(n, stride);
        for (int j = 1; j <= nw; ++j, ++i) {
            w[i] = online_window(n, stride, history, j);
            w[i].start += base; w[i].end += base; w[i].read0 += base;
            w[i].video = v;
        }
        base += n;
    }
}

// A pass is a run of at most micro_batch windows.  It reads packed rows from src_base on (its first window's start: starts never
// decrease within a call) and writes the results of packed rows [out_base, out_base + out_rows): its first window's read0 up to its
// last window's end, contiguous because every snippet is read exactly once, in order.
struct OnlinePass { long long first; int count; long long src_base, out_base; int out_rows; };
static inline OnlinePass online_pass(const OnlineWindow* w, long long total, int micro_batch, long long first) {
    OnlinePass p;
    p.first = first;
    p.count = (int)(total - first < micro_batch ? total - first : micro_batch);
    p.src_base = w[first].start;
    p.out_base = w[first].read0;
    p.out_rows = (int)(w[first + p.count - 1].end - p.out_base);
    return p;
}

// What the read-out gather needs of a window beside its RaggedChunk (common.h): it copies rows enc_row + skip .. + count of the
// encoder's row set to rows dst .. of the pass's packed read-out order.
struct OnlineRead { int skip, count, dst; };
static inline OnlineRead online_read(const OnlineWindow& w, const OnlinePass& p) {
    return OnlineRead{(int)(w.read0 - w.start), (int)(w.end - w.read0), (int)(w.read0 - p.out_base)};
}

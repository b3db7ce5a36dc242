// What lies behind the base workspace of a forward call, and where.  Host-only C++17 -- no HIP, no pointers, no handle -- so that
// tests/cabi/workspace_tail.cpp (g++, no GPU) pins every offset (tests/test_workspace_tail_cpu.py).  Every public *_workspace_bytes
// query and both route implementations (forward_impl in iefvad.hip, forward_videos_impl in videos.h) take sizes and places from here.
//
// The regions, in this order, each present only if asked for; nb = chunks of a pass, R = nb * 256 rows, V = the variants count:
//   w_rows   [2, R, D] floats     the fusion weights of the pass's row set, stored for w_colsum or a wide w_i / w_e: no region of the
//                                 base workspace is dead in every arithmetic while the tail runs
//   colsum   [nb, 2, D] doubles   the slab partials of the column sums
//   z_prev   [R, D] floats        the second state buffer of a trajectory pass (trajectory.h)
//   var      variants_bytes(V)    the stacked states of the fusion ablations (variants.h)
//   smp      variants_bytes(4)    one group of stacked sample states, whatever the sample count (samples.h)
#pragma once
#include <stddef.h>

static const size_t kTailChunkRows = 256;   // IEF_T
static const int kTailSampleGroup = 4;      // IEF_MAX_VARIANTS: the samples run in groups of this many stacked states

// `count` stacked states of a pass: the state [count, R, D], its h scratch of the same size and the [count, R] logits
static inline size_t variants_bytes(size_t pass_chunks, int D, int count) {
    return (size_t)count * pass_chunks * kTailChunkRows * (2 * (size_t)D + 1) * sizeof(float);
}

struct TailWants {
    bool w_rows;      // the fusion stage stores its weights
    bool colsum;      // the column sums of those weights (they need the w_rows region too)
    bool traj;
    int variants;     // 0: none
    bool samples;
};

// byte offsets from the start of the workspace (meaningful only for a region that is asked for) and the size of the whole
struct WorkspaceTail {
    size_t w_rows, colsum, z_prev, var, smp, total;
};

static inline WorkspaceTail workspace_tail(size_t base, size_t pass_chunks, int D, const TailWants& w) {
    const size_t RD = pass_chunks * kTailChunkRows * (size_t)D;
    WorkspaceTail t;
    size_t at = base;
    t.w_rows = at; at += (w.w_rows || w.colsum) ? 2 * RD * sizeof(float) : 0;
    t.colsum = at; at += w.colsum ? pass_chunks * 2 * (size_t)D * sizeof(double) : 0;
    t.z_prev = at; at += w.traj ? RD * sizeof(float) : 0;
    t.var = at;    at += w.variants ? variants_bytes(pass_chunks, D, w.variants) : 0;
    t.smp = at;    at += w.samples ? variants_bytes(pass_chunks, D, kTailSampleGroup) : 0;
    t.total = at;
    return t;
}

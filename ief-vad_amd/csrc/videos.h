// Whole videos: valid rows in, per-snippet results out (include/iefvad.h, csrc/ragged.h).  Included by iefvad.hip behind forward_pass.
//
// The seven entries of this route (iefvad_forward_videos, _scaled, _similarity, _full here; the three host-list entries in
// hostpipe.h) each fill one VideosOut -- where the call's results go (iefvad.hip) -- and call forward_videos_impl, which cuts the list
// into micro-batch passes and hands pass k the view `out.at(first packed row of pass k)`.
#pragma once

// chunk count of a video as the evaluation loop needs it: process_split's len // 256 + 1 chunks (tools.py:105-112) minus the
// all-zero one of a len % 256 == 0 video, whose rows test.py:121 slices away
static int video_chunks(int n) { return n < IEF_T ? 1 : n / IEF_T + (n % IEF_T ? 1 : 0); }

// per-call metadata (chunk table, NaN flags) travels through a small ring of pinned host / device buffer pairs: the copy is
// asynchronous, so a slot is reused only after the event recorded behind its last use has completed
struct MetaRing {
    static const int kSlots = 4;
    void* host[kSlots] = {nullptr, nullptr, nullptr, nullptr};
    void* dev[kSlots] = {nullptr, nullptr, nullptr, nullptr};
    size_t cap[kSlots] = {0, 0, 0, 0};
    hipEvent_t done[kSlots] = {nullptr, nullptr, nullptr, nullptr};
    int turn = 0;
};

static void release_meta(iefvad_handle* h) {
    if (!h->meta) return;
    for (int i = 0; i < MetaRing::kSlots; ++i) {
        if (h->meta->host[i]) (void)hipHostFree(h->meta->host[i]);
        if (h->meta->dev[i]) (void)hipFree(h->meta->dev[i]);
        if (h->meta->done[i]) (void)hipEventDestroy(h->meta->done[i]);
    }
    delete h->meta;
    h->meta = nullptr;
}

// The ring's next slot, idle and with room for `bytes`: waits for the event behind the slot's last use, grows its buffer pair
static int meta_slot(iefvad_handle* h, size_t bytes, const char* who, int* slot_out) {
    if (!h->meta) {
        h->meta = new (std::nothrow) MetaRing();
        if (!h->meta) return fail("%s: out of host memory", who);
    }
    MetaRing& mr = *h->meta;
    const int slot = *slot_out = mr.turn;
    mr.turn = (mr.turn + 1) % MetaRing::kSlots;
    HIP_TRY(hipSetDevice(h->device));
    if (mr.done[slot]) HIP_TRY(hipEventSynchronize(mr.done[slot]));
    else HIP_TRY(hipEventCreateWithFlags(&mr.done[slot], hipEventDisableTiming));
    if (mr.cap[slot] < bytes) {
        if (mr.host[slot]) (void)hipHostFree(mr.host[slot]);
        if (mr.dev[slot]) (void)hipFree(mr.dev[slot]);
        mr.host[slot] = mr.dev[slot] = nullptr;
        mr.cap[slot] = 0;
        const size_t cap = bytes * 2 + 4096;
        HIP_TRY(hipHostMalloc(&mr.host[slot], cap, hipHostMallocDefault));
        HIP_TRY(hipMalloc(&mr.dev[slot], cap));
        mr.cap[slot] = cap;
    }
    return 0;
}

static int videos_layout(const int32_t* lengths, int32_t nvideos, long long* total_rows, long long* total_chunks,
                         const char* who = "iefvad_forward_videos") {
    long long rows = 0, chunks = 0;
    for (int v = 0; v < nvideos; ++v) {
        if (lengths[v] <= 0) return fail("%s: lengths[%d] = %d", who, v, lengths[v]);
        rows += lengths[v];
        chunks += video_chunks(lengths[v]);
    }
    *total_rows = rows;
    *total_chunks = chunks;
    return 0;
}

// What lies behind the base workspace of a call of `chunks` chunks, sized for a pass of it (workspace_tail.h)
static size_t videos_pass_chunks(const iefvad_handle* h, long long chunks) { return (size_t)(chunks < micro_batch(h) ? chunks : micro_batch(h)); }
static WorkspaceTail videos_tail(const iefvad_handle* h, long long chunks, const TailWants& w) {
    return workspace_tail(iefvad_workspace_bytes(h, (int32_t)chunks), videos_pass_chunks(h, chunks), h->D, w);
}

// the public workspace queries: 0 for arguments no call would accept
static size_t videos_workspace_bytes(const iefvad_handle* h, const int32_t* lengths, int32_t nvideos, const TailWants& w) {
    if (!h || !lengths || nvideos <= 0) return 0;
    long long rows, chunks;
    if (videos_layout(lengths, nvideos, &rows, &chunks) || chunks > 0x7fffffffLL) return 0;
    return iefvad_workspace_bytes(h, (int32_t)chunks) ? videos_tail(h, chunks, w).total : 0;
}
extern "C" size_t iefvad_videos_workspace_bytes(const iefvad_handle* h, const int32_t* lengths, int32_t nvideos) {
    return videos_workspace_bytes(h, lengths, nvideos, TailWants{});
}
extern "C" size_t iefvad_videos_scaled_workspace_bytes(const iefvad_handle* h, const int32_t* lengths, int32_t nvideos, int32_t with_colsum) {
    TailWants w = {};
    w.colsum = with_colsum != 0;
    return videos_workspace_bytes(h, lengths, nvideos, w);
}
extern "C" size_t iefvad_videos_full_workspace_bytes(const iefvad_handle* h, const int32_t* lengths, int32_t nvideos, const iefvad_outputs* out) {
    TailWants w = {};
    w.w_rows = out && (out->w_i || out->w_e);
    return videos_workspace_bytes(h, lengths, nvideos, w);
}

// The checks of a whole-video call that look at neither the handle nor the rows; none makes a HIP call.  forward_videos_impl and
// forward_videos_host_impl make them behind their null-argument and weights checks; the similarity and full entries, which refuse
// these faults before they look at the handle, make them once more up front, behind their own null checks.
static int videos_args(const char* who, const VideosOut& out, int32_t in_dtype, int32_t nvideos) {
    if ((uintptr_t)out.similarity & 3) return fail("%s: similarity must be 4-byte aligned", who);
    for (int t = 0; t < ROWS_OUT_WIDE_MAX; ++t)
        if ((uintptr_t)out.wide[t] & 15) return fail("%s: the [rows, D] outputs must be 16-byte aligned", who);
    if (in_dtype != IEFVAD_IN_F32 && in_dtype != IEFVAD_IN_F16 && in_dtype != IEFVAD_IN_BF16) return fail("%s: unknown in_dtype %d", who, in_dtype);
    if (nvideos <= 0) return fail("%s: nvideos must be positive (got %d)", who, nvideos);
    if ((uintptr_t)out.w_colsum & 7) return fail("%s: w_colsum must be 8-byte aligned", who);
    if (((uintptr_t)out.x.scale[0] | (uintptr_t)out.x.scale[1]) & 3) return fail("%s: row scale vectors must be 4-byte aligned", who);
    if (((uintptr_t)out.x.noise.amp[0] | (uintptr_t)out.x.noise.amp[1] | (uintptr_t)out.x.noise.id) & 3)
        return fail("%s: noise amplitude and noise row vectors must be 4-byte aligned", who);
    return 0;
}

// the record every entry starts from: the three vectors and the entry's nan_to_num as given; the rest null
static VideosOut videos_out(float* logits, float* w_i_mean, float* w_e_mean, int32_t nan_to_num) {
    VideosOut out = {};
    out.logits = logits; out.w_i_mean = w_i_mean; out.w_e_mean = w_e_mean;
    out.nan_mode = nan_to_num;
    return out;
}
// the destinations of a full entry's `iefvad_outputs` (non-null, logits set: full_out is called behind full_nulls)
static VideosOut full_out(const iefvad_outputs& o, int32_t nan_to_num) {
    VideosOut out = videos_out(o.logits, o.w_i_mean, o.w_e_mean, nan_to_num);
    float* const wide[ROWS_OUT_WIDE_MAX] = {o.fused, o.image_mu, o.event_mu, o.image_logvar, o.event_logvar, o.w_i, o.w_e};
    for (int t = 0; t < ROWS_OUT_WIDE_MAX; ++t) out.wide[t] = wide[t];
    return out;
}
static int full_nulls(const char* who, const iefvad_handle* h, const iefvad_outputs* out) {
    if (!h) return fail("%s: null handle", who);
    if (!out) return fail("%s: null out", who);
    if (!out->logits) return fail("%s: null logits (out->logits is required)", who);
    return 0;
}

// `in`: the packed valid rows of the call's videos on the device; `out`: where the results go, at the call's first row
static int forward_videos_impl(iefvad_handle* h, const RowsIn& in, const int32_t* lengths, int32_t nvideos, void* workspace,
                               size_t workspace_bytes, const VideosOut& out, hipStream_t stream, Timer& tm, const char* who) {
    if (!h || !in.img || !in.ev || !lengths || !out.logits) return fail("%s: null argument", who);
    if (!h->weights_set) return fail("%s: weights not set", who);
    if (int rc = videos_args(who, out, in.in_dtype, nvideos)) return rc;
    int nan_mode = out.nan_mode;
    if (nan_mode < 0 || nan_mode > (out.sweep_codes ? 2 : 1)) {
        if (out.sweep_codes) return fail("%s: unknown nan_to_num %d (0: off, 1: per video with a NaN, 2: always)", who, nan_mode);
        nan_mode = 1;       // iefvad_forward_videos: any non-zero value is the per-video rule
    }
    long long total_rows, total_chunks;
    if (int rc = videos_layout(lengths, nvideos, &total_rows, &total_chunks, who)) return rc;
    if (total_chunks > 0x7fffffffLL / IEF_T) return fail("%s: too many chunks", who);
    const WorkspaceTail tail = videos_tail(h, total_chunks, out.wants());
    if (!workspace || workspace_bytes < tail.total) return fail("%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, tail.total);
    if (((uintptr_t)workspace & 15) || ((uintptr_t)in.img & 15) || ((uintptr_t)in.ev & 15)) return fail("%s: buffers must be 16-byte aligned", who);

    // ---- metadata: the chunk table of the whole call (src_row relative to its pass, filled below) + the flag words
    const size_t chunk_bytes = (size_t)total_chunks * sizeof(RaggedChunk);
    const size_t flag_off = (chunk_bytes + 255) & ~(size_t)255;
    const size_t flag_bytes = nan_mode == 1 ? (size_t)nvideos * 2 * sizeof(int) : 0;
    const size_t meta_bytes = flag_off + flag_bytes;
    int slot;
    if (int rc = meta_slot(h, meta_bytes, who, &slot)) return rc;
    MetaRing& mr = *h->meta;
    RaggedChunk* hc = (RaggedChunk*)mr.host[slot];
    const int mb = micro_batch(h);
    // fp16x3 carries one operand scale per 256-row chunk of the row set: it keeps whole chunks
    const bool enc_rows_mode = !h->policy.dense_encoder && h->cfg.compute != IEFVAD_COMPUTE_FP16X3;
    {
        // chunk table; src_row and enc_row are relative to the chunk's PASS (passes are runs of <= mb chunks)
        long long row = 0, pass_row0 = 0;
        long long ci = 0;
        int enc = 0;
        for (int v = 0; v < nvideos; ++v) {
            const int n = lengths[v], nch = video_chunks(n);
            for (int j = 0; j < nch; ++j, ++ci) {
                if (ci % mb == 0) { pass_row0 = row; enc = 0; }
                const int valid = (n - j * IEF_T) < IEF_T ? (n - j * IEF_T) : IEF_T;
                hc[ci].src_row = (int)(row - pass_row0);
                hc[ci].valid = valid;
                hc[ci].video = v;
                hc[ci].enc_row = enc;
                enc += enc_rows_mode ? ragged_rows(valid) : IEF_T;
                row += valid;
            }
        }
        if (flag_bytes) memset((char*)mr.host[slot] + flag_off, 0, flag_bytes);
    }
    HIP_TRY(hipMemcpyAsync(mr.dev[slot], mr.host[slot], meta_bytes, hipMemcpyHostToDevice, stream));
    const RaggedChunk* dc = (const RaggedChunk*)mr.dev[slot];
    const int* dflags = flag_bytes ? (const int*)((const char*)mr.dev[slot] + flag_off) : nullptr;

    if (dflags) {
        // The conditional nan_to_num of test.py:90-95 is decided on the WHOLE video tensor, and a video may straddle micro-batch
        // passes: every chunk of the call is scanned before the first pass lays out (and fixes up) its rows.  src_row is
        // pass-relative, so the scan goes pass by pass too, with the pass's base pointers.
        hipEvent_t e = tm.begin(ST_CAST);
        long long r0 = 0;
        for (long long c0 = 0; c0 < total_chunks; c0 += mb) {
            const int nb = (int)((total_chunks - c0 < mb) ? (total_chunks - c0) : mb);
            const RowsIn pin = in.at((size_t)r0, h->D);
            dispatch_in(in.in_dtype, h->D == IEF_D512, [&](auto t, auto w) {
                using T = typename decltype(t)::type;
                hipLaunchKernelGGL((iefvad_nanflag_kernel<T, decltype(w)::value>), dim3(nb, 2, IEF_RAGGED_SLICES), dim3(256), 0, stream,
                                   (const T*)pin.img, (const T*)pin.ev, dc + c0, (int*)dflags);
                return 0;
            });
            for (int j = 0; j < nb; ++j) r0 += hc[c0 + j].valid;
        }
        tm.end(e);
        HIP_TRY(hipGetLastError());
    }
    RaggedPass rg;
    memset(&rg, 0, sizeof(rg));
    rg.d_flags = dflags;
    // the homes behind the base workspace, the same for every pass
    if (out.wants_w_rows()) {
        rg.w_rows[0] = (float*)((char*)workspace + tail.w_rows);
        rg.w_rows[1] = rg.w_rows[0] + videos_pass_chunks(h, total_chunks) * IEF_T * h->D;
        if (out.w_colsum) rg.colsum_part = (double*)((char*)workspace + tail.colsum);
    }
    VideosOut call = out;
    call.nan_mode = nan_mode;
    call.x.place(workspace, tail);
    iefvad_outputs none;
    memset(&none, 0, sizeof(none));
    long long row0 = 0;
    int rc = 0;
    for (long long c0 = 0; c0 < total_chunks && !rc; c0 += mb) {
        const int nb = (int)((total_chunks - c0 < mb) ? (total_chunks - c0) : mb);
        long long vrows = 0;
        for (int j = 0; j < nb; ++j) vrows += hc[c0 + j].valid;
        rg.d_chunks = dc + c0;
        rg.valid_rows = (int)vrows;
        if (enc_rows_mode) {
            rg.enc_used_rows = hc[c0 + nb - 1].enc_row + ragged_rows(hc[c0 + nb - 1].valid);
            rg.enc_rows = (rg.enc_used_rows + IEF_T - 1) / IEF_T * IEF_T;        // <= nb * 256
        }
        rg.first_pass = c0 == 0;
        rg.out = call.at(row0, h->D);         // pass-relative, like src_row
        rc = forward_pass(h, in.at((size_t)row0, h->D), rg.out.x, nb, 0, workspace, &none, &rg, stream, tm);
        row0 += vrows;
    }
    (void)hipEventRecord(mr.done[slot], stream);       // the slot's buffers are free once everything enqueued above has run
    return rc;
}

extern "C" int iefvad_forward_videos(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype,
                                     const int32_t* lengths, int32_t nvideos, int32_t nan_to_num, void* workspace,
                                     size_t workspace_bytes, float* logits, float* w_i_mean, float* w_e_mean, void* stream) {
    Timer tm;
    VideosOut out = videos_out(logits, w_i_mean, w_e_mean, nan_to_num);
    return forward_videos_impl(h, RowsIn{img_rows, ev_rows, in_dtype}, lengths, nvideos, workspace, workspace_bytes, out, (hipStream_t)stream, tm,
                               "iefvad_forward_videos");
}

extern "C" int iefvad_forward_videos_attn(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype,
                                          const int32_t* lengths, int32_t nvideos, int32_t nan_to_num, void* workspace,
                                          size_t workspace_bytes, float* logits, float* w_i_mean, float* w_e_mean,
                                          const iefvad_attn_maps* maps, void* stream) {
    static const char* const who = "iefvad_forward_videos_attn";
    Timer tm;
    VideosOut out = videos_out(logits, w_i_mean, w_e_mean, nan_to_num);
    if (int rc = attn_maps_args(who, h, maps, &out.x.attn)) return rc;
    return forward_videos_impl(h, RowsIn{img_rows, ev_rows, in_dtype}, lengths, nvideos, workspace, workspace_bytes, out, (hipStream_t)stream, tm, who);
}

// The two sweep entries: the record carries the scales and, for _perturbed, the noise amplitudes, ids and seed to the chunker
static int forward_videos_perturbed(const char* who, iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype,
                                    const int32_t* lengths, int32_t nvideos, int32_t nan_to_num, const iefvad_perturb& p, void* workspace,
                                    size_t workspace_bytes, float* logits, float* w_i_mean, float* w_e_mean, double* w_colsum, void* stream) {
    Timer tm;
    VideosOut out = videos_out(logits, w_i_mean, w_e_mean, nan_to_num);
    out.x = perturb_extras(p);
    out.w_colsum = w_colsum;
    out.sweep_codes = true;
    return forward_videos_impl(h, RowsIn{img_rows, ev_rows, in_dtype}, lengths, nvideos, workspace, workspace_bytes, out, (hipStream_t)stream, tm, who);
}

extern "C" int iefvad_forward_videos_perturbed(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype,
                                               const int32_t* lengths, int32_t nvideos, int32_t nan_to_num, const iefvad_perturb* perturb,
                                               void* workspace, size_t workspace_bytes, float* logits, float* w_i_mean, float* w_e_mean,
                                               double* w_colsum, void* stream) {
    if (!perturb) return fail("iefvad_forward_videos_perturbed: null perturbation");
    return forward_videos_perturbed("iefvad_forward_videos_perturbed", h, img_rows, ev_rows, in_dtype, lengths, nvideos, nan_to_num, *perturb,
                                    workspace, workspace_bytes, logits, w_i_mean, w_e_mean, w_colsum, stream);
}

extern "C" int iefvad_forward_videos_scaled(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype,
                                            const int32_t* lengths, int32_t nvideos, int32_t nan_to_num, const float* img_row_scale,
                                            const float* ev_row_scale, void* workspace, size_t workspace_bytes, float* logits,
                                            float* w_i_mean, float* w_e_mean, double* w_colsum, void* stream) {
    iefvad_perturb p = {};
    p.scale[0] = img_row_scale; p.scale[1] = ev_row_scale;
    return forward_videos_perturbed("iefvad_forward_videos_scaled", h, img_rows, ev_rows, in_dtype, lengths, nvideos, nan_to_num, p, workspace,
                                    workspace_bytes, logits, w_i_mean, w_e_mean, w_colsum, stream);
}

extern "C" int iefvad_forward_videos_similarity(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype,
                                                const int32_t* lengths, int32_t nvideos, int32_t nan_to_num, void* workspace,
                                                size_t workspace_bytes, float* logits, float* w_i_mean, float* w_e_mean, void* stream,
                                                float* similarity) {
    static const char* const who = "iefvad_forward_videos_similarity";
    if (!similarity) return fail("%s: null similarity", who);
    Timer tm;
    VideosOut out = videos_out(logits, w_i_mean, w_e_mean, nan_to_num);
    out.similarity = similarity;
    if (int rc = videos_args(who, out, in_dtype, nvideos)) return rc;
    if (!h || !lengths) return fail("%s: null argument", who);
    long long chunks;
    if (int rc = videos_layout(lengths, nvideos, &out.sim_stride, &chunks, who)) return rc;       // the series' stride: the call's rows
    return forward_videos_impl(h, RowsIn{img_rows, ev_rows, in_dtype}, lengths, nvideos, workspace, workspace_bytes, out, (hipStream_t)stream, tm, who);
}

extern "C" int iefvad_forward_videos_full(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype, const int32_t* lengths,
                                          int32_t nvideos, int32_t nan_to_num, void* workspace, size_t workspace_bytes,
                                          const iefvad_outputs* out, void* stream) {
    static const char* const who = "iefvad_forward_videos_full";
    if (int rc = full_nulls(who, h, out)) return rc;
    const VideosOut dst = full_out(*out, nan_to_num);
    if (int rc = videos_args(who, dst, in_dtype, nvideos)) return rc;
    Timer tm;
    return forward_videos_impl(h, RowsIn{img_rows, ev_rows, in_dtype}, lengths, nvideos, workspace, workspace_bytes, dst, (hipStream_t)stream, tm, who);
}

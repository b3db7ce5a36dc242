// Online scores: every video evaluated over trailing windows on the valid-row route (include/iefvad.h, csrc/window_plan.h).  Included
// by iefvad.hip behind videos.h.
//
// The windows of a call overlap in their SOURCE rows, which the chunker does not mind (iefvad_scatter_rows_kernel reads src_row,
// writes enc_row, chunk by chunk); the encoder runs on them as on the chunks of iefvad_forward_videos; behind the last LayerNorm
// iefvad_readout_rows_kernel (ragged.h) gathers each window's read-out rows, and from there on the pass is a compacted set of exactly
// the call's own rows (pass_compact_rows).  Only the encoder's cost is multiplied by the number of windows.
#pragma once

static int online_args(const char* who, const iefvad_online* online) {
    if (!online) return fail("%s: null online parameters", who);
    if (!online_params_ok(online->stride, online->history))
        return fail("%s: 1 <= stride <= history <= %d required (got stride %d, history %d)", who, kWindowRows, online->stride, online->history);
    return 0;
}

// the base workspace of a pass of the call's windows; nothing lies behind it (the read-out rows live in the attention-output
// region, dead behind the last layer), so the layout is workspace_tail's with nothing asked for
static WorkspaceTail online_tail(const iefvad_handle* h, long long windows) { return videos_tail(h, windows, TailWants{}); }

extern "C" size_t iefvad_videos_online_workspace_bytes(const iefvad_handle* h, const int32_t* lengths, int32_t nvideos, const iefvad_online* online) {
    if (!h || !lengths || nvideos <= 0 || !online || !online_params_ok(online->stride, online->history)) return 0;
    const long long windows = online_call_windows(lengths, nvideos, online->stride);
    if (windows <= 0 || windows > 0x7fffffffLL / IEF_T) return 0;
    return iefvad_workspace_bytes(h, (int32_t)windows) ? online_tail(h, windows).total : 0;
}

extern "C" int iefvad_forward_videos_online(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype, const int32_t* lengths,
                                            int32_t nvideos, int32_t nan_to_num, const iefvad_online* online, void* workspace,
                                            size_t workspace_bytes, float* logits, float* w_i_mean, float* w_e_mean, void* stream_) {
    static const char* const who = "iefvad_forward_videos_online";
    hipStream_t stream = (hipStream_t)stream_;
    Timer tm;
    if (!h || !img_rows || !ev_rows || !lengths || !logits) return fail("%s: null argument", who);
    if (!h->weights_set) return fail("%s: weights not set", who);
    VideosOut out = videos_out(logits, w_i_mean, w_e_mean, nan_to_num ? 1 : 0);
    if (int rc = videos_args(who, out, in_dtype, nvideos)) return rc;
    if (int rc = online_args(who, online)) return rc;
    if (h->cfg.compute == IEFVAD_COMPUTE_FP16X3)
        return fail("%s: compute = fp16x3 is not supported (its operand scales are per chunk and its tail keeps whole chunks)", who);
    const int stride = online->stride, history = online->history;
    long long total_rows, total_chunks;
    if (int rc = videos_layout(lengths, nvideos, &total_rows, &total_chunks, who)) return rc;
    const long long W = online_call_windows(lengths, nvideos, stride);
    if (W > 0x7fffffffLL / IEF_T || total_chunks > 0x7fffffffLL / IEF_T) return fail("%s: too many windows", who);
    const WorkspaceTail tail = online_tail(h, W);
    if (!workspace || workspace_bytes < tail.total) return fail("%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, tail.total);
    if (((uintptr_t)workspace & 15) || ((uintptr_t)img_rows & 15) || ((uintptr_t)ev_rows & 15)) return fail("%s: buffers must be 16-byte aligned", who);

    std::vector<OnlineWindow> win;
    try { win.resize((size_t)W); } catch (const std::exception&) { return fail("%s: out of host memory", who); }
    online_fill_windows(lengths, nvideos, stride, history, win.data());

    // ---- metadata: the window table (src_row relative to the pass's source base) | the read-out map | the NaN scan's table, the
    // plain chunks of every video (src_row in packed rows of the call): a video is scanned once, not once per window | the flag words
    const RowsIn in{img_rows, ev_rows, in_dtype};
    const bool scan = out.nan_mode == 1;
    const size_t read_off = ((size_t)W * sizeof(RaggedChunk) + 255) & ~(size_t)255;
    const size_t scan_off = (read_off + (size_t)W * sizeof(OnlineRead) + 255) & ~(size_t)255;
    const size_t flag_off = (scan_off + (scan ? (size_t)total_chunks * sizeof(RaggedChunk) : 0) + 255) & ~(size_t)255;
    const size_t meta_bytes = flag_off + (scan ? (size_t)nvideos * 2 * sizeof(int) : 0);
    int slot;
    if (int rc = meta_slot(h, meta_bytes, who, &slot)) return rc;
    MetaRing& mr = *h->meta;
    RaggedChunk* const hc = (RaggedChunk*)mr.host[slot];
    OnlineRead* const hr = (OnlineRead*)((char*)mr.host[slot] + read_off);
    const int mb = micro_batch(h);
    const bool enc_rows_mode = !h->policy.dense_encoder;
    for (long long c0 = 0; c0 < W; c0 += mb) {
        const OnlinePass p = online_pass(win.data(), W, mb, c0);
        int enc = 0;
        for (int j = 0; j < p.count; ++j) {
            const OnlineWindow& w = win[c0 + j];
            RaggedChunk& c = hc[c0 + j];
            c.src_row = (int)(w.start - p.src_base);
            c.valid = (int)(w.end - w.start);
            c.video = w.video;
            c.enc_row = enc;
            enc += enc_rows_mode ? ragged_rows(c.valid) : IEF_T;
            hr[c0 + j] = online_read(w, p);
        }
    }
    if (scan) {
        RaggedChunk* const hs = (RaggedChunk*)((char*)mr.host[slot] + scan_off);
        long long row = 0, ci = 0;
        for (int v = 0; v < nvideos; ++v)
            for (int n = lengths[v]; n > 0; n -= IEF_T, ++ci) {
                hs[ci] = RaggedChunk{(int)row, n < IEF_T ? n : IEF_T, v, 0};
                row += hs[ci].valid;
            }
        memset((char*)mr.host[slot] + flag_off, 0, (size_t)nvideos * 2 * sizeof(int));
    }
    HIP_TRY(hipMemcpyAsync(mr.dev[slot], mr.host[slot], meta_bytes, hipMemcpyHostToDevice, stream));
    const RaggedChunk* const dc = (const RaggedChunk*)mr.dev[slot];
    const OnlineRead* const dr = (const OnlineRead*)((const char*)mr.dev[slot] + read_off);
    const int* const dflags = scan ? (const int*)((const char*)mr.dev[slot] + flag_off) : nullptr;

    if (scan) {
        // the NaN rule stays per video over the WHOLE video (test.py:90-95), so it is not causal: one scan of the call's rows
        const RaggedChunk* const ds = (const RaggedChunk*)((const char*)mr.dev[slot] + scan_off);
        hipEvent_t e = tm.begin(ST_CAST);
        dispatch_in(in_dtype, h->D == IEF_D512, [&](auto t, auto w) {
            using T = typename decltype(t)::type;
            hipLaunchKernelGGL((iefvad_nanflag_kernel<T, decltype(w)::value>), dim3((unsigned)total_chunks, 2, IEF_RAGGED_SLICES), dim3(256), 0, stream,
                               (const T*)img_rows, (const T*)ev_rows, ds, (int*)dflags);
            return 0;
        });
        tm.end(e);
        HIP_TRY(hipGetLastError());
    }

    RaggedPass rg;
    memset(&rg, 0, sizeof(rg));
    rg.d_flags = dflags;
    iefvad_outputs none;
    memset(&none, 0, sizeof(none));
    int rc = 0;
    for (long long c0 = 0; c0 < W && !rc; c0 += mb) {
        const OnlinePass p = online_pass(win.data(), W, mb, c0);
        rg.d_chunks = dc + c0;
        rg.d_reads = dr + c0;
        rg.valid_rows = p.out_rows;
        // a workgroup of the gather takes 16-row groups: no more of them per window than the pass's largest read-out count fills
        // (stride 16: one, where IEF_RAGGED_SLICES would leave three of four without a row)
        int most = 1;
        for (int j = 0; j < p.count; ++j) most = hr[c0 + j].count > most ? hr[c0 + j].count : most;
        rg.read_slices = (most + 15) / 16 < IEF_RAGGED_SLICES ? (most + 15) / 16 : IEF_RAGGED_SLICES;
        if (enc_rows_mode) {
            rg.enc_used_rows = hc[c0 + p.count - 1].enc_row + ragged_rows(hc[c0 + p.count - 1].valid);
            rg.enc_rows = (rg.enc_used_rows + IEF_T - 1) / IEF_T * IEF_T;        // <= p.count * 256
        }
        rg.first_pass = c0 == 0;
        rg.out = out.at(p.out_base, h->D);
        rc = forward_pass(h, in.at((size_t)p.src_base, h->D), rg.out.x, p.count, 0, workspace, &none, &rg, stream, tm);
    }
    (void)hipEventRecord(mr.done[slot], stream);       // the slot's buffers are free once everything enqueued above has run
    return rc;
}

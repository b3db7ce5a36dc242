// Orchestration of the train-mode forward and of the model's backward pass (include/iefvad.h: iefvad_train_forward /
// iefvad_train_backward; kernels in backward.h).  Included by iefvad.hip behind the handle, launch, launch_proj(ProjCtx, Proj, stage)
// and the error helpers.  The backward is written per Linear -- linear_param_grads(BwdCtx, LinearGrads) for dW and db (launch_dw, then
// launch_db unless the bias sums rode along), launch_dx(BwdCtx, ProjW, ...) for dX -- and per head product (head_product over HeadViews).
//
// What the reference does per training step (/root/reference/train/ucf_train.py:43-106, train/xd_train.py:35-78): model.train(),
// outputs = model(img, ev, None, prompt_text, lengths), the three loss terms, loss.backward(), optimizer.step().  Here:
//   iefvad_train_forward   the forward of imf_vad.py:109-161 in train mode (attention dropout, imf_vad.py:70) that KEEPS what the
//                          backward needs, in a caller-owned buffer:
//                            per modality and layer: the layer input x_l, q | k | v (q pre-scaled by 1 / sqrt(96)), the attention
//                            probabilities P (ONE tensor, the dropout mask in its sign bits -- attention_split.h, backward.h),
//                            the attention output, the pre-LayerNorm sum;
//                            the last LayerNorm output, the whitened rows, mu and logvar of both modalities;
//                            the refinement states z_0 .. z_K and hidden activations h_0 .. h_{K-1}
//   iefvad_train_backward  the gradients of every parameter, given the gradients of the eight outputs
//   iefvad_train_backward_inputs  the same, plus the gradients of the two input feature tensors where asked for
// Arithmetic: the dense projections of the forward run on the handle's kernels (fp32 MFMA, or the exact bf16x6 split when
// the batch fills its grid); every product of the backward and the two attention products of the train forward run on
// iefvad_bgemm_f32_kernel (fp32 MFMA).  Reductions over rows are fixed-order (no atomics): gradients are bit-reproducible.
#pragma once

// ---- layout of the caller's training buffer, in floats ----------------------------------------------------------------------------
struct TrainLayout {
    size_t U;                       // one [rows, 768] tensor
    size_t PU;                      // one [B, 8, 256, 256] tensor
    size_t x[2][IEFVAD_MAX_LAYERS + 1], qkv[2][IEFVAD_MAX_LAYERS], att[2][IEFVAD_MAX_LAYERS], s[2][IEFVAD_MAX_LAYERS];
    size_t P[2][IEFVAD_MAX_LAYERS];
    size_t E[2], mu[2], lv[2];
    size_t z[IEFVAD_MAX_STEPS + 1], hid[IEFVAD_MAX_STEPS];
    size_t logits;
    // backward scratch
    size_t g, da, dh[2], gx, datt, dqkv, dP, part, cpart, rpart;
    size_t part_floats, cpart_floats, rpart_floats;
    size_t total;
};

static const int kColsumRows = 128;

static int splitk_splits(int rows, int n_out) {
    const int tiles = (n_out / 128) * (IEF_D / 128);
    int want = (1024 + tiles - 1) / tiles, s = 1;
    while (s < want && s < 64) s <<= 1;
    while (s > 1 && ((rows / 16) % s)) s >>= 1;
    return s;
}

// Train-mode attention runs as two fused launches per layer in bf16x6 (attention_split.h TRAIN / BWD) and as the three-launch path in
// the f32 arithmetic (or with IEFVAD_TRAIN_ATTN=unfused at iefvad_create, the A/B test's switch; the backward follows its forward's
// record).  Both keep P and dropout(P) as ONE sign-carrying tensor: the layout is the same.
static bool train_attn_fused(const iefvad_handle* h) { return h->cfg.compute == IEFVAD_COMPUTE_BF16X6 && !h->train_attn_unfused; }

static TrainLayout train_layout(int L, int K, int B) {
    TrainLayout t;
    memset(&t, 0, sizeof(t));
    const size_t rows = (size_t)B * IEF_T;
    t.U = rows * IEF_D;
    t.PU = (size_t)B * IEF_H * IEF_T * IEF_T;
    size_t o = 0;
    auto take = [&](size_t n) { const size_t r = o; o += (n + 63) & ~(size_t)63; return r; };
    for (int m = 0; m < 2; ++m) {
        for (int l = 0; l <= L; ++l) t.x[m][l] = take(t.U);
        for (int l = 0; l < L; ++l) {
            t.qkv[m][l] = take(3 * t.U);
            t.att[m][l] = take(t.U);
            t.s[m][l] = take(t.U);
            t.P[m][l] = take(t.PU);
        }
        t.E[m] = take(t.U);
        t.mu[m] = take(t.U);
        t.lv[m] = take(t.U);
    }
    for (int k = 0; k <= K; ++k) t.z[k] = take(t.U);
    for (int k = 0; k < K; ++k) t.hid[k] = take(t.U);
    t.logits = take(rows);
    t.g = take(t.U);
    t.da = take(t.U);
    // Scratch of the backward's second half (fusion, heads, encoder layers).  By then the refinement steps have been differentiated and
    // their saved states z_0 .. z_K, h_0 .. h_{K-1} -- (2K + 1) U contiguous floats -- are dead: the scratch tensors live THERE as far as
    // they fit (all of them from K = 6 on), largest first.  The backward therefore consumes the buffer: one backward per forward
    // (iefvad_train_backward retires the forward's record).
    {
        size_t dead = t.z[0];
        const size_t dead_end = t.z[0] + (size_t)(2 * K + 1) * t.U;
        auto place = [&](size_t n) {
            const size_t n64 = (n + 63) & ~(size_t)63;
            if (dead + n64 <= dead_end) { const size_t r = dead; dead += n64; return r; }
            return take(n);
        };
        t.dqkv = place(3 * t.U);
        t.dP = place(t.PU);
        t.dh[0] = place(2 * t.U);
        t.dh[1] = place(2 * t.U);
        t.gx = place(t.U);
        t.datt = place(t.U);
    }
    size_t pf = 0;
    const int nouts[3] = {IEF_D, 2 * IEF_D, 3 * IEF_D};
    for (int n : nouts) {
        const size_t f = (size_t)splitk_splits((int)rows, n) * n * IEF_D;
        if (f > pf) pf = f;
    }
    t.part_floats = pf;
    t.part = take(pf);
    t.cpart_floats = ((rows + kColsumRows - 1) / kColsumRows) * 3 * IEF_D;
    t.cpart = take(t.cpart_floats);
    t.rpart_floats = ((rows + BWD_ROWS_PER_BLOCK - 1) / BWD_ROWS_PER_BLOCK) * (2 * IEF_D + 1);
    t.rpart = take(t.rpart_floats);
    t.total = o;
    return t;
}

extern "C" size_t iefvad_train_workspace_bytes(const iefvad_handle* h, int32_t B) {
    if (!h || B <= 0 || B > 4096) return 0;
    if (h->D != IEF_D) { fail("iefvad_train_workspace_bytes: training is built for D=768 (this handle has D=%d)", h->D); return 0; }
    return train_layout(h->cfg.num_layers, h->cfg.num_steps, B).total * sizeof(float) + 256;
}

// ---- launch helpers -----------------------------------------------------------------------------------------------------------------
static int launch_bgemm(const BgemmArgs& a, bool akc, bool bkc, int nz, hipStream_t stream) {
    const int bn = (a.N % 128 == 0) ? 128 : 96;
    if (a.M % BG_BM || a.N % bn || a.K % BG_BK || a.M <= 0 || a.N <= 0 || a.K <= 0 || nz <= 0 || a.nz2 <= 0)
        return fail("bgemm: shape M=%d N=%d K=%d is not a multiple of the 128 x %d x 16 tile", a.M, a.N, a.K, bn);
    if ((a.lda | a.ldb) & 3) return fail("bgemm: leading dimensions must be multiples of 4 floats");
    dim3 grid((unsigned)((a.M / BG_BM) * (a.N / bn) * nz));
#define BG_LAUNCH(AK, BK_, BN_) return launch(iefvad_bgemm_f32_kernel<AK, BK_, BN_>, grid, dim3(256), 0, stream, a)
    if (bn == 128) {
        if (akc && bkc) BG_LAUNCH(true, true, 128);
        else if (akc) BG_LAUNCH(true, false, 128);
        else if (bkc) BG_LAUNCH(false, true, 128);
        else BG_LAUNCH(false, false, 128);
    } else {
        if (akc && bkc) BG_LAUNCH(true, true, 96);
        else if (akc) BG_LAUNCH(true, false, 96);
        else if (bkc) BG_LAUNCH(false, true, 96);
        else BG_LAUNCH(false, false, 96);
    }
#undef BG_LAUNCH
}

// The five tensors the per-(chunk, head) products of attention index: the q, k and v column blocks of qkv [rows, 2304], the
// probabilities P [B, 8, 256, 256], and a [rows, 768] tensor read 96 columns per head.  Strides in floats.
struct HeadView { float* p; int ld; long long chunk_stride, head_stride; };
static HeadView q_of(float* qkv) { return HeadView{qkv, 3 * IEF_D, (long long)IEF_T * 3 * IEF_D, IEF_DH}; }
static HeadView k_of(float* qkv) { return q_of(qkv + IEF_D); }
static HeadView v_of(float* qkv) { return q_of(qkv + 2 * IEF_D); }
static HeadView probs(float* P) { return HeadView{P, IEF_T, (long long)IEF_H * IEF_T * IEF_T, (long long)IEF_T * IEF_T}; }
static HeadView head_rows(float* att) { return HeadView{att, IEF_D, (long long)IEF_T * IEF_D, IEF_DH}; }

// C[M, N] = alpha * A B over K for every (chunk, head) of `nchunks` chunks; akc / bkc: K runs along the columns of A / of B as stored
// (launch_bgemm).  a_drop != 0: A is the sign-carrying P and dropout(P) is formed from it (BgemmArgs.a_drop).
static int head_product(HeadView C, HeadView A, bool akc, HeadView B, bool bkc, int M, int N, int K, float alpha, float a_drop, int nchunks,
                        hipStream_t stream) {
    BgemmArgs a;
    memset(&a, 0, sizeof(a));
    a.A = A.p; a.B = B.p; a.C = C.p;
    a.M = M; a.N = N; a.K = K; a.lda = A.ld; a.ldb = B.ld; a.ldc = C.ld;
    a.a1 = A.chunk_stride; a.a2 = A.head_stride; a.b1 = B.chunk_stride; a.b2 = B.head_stride; a.c1 = C.chunk_stride; a.c2 = C.head_stride;
    a.nz2 = IEF_H; a.alpha = alpha; a.a_drop = a_drop;
    return launch_bgemm(a, akc, bkc, nchunks * IEF_H, stream);
}

// The dropout stream of (modality, layer) of the library's generator, and the slice of an injected mask that replaces it
static unsigned long long dropout_seed(unsigned long long opt_seed, int m, int l) {
    return opt_seed * 0x100000001B3ull + (unsigned long long)(m * IEFVAD_MAX_LAYERS + l + 1) * 0x9E3779B97F4A7C15ull;
}
static const uint8_t* keep_mask_of(const iefvad_train_options* opt, int m, int l, int L, size_t PU) {
    return opt->keep_mask ? opt->keep_mask + ((size_t)m * L + l) * PU : nullptr;
}

// bf16x6 handles: the three-plane splits of every TRANSPOSED projection matrix, so that dX = dY W runs as the NT product
// dX[rows, 768] = dY[rows, n_out] (W^T)[768, n_out]^T on iefvad_gemm_split_n128_kernel (fp32-accurate, 1.7x the fp32 MFMA rate)
static int ensure_train_planes(iefvad_handle* h, hipStream_t stream) {
    if (h->cfg.compute != IEFVAD_COMPUTE_BF16X6 || h->tplanes_valid) return 0;
    if (!h->arena_st) HIP_TRY(hipMalloc((void**)&h->arena_st, 3 * proj_elems(h) * sizeof(bf16_t)));
    if (!h->zero_bias) {
        HIP_TRY(hipMalloc((void**)&h->zero_bias, 3 * IEF_D * sizeof(float)));
        HIP_TRY(hipMemsetAsync(h->zero_bias, 0, 3 * IEF_D * sizeof(float), stream));
    }
    bf16_t* q = h->arena_st;
    SplitMany sm(stream);                     // one launch for all of them (gemm_split.h: transpose and split in one pass)
    if (int rc = for_each_proj(h, [&](ProjW& r) {      // W [N, 768] -> planes of W^T [768, N]
            const size_t n = (size_t)r.N * IEF_D;
            r.wst = q;
            q += 3 * n;
            return sm.add(r.w, r.wst, n, r.N);
        })) return rc;
    if (int rc = sm.flush()) return rc;
    h->tplanes_valid = true;
    return 0;
}

// What the whole backward shares: the split-K scratch `part` and the column-sum scratch `cpart` of the training buffer, and which
// products of a bf16x6 handle run on the split kernels
struct BwdCtx {
    iefvad_handle* h;
    int rows;
    hipStream_t stream;
    float* part; size_t part_floats;
    float* cpart; size_t cpart_floats;
    bool split_tn;      // dW on the split TN kernel (gemm_split_tn.h)
    bool split_dx;      // dX on the split kernel over ProjW::wst, where the grid fills it
};

// dX[rows, 768] = alpha * dY[rows, w.N] * W[w.N, 768] (+ R) (gated by G): the input gradient of a Linear whose weight is stored
// [out, in] as torch stores it.
static int launch_dx(const BwdCtx& x, const ProjW& w, const float* dY, float* dX, const float* R, const float* G, float alpha) {
    if (x.split_dx && w.wst && split_eligible(x.rows, IEF_D, w.N, 1) && (!R || !G) && (G || alpha == 1.f)) {
        GemmBArgs g;
        memset(&g, 0, sizeof(g));
        g.M = x.rows; g.N = IEF_D; g.K = w.N; g.lda = w.N; g.ldc = IEF_D; g.alpha = alpha;
        g.epi = G ? EPI_GATE : (R ? EPI_BIAS_RESID : EPI_BIAS);
        g.wplane = IEF_D * w.N * 2;
        g.p[0].A = (const bf16_t*)dY;            // fp32 data behind the typed pointer
        g.p[0].W = w.wst; g.p[0].bias = x.h->zero_bias; g.p[0].C = dX; g.p[0].R = G ? G : R;
        Timer tm;
        return launch_gemm_split(g, 1, x.stream, tm, ST_REFINE, false, x.h->policy.split_tile);      // N = 768: either tiling takes it
    }
    BgemmArgs a;
    memset(&a, 0, sizeof(a));
    a.A = dY; a.B = w.w; a.C = dX; a.R = R; a.G = G;
    a.M = x.rows; a.N = IEF_D; a.K = w.N; a.lda = w.N; a.ldb = IEF_D; a.ldc = IEF_D; a.nz2 = 1; a.alpha = alpha;
    return launch_bgemm(a, true, false, 1, x.stream);
}

static int reduce_parts(const float* part, size_t stride, int nparts, size_t n, float* out, float alpha, hipStream_t stream) {
    if (!out) return 0;
    return launch(iefvad_reduce_parts_kernel, dim3((unsigned)((n + RED_STRIP - 1) / RED_STRIP)), dim3(256), 0, stream, part, stride, nparts, n, out, alpha);
}

// a batch of fixed-order reductions for one launch of iefvad_reduce_parts_multi_kernel (null destinations are skipped)
struct ReduceBatch {
    ReduceJobs j;
    ReduceBatch() { memset(&j, 0, sizeof(j)); }
    void add(const float* part, size_t stride, int nparts, size_t n, float* out, float alpha) {
        if (!out || n == 0 || j.count == 4) return;
        const int c = j.count++;
        j.part[c] = part; j.stride[c] = stride; j.nparts[c] = nparts; j.n[c] = n; j.out[c] = out; j.alpha[c] = alpha;
        j.first[c + 1] = j.first[c] + (unsigned)((n + RED_STRIP - 1) / RED_STRIP);
    }
    int launch(hipStream_t stream) {
        if (j.count == 0) return 0;
        return ::launch(iefvad_reduce_parts_multi_kernel, dim3(j.first[j.count]), dim3(256), 0, stream, j);
    }
};

// The launches of the row kernels of backward.h, each with the grid its kernel is written for: train_forward / train_backward below and
// the unit entry iefvad_backward_unit (include/iefvad.h) launch through these, so a unit test runs the launch the training step runs.
static int bwd_row_blocks(int rows) { return (rows + BWD_ROWS_PER_BLOCK - 1) / BWD_ROWS_PER_BLOCK; }      // scorer / LayerNorm backward
static int colsum_blocks(int rows) { return (rows + kColsumRows - 1) / kColsumRows; }
static int launch_softmax_dropout(const SoftmaxDropArgs& a, hipStream_t stream) {
    return launch(iefvad_softmax_dropout_kernel, dim3((unsigned)((a.rows + 3) / 4)), dim3(256), 0, stream, a);
}
static int launch_softmax_bwd(const float* Ps, float scale, float* dPd, long long rows, hipStream_t stream) {
    return launch(iefvad_softmax_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, Ps, scale, dPd, rows);
}
// part[colsum_blocks(rows)][ncols]: column sums of Y [rows, ld] per block of kColsumRows rows
static int launch_colsum(const float* Y, int ld, int rows, int ncols, float* part, hipStream_t stream) {
    const dim3 grid((ncols + 255) / 256, colsum_blocks(rows));
    return launch(iefvad_colsum_kernel, grid, dim3(256), 0, stream, Y, ld, rows, ncols, kColsumRows, part);
}
static int launch_scorer_bwd(const ScorerBwdArgs& a, hipStream_t stream) {
    return launch(iefvad_scorer_bwd_kernel, dim3(bwd_row_blocks(a.rows)), dim3(256), 0, stream, a);
}
static int launch_fusion_bwd(const FusionBwdArgs& a, hipStream_t stream) {
    return launch(iefvad_fusion_bwd_kernel, dim3((a.rows + ROW_WAVES - 1) / ROW_WAVES), dim3(256), 0, stream, a);
}
static int launch_layernorm_bwd(const LnBwdArgs& a, hipStream_t stream) {
    return launch(iefvad_layernorm_bwd_kernel, dim3(bwd_row_blocks(a.rows)), dim3(256), 0, stream, a);
}

// The parameter gradients of one Linear y = x W^T + b with W = w->w [w->N, 768]: dW = alpha * dY^T X and db = alpha * column sums of dY
// over the rows; null destinations are frozen parameters.  dW2 / db2 (nullable) receive rows / columns [n_split, w->N) as tensors of
// their own (the stacked mu | logvar heads).
struct LinearGrads {
    const float* dY; const ProjW* w; const float* X; float alpha;
    float *dW, *db; float *dW2 = nullptr, *db2 = nullptr; int n_split = 0;
    int n_first() const { return n_split > 0 ? n_split : w->N; }      // outputs of dW / db; the rest, if any, are dW2's / db2's
};

// dW (and db) of one Linear on the split TN kernel (gemm_split_tn.h): `slices` ragged row slices write their partial products
// part[slices][n_out][768] (and, colsum != null, their partial column sums of dY colsum[slices][n_out]); ONE launch of the fixed-order
// reduction behind them adds the weight partials (both halves of a stacked product, split at output n1) and the bias partials.
// rows % 16 == 0, n_out % 128 == 0, 1 <= slices <= rows / 16 / 8.  Shared by launch_dw and iefvad_backward_unit.
static int launch_dw_split_tn(const float* dY, const float* X, int rows, int n_out, int slices, float* part, float* colsum, int n1, float alpha,
                              float* dW, float* dW2, float* db, float* db2, hipStream_t stream) {
    const size_t per = (size_t)n_out * IEF_D;
    TnArgs t;
    memset(&t, 0, sizeof(t));
    t.A = dY; t.B = X; t.C = part; t.M = n_out; t.N = IEF_D; t.lda = n_out; t.ldb = IEF_D; t.ldc = IEF_D;
    t.nk_total = rows / TN_BK;
    t.slices = slices;
    t.tiles_n = IEF_D / 256;
    // the bias gradient of the same Linear (column sums of dY) rides along in the first column block's workgroups
    t.colsum = colsum;
    if (int rc = launch(iefvad_gemm_split_tn256_kernel, dim3((unsigned)((n_out / 128) * t.tiles_n * slices)), dim3(256), TN_LDS_BYTES_OF(4), stream, t))
        return rc;
    // one launch reduces the weight partials (both halves of a stacked product) and the bias partials that rode along
    ReduceBatch rb;
    rb.add(part, per, slices, (size_t)n1 * IEF_D, dW, alpha);
    if (dW2) rb.add(part + (size_t)n1 * IEF_D, per, slices, (size_t)(n_out - n1) * IEF_D, dW2, alpha);
    if (colsum) {
        rb.add(colsum, (size_t)n_out, slices, (size_t)n1, db, alpha);
        if (db2) rb.add(colsum + n1, (size_t)n_out, slices, (size_t)(n_out - n1), db2, alpha);
    }
    return rb.launch(stream);
}

// dW by split-K with fixed-order reduction.  `db_done`: the bias sums rode along (the split TN kernel, room in cpart) and are reduced too.
static int launch_dw(const BwdCtx& x, const LinearGrads& g, bool& db_done) {
    db_done = false;
    if (!g.dW && !g.dW2) return 0;
    const int rows = x.rows, n_out = g.w->N, n1 = g.n_first();
    const int splits = splitk_splits(rows, n_out);
    const size_t per = (size_t)n_out * IEF_D;
    if ((size_t)splits * per > x.part_floats) return fail("train_backward: split-K scratch too small");
    const int ms = rows / splits;
    if (x.split_tn && ms % TN_BK == 0 && n_out % 128 == 0) {
        // bf16x6 handles: the same partial products on the bf16 matrix pipe (gemm_split_tn.h), the same fixed-order reduction behind them:
        // the 128 x 256 block (64 x 128 per wave, two workgroups per CU) over as many RAGGED row slices as fill the chip's workgroup slots
        // once (at most the slices the scratch was sized for)
        const int nk_total = rows / TN_BK;
        const int tiles = (n_out / 128) * (IEF_D / 256);
        int slices = (2 * g_num_cus) / tiles;
        if (slices > nk_total / 8) slices = nk_total / 8;
        if (slices > splits) slices = splits;          // the scratch (part, cpart) holds `splits` partial results
        if (slices < 1) slices = 1;
        // the bias gradient of the same Linear (column sums of dY) rides along where cpart has room for it
        db_done = (g.db || g.db2) && (size_t)slices * n_out <= x.cpart_floats;
        return launch_dw_split_tn(g.dY, g.X, rows, n_out, slices, x.part, db_done ? x.cpart : nullptr, n1, g.alpha, g.dW, g.dW2, g.db, g.db2, x.stream);
    }
    BgemmArgs a;
    memset(&a, 0, sizeof(a));
    a.A = g.dY; a.B = g.X; a.C = x.part;
    a.M = n_out; a.N = IEF_D; a.K = ms; a.lda = n_out; a.ldb = IEF_D; a.ldc = IEF_D;
    a.a1 = (long long)ms * n_out; a.b1 = (long long)ms * IEF_D; a.c1 = (long long)per; a.nz2 = 1; a.alpha = 1.f;
    if (int rc = launch_bgemm(a, false, false, splits, x.stream)) return rc;
    if (int rc = reduce_parts(x.part, per, splits, (size_t)n1 * IEF_D, g.dW, g.alpha, x.stream)) return rc;
    return reduce_parts(x.part + (size_t)n1 * IEF_D, per, splits, (size_t)(n_out - n1) * IEF_D, g.dW2, g.alpha, x.stream);
}

// db (and db2) from a colsum launch of their own
static int launch_db(const BwdCtx& x, const LinearGrads& g) {
    if (!g.db && !g.db2) return 0;
    const int ncols = g.w->N, n1 = g.n_first();
    const int nblk = colsum_blocks(x.rows);
    if (int rc = launch_colsum(g.dY, ncols, x.rows, ncols, x.cpart, x.stream)) return rc;
    if (int rc = reduce_parts(x.cpart, (size_t)ncols, nblk, (size_t)n1, g.db, g.alpha, x.stream)) return rc;
    return reduce_parts(x.cpart + n1, (size_t)ncols, nblk, (size_t)(ncols - n1), g.db2, g.alpha, x.stream);
}

static int linear_param_grads(const BwdCtx& x, const LinearGrads& g) {
    bool db_done = false;
    if (int rc = launch_dw(x, g, db_done)) return rc;
    return db_done ? 0 : launch_db(x, g);
}

// What a train-mode forward leaves on the handle for its backward: which buffer it filled, at which batch size, and whether the
// stored probabilities carry a dropout mask.  A handful of forwards may be outstanding (one record per training buffer).
// Five saved tensors are also outputs (mu and logvar of both modalities, the refined state z_K = `fused`) and two are the inputs: where
// the caller hands over fp32 buffers of its own, the forward writes / reads THOSE and the backward reads them again (x0, mu, lv, zK
// below) -- seven device-to-device copies of [rows, 768] per step less (0.33 ms of a 26 ms step).  The caller keeps them untouched
// until the backward has run (include/iefvad.h).
struct TrainRecord {
    const void* ws; int B; bool drop[2][IEFVAD_MAX_LAYERS]; float drop_p[2][IEFVAD_MAX_LAYERS]; bool fused; unsigned long long stamp;
    const float* x0[2]; float* mu[2]; float* lv[2]; float* zK;
};
struct TrainState { TrainRecord rec[8]; unsigned long long clock = 0; };

static void release_train(iefvad_handle* h) {
    delete h->train;
    h->train = nullptr;
}

static int train_check(const iefvad_handle* h, int32_t B, const void* ws, size_t ws_bytes, const char* who) {
    if (!h) return fail("%s: null handle", who);
    if (!h->weights_set) return fail("%s: weights not set", who);
    if (h->cfg.compute != IEFVAD_COMPUTE_F32 && h->cfg.compute != IEFVAD_COMPUTE_BF16X6)
        return fail("%s: training runs in the fp32-accurate arithmetics only (compute f32 or bf16x6)", who);
    if (B <= 0 || B > 4096) return fail("%s: B = %d outside 1..4096", who, B);
    const size_t need = iefvad_train_workspace_bytes(h, B);
    if (!ws || ws_bytes < need) return fail("%s: training buffer too small (%zu < %zu bytes)", who, ws_bytes, need);
    if ((uintptr_t)ws & 255) return fail("%s: the training buffer must be 256-byte aligned", who);
    return 0;
}

// ---- the trainers' NaN rule on the device ----------------------------------------------------------------------------------------------
// /root/reference/train/ucf_train.py:50-53 (xd_train.py has no such rule): `if torch.isnan(x).any(): x = torch.nan_to_num(x, nan=0.0)` per input
// tensor -- in torch an isnan pass that writes a bool tensor, a reduction, a HOST read of the flag (the step's launches cannot run
// ahead of the device) and, when it fires, a rewriting pass.  Here: one scan of both tensors (a flag word each, set by any thread
// that sees a NaN) and a repair launch whose workgroups return at once when their tensor's flag is clear; nothing comes back to the
// host.  The repair is torch.nan_to_num(x, nan=0.0) element for element (NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX), IN PLACE.
__global__ __launch_bounds__(256) void iefvad_nan_scan_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n4, unsigned* flags) {
    const float* x = blockIdx.y ? b : a;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const f32x4 v = ((const f32x4*)x)[i];
        bad |= (v[0] != v[0]) | (v[1] != v[1]) | (v[2] != v[2]) | (v[3] != v[3]);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) flags[blockIdx.y] = 1u;      // every writer writes the same value
}
__global__ __launch_bounds__(256) void iefvad_nan_fix_kernel(float* a, float* b, size_t n4, const unsigned* flags) {
    if (!flags[blockIdx.y]) return;
    float* x = blockIdx.y ? b : a;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        f32x4 v = ((f32x4*)x)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float f = v[e];
            v[e] = f != f ? 0.f : f == __builtin_inff() ? 3.402823466e+38f : f == -__builtin_inff() ? -3.402823466e+38f : f;
        }
        ((f32x4*)x)[i] = v;
    }
}
extern "C" int iefvad_nan_rule(float* a, float* b, size_t n, void* flags_ws, void* stream_) {
    if (!a || !b || !flags_ws) return fail("iefvad_nan_rule: null argument");
    if (n % 4 || (((uintptr_t)a | (uintptr_t)b) & 15) || ((uintptr_t)flags_ws & 7)) return fail("iefvad_nan_rule: n %% 4 == 0 and 16-byte aligned tensors, please");
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipMemsetAsync(flags_ws, 0, 8, stream));
    if (int rc = launch(iefvad_nan_scan_kernel, dim3(2048, 2), dim3(256), 0, stream, a, b, n / 4, (unsigned*)flags_ws)) return rc;
    return launch(iefvad_nan_fix_kernel, dim3(2048, 2), dim3(256), 0, stream, a, b, n / 4, (const unsigned*)flags_ws);
}

// ---- train-mode forward -------------------------------------------------------------------------------------------------------------
extern "C" int iefvad_train_forward(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B,
                                    const iefvad_train_options* opt, void* train_ws, size_t train_ws_bytes, const iefvad_outputs* out,
                                    void* stream_) {
    if (!h) return fail("iefvad_train_forward: null handle");
    if (h->D != IEF_D) return fail("iefvad_train_forward: training is built for D=768 (this handle has D=%d)", h->D);
    if (h->steps != h->cfg.num_steps)
        return fail("iefvad_train_forward: the handle runs %d of its %d refinement steps (iefvad_set_steps); training takes all of them", h->steps,
                    h->cfg.num_steps);
    const bool fused = train_attn_fused(h);
    if (int rc = train_check(h, B, train_ws, train_ws_bytes, "iefvad_train_forward")) return rc;
    if (!img || !ev || !out || !opt) return fail("iefvad_train_forward: null argument");
    if (in_dtype != IEFVAD_IN_F32 && in_dtype != IEFVAD_IN_F16 && in_dtype != IEFVAD_IN_BF16)
        return fail("iefvad_train_forward: unknown in_dtype %d", in_dtype);
    if (((uintptr_t)img | (uintptr_t)ev) & 15) return fail("iefvad_train_forward: buffers must be 16-byte aligned");
    if (((uintptr_t)out->fused | (uintptr_t)out->image_mu | (uintptr_t)out->event_mu | (uintptr_t)out->image_logvar | (uintptr_t)out->event_logvar) & 15)
        return fail("iefvad_train_forward: output buffers must be 16-byte aligned");
    const iefvad_config& c = h->cfg;
    const int L = c.num_layers, K = c.num_steps;
    for (int m = 0; m < 2; ++m)
        for (int l = 0; l < L; ++l)
            if (!(opt->dropout_p[m][l] >= 0.f && opt->dropout_p[m][l] < 1.f))
                return fail("iefvad_train_forward: dropout_p[%d][%d] = %g outside [0, 1)", m, l, (double)opt->dropout_p[m][l]);
    hipStream_t stream = (hipStream_t)stream_;
    const TrainLayout t = train_layout(L, K, B);
    float* ws = (float*)train_ws;
    const int rows = B * IEF_T;
    Timer tm;
    if (!h->train) {
        h->train = new (std::nothrow) TrainState();
        if (!h->train) return fail("iefvad_train_forward: out of host memory");
        memset(h->train->rec, 0, sizeof(h->train->rec));
    }
    TrainRecord* rec = nullptr;
    {   // the record of this forward replaces the one of the same buffer, else the oldest
        TrainState& ts = *h->train;
        int slot = 0;
        for (int i = 0; i < 8; ++i) {
            if (ts.rec[i].ws == train_ws) { slot = i; break; }
            if (ts.rec[i].stamp < ts.rec[slot].stamp) slot = i;
        }
        TrainRecord& r = ts.rec[slot];
        rec = &r;
        r.ws = train_ws; r.B = B; r.fused = fused; r.stamp = ++ts.clock;
        const bool f32in = in_dtype == IEFVAD_IN_F32;
        r.x0[0] = f32in ? (const float*)img : ws + t.x[0][0];
        r.x0[1] = f32in ? (const float*)ev : ws + t.x[1][0];
        r.mu[0] = out->image_mu ? out->image_mu : ws + t.mu[0];
        r.mu[1] = out->event_mu ? out->event_mu : ws + t.mu[1];
        r.lv[0] = out->image_logvar ? out->image_logvar : ws + t.lv[0];
        r.lv[1] = out->event_logvar ? out->event_logvar : ws + t.lv[1];
        r.zK = out->fused ? out->fused : ws + t.z[K];
        for (int m = 0; m < 2; ++m)
            for (int l = 0; l < IEFVAD_MAX_LAYERS; ++l) {
                r.drop[m][l] = l < L && (opt->dropout_p[m][l] > 0.f || opt->keep_mask);
                r.drop_p[m][l] = l < L ? opt->dropout_p[m][l] : 0.f;
            }
    }
    const bool splitmb = c.compute == IEFVAD_COMPUTE_BF16X6 && split_eligible(rows, IEF_D, IEF_D, 1);
    // invariant = false on purpose: the batch-invariant mode is the evaluation forward's, training keeps its own rule
    const ProjCtx px{c.compute, splitmb, IEF_D, rows, stream, &tm, h->policy.split_tile, false};
    const dim3 row_grid((rows + ROW_WAVES - 1) / ROW_WAVES);

    auto xin = [&](int m, int l) -> const float* { return l == 0 ? rec->x0[m] : ws + t.x[m][l]; };
    auto zst = [&](int k) -> float* { return k == K ? rec->zK : ws + t.z[k]; };
    // `.to(torch.float)` (imf_vad.py:41-42) into the saved layer-0 inputs; fp32 inputs are read where they are
    if (in_dtype != IEFVAD_IN_F32) {
        if (int rc = dispatch_in(in_dtype, false, [&](auto ty, auto) {
                return launch_cast<typename decltype(ty)::type>(img, ev, ws + t.x[0][0], ws + t.x[1][0], nullptr, nullptr, t.U, 2, stream);
            })) return rc;
    }
    // a plain LayerNorm of both modalities: of(m) names modality m's rows, gain, bias and result
    struct LnOne { const float* x; const float* g; const float* b; float* y; };
    auto layernorm = [&](auto of) -> int {
        LnArgs la;
        memset(&la, 0, sizeof(la));
        la.nrows = rows; la.eps = 1e-5f;
        for (int m = 0; m < 2; ++m) {
            const LnOne o = of(m);
            la.x[m] = o.x; la.g1[m] = o.g; la.b1[m] = o.b; la.y[m] = o.y;
        }
        return launch(iefvad_layernorm_kernel<IEF_D>, dim3(row_grid.x, 2), dim3(256), 0, stream, la);
    };

    for (int l = 0; l < L; ++l) {
        Proj p = Proj::of(EPI_QKV, 3 * IEF_D, 3 * IEF_D, h->in[0][l], &h->in[1][l]);
        p.qcols = IEF_D;
        p.alpha = 1.0f / sqrtf((float)IEF_DH);          // q * 1/sqrt(dh) before the bmm, as F.multi_head_attention_forward does
        for (int m = 0; m < 2; ++m) { p.A32[m] = xin(m, l); p.C[m] = ws + t.qkv[m][l]; }
        if (int rc = launch_proj(px, p, ST_QKV)) return rc;

        // bf16x6: S = q k^T -> softmax -> dropout -> Pd v in ONE launch for both modalities (attention_split.h, TRAIN: the eval kernel
        // with the sign-carrying P stored for the backward); IEFVAD_TRAIN_ATTN=unfused keeps the three launches below (A/B: the test
        // runs one model of each).  The fp32 arithmetic keeps them: its products stay on the fp32 MFMA instruction.
        AttnArgs aa;
        AttnTrainArgs tx;
        memset(&aa, 0, sizeof(aa));
        memset(&tx, 0, sizeof(tx));
        aa.nchunks = B;
        for (int m = 0; m < 2; ++m) {
            float* const qkv = ws + t.qkv[m][l];
            float* const P = ws + t.P[m][l];
            float* const att = ws + t.att[m][l];
            const float pdrop = opt->dropout_p[m][l];
            const bool drop = pdrop > 0.f || opt->keep_mask;
            const uint8_t* const keep = keep_mask_of(opt, m, l, L, t.PU);
            const unsigned long long seed = dropout_seed(opt->seed, m, l);
            if (fused) {
                aa.qkv[m] = qkv; aa.out[m] = att;
                tx.P[m] = P; tx.drop[m] = drop ? 1 : 0; tx.keep[m] = keep; tx.seed[m] = seed; tx.drop_p[m] = pdrop;
                continue;
            }
            // S = q k^T per (chunk, head)
            if (int rc = head_product(probs(P), q_of(qkv), true, k_of(qkv), true, IEF_T, IEF_T, IEF_DH, 1.f, 0.f, B, stream)) return rc;
            SoftmaxDropArgs sa;
            sa.S = P; sa.drop = drop ? 1 : 0; sa.keep = keep; sa.seed = seed; sa.p = pdrop;
            sa.rows = (long long)B * IEF_H * IEF_T;
            if (int rc = launch_softmax_dropout(sa, stream)) return rc;
            // attention output = dropout(P) v: dropout(P) from the sign-carrying tensor, in the A tile's staging
            const float a_drop = drop ? (float)(1.0 / (1.0 - (double)pdrop)) : 0.f;
            if (int rc = head_product(head_rows(att), probs(P), true, v_of(qkv), false, IEF_T, IEF_DH, IEF_T, 1.f, a_drop, B, stream)) return rc;
        }
        if (fused)
            if (int rc = launch(opt->keep_mask ? iefvad_attention_split_train_mask_kernel : iefvad_attention_split_train_kernel, dim3(IEF_H, 2, 2 * B),
                                dim3(256), ATS_LDS_BYTES, stream, aa, tx)) return rc;

        p = Proj::of(EPI_BIAS_RESID, IEF_D, IEF_D, h->out[0][l], &h->out[1][l]);
        for (int m = 0; m < 2; ++m) { p.A32[m] = ws + t.att[m][l]; p.C[m] = ws + t.s[m][l]; p.R[m] = xin(m, l); }
        if (int rc = launch_proj(px, p, ST_OUT)) return rc;
        if (int rc = layernorm([&](int m) { return LnOne{ws + t.s[m][l], h->norm_w[m][l], h->norm_b[m][l], ws + t.x[m][l + 1]}; })) return rc;
    }
    // whitening LayerNorm (imf_vad.py:117,123) as a launch of its own: the backward needs its input, the last norm's output
    if (int rc = layernorm([&](int m) { return LnOne{ws + t.x[m][L], h->whiten_w[m], h->whiten_b[m], ws + t.E[m]}; })) return rc;
    {
        Proj p = Proj::of(EPI_HEADS, 2 * IEF_D, IEF_D, h->head[0], &h->head[1]);
        for (int m = 0; m < 2; ++m) { p.A32[m] = ws + t.E[m]; p.C[m] = rec->mu[m]; p.C2[m] = rec->lv[m]; }
        if (int rc = launch_proj(px, p, ST_HEAD)) return rc;
    }
    {
        FusionArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.mu_i = rec->mu[0]; fa.lv_i = rec->lv[0]; fa.mu_e = rec->mu[1]; fa.lv_e = rec->lv[1];
        fa.n_i = out->w_i; fa.n_e = out->w_e; fa.z = zst(0);
        fa.n_i_mean = out->w_i_mean; fa.n_e_mean = out->w_e_mean;
        fa.nrows = rows; fa.factor = precision_factor(c); fa.eps = c.epsilon;
        if (int rc = launch(iefvad_fusion_kernel<IEF_D>, row_grid, dim3(256), 0, stream, fa)) return rc;
    }
    for (int k = 0; k < K; ++k) {
        Proj p = Proj::of(EPI_BIAS_RELU, IEF_D, IEF_D, h->ref1[k]);
        p.A32[0] = zst(k); p.C[0] = ws + t.hid[k];
        if (int rc = launch_proj(px, p, ST_REFINE)) return rc;
        p = Proj::of(EPI_REFINE, IEF_D, IEF_D, h->ref2[k]);
        p.alpha = c.lambda_ref;
        p.A32[0] = ws + t.hid[k]; p.C[0] = zst(k + 1); p.R[0] = zst(k);
        if (int rc = launch_proj(px, p, ST_REFINE)) return rc;
    }
    float* logits = out->logits ? out->logits : ws + t.logits;
    // (the dict entries of imf_vad.py:152-161 that are also saved tensors were written in place: TrainRecord)
    return launch(iefvad_scorer_kernel<IEF_D>, row_grid, dim3(256), 0, stream, rec->zK, h->cls_w, h->cls_b, logits, rows);
}

// ---- backward -------------------------------------------------------------------------------------------------------------------------
// One walk serves both entries (`who` names the caller's in the messages).  `dx` (nullable, each member nullable): the gradients of the
// input features, the layer-0 instance of the d x product every layer above it runs.  A frozen model hands a `dw` of null pointers:
// launch_dw / launch_db return before any launch for null destinations and ReduceBatch skips them, so what remains is the chain of
// d x products, the attention backward and the row kernels (whose partial sums for the affine gradients are by-products nobody reduces).
static int train_backward(iefvad_handle* h, int32_t B, void* train_ws, size_t train_ws_bytes, const iefvad_output_grads* dout,
                          const iefvad_weight_grads* dw, const iefvad_input_grads* dxin, void* stream_, const char* who) {
    if (!h) return fail("%s: null handle", who);
    float* dx[2] = {dxin ? dxin->img : nullptr, dxin ? dxin->ev : nullptr};      // checked before the handle is looked at
    if (((uintptr_t)dx[0] | (uintptr_t)dx[1]) & 15) return fail("%s: input-gradient buffers must be 16-byte aligned", who);
    if (h->D != IEF_D) return fail("%s: training is built for D=768 (this handle has D=%d)", who, h->D);
    if (!dout || !dw) return fail("%s: null argument", who);
    TrainRecord* live = nullptr;
    if (h->train)
        for (int i = 0; i < 8; ++i)
            if (h->train->rec[i].ws == train_ws && h->train->rec[i].stamp) live = &h->train->rec[i];
    if (!live || live->B != B) return fail("%s: no iefvad_train_forward with B = %d has filled this training buffer", who, B);
    if (int rc = train_check(h, B, train_ws, train_ws_bytes, who)) return rc;
    // The scratch tensors overwrite the saved refinement states (train_layout): the forward's record is retired HERE, before the first
    // launch, so that a backward that fails midway leaves no live record over clobbered data.  `rec` is this call's copy.
    const TrainRecord taken = *live;
    const TrainRecord* rec = &taken;
    live->stamp = 0;
    const iefvad_config& c = h->cfg;
    const int L = c.num_layers, K = c.num_steps;
    hipStream_t stream = (hipStream_t)stream_;
    const TrainLayout t = train_layout(L, K, B);
    float* ws = (float*)train_ws;
    const int rows = B * IEF_T;
    const int nblk = bwd_row_blocks(rows);
    const float qscale = 1.0f / sqrtf((float)IEF_DH);
    float* rpart = ws + t.rpart;
    float* g = ws + t.g;
    float* da = ws + t.da;
    if (int rc = ensure_train_planes(h, stream)) return rc;
    const bool x6 = c.compute == IEFVAD_COMPUTE_BF16X6;
    const BwdCtx bx{h, rows, stream, ws + t.part, t.part_floats, ws + t.cpart, t.cpart_floats, x6, x6 && h->tplanes_valid};

    // classifier (imf_vad.py:150)
    {
        ScorerBwdArgs sa;
        sa.dlogit = dout->logits; sa.dfused = dout->fused; sa.z = rec->zK; sa.w = h->cls_w; sa.g = g;
        sa.part_w = rpart; sa.part_b = rpart + (size_t)nblk * IEF_D; sa.rows = rows;
        if (int rc = launch_scorer_bwd(sa, stream)) return rc;
        ReduceBatch rb;
        rb.add(rpart, (size_t)IEF_D, nblk, (size_t)IEF_D, dw->cls_w, 1.f);
        rb.add(rpart + (size_t)nblk * IEF_D, (size_t)1, nblk, (size_t)1, dw->cls_b, 1.f);
        if (int rc = rb.launch(stream)) return rc;
    }
    // refinement steps, last to first (imf_vad.py:146-149): z_{k+1} = z_k - lambda (W2 relu(W1 z_k + b1) + b2); g = d z_{k+1}
    for (int k = K - 1; k >= 0; --k) {
        const float nl = -c.lambda_ref;
        float* const hid = ws + t.hid[k];
        if (int rc = linear_param_grads(bx, LinearGrads{g, &h->ref2[k], hid, nl, dw->ref_w2[k], dw->ref_b2[k]})) return rc;
        // d a = (-lambda g W2) gated by h > 0  (ReLU backward on the saved activation)
        if (int rc = launch_dx(bx, h->ref2[k], g, da, nullptr, hid, nl)) return rc;
        if (int rc = linear_param_grads(bx, LinearGrads{da, &h->ref1[k], ws + t.z[k], 1.f, dw->ref_w1[k], dw->ref_b1[k]})) return rc;
        // d z_k = g + d a W1   (in place: every element of g is read by the thread that overwrites it)
        if (int rc = launch_dx(bx, h->ref1[k], da, g, g, nullptr, 1.f)) return rc;
    }
    // fusion (imf_vad.py:130-144) -> d mu | d logvar of both modalities, stacked
    {
        FusionBwdArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.mu_i = rec->mu[0]; fa.lv_i = rec->lv[0]; fa.mu_e = rec->mu[1]; fa.lv_e = rec->lv[1];
        fa.gz = g;
        fa.d_mu_i = dout->image_mu; fa.d_lv_i = dout->image_logvar; fa.d_mu_e = dout->event_mu; fa.d_lv_e = dout->event_logvar;
        fa.d_n_i = dout->w_i; fa.d_n_e = dout->w_e;
        fa.dh_i = ws + t.dh[0]; fa.dh_e = ws + t.dh[1];
        fa.rows = rows; fa.factor = precision_factor(c); fa.eps = c.epsilon;
        if (int rc = launch_fusion_bwd(fa, stream)) return rc;
    }
    for (int m = 0; m < 2; ++m) {
        const float* dhm = ws + t.dh[m];
        float* gx = ws + t.gx;
        // heads (imf_vad.py:125-128): mu.weight | logvar.weight are stacked [1536, 768] in the handle
        if (int rc = linear_param_grads(bx, LinearGrads{dhm, &h->head[m], ws + t.E[m], 1.f, dw->mu_w[m], dw->mu_b[m], dw->logvar_w[m], dw->logvar_b[m], IEF_D}))
            return rc;
        if (int rc = launch_dx(bx, h->head[m], dhm, gx, nullptr, nullptr, 1.f)) return rc;
        // whitening LayerNorm (imf_vad.py:117,123), then the layers last to first
        auto ln_bwd = [&](const float* x, const float* gamma, float* dgamma, float* dbeta) -> int {
            LnBwdArgs la;
            la.x = x; la.dy = gx; la.g = gamma; la.dx = gx; la.part_g = rpart; la.part_b = rpart + (size_t)nblk * IEF_D; la.rows = rows; la.eps = 1e-5f;
            if (int rc = launch_layernorm_bwd(la, stream)) return rc;
            ReduceBatch rb;
            rb.add(rpart, (size_t)IEF_D, nblk, (size_t)IEF_D, dgamma, 1.f);
            rb.add(rpart + (size_t)nblk * IEF_D, (size_t)IEF_D, nblk, (size_t)IEF_D, dbeta, 1.f);
            return rb.launch(stream);
        };
        if (int rc = ln_bwd(ws + t.x[m][L], h->whiten_w[m], dw->whiten_w[m], dw->whiten_b[m])) return rc;
        for (int l = L - 1; l >= 0; --l) {
            // x_{l+1} = LayerNorm(s_l), s_l = x_l + out_proj(attention(x_l))   (imf_vad.py:115-116)
            if (int rc = ln_bwd(ws + t.s[m][l], h->norm_w[m][l], dw->norm_w[m][l], dw->norm_b[m][l])) return rc;
            // gx = d s_l
            float* datt = ws + t.datt;
            float* dqkv = ws + t.dqkv;
            float* dP = ws + t.dP;
            float* qkv = ws + t.qkv[m][l];
            float* P = ws + t.P[m][l];
            // P carries the dropout mask in its sign bits (when a probability or a mask was in force in the forward): dropout(P) is formed
            // from it where it is read (the d S launch / the softmax backward, the A operand of d v)
            const bool signed_p = rec->drop[m][l];
            const float drop_scale = signed_p ? (float)(1.0 / (1.0 - (double)rec->drop_p[m][l])) : 1.0f;
            if (int rc = linear_param_grads(bx, LinearGrads{gx, &h->out[m][l], ws + t.att[m][l], 1.f, dw->out_proj_w[m][l], dw->out_proj_b[m][l]})) return rc;
            // layer 0 of a modality whose in_proj gradients and input gradient are all unasked for: nothing reads its d qkv
            if (l == 0 && !dx[m] && !dw->in_proj_w[m][0] && !dw->in_proj_b[m][0]) break;
            if (int rc = launch_dx(bx, h->out[m][l], gx, datt, nullptr, nullptr, 1.f)) return rc;
            // bf16x6: d S = Pd .* d Pd - P rowsum(Pd .* d Pd) with d Pd = d att v^T in ONE launch (attention_split.h, BWD: the product on the
            // split arithmetic, the softmax backward on its accumulators); after an IEFVAD_TRAIN_ATTN=unfused forward the product stays on
            // the fp32 MFMA kernel with the stand-alone softmax backward (A/B)
            const bool ds_fused = rec->fused;
            if (ds_fused) {
                AttnArgs aa;
                AttnTrainArgs tx;
                memset(&aa, 0, sizeof(aa));
                memset(&tx, 0, sizeof(tx));
                aa.nchunks = B;
                aa.qkv[0] = qkv;
                tx.dO[0] = datt; tx.P[0] = P; tx.drop[0] = signed_p ? 1 : 0; tx.drop_p[0] = rec->drop_p[m][l]; tx.dS[0] = dP;
                tx.dQ[0] = dqkv; tx.q_scale = qscale;
                if (int rc = launch(iefvad_attention_split_ds_kernel, dim3(IEF_H, 2, B), dim3(256), ATS_LDS_BYTES, stream, aa, tx)) return rc;
            } else {
                // d Pd = d att v^T
                if (int rc = head_product(probs(dP), head_rows(datt), true, v_of(qkv), true, IEF_T, IEF_T, IEF_DH, 1.f, 0.f, B, stream)) return rc;
            }
            // d v = Pd^T d att
            if (int rc = head_product(v_of(dqkv), probs(P), false, head_rows(datt), false, IEF_T, IEF_DH, IEF_T, 1.f, signed_p ? drop_scale : 0.f, B, stream))
                return rc;
            if (!ds_fused) {
                // d S = Pd .* d Pd - P rowsum(Pd .* d Pd)
                const long long srows = (long long)B * IEF_H * IEF_T;
                if (int rc = launch_softmax_bwd(P, drop_scale, dP, srows, stream)) return rc;
                // d q (before the 1/sqrt(96) scale) = qscale * d S k  (ds_fused: done by the same launch, on the d S in its registers)
                if (int rc = head_product(q_of(dqkv), probs(dP), true, k_of(qkv), false, IEF_T, IEF_DH, IEF_T, qscale, 0.f, B, stream)) return rc;
            }
            // d k = d S^T q_scaled
            if (int rc = head_product(k_of(dqkv), probs(dP), false, q_of(qkv), false, IEF_T, IEF_DH, IEF_T, 1.f, 0.f, B, stream)) return rc;
            // in_proj (packed q | k | v, imf_vad.py:69-72)
            const float* xl = l == 0 ? rec->x0[m] : ws + t.x[m][l];
            if (int rc = linear_param_grads(bx, LinearGrads{dqkv, &h->in[m][l], xl, 1.f, dw->in_proj_w[m][l], dw->in_proj_b[m][l]})) return rc;
            // d x_l = d s_l (residual) + d qkv W_in: in place for the layers above the first; at layer 0 it is the gradient of the input
            // features, written to the caller's buffer where one is given (gx is only read there)
            float* dxl = l > 0 ? gx : dx[m];
            if (dxl)
                if (int rc = launch_dx(bx, h->in[m][l], dqkv, dxl, gx, nullptr, 1.f)) return rc;
        }
    }
    return 0;
}

extern "C" int iefvad_train_backward(iefvad_handle* h, int32_t B, void* train_ws, size_t train_ws_bytes, const iefvad_output_grads* dout,
                                     const iefvad_weight_grads* dw, void* stream) {
    return train_backward(h, B, train_ws, train_ws_bytes, dout, dw, nullptr, stream, "iefvad_train_backward");
}

extern "C" int iefvad_train_backward_inputs(iefvad_handle* h, int32_t B, void* train_ws, size_t train_ws_bytes,
                                            const iefvad_output_grads* dout, const iefvad_weight_grads* dw,
                                            const iefvad_input_grads* dx, void* stream) {
    return train_backward(h, B, train_ws, train_ws_bytes, dout, dw, dx, stream, "iefvad_train_backward_inputs");
}

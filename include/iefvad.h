/*
 * iefvad.h -- C ABI of libiefvad.so: the MI355X (gfx950) implementation of IEF-VAD's
 * uncertainty-weighted image-event fusion inference forward.
 *
 * The reference has NO native/FFI/plugin boundary for this path: the boundary is a Python
 * nn.Module call, `outputs = model(img, ev, padding_mask, text, lengths)`
 * (/root/reference/test.py:111-117, train/ucf_test.py:104-110, train/xd_test.py:98-104,
 * test2.py:62,79), implemented by `MMFMIL.forward` -> `MultiModal_Fusion_Attn_Iter.forward`
 * (/root/reference/model/imf_vad.py:40-44, :109-161).  The entry points below are what a
 * Python `MMFMIL` shim binds with ctypes to replace that forward; INTEGRATION.md shows the
 * binding.  Plain C types only: pointers are DEVICE pointers (HIP), sizes are in elements
 * or bytes as stated, the stream is a `hipStream_t` passed as `void*`.
 *
 * Ownership: the caller allocates and owns every input, output and workspace buffer.  The
 * library owns the handle and its repacked copies of the weights.
 * Errors: every int-returning function returns 0 on success, non-zero on failure, and never
 * throws or aborts across the ABI; `iefvad_last_error()` returns a thread-local message.
 * Threading: a handle is bound to the device current at `iefvad_create` and is not
 * re-entrant; kernels are enqueued on the caller's stream and the call returns without
 * synchronising.
 */
#ifndef IEFVAD_H
#define IEFVAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IEFVAD_ABI_VERSION 8
#define IEFVAD_MAX_LAYERS 8   /* args.visual_layers (reference default 2, parser.py:5)            */
#define IEFVAD_MAX_STEPS 64   /* args.num_refinement_steps (reference default 10, test.py:406)    */

/* noise_model of MultiModal_Fusion_Attn_Iter (/root/reference/model/imf_vad.py:130-138) */
enum { IEFVAD_NOISE_GAUSSIAN = 0, IEFVAD_NOISE_STUDENT_T = 1 };
/* element type of the img / ev feature blocks handed to iefvad_forward (the reference casts
 * whatever arrives with `.to(torch.float)`, imf_vad.py:41-42) */
enum { IEFVAD_IN_F32 = 0, IEFVAD_IN_F16 = 1, IEFVAD_IN_BF16 = 2 };
/* arithmetic of the dense projections:
 *   F32    = fp32 MFMA (v_mfma_f32_32x32x2_f32), bit-reproducible across batch sizes (parity mode);
 *   BF16   = operands rounded to bf16, fp32 accumulation and fp32 fusion state (throughput mode);
 *   BF16X6 = fp32 operands, each split exactly into three bf16 terms and multiplied as six bf16 MFMA
 *            products with fp32 accumulation: fp32-accurate (held to the F32 mode's tolerances, product
 *            error <= 2^-23 relative worst case, ~2^-27 typical) at the bf16 matrix-core rate; everything else is the F32 path.
 *            Small batches (grids that would not fill the chip) use the F32 kernels, so results are
 *            fp32-accurate but not bit-identical across batch sizes in this mode.
 *   FP16X3 = opt-in, near-fp32: the BF16X6 data flow with two fp16 terms per operand and three products per
 *            multiply-add (22-bit products, half the MFMAs).  Operands are scaled by powers of two from running
 *            max |.| words that the producing kernels maintain, so the result is range-safe; error against fp64 is
 *            ~1.8x the fp32 MFMA path's (rms) per projection, below it end to end. */
enum { IEFVAD_COMPUTE_F32 = 0, IEFVAD_COMPUTE_BF16 = 1, IEFVAD_COMPUTE_BF16X6 = 2, IEFVAD_COMPUTE_FP16X3 = 3 };

typedef struct iefvad_handle iefvad_handle;

/* Replaces the constructor arguments that reach the computation:
 * MMFMIL.__init__ -> MultiModal_Fusion_Attn_Iter(embed_dim, num_layers, num_heads,
 * num_refinement_steps, lambda_ref, noise_model, nu) (/root/reference/model/imf_vad.py:30-38),
 * plus epsilon (always 1e-8 in the reference, :58) and visual_length T. */
typedef struct iefvad_config {
    int32_t abi_version;   /* IEFVAD_ABI_VERSION */
    int32_t embed_dim;     /* D: 768 (iefvad_create), or 768 / 512 (iefvad_create_ex; 512 with compute = IEFVAD_COMPUTE_F32) */
    int32_t seq_len;       /* T, must be 256 */
    int32_t num_heads;     /* H, must be 8 (head dim 96 at D = 768, 64 at D = 512) */
    int32_t num_layers;    /* L, 1..IEFVAD_MAX_LAYERS */
    int32_t num_steps;     /* K, 0..IEFVAD_MAX_STEPS */
    int32_t noise_model;   /* IEFVAD_NOISE_* */
    int32_t compute;       /* IEFVAD_COMPUTE_* */
    float lambda_ref;
    float nu;
    float epsilon;
    int32_t micro_batch;   /* chunks processed per internal pass; 0 = library default */
    int32_t graph_chunks;  /* calls with B <= graph_chunks replay a cached hipGraph of the forward (the reference's
                              per-video pattern, /root/reference/test.py:76-117: B = 1 .. a few chunks, 31 launches of a
                              few microseconds each, host-bound when launched one by one); 0 = library default (8),
                              negative = never.  Results are bit-identical to the direct launches. */
} iefvad_config;

/* Device pointers to the reference's state_dict tensors, fp32, laid out
 * as torch stores them: Linear.weight is [out, in] row-major.  Index 0 = image, 1 = event.
 * Replaces `model.load_state_dict(...)` (/root/reference/test.py:377-378). */
typedef struct iefvad_weights {
    const float* in_proj_w[2][IEFVAD_MAX_LAYERS];   /* {m}_attn_layers.l.in_proj_weight [3D, D] */
    const float* in_proj_b[2][IEFVAD_MAX_LAYERS];   /* ....in_proj_bias   [3D] */
    const float* out_proj_w[2][IEFVAD_MAX_LAYERS];  /* ....out_proj.weight [D, D] */
    const float* out_proj_b[2][IEFVAD_MAX_LAYERS];  /* ....out_proj.bias   [D] */
    const float* norm_w[2][IEFVAD_MAX_LAYERS];      /* {m}_norms.l.weight [D] */
    const float* norm_b[2][IEFVAD_MAX_LAYERS];      /* {m}_norms.l.bias   [D] */
    const float* whiten_w[2];                       /* whiten_{m}.weight [D] */
    const float* whiten_b[2];                       /* whiten_{m}.bias   [D] */
    const float* mu_w[2];                           /* {m}_mu.weight [D, D] */
    const float* mu_b[2];                           /* {m}_mu.bias   [D] */
    const float* logvar_w[2];                       /* {m}_logvar.weight [D, D] */
    const float* logvar_b[2];                       /* {m}_logvar.bias   [D] */
    const float* ref_w1[IEFVAD_MAX_STEPS];          /* refinement_blocks.k.0.weight [D, D] */
    const float* ref_b1[IEFVAD_MAX_STEPS];          /* refinement_blocks.k.0.bias   [D] */
    const float* ref_w2[IEFVAD_MAX_STEPS];          /* refinement_blocks.k.2.weight [D, D] */
    const float* ref_b2[IEFVAD_MAX_STEPS];          /* refinement_blocks.k.2.bias   [D] */
    const float* cls_w;                             /* classifier.weight [1, D] */
    const float* cls_b;                             /* classifier.bias   [1] */
} iefvad_weights;

/* Device output buffers; every pointer is optional (NULL = not materialised).  The eight
 * dict entries of the reference's return value (/root/reference/model/imf_vad.py:152-161),
 * all fp32, row-major [B*T, D] (logits: [B*T]), plus the per-row means over D of w_i / w_e
 * that the harness derives on the host (/root/reference/test.py:131-136). */
typedef struct iefvad_outputs {
    float* fused;         /* [B*T, D] */
    float* logits;        /* [B*T]    */
    float* image_mu;      /* [B*T, D] */
    float* event_mu;      /* [B*T, D] */
    float* image_logvar;  /* [B*T, D] */
    float* event_logvar;  /* [B*T, D] */
    float* w_i;           /* [B*T, D]  normalised image weight */
    float* w_e;           /* [B*T, D]  normalised event weight */
    float* w_i_mean;      /* [B*T]     mean over D of w_i */
    float* w_e_mean;      /* [B*T]     mean over D of w_e */
} iefvad_outputs;

/* Per-stage device time of the last iefvad_forward_timed call, milliseconds (hipEvents on the
 * caller's stream).  Measurement aid for bench.py's roofline block. */
typedef struct iefvad_stage_times {
    float total_ms;
    float qkv_gemm_ms;
    float attention_ms;
    float out_gemm_ms;
    float layernorm_ms;
    float head_gemm_ms;
    float fusion_ms;
    float refine_gemm_ms;
    float scorer_ms;
    float cast_ms;           /* input casts and bf16 operand copies */
    int32_t gemm_launches;   /* number of dense-projection GEMM launches in the pass */
} iefvad_stage_times;

int iefvad_abi_version(void);

/* Build a handle on the current HIP device.  Unsupported dimensions or noise_model -> error.  embed_dim must be 768. */
int iefvad_create(const iefvad_config* cfg, iefvad_handle** out);

/* As iefvad_create, and embed_dim may also be 512 (head dim 64) with compute = IEFVAD_COMPUTE_F32: the ViT-B/16 features of the
 * reference's `--ds vitb_rgb` model.  Such a handle runs the evaluation forward -- iefvad_forward / _scaled / _timed, the hipGraph
 * replay, iefvad_forward_videos and iefvad_forward_videos_host (D = 512 rows everywhere) -- and the training entries and
 * iefvad_rowblock_unit refuse it by name.  Every check runs before the first HIP call.  For D = 768 it is iefvad_create. */
int iefvad_create_ex(const iefvad_config* cfg, iefvad_handle** out);

/* Copy/repack the weights into library-owned device memory (stream-ordered on `stream`). */
int iefvad_set_weights(iefvad_handle* h, const iefvad_weights* w, void* stream);

/* Bytes of caller-provided scratch that iefvad_forward needs for a call with B chunks. */
size_t iefvad_workspace_bytes(const iefvad_handle* h, int32_t B);

/* The forward: img, ev are device pointers to [B, T, D] blocks of `in_dtype`, contiguous.
 * Enqueues on `stream` (hipStream_t) and returns without synchronising. */
int iefvad_forward(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B,
                   void* workspace, size_t workspace_bytes, const iefvad_outputs* out, void* stream);

/* Same forward, bracketing each stage with hipEvents; synchronises the stream before returning. */
int iefvad_forward_timed(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B,
                         void* workspace, size_t workspace_bytes, const iefvad_outputs* out, void* stream,
                         iefvad_stage_times* times);

/* ---- whole videos --------------------------------------------------------------------------------------------------
 * The hot loop of the reference's evaluation, one level up from the forward: for every video the loader pads the [len, D]
 * feature files to whole T = 256 chunks on the host (process_split, /root/reference/data/tools.py:100-114; dataset.py:34-52),
 * test() scans the padded tensors for NaN and replaces them (`if torch.isnan(x).any(): x = torch.nan_to_num(x, nan=0.0)`,
 * /root/reference/test.py:90-95), runs the model on every chunk row and keeps `logits.reshape(-1)[0:len]`
 * (test.py:119-121) and the first len row means of w_i / w_e (test.py:131-138).  iefvad_forward_videos does exactly that
 * for a batch of videos with only the VALID rows crossing the boundary:
 *   img_rows, ev_rows   device, [sum(lengths), D] of `in_dtype`: the videos' feature rows concatenated in list order (no padding)
 *   lengths             HOST array of nvideos snippet counts (>= 1)
 *   nan_to_num          non-zero: the conditional replacement above, decided per WHOLE video and per modality on the device: every
 *                       chunk of the call is scanned before the first micro-batch pass lays out its rows, so a video that
 *                       straddles passes is treated as the reference treats its one tensor
 *                       (NaN -> 0, +-inf -> the largest / smallest finite value of `in_dtype`); zero: rows are used as they are
 *   logits, w_i_mean, w_e_mean   device, [sum(lengths)] fp32 each, the means nullable: per-snippet results in the same order
 * Chunks are laid out on the device (zero padded; the all-zero chunk that process_split appends to a len % 256 == 0 video,
 * whose rows test.py:121 slices away, is not built).  Attention is unmasked over the padded window, as in the reference,
 * but the pad rows of a window are identical in every layer: the row set holds ONE of them per chunk, the row-wise stages
 * (projections, LayerNorms and everything behind the encoder, imf_vad.py:125-150) run on valid + 1 rows per chunk, and the
 * attention kernels read row min(r, valid) for row r of the window -- every product and sum of the padded computation.
 * Results equal those of iefvad_forward on the host-padded chunks (bit for bit in the F32 and BF16 modes).  FP16X3 (one
 * operand scale per whole chunk) and IEFVAD_DENSE_ENCODER=1 (environment, read at iefvad_create) keep whole chunks in the
 * encoder and gather the valid rows behind it.
 * Workspace: iefvad_videos_workspace_bytes.  Enqueued on `stream`; `lengths` is consumed before the call returns. */
size_t iefvad_videos_workspace_bytes(const iefvad_handle* h, const int32_t* lengths, int32_t nvideos);
int iefvad_forward_videos(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype,
                          const int32_t* lengths, int32_t nvideos, int32_t nan_to_num, void* workspace,
                          size_t workspace_bytes, float* logits, float* w_i_mean, float* w_e_mean, void* stream);

/* iefvad_forward_videos for the robustness sweep (/root/reference/test2.py:35-123: twelve levels over one list): the same call, plus
 *   nan_to_num          gains the value 2: torch.nan_to_num on EVERY video and modality (test2.py:59-60; NaN -> 0, +-inf -> the
 *                       largest / smallest finite value of `in_dtype`), with no scan and no flag words.  0 and 1 as above; any other
 *                       value is refused
 *   img_row_scale, ev_row_scale   DEVICE fp32 [sum(lengths)], each nullable, indexed by the packed row of the CALL: packed row r of
 *                       modality m enters the model as x[r] * scale_m[r] (test2.py:70-77's `x[:, idx] * 0.01` on valid rows), the
 *                       product formed as iefvad_forward_scaled forms it (fp32, rounded to `in_dtype` before the widening; a scale
 *                       of exactly 1, or a NULL vector, leaves the row's bits alone) and AFTER the NaN rule; pad rows are the zeros
 *                       the library writes and are not scaled
 *   w_colsum            DEVICE [2, D] doubles (8-byte aligned), nullable: on return (stream-ordered) w_colsum[0][d] is the sum over
 *                       all valid rows of the call of w_i[r][d], w_colsum[1][d] the same for w_e (test2.py:86-87,102-103): the fp32
 *                       values the fusion stage stores, added in fp64, per-slab partial sums finished in a fixed order without
 *                       atomics (the same call gives the same bits).  Pad rows and tile-rounding rows are not included.  The buffer
 *                       is overwritten.
 * Workspace: iefvad_videos_scaled_workspace_bytes(h, lengths, nvideos, with_colsum) -- with_colsum != 0 adds a home for the w_i / w_e
 * rows of one pass and the slab partials; with w_colsum == NULL the size of iefvad_videos_workspace_bytes is enough.  With
 * w_colsum == NULL and both scale vectors NULL (and nan_to_num 0 or 1) the call launches exactly what iefvad_forward_videos launches.
 * Per-snippet results equal those of iefvad_forward_scaled on the host-padded chunks, as above.  D = 512 handles are served.
 * Added without a change to any other entry or struct: IEFVAD_ABI_VERSION stays. */
size_t iefvad_videos_scaled_workspace_bytes(const iefvad_handle* h, const int32_t* lengths, int32_t nvideos, int32_t with_colsum);
int iefvad_forward_videos_scaled(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype,
                                 const int32_t* lengths, int32_t nvideos, int32_t nan_to_num, const float* img_row_scale,
                                 const float* ev_row_scale, void* workspace, size_t workspace_bytes, float* logits,
                                 float* w_i_mean, float* w_e_mean, double* w_colsum, void* stream);

/* The whole evaluation LIST in one call: host rows in, per-snippet results on the device.  Replaces the Python loop around
 * iefvad_forward_videos (one iteration per video in the reference, /root/reference/test.py:76-121; one per packed batch in this
 * package until round 3): the library cuts the list into passes of >= batch_chunks chunks (whole videos; 0 = 128), a worker thread
 * gathers the rows of the next passes into a ring of four pinned staging slots (host_threads copy threads, 0 = 8, at most 16) while
 * this thread sends pass k on an internal copy stream and enqueues its forward on one of TWO internal non-blocking compute streams
 * (alternating; both wait for what `stream` held at entry, and `stream` waits for both before the call returns); results land in
 * list order.
 *   img_rows, ev_rows   HOST arrays of nvideos HOST pointers: video v's [lengths[v], D] feature rows of `in_dtype`, contiguous
 *                       (e.g. the first lengths[v] rows of the zero-padded tensor a DataLoader delivers)
 *   wire_dtype          the element type the rows cross PCIe in: `in_dtype` (the rows as they are), or IEFVAD_IN_BF16 for F32 rows
 *                       on a BF16-mode handle -- the throughput mode's down-conversion on the wire: the gather
 *                       threads round to bf16 (nearest even, as the device would) while they stage, half the bytes are copied, and the
 *                       forward runs as iefvad_forward_videos does on IEFVAD_IN_BF16 rows.  The bf16 mode rounds these rows for its
 *                       first projection anyway; what changes is the first layer's residual, which reads the rounded row too
 *                       (and nan_to_num's +-inf replacement is the bf16 extreme).  Other combinations are refused.
 *   logits, w_i_mean, w_e_mean   DEVICE, [sum(lengths)] fp32 each (the means nullable), valid once `stream` has run
 * Returns when every pass has been enqueued and every host row has been read (the caller's host tensors are free again);
 * staging slots, device input slots and the workspace belong to the handle.  Same results as iefvad_forward_videos on the
 * same batches. */
int iefvad_forward_videos_host(iefvad_handle* h, const void* const* img_rows, const void* const* ev_rows, int32_t in_dtype,
                               int32_t wire_dtype, const int32_t* lengths, int32_t nvideos, int32_t nan_to_num, int32_t batch_chunks,
                               int32_t host_threads, float* logits, float* w_i_mean, float* w_e_mean, void* stream);

/* The two whole-video entries above with the four similarity series of the reference's plots (test.py:235-238; iefvad_similarity_rows
 * below) of every valid snippet as a further result -- what a vis=True evaluation needs, without a D-wide tensor leaving the library
 * and without computing the padding.  The arguments of iefvad_forward_videos / iefvad_forward_videos_host, then
 *   similarity          DEVICE [4, sum(lengths)] fp32, series-major (cos_i, cos_e, dist_i, dist_e: the layout iefvad_similarity_rows
 *                       writes with nout = sum(lengths)), 4-byte aligned, not NULL; column r is packed row r of the call (of the whole
 *                       list for the host entry: every pass writes at its own row offset).  Valid once `stream` has run.
 * A pass keeps fused (= z_K), image_mu and event_mu of its row set in its workspace -- the heads stage stores mu where a score-only
 * pass would not, the last refinement step forms z_K where a score-only pass folds it into the scorer -- and one launch of
 * iefvad_similarity_rowset_kernel (csrc/similarity.h) reduces the valid rows before the pass ends; pad rows and tile-rounding rows are
 * not read.  The kernel shares its row arithmetic with iefvad_similarity_rows: in the f32, bf16 and fp16x3 arithmetics the series
 * equal, bit for bit, those of iefvad_similarity_rows on the outputs of iefvad_forward on the host-padded chunks.  logits, w_i_mean
 * and w_e_mean are the bits of the entry without `similarity`, in every arithmetic.  Workspace: iefvad_videos_workspace_bytes, no
 * more.  Served: every arithmetic, D = 768 and 512, the three input dtypes, videos that straddle micro-batch passes,
 * IEFVAD_DENSE_ENCODER=1.  A NULL or misaligned `similarity`, an unknown in_dtype and nvideos <= 0 are refused by name before the
 * handle is looked at.  NOT covered: iefvad_forward_videos_scaled (row scales, w_colsum) takes no `similarity`.
 * Added without a change to any other entry or struct: IEFVAD_ABI_VERSION stays. */
int iefvad_forward_videos_similarity(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype,
                                     const int32_t* lengths, int32_t nvideos, int32_t nan_to_num, void* workspace,
                                     size_t workspace_bytes, float* logits, float* w_i_mean, float* w_e_mean, void* stream,
                                     float* similarity);
int iefvad_forward_videos_host_similarity(iefvad_handle* h, const void* const* img_rows, const void* const* ev_rows, int32_t in_dtype,
                                          int32_t wire_dtype, const int32_t* lengths, int32_t nvideos, int32_t nan_to_num,
                                          int32_t batch_chunks, int32_t host_threads, float* logits, float* w_i_mean, float* w_e_mean,
                                          void* stream, float* similarity);

/* The two whole-video entries with the reference's full output dict (imf_vad.py:152-161) of every valid snippet: what the padded route
 * returns through an iefvad_outputs, without computing or writing the padding.  The arguments of iefvad_forward_videos /
 * iefvad_forward_videos_host with the three result pointers replaced by
 *   out                 device buffers in PACKED order (row r = packed row r of the call; of the whole list for the host entry, every
 *                       pass writes at its own row offset): logits, w_i_mean, w_e_mean [sum(lengths)] fp32; fused, image_mu, event_mu,
 *                       image_logvar, event_logvar, w_i, w_e [sum(lengths), D] fp32, 16-byte aligned.  logits is required, every other
 *                       pointer is optional and any subset is valid; a NULL tensor is neither computed for the caller nor written.
 * A pass keeps the asked-for tensors of its row set -- mu / logvar / fused (= z_K) in its workspace, as the similarity entries keep
 * theirs, w_i / w_e behind the base workspace, where the scaled entry keeps them -- and one launch of iefvad_rows_out_wide_kernel
 * (csrc/ragged.h) behind the pass's scores copies the valid rows to the caller's tensors; pad rows and tile-rounding rows are not read.
 * In the f32, bf16 and fp16x3 arithmetics every tensor equals, bit for bit, the `[0:len]` rows of iefvad_forward on the host-padded
 * chunks; logits, w_i_mean and w_e_mean are the bits of the plain entries in every arithmetic.  Workspace:
 * iefvad_videos_full_workspace_bytes(h, lengths, nvideos, out) -- the plain size, plus [2, R, D] floats (R = rows of one pass's chunks)
 * when out->w_i or out->w_e is set (out == NULL: the plain size); a smaller workspace is refused by name before anything is launched.
 * The host entry's two lanes each own such a workspace.  Served: every arithmetic, D = 768 and 512, the three input dtypes, videos
 * that straddle micro-batch passes, IEFVAD_DENSE_ENCODER=1.  A NULL handle, a NULL out, a NULL out->logits and a misaligned [rows, D]
 * tensor are refused by name before any HIP call.  NOT covered: the full entries do not combine with iefvad_forward_videos_scaled
 * (row scales, nan_to_num = 2, w_colsum) or with the similarity entries -- reduce the returned rows with iefvad_similarity_rows instead.
 * Added without a change to any other entry or struct: IEFVAD_ABI_VERSION stays. */
size_t iefvad_videos_full_workspace_bytes(const iefvad_handle* h, const int32_t* lengths, int32_t nvideos, const iefvad_outputs* out);
int iefvad_forward_videos_full(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype, const int32_t* lengths,
                               int32_t nvideos, int32_t nan_to_num, void* workspace, size_t workspace_bytes, const iefvad_outputs* out,
                               void* stream);
int iefvad_forward_videos_host_full(iefvad_handle* h, const void* const* img_rows, const void* const* ev_rows, int32_t in_dtype,
                                    int32_t wire_dtype, const int32_t* lengths, int32_t nvideos, int32_t nan_to_num,
                                    int32_t batch_chunks, int32_t host_threads, const iefvad_outputs* out, void* stream);

/* ---- head-averaged attention maps of the temporal encoder (opt-in) ---------------------------------------------------
 * What nn.MultiheadAttention(...)(x, x, x) returns second with need_weights=True (imf_vad.py:115,121 form it on every call and
 * discard it): per encoder layer and modality the mean over the 8 heads of softmax(Q_h K_h^T / sqrt(d_h)), one [256, 256] fp32 map
 * per 256-snippet chunk; row = query snippet, column = key snippet of the chunk, every row sums to 1.
 *   iefvad_forward_attn          iefvad_forward plus `maps`; a map is [B*T, T]: query row r of chunk c at row c*256 + r.
 *   iefvad_forward_videos_attn   iefvad_forward_videos plus `maps`; a map is [sum(lengths), T] in PACKED order: valid query row r
 *                                of a chunk at the chunk's packed row + r, pad rows are not written.  Key columns >= the chunk's
 *                                valid rows hold the weight of a pad key, as the padded route gives them (the reference attends
 *                                to its zero rows).  A video that straddles micro-batch passes lands at each pass's row offset.
 * A NULL layer is neither computed nor written; image and event are asked for separately.  The maps are formed in fp32 from the
 * layer's fp32 q | k | v rows by iefvad_attention_maps_kernel (csrc/attention_maps.h) right behind the attention kernel, in a fixed
 * order without atomics: the same call gives the same bits, and in the f32 arithmetic the valid-row maps equal the `[0:len]` rows of
 * the dense maps on host-padded chunks bit for bit.  Every other result of the call has the bits of the call without maps.
 * Workspace: iefvad_workspace_bytes / iefvad_videos_workspace_bytes, unchanged.  Served: compute F32, BF16X6 and FP16X3, D = 768 and
 * 512, the three input dtypes, IEFVAD_DENSE_ENCODER=1.  These calls launch directly (the hipGraph replay of small batches is not
 * used: the map pointers are per call).  Refused by name before any HIP call: a NULL handle, NULL maps, maps with every pointer NULL,
 * a pointer at a layer index >= num_layers, a pointer that is not 16-byte aligned, compute = BF16 (its q | k | v are bf16 planes in
 * another layout).  NOT covered: the host-list, scaled, similarity and full entries and training take no maps.
 * Added without a change to any other entry or struct: IEFVAD_ABI_VERSION stays. */
typedef struct iefvad_attn_maps {        /* DEVICE fp32, each nullable: a NULL layer is not computed */
    float* image[IEFVAD_MAX_LAYERS];     /* dense: [B*T, T]; videos: [sum(lengths), T] */
    float* event[IEFVAD_MAX_LAYERS];
} iefvad_attn_maps;
int iefvad_forward_attn(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B, void* workspace,
                        size_t workspace_bytes, const iefvad_outputs* out, const iefvad_attn_maps* maps, void* stream);
int iefvad_forward_videos_attn(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype, const int32_t* lengths,
                               int32_t nvideos, int32_t nan_to_num, void* workspace, size_t workspace_bytes, float* logits,
                               float* w_i_mean, float* w_e_mean, const iefvad_attn_maps* maps, void* stream);

/* ---- training-side loss head: forward, and its gradients w.r.t. the model's outputs -----------------
 * The three terms the reference's trainers add up (/root/reference/train/ucf_train.py:68-101, train/xd_train.py:60-75), as
 * device reductions over tensors iefvad_forward already produces:
 *   out[0] classification  CLAS2(logits, labels, lengths) (/root/reference/train/loss.py:18-30): per video the mean of the
 *                          int(len / 16 + 1) largest sigmoid(logit[0:len]), binary cross entropy against targets
 *   out[1] reg = out[2] + out[3]: mean(1 - cosine_similarity(normalize(mu_i), normalize(mu_e))) + mean(| ||mu_i|| - ||mu_e|| |)
 *   out[4] kl = out[5] + out[6]: -0.5 mean(1 + l - mu^2 - exp(l)) per modality, l = logvar (Gaussian) or
 *                          logvar + log(nu / (nu + 1)) (StudentT; the trainers read model.temporal.nu, ucf_train.py:94-95)
 *   out[7] total = classification + lambda_reg * reg + lambda_kl * kl   (1, 1 in ucf_train.py:100-102; 0.01, 0.01 in xd_train.py:73-75)
 * logits [B, T]; the four 768-d tensors [B*T, 768]; lengths int32 [B] and targets fp32 [B] (1 = abnormal, i.e.
 * 1 - labels[:, 0], loss.py:20) on the DEVICE; out: 8 fp32 on the device.  T must be 256.  Deterministic (no atomics).
 * `workspace`: iefvad_loss_workspace_bytes(B, T) device bytes, 16-byte aligned.  Layout, readable once the call's work on the
 * stream is done: fp32 part[B*T][4] (per row: 1 - cos, | ||mu_i|| - ||mu_e|| |, and the row sums of 1 + l - mu^2 - exp(l) for the
 * image and the event modality; left unwritten when the four 768-d pointers are NULL), then fp32 inst[B] (per video the top-k mean
 * of the sigmoid scores; NaN for a length <= 0 or a k beyond the 256 snippets).  out[] is the fixed-order sum of exactly these.
 * The four 768-d pointers may all be NULL: then only out[0] (and out[7] = out[0]) is computed -- CLAS2 alone.
 * iefvad_loss_backward: the gradients of grad_scale * total with respect to logits [B, T] and the four 768-d tensors (what
 * `loss.backward()` hands to the model's outputs in /root/reference/train/ucf_train.py:103): CLAS2 through torch's BCE
 * backward ((p - y) / max((1 - p) p, 1e-12)) and the top-k selection, the cosine / norm regulariser, the KL terms.
 * `grad_scale_dev` (nullable) is the upstream gradient as a DEVICE scalar that multiplies grad_scale inside the kernels, so an
 * autograd node never has to read it back to the host.  Each
 * d_* pointer may be NULL (that gradient is not written).  The model's own backward pass: iefvad_train_backward below. */
size_t iefvad_loss_workspace_bytes(int32_t B, int32_t T);
int iefvad_loss_forward(const float* logits, const float* image_mu, const float* event_mu, const float* image_logvar,
                        const float* event_logvar, const int32_t* lengths, const float* targets, int32_t B, int32_t T,
                        int32_t noise_model, float nu, float lambda_reg, float lambda_kl, float* out, void* workspace,
                        size_t workspace_bytes, void* stream);
int iefvad_loss_backward(const float* logits, const float* image_mu, const float* event_mu, const float* image_logvar,
                         const float* event_logvar, const int32_t* lengths, const float* targets, int32_t B, int32_t T,
                         int32_t noise_model, float nu, float lambda_reg, float lambda_kl, float grad_scale,
                         float* d_logits, float* d_image_mu, float* d_event_mu, float* d_image_logvar,
                         float* d_event_logvar, const float* grad_scale_dev, void* stream);

/* ---- training: the train-mode forward and the model's backward pass ----------------------------------------------
 * What `model.train(); outputs = model(...); loss.backward()` does to the model in the reference's trainers
 * (/root/reference/train/ucf_train.py:43,60-66,103; train/xd_train.py:37,46-52,78): the forward of
 * /root/reference/model/imf_vad.py:109-161 with the attention dropout of nn.MultiheadAttention(dropout=0.1) (imf_vad.py:70) active,
 * and the gradient of every parameter of SURVEY.md Appendix B.  The reference has no backward code of its own (autograd derives it);
 * the entry points below are what a torch.autograd.Function around the model binds.
 *
 * iefvad_train_forward computes the eight outputs like iefvad_forward and keeps what the backward needs in `train_ws`
 * (iefvad_train_workspace_bytes; 256-byte aligned; owned by the caller, who keeps it untouched until the matching
 * iefvad_train_backward has run on the same stream).  compute must be IEFVAD_COMPUTE_F32 or IEFVAD_COMPUTE_BF16X6 (fp32-accurate);
 * the whole batch runs as one pass (B <= 4096).  Five of the outputs are also saved tensors (fused, image_mu, event_mu, image_logvar,
 * event_logvar) and fp32 inputs are saved as they are: the forward writes / reads the caller's buffers in place and the backward
 * READS THEM AGAIN, so `img`, `ev` (in_dtype f32) and those five output buffers stay untouched until iefvad_train_backward has run
 * (a null output pointer keeps that tensor in train_ws).  ONE backward per forward: the backward's scratch tensors overwrite saved states
 * it has already differentiated, so a second iefvad_train_backward on the same buffer fails ("no iefvad_train_forward ...") until a
 * new forward has filled it.
 *   dropout_p[m][l]  the probability nn.MultiheadAttention m / layer l drops an attention weight with (0 = none); kept weights
 *                    are scaled by 1 / (1 - p) as torch.nn.functional.dropout does
 *   seed             stream of the library's counter-based mask generator for this step.  torch draws its mask from its own Philox
 *                    stream, so a p > 0 run is statistically, not bit-wise, the reference's; p = 0 and injected masks are exact
 *   keep_mask        device, nullable: uint8 [2][L][B][8][T][T], 1 = keep -- an injected mask replaces the generator (tests, replay)
 * iefvad_train_backward: `dout` holds the gradients handed to the eight outputs (each nullable = zero; [B*T, D], logits [B*T]);
 * every non-null pointer of `dw` ([same shape as the parameter], fp32) receives that parameter's gradient (overwritten, not
 * accumulated).  Reductions over rows are fixed-order: the same inputs give the same bits on every run.
 *
 * iefvad_train_backward_inputs is the same backward with one more request: `dx` names where the gradients of the two INPUT feature
 * tensors go (each [B*T, D] fp32, device, 16-byte aligned, nullable; overwritten, not accumulated).  For a non-null member, layer 0 of
 * that modality runs the product the layers above it already run, d x = d s (residual) + d qkv W_in (K = 2304), into the caller's
 * buffer: on the exact split kernel where the batch fills its grid (IEFVAD_COMPUTE_BF16X6), on the fp32 MFMA kernel otherwise.  The
 * gradient is with respect to the fp32 values the forward computed on: for in_dtype f16 / bf16 that is the WIDENED rows, so the caller
 * rounds it to the narrow type if it wants `.grad` in the feature dtype.  Nothing else changes: the residual gradient is only read, no
 * parameter gradient moves by a bit because an input gradient was asked for, and dx = NULL (or both members null) launches exactly what
 * iefvad_train_backward launches -- that entry IS this one with dx = NULL.  The rule of ONE backward per forward is unchanged.
 * A frozen model: every pointer of `dw` may be null.  Then the backward skips every weight-gradient product (the split-K d W launches
 * and their reductions), every bias column sum, and the reductions of the classifier / LayerNorm-affine partial sums (the partial sums
 * themselves are by-products of the kernels that form d x and stay); and where neither the in_proj gradients of a modality's layer 0
 * nor its input gradient are asked for, layer 0's attention backward (nothing reads its d qkv) is skipped too. */
typedef struct iefvad_train_options {
    float dropout_p[2][IEFVAD_MAX_LAYERS];
    uint64_t seed;
    const uint8_t* keep_mask;
} iefvad_train_options;

typedef struct iefvad_output_grads {
    const float* fused;  const float* logits;  const float* image_mu;  const float* event_mu;
    const float* image_logvar;  const float* event_logvar;  const float* w_i;  const float* w_e;
} iefvad_output_grads;

/* gradient destinations, field for field the layout of iefvad_weights */
typedef struct iefvad_weight_grads {
    float* in_proj_w[2][IEFVAD_MAX_LAYERS];
    float* in_proj_b[2][IEFVAD_MAX_LAYERS];
    float* out_proj_w[2][IEFVAD_MAX_LAYERS];
    float* out_proj_b[2][IEFVAD_MAX_LAYERS];
    float* norm_w[2][IEFVAD_MAX_LAYERS];
    float* norm_b[2][IEFVAD_MAX_LAYERS];
    float* whiten_w[2];
    float* whiten_b[2];
    float* mu_w[2];
    float* mu_b[2];
    float* logvar_w[2];
    float* logvar_b[2];
    float* ref_w1[IEFVAD_MAX_STEPS];
    float* ref_b1[IEFVAD_MAX_STEPS];
    float* ref_w2[IEFVAD_MAX_STEPS];
    float* ref_b2[IEFVAD_MAX_STEPS];
    float* cls_w;
    float* cls_b;
} iefvad_weight_grads;

/* Training is built for D = 768: a D = 512 handle (iefvad_create_ex) gets 0 bytes / an error that names the width. */
size_t iefvad_train_workspace_bytes(const iefvad_handle* h, int32_t B);
int iefvad_train_forward(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B,
                         const iefvad_train_options* opt, void* train_ws, size_t train_ws_bytes, const iefvad_outputs* out,
                         void* stream);
int iefvad_train_backward(iefvad_handle* h, int32_t B, void* train_ws, size_t train_ws_bytes, const iefvad_output_grads* dout,
                          const iefvad_weight_grads* dw, void* stream);
typedef struct iefvad_input_grads { float* img; float* ev; } iefvad_input_grads;   /* device, [B*T, D] fp32, each nullable */
int iefvad_train_backward_inputs(iefvad_handle* h, int32_t B, void* train_ws, size_t train_ws_bytes,
                                 const iefvad_output_grads* dout, const iefvad_weight_grads* dw,
                                 const iefvad_input_grads* dx, void* stream);

/* The trainers' input rule (/root/reference/train/ucf_train.py:50-53; xd_train.py has none: `if torch.isnan(x).any(): x =
 * torch.nan_to_num(x, nan=0.0)`, per tensor) for the two fp32 input tensors of a step, without the host read of the flag: one scan,
 * one repair launch that returns at once for a tensor without NaN; a tensor WITH a NaN is rewritten IN PLACE as torch.nan_to_num
 * does (NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX).  a, b: device, n floats each (n % 4 == 0, 16-byte aligned); flags_ws: 8 device
 * bytes (8-byte aligned) that hold the two flags afterwards (1 = that tensor had a NaN). */
int iefvad_nan_rule(float* a, float* b, size_t n, void* flags_ws, void* stream);

/* One torch.optim.AdamW step (as /root/reference/train/ucf_train.py:28 constructs it: betas (0.9, 0.999), eps 1e-8, weight_decay
 * 0.01, amsgrad off) on one flat fp32 tensor, in place, in torch's operation order; `step` counts from 1.  The hyper-parameters
 * travel as doubles: torch forms 1 - lr wd, 1 - beta1, 1 - beta2, lr / (1 - beta1^t) and sqrt(1 - beta2^t) in Python floats
 * and rounds each to fp32 once; so does this.  All pointers are device pointers of n floats. */
int iefvad_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                      double beta2, double eps, double weight_decay, int32_t step, void* stream);

/* The same update for many tensors in ONE launch (a model of SURVEY.md Appendix B has 78 parameter tensors, most of them 768-element
 * vectors): `table` is a DEVICE array of `count` entries, each with its four device pointers, its element count and the index of
 * its first 4096-element chunk (first_chunk[0] = 0, first_chunk[i+1] = first_chunk[i] + ceil(n[i] / 4096)); total_chunks = the sum.
 * All tensors take the same hyper-parameters and step count.  Element for element the arithmetic of iefvad_adamw_step. */
typedef struct iefvad_adamw_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    uint64_t n;
    uint64_t first_chunk;
} iefvad_adamw_tensor;
int iefvad_adamw_step_multi(const iefvad_adamw_tensor* table, int32_t count, uint64_t total_chunks, double lr, double beta1, double beta2,
                            double eps, double weight_decay, int32_t step, void* stream);

/* Host helper of the whole-video path (the loader side, /root/reference/data/dataset.py:34-52 + test.py:90-95's `.to(device)`):
 * dst[0 ..) = srcs[0] | srcs[1] | ... (nbytes[i] bytes each), copied by up to `threads` host threads.  `dst` is normally a
 * pinned staging buffer that one asynchronous copy then sends to the device as iefvad_forward_videos's img_rows / ev_rows.
 * Pure host code: all pointers are HOST pointers. */
int iefvad_host_gather(void* dst, const void* const* srcs, const size_t* nbytes, int64_t count, int32_t threads);
/* The same gather with the rows narrowed on the way: srcs[i] holds nbytes[i] bytes of fp32 (multiples of 64), dst receives them as
 * bf16 (sum(nbytes) / 2 bytes; round to nearest even, NaN stays NaN with its sign, overflow to +-inf -- the device's conversion).
 * This is what iefvad_forward_videos_host's copy threads run for wire_dtype = IEFVAD_IN_BF16. */
int iefvad_host_gather_bf16(void* dst, const void* const* srcs, const size_t* nbytes, int64_t count, int32_t threads);

/* iefvad_forward with a per-row scale on the INPUT features: row r of modality m enters the model as x[r] * scale_m[r] (the
 * product rounded to the input type, as torch does for fp16 / bf16 tensors, before imf_vad.py:41-42 widens it); a NULL vector
 * scales nothing.  This is the perturbation of the reference's robustness sweep (/root/reference/test2.py:71-77:
 * `v_p[:, indexs] = v_p[:, indexs] * 0.01` on a random subset of time steps) folded into the input load, so the packed clean
 * features can stay resident on the device across the sweep's twelve levels.  img_row_scale, ev_row_scale: DEVICE [B*T] fp32. */
int iefvad_forward_scaled(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B, const float* img_row_scale,
                          const float* ev_row_scale, void* workspace, size_t workspace_bytes, const iefvad_outputs* out, void* stream);

/* ---- row perturbations for the noise study: additive Gaussian noise next to the row scale ---------------------------------------
 * test2.py declares the study's arguments (run_test's outlier_img / outlier_ev :35-37, --noise_sigma_img / _ev :214-217,
 * --outlier_ratio :218, --dropout_prob :220) and reads none of them: the reference implements no Gaussian noise, no outliers and no
 * modality drop.  The semantics below are therefore this library's own -- PARITY UNPINNED -- and what is pinned is internal
 * consistency: the fused load equals perturbed rows materialised first (iefvad_perturb_rows), the generator equals its host model
 * (harness.gaussian_rows), the padded and the valid-row route agree.
 * Row r of modality m (m = 0 image, 1 event) of a call enters the model as follows, in this order:
 *   1. the NaN rule of the entry, as without a perturbation;
 *   2. y = x if scale[m] is NULL or scale[m][r] == 1, else y = T(fp32(x) * scale[m][r])                 (iefvad_forward_scaled, T = in_dtype);
 *   3. z = y, bits untouched, if noise_amp[m] is NULL or noise_amp[m][r] == 0, else z = T(fp32(y) + p), p = noise_amp[m][r] * eps
 *      rounded to fp32 on its own (no fused multiply-add): what `y + amp * eps` gives in torch for a tensor of dtype T and an fp32 eps.
 * Pad rows of the valid-row entry are the zeros the library writes and are never perturbed; on the padded entry they are rows of the
 * caller's tensor: give them amplitude 0 and scale 1.
 * eps is a standard normal in fp32, a pure function of (seed, m, id, column d): columns are generated in pairs (2q, 2q + 1) by Box-Muller
 * from the library's 24-bit counter-based generator g(seed, index) (the one behind the train-mode dropout mask):
 *     idx = ((uint64(id) * 2 + m) << 11) | (q << 1);   b1 = g(seed, idx);   b2 = g(seed, idx | 1)
 *     u1 = (b1 + 1) 2^-24 in (0, 1];   u2 = b2 2^-24 in [0, 1);   rho = sqrt(-2 ln u1)
 *     eps[2q] = rho cos(2 pi u2);   eps[2q + 1] = rho sin(2 pi u2)                        |eps| <= sqrt(48 ln 2) = 5.77
 * id is noise_row[r], or -- noise_row NULL -- the row's index in the CALL: b T + t on the padded entry, the packed row on the valid-row
 * entry (whatever micro-batch pass it falls into).  With ids that name the snippet in the list the same snippet gets the same noise on
 * either route, in any batch composition.
 * With both noise_amp NULL the two forward entries launch, and return the bits of, iefvad_forward_scaled / iefvad_forward_videos_scaled
 * (which are thin wrappers over them).  A call with an amplitude vector launches directly (no graph replay: seed and pointers are per
 * call).  iefvad_forward_videos_perturbed takes the arguments of iefvad_forward_videos_scaled with the two scale pointers replaced by the
 * struct; its workspace is iefvad_videos_scaled_workspace_bytes.  iefvad_perturb_rows writes rows 1.-3. of `rows` rows of width D (768 or
 * 512) in `in_dtype`, nan_to_num_all != 0 applying torch.nan_to_num to every row first; either source may be NULL when its output is.
 * Refused by name before any launch: a NULL struct, an unknown in_dtype, D other than 768 / 512 (the unit entry), vectors that are not
 * 4-byte aligned.  NOT covered: the host-list entries, the similarity / full / maps entries, and training take no perturbation.
 * Added without a change to any other entry or struct: IEFVAD_ABI_VERSION stays. */
typedef struct {
    const float*   scale[2];      /* DEVICE [rows] fp32, nullable each: the row scales (image, event) */
    const float*   noise_amp[2];  /* DEVICE [rows] fp32, nullable each */
    const int32_t* noise_row;     /* DEVICE [rows] int32 >= 0, nullable: noise ids; NULL = the call's row index */
    uint64_t       seed;
} iefvad_perturb;
int iefvad_forward_perturbed(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B, const iefvad_perturb* perturb,
                             void* workspace, size_t workspace_bytes, const iefvad_outputs* out, void* stream);          /* rows = B*T */
int iefvad_forward_videos_perturbed(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype, const int32_t* lengths,
                                    int32_t nvideos, int32_t nan_to_num, const iefvad_perturb* perturb, void* workspace,
                                    size_t workspace_bytes, float* logits, float* w_i_mean, float* w_e_mean, double* w_colsum, void* stream);
int iefvad_perturb_rows(const void* img_rows, const void* ev_rows, int32_t in_dtype, int32_t D, int64_t rows, int32_t nan_to_num_all,
                        const iefvad_perturb* perturb, void* out_img, void* out_ev, void* stream);                      /* outputs in in_dtype */

/* ---- metric tail of the evaluation loop --------------------------------------------------------------
 * What /root/reference/test.py:158-159 (train/ucf_test.py:153-154, train/xd_test.py:146-147) computes with sklearn on the host,
 *     ROC1 = roc_auc_score(gt, np.repeat(ap1, 16));   AP1 = average_precision_score(gt, np.repeat(ap1, 16))
 * (the GLOBAL pair; the per-class pairs and the Ano-AUC behind it are iefvad_auc_ap_grouped below)
 * on the DEVICE from the n per-snippet scores and the frame-level ground truth, without materialising the x`repeat` copy: one
 * radix sort of n (score, positive-frames-of-the-snippet) pairs, a scan, a reduction over the tie groups.  Thresholds are the
 * DISTINCT score values as in sklearn's _binary_clf_curve (tied snippets share one threshold; -0.0 == +0.0); the AUC numerator is
 * accumulated exactly in 64-bit integers, the AP terms in doubles in a fixed order: deterministic, and equal to sklearn to ~1e-15.
 *   scores      DEVICE [n] fp32 (e.g. sigmoid of iefvad_forward_videos_host's logits, or iefvad_gather_scores's output)
 *   gt_frames   DEVICE [n * repeat] bytes, non-zero = anomalous frame (the reference's gt.npy holds 0.0 / 1.0, test.py:379)
 *   auc, ap     DEVICE doubles, each nullable (not both); valid once `stream` has run.  A NaN score makes both NaN; only one class
 *               in gt_frames makes *auc NaN (sklearn raises there) and, with no positive frame, *ap 0 (as sklearn returns)
 *   workspace   DEVICE, iefvad_auc_ap_workspace_bytes(n) bytes (16 n + ~1.1 KB per 4096 snippets), 256-byte aligned
 * n * repeat must stay below 2^32 frames.  Enqueued on `stream`; returns without synchronising. */
size_t iefvad_auc_ap_workspace_bytes(int64_t n);
int iefvad_auc_ap(const float* scores, const uint8_t* gt_frames, int64_t n, int32_t repeat, double* auc, double* ap,
                  void* workspace, size_t workspace_bytes, void* stream);

/* The same two numbers for up to 64 disjoint GROUPS of the snippets in one pass: the per-class ROC-AUC / AP loops of test.py:165-174
 * (train/ucf_test.py, train/xd_test.py alike) with group = class of the snippet's video, and the Ano-AUC of test.py:161
 * (compute_ano_auc, :332-348) with one group that leaves the normal videos out.  These two tails are OPT-IN in the Python harness
 * (metric_tail="device"); its default keeps sklearn on the host.  The group byte is a fifth radix digit above the score key, so
 * the pairs are sorted by (group, score) once; within a group everything is iefvad_auc_ap: thresholds are the group's distinct
 * scores (-0.0 == +0.0; a tie never spans two groups), exact 64-bit integer AUC numerators, AP terms in doubles reduced in a
 * fixed order (no floating-point atomics: the same bits every run).
 *   group       DEVICE [n] bytes: a value in [0, ngroups) puts the snippet into that group, 255 into none; every other value is
 *               treated as 255
 *   ngroups     1 .. 64
 *   auc, ap     DEVICE [ngroups] doubles, each nullable (not both).  Per group: a NaN score makes ITS two results NaN (no other
 *               group's); one class only -> auc NaN; no positive frame -> ap 0; an empty group -> both NaN
 *   frames      DEVICE [2 * ngroups] int64, nullable: {frames in the group, positive frames in the group} -- what the reference's
 *               skip rule `len(cls_gt) == 0 or sum(cls_gt) == 0` and its "Total Samples" print need
 *   workspace   DEVICE, iefvad_auc_ap_grouped_workspace_bytes(n, ngroups) bytes (the ungrouped call's plus 8 ngroups bytes per 4096
 *               snippets and ~2 KB), 256-byte aligned; 0 for n <= 0 or ngroups outside 1 .. 64
 * n * repeat must stay below 2^32 frames, and repeat below 2^24: a snippet's positive-frame count shares the pair's 32-bit payload
 * with the group byte.  Every argument is checked before the first HIP call.  Enqueued on `stream`; returns without synchronising. */
size_t iefvad_auc_ap_grouped_workspace_bytes(int64_t n, int32_t ngroups);
int iefvad_auc_ap_grouped(const float* scores, const uint8_t* gt_frames, const uint8_t* group, int64_t n, int32_t repeat, int32_t ngroups,
                          double* auc, double* ap, int64_t* frames, void* workspace, size_t workspace_bytes, void* stream);

/* The four per-snippet series of the reference's similarity plots (/root/reference/test.py:235-238, train/ucf_test.py:243-247) in ONE
 * launch (csrc/similarity.h): for output row j and source row s = src_rows ? src_rows[j] : j
 *   out[0][j] = F.cosine_similarity(fused[s], image_mu[s])      out[2][j] = torch.norm(fused[s] - image_mu[s])
 *   out[1][j] = F.cosine_similarity(fused[s], event_mu[s])      out[3][j] = torch.norm(fused[s] - event_mu[s])
 * cosine = dot / (max(|a|, 1e-8) max(|b|, 1e-8)); the squared distance is summed directly.  fp32 sums in the library's own order (not
 * torch's bits); NaN propagates as in torch.  Rows whose squared sums overflow fp32 are outside the contract.
 *   fused, image_mu, event_mu   DEVICE [rows, D] fp32, 16-byte aligned; D is 768 or 512
 *   src_rows    DEVICE int32 [nout], nullable (identity; then nout <= rows).  Every entry lies in [0, rows): a precondition the
 *               caller keeps; an entry outside it is not read for and yields four NaNs
 *   out         DEVICE [4, nout] fp32, 16-byte aligned
 * Null tensors or a null out, rows <= 0, nout < 0, another D and misaligned pointers are refused before any launch; nout == 0 succeeds
 * without one.  Enqueued on `stream`; returns without synchronising. */
int iefvad_similarity_rows(const float* fused, const float* image_mu, const float* event_mu, int64_t rows, int32_t D, const int32_t* src_rows,
                           int64_t nout, float* out, void* stream);

/* ---- training input pipeline ----------------------------------------------------------
 * The reference's train-mode loader rule (/root/reference/data/tools.py:65-97: process_feat -> uniform_extract / pad) on the DEVICE:
 * a video of n feature rows becomes one [256, D] fp32 window.  n <= 256: the rows, zero rows behind them, length n.  n > 256: 256
 * segments with boundaries (i n) >> 8 (= np.linspace(0, n, 257, dtype=np.int32)), output row i = np.mean of its segment, length 256.
 * The mean is numpy's bit for bit: an fp32 accumulator starting at +0, rows added in ascending order, one correctly rounded fp32
 * division by the count; the quotient of an fp16 file is rounded to fp16 and widened again.  No NaN rule is applied.
 *   rows        DEVICE [sum(lengths), D], IEFVAD_IN_F32 or IEFVAD_IN_F16: the videos' rows concatenated in list order, 16-byte aligned
 *   lengths     HOST [nvideos], every entry >= 1; consumed before the call returns
 *   T, D        T must be 256; D a multiple of 8 (768 and 512 occur)
 *   workspace   DEVICE, iefvad_resample_workspace_bytes(nvideos) bytes (16 per video), 16-byte aligned
 *   out         DEVICE [nvideos, 256, D] fp32, window v = video v whatever order the kernel takes them in (longest first)
 *   out_lengths DEVICE int32 [nvideos]: min(lengths[v], 256)
 * Enqueued on `stream`; the call waits for what `stream` held before it (the table upload), not for the resampling itself. */
size_t iefvad_resample_workspace_bytes(int32_t nvideos);
int iefvad_resample_videos(const void* rows, int32_t in_dtype, const int32_t* lengths, int32_t nvideos, int32_t T, int32_t D,
                           void* workspace, size_t workspace_bytes, float* out, int32_t* out_lengths, void* stream);

/* One training step's batch out of a cached set of windows, in ONE launch: img_out[b] = img_set[index[b]], ev_out[b] =
 * ev_set[index[b]], len_out[b] = set_lengths[index[b]].  img_set, ev_set: DEVICE [nset, 256, D] fp32; set_lengths: DEVICE int32
 * [nset]; index: DEVICE int32 [B], every entry in [0, nset) -- the caller checks that on the host; an entry outside it does not
 * fault, it yields a zero window of length 0; img_out, ev_out: DEVICE [B, 256, D] fp32; len_out: DEVICE int32 [B].  T must be 256,
 * D a multiple of 8, B <= 65535, the window tensors 16-byte aligned.  Enqueued on `stream`; returns without synchronising. */
int iefvad_gather_windows(const float* img_set, const float* ev_set, const int32_t* set_lengths, int32_t nset, const int32_t* index,
                          int32_t B, int32_t T, int32_t D, float* img_out, float* ev_out, int32_t* len_out, void* stream);

/* ---- the VadCLIP-residue modules the north star names (SURVEY.md 8 rows a12 / a13 = f-5) ------------------------------------------
 * /root/reference/model/layers.py and /root/reference/model/module.py are dead code upstream (nothing imports them, a checkpoint holds
 * no key of theirs), so they are exposed at MODULE level: one entry per class, fp32, on the library's MFMA GEMM + LayerNorm kernels
 * (csrc/vadclip.h).  All tensors are DEVICE fp32, row-major, 16-byte aligned; every entry takes a caller-owned workspace of
 * iefvad_*_workspace_bytes(...) bytes and enqueues on `stream`.  The products run on 128 x (128 | 96) x 16 tiles: T (and N for the
 * GAT layer) must be a multiple of 128, feature widths multiples of 128 (or 96) and of 16.
 *
 * iefvad_similarity_adj  layers.py:114-163  x [B,T,d_in], weight0 [d_in,d_out] (weight1 is never read upstream, :132-133),
 *                        seq_len int32 [B] on the device or NULL -> adj [B,T,T]: cosine similarity of x W0 rows, F.threshold(0.7, 0),
 *                        row softmax (over [:len, :len] when seq_len is given; zero outside)
 * iefvad_distance_adj    layers.py:166-179  adj[b,i,j] = exp(-|i - j| / e)
 * iefvad_gcn_forward     layers.py:64-111   out = adj (x W) (+ bias) + residual.  weight [d_in,d_out]; residual 0 none, 1 identity (d_in ==
 *                        d_out), 2 Conv1d(d_in, d_out, kernel_size=5, padding=2) over time with conv_w [d_out,d_in,5], conv_b [d_out];
 *                        act 1 applies QuickGELU to the result (what VadCLIP's caller did), 0 leaves it
 * iefvad_gat_forward     layers.py:12-49    input [N,f_in], adj [N,N], W [f_in,f_out], a [2 f_out]; alpha = LeakyReLU slope;
 *                        concat != 0 applies ELU; eval semantics (dropout inactive)
 * iefvad_resblock_forward module.py:20-43   x, out [T,B,768] sequence-first; attn_mask [T,T] additive fp32 or NULL; key_padding_mask
 *                        [B,T] bytes (non-zero = padding) or NULL; n_head with 768 / n_head in {96, 128} */
typedef struct iefvad_resblock_weights {
    const float* in_proj_w;   /* attn.in_proj_weight [2304,768] */
    const float* in_proj_b;   /* [2304] */
    const float* out_proj_w;  /* attn.out_proj.weight [768,768] */
    const float* out_proj_b;
    const float* ln_1_w; const float* ln_1_b;
    const float* ln_2_w; const float* ln_2_b;
    const float* c_fc_w;      /* mlp.c_fc.weight [3072,768] */
    const float* c_fc_b;
    const float* c_proj_w;    /* mlp.c_proj.weight [768,3072] */
    const float* c_proj_b;
} iefvad_resblock_weights;
size_t iefvad_similarity_adj_workspace_bytes(int32_t B, int32_t T, int32_t d_out);
int iefvad_similarity_adj(const float* x, const float* weight0, const int32_t* seq_len, int32_t B, int32_t T, int32_t d_in, int32_t d_out,
                          float* adj, void* workspace, size_t workspace_bytes, void* stream);
int iefvad_distance_adj(int32_t B, int32_t T, float* adj, void* stream);
size_t iefvad_gcn_workspace_bytes(int32_t B, int32_t T, int32_t d_in, int32_t d_out, int32_t residual);
int iefvad_gcn_forward(const float* x, const float* adj, const float* weight, const float* bias, const float* conv_w, const float* conv_b,
                       int32_t residual, int32_t act, int32_t B, int32_t T, int32_t d_in, int32_t d_out, float* out, void* workspace,
                       size_t workspace_bytes, void* stream);
size_t iefvad_gat_workspace_bytes(int32_t N, int32_t f_out);
int iefvad_gat_forward(const float* input, const float* adj, const float* W, const float* a, float alpha, int32_t concat, int32_t N, int32_t f_in,
                       int32_t f_out, float* out, void* workspace, size_t workspace_bytes, void* stream);
size_t iefvad_resblock_workspace_bytes(int32_t T, int32_t B, int32_t n_head);
int iefvad_resblock_forward(const float* x, const iefvad_resblock_weights* w, const float* attn_mask, const uint8_t* key_padding_mask, int32_t T,
                            int32_t B, int32_t d_model, int32_t n_head, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- unit entry for the bf16 mode's row-block kernels (per-kernel parity tests) -----------------------------------------
 * Launches ONE production kernel of compute = IEFVAD_COMPUTE_BF16 -- the symbol, grid and LDS size iefvad_forward uses at that row
 * count (the persistent variants from two 64-row blocks per workgroup on) -- on caller-supplied DEVICE rows, with the handle's
 * weights.  `rows` is a multiple of 64; both modalities ride one launch as in the forward.  Stages and the fields they read:
 *   IEFVAD_UNIT_INPROJ      layer l: x[m] = the layer's input rows [rows,768] (fp32 for l == 0, bf16 otherwise) ->
 *                           y[m] = bf16 q | k | v, head-major [3][8 heads][rows][96], q pre-scaled by log2(e)/sqrt(96)
 *                           (/root/reference/model/imf_vad.py:115,121: nn.MultiheadAttention's packed in_proj)
 *   IEFVAD_UNIT_OUTPROJ_LN  layer l: x[m] = attention output bf16 [rows,768], resid[m] = the layer's fp32 input rows ->
 *                           LayerNorm(resid + x W_o^T + b_o) (imf_vad.py:116,122), and for l == L-1 the whitening LayerNorm
 *                           behind it (:117,:123): y[m] fp32 and / or yb[m] bf16 [rows,768] (each nullable, not both)
 *   IEFVAD_UNIT_HEADS       x[m] = whitened rows bf16 [rows,768] -> mu[m], logvar[m], w[m] (each nullable) and the fused z
 *                           (imf_vad.py:125-144)
 *   IEFVAD_UNIT_REFINE      x[0] = z_0 fp32 [rows,768] -> z = z_K (nullable), logits [rows] (imf_vad.py:146-150)
 *   IEFVAD_UNIT_ATTENTION   x[m] = bf16 q | k | v in the head-major layout IEFVAD_UNIT_INPROJ writes (q in log2 units: the kernels
 *                           compute softmax2(q k^T) v per 256-row chunk and head, imf_vad.py:115,121) -> yb[m] = bf16 [rows,768];
 *                           rows is a multiple of 256; the one-block kernel, or the persistent one from two (chunk, head,
 *                           modality) items per compute unit on, as in the forward.  `layer` is ignored (no weights are read).
 * All pointers 16-byte aligned.  Enqueued on `stream`. */
#define IEFVAD_UNIT_INPROJ 0
#define IEFVAD_UNIT_OUTPROJ_LN 1
#define IEFVAD_UNIT_HEADS 2
#define IEFVAD_UNIT_REFINE 3
#define IEFVAD_UNIT_ATTENTION 4   /* added without a change of layout or of the other stages: IEFVAD_ABI_VERSION stays */
typedef struct iefvad_unit_io {
    const void* x[2];
    const float* resid[2];
    void* y[2];
    void* yb[2];
    float* mu[2];
    float* logvar[2];
    float* w[2];
    float* z;
    float* logits;
} iefvad_unit_io;
int iefvad_rowblock_unit(iefvad_handle* h, int32_t stage, int32_t layer, int32_t rows, const iefvad_unit_io* io, void* stream);

/* Stand-alone dense projection C[M,N] = A[M,K] * W[N,K]^T + bias[N] on the library's GEMM
 * kernels (unit tests and the roofline micro-benchmark).  M % 128 == 0, N % 128 == 0, K % 64 == 0.
 * compute = IEFVAD_COMPUTE_F32: A and W are fp32; IEFVAD_COMPUTE_BF16: A and W are bf16 (same shapes);
 * IEFVAD_COMPUTE_BF16X6: A is fp32, W is the three-plane split [3][N][K] bf16 made by iefvad_split_bf16x3
 * (K % 64 == 0); bias and C are fp32 in all three. */
int iefvad_gemm_bias(const void* A, const void* W, const float* bias, float* C,
                     int32_t M, int32_t N, int32_t K, int32_t compute, void* stream);

/* One projection (or nz = 2 problems of one shape in one launch) on the bf16x6 split kernel, on the tiling the caller names:
 * tile_n = 128 (128 x 128 block tile) or 256 (128 x 256 as two column halves; N % 256 == 0).  The two tilings sum every output
 * element in the same order, so they agree bit for bit; the library's own launches choose between them by grid size, and this entry
 * lets a unit test hold one against the other on every epilogue.  A[m] is fp32 [M, K]; W[m] the three-plane split [3][N][K] of
 * iefvad_split_bf16x3; bias[m] fp32 [N].  M % 128 == 0, N % tile_n == 0, K % 64 == 0; every pointer 16-byte aligned.  With
 * acc = A W^T:
 *   IEFVAD_SPLIT_EPI_BIAS            C[M, ldc] = acc + bias
 *   IEFVAD_SPLIT_EPI_QKV             C = (acc + bias) * (column < qcols ? alpha : 1)
 *   IEFVAD_SPLIT_EPI_BIAS_RELU       C = relu(acc + bias)
 *   IEFVAD_SPLIT_EPI_BIAS_RESID      C = acc + bias + R                       (R [M, ldc])
 *   IEFVAD_SPLIT_EPI_REFINE          C = R - alpha * (acc + bias)             (C may be R: in place)
 *   IEFVAD_SPLIT_EPI_HEADS           N = 2 ldc: columns < ldc go to C, the others to C2, both [M, ldc]
 *   IEFVAD_SPLIT_EPI_BIAS_RELU_DOT   nz = 1: h = relu(acc + bias); C2[M, N / 128] receives, per 128-column tile, the sum of
 *                                    h[m][n] * R[n] (R [N]); h goes to C unless C is null
 * Added without a change to any other entry: IEFVAD_ABI_VERSION stays. */
#define IEFVAD_SPLIT_EPI_BIAS 0
#define IEFVAD_SPLIT_EPI_QKV 1
#define IEFVAD_SPLIT_EPI_BIAS_RELU 2
#define IEFVAD_SPLIT_EPI_BIAS_RESID 3
#define IEFVAD_SPLIT_EPI_REFINE 4
#define IEFVAD_SPLIT_EPI_HEADS 5
#define IEFVAD_SPLIT_EPI_BIAS_RELU_DOT 6
typedef struct iefvad_gemm_split_io {
    const float* A[2];
    const void* W[2];
    const float* bias[2];
    const float* R[2];
    float* C[2];
    float* C2[2];
} iefvad_gemm_split_io;
/* Launches of the 128 x 256 tiling since the library was loaded, by any handle or entry of the process (counted where the kernel
 * is launched; a replayed hipGraph counts at capture).  The two tilings give the same bits, so nothing else shows which one ran. */
uint64_t iefvad_gemm_split_wide_launches(void);
int iefvad_gemm_split_unit(const iefvad_gemm_split_io* io, int32_t M, int32_t N, int32_t K, int32_t ldc, int32_t epilogue,
                           int32_t qcols, float alpha, int32_t nz, int32_t tile_n, void* stream);

/* The same projection on the SMALL tiling of the bf16x6 arithmetic (32 x 128 block tile, four waves of 32 x 32: a quarter of the
 * 128 x 128 tiling's MFMAs per wave and k-tile), the kernel the batch-invariant mode launches below the split kernels' crossover.
 * Same operands and epilogues as iefvad_gemm_split_unit, no tile_n; M % 32 == 0, N % 128 == 0, K % 64 == 0, K >= 64.  Every
 * output element is summed in the order of the other two tilings: the results agree with theirs bit for bit, and this entry lets a
 * unit test say so.  iefvad_gemm_split_small_launches counts this kernel's launches the way iefvad_gemm_split_wide_launches
 * counts the wide tiling's.  Added without a change to any other entry: IEFVAD_ABI_VERSION stays. */
int iefvad_gemm_split_small_unit(const iefvad_gemm_split_io* io, int32_t M, int32_t N, int32_t K, int32_t ldc, int32_t epilogue,
                                 int32_t qcols, float alpha, int32_t nz, void* stream);
uint64_t iefvad_gemm_split_small_launches(void);

/* ---- unit entry for the kernels of the training step's backward pass (per-kernel parity tests) --------------------------
 * Launches ONE kernel of csrc/backward.h (or the split TN product of csrc/gemm_split_tn.h with its reduction) through the launch
 * helper iefvad_train_forward / iefvad_train_backward use, on caller-supplied DEVICE buffers: the kernel symbol and the grid are
 * the training step's.  No handle.  `args` points to the kind's argument block below, `args_bytes` is its sizeof (checked).  The
 * entry checks shapes as the helpers do and nothing about buffer sizes: the caller owns every extent named below.  Floats
 * throughout; 16-byte aligned pointers unless said otherwise.  Enqueued on `stream`.
 *   IEFVAD_BWD_BGEMM               iefvad_bwd_bgemm: C[z][i, j] = act(alpha * sum_k A(i, k) B(j, k) + bias[j] + R[z][i, j]), zeroed where
 *                                  G[z][i, j] <= 0; akc != 0: A(i, k) = A[i * lda + k], else A[k * lda + i]; bkc likewise; batch
 *                                  z = z1 * nz2 + z2 < nz at operand offsets z1 * x1 + z2 * x2; a_drop != 0: A carries a dropout mask
 *                                  in its sign bits, A(i, k) = sign ? 0 : stored * a_drop; act 0 none, 1 QuickGELU, 2 ELU.
 *                                  M % 128 == 0, N % 128 == 0 or N % 96 == 0, K % 16 == 0, lda and ldb multiples of 4.
 *   IEFVAD_BWD_SPLIT_TN            iefvad_bwd_split_tn: part[z] = dY[rows of slice z]^T X[rows of slice z] for `slices` ragged row
 *                                  slices (slice z owns the 16-row tiles [z nk / slices, (z + 1) nk / slices), nk = rows / 16),
 *                                  dW = alpha * sum_z part[z]; with colsum_part: colsum_part[z] = column sums of dY over slice z and
 *                                  db = alpha * their sum.  dY [rows, n_out], X [rows, 768], part [slices, n_out, 768], dW [n_out, 768],
 *                                  colsum_part [slices, n_out], db [n_out].  rows % 16 == 0, n_out % 128 == 0, 1 <= slices <= nk / 8.
 *   IEFVAD_BWD_SOFTMAX_DROPOUT     iefvad_bwd_softmax_dropout: S [rows, 256] scores in, sign-carrying probabilities out; drop != 0:
 *                                  element idx is dropped (sign set) where keep[idx] == 0, or without keep where the library's
 *                                  generator draws below p for (seed, idx)
 *   IEFVAD_BWD_SOFTMAX_BWD         iefvad_bwd_softmax_bwd: dPd [rows, 256] <- Pd .* dPd - |Ps| rowsum(Pd .* dPd), Pd = sign ? 0 : Ps * scale
 *   IEFVAD_BWD_COLSUM              iefvad_bwd_colsum: part[b][j] = sum of Y[r, j] over rows [128 b, 128 b + 128) below `rows`;
 *                                  Y [rows, ld], part [ceil(rows / 128), ncols]; any alignment
 *   IEFVAD_BWD_REDUCE_PARTS        iefvad_bwd_reduce, job 0 alone: out[i] = alpha * sum_p part[p * stride + i], i < n; any alignment
 *   IEFVAD_BWD_REDUCE_PARTS_MULTI  iefvad_bwd_reduce: jobs 0 .. count - 1 in ONE launch (a fifth job is ignored, as a null `out` is)
 *   IEFVAD_BWD_SCORER              iefvad_bwd_scorer: g = dlogit w (+ dfused) [rows, 768]; part_w [ceil(rows / 32), 768] and part_b
 *                                  [ceil(rows / 32)]: per 32-row block, the sums of dlogit * z and of dlogit
 *   IEFVAD_BWD_FUSION              iefvad_bwd_fusion: the precision-weighted fusion's backward; dh_i, dh_e [rows, 1536] = d mu | d logvar
 *   IEFVAD_BWD_LAYERNORM           iefvad_bwd_layernorm: dx [rows, 768] (may be dy), part_g and part_b [ceil(rows / 32), 768]
 * Added without a change to any other entry: IEFVAD_ABI_VERSION stays. */
#define IEFVAD_BWD_BGEMM 0
#define IEFVAD_BWD_SPLIT_TN 1
#define IEFVAD_BWD_SOFTMAX_DROPOUT 2
#define IEFVAD_BWD_SOFTMAX_BWD 3
#define IEFVAD_BWD_COLSUM 4
#define IEFVAD_BWD_REDUCE_PARTS 5
#define IEFVAD_BWD_REDUCE_PARTS_MULTI 6
#define IEFVAD_BWD_SCORER 7
#define IEFVAD_BWD_FUSION 8
#define IEFVAD_BWD_LAYERNORM 9
typedef struct iefvad_bwd_bgemm {
    const float* A; const float* B; float* C; const float* R; const float* G; const float* bias;
    int64_t a1, a2, b1, b2, c1, c2;
    int32_t M, N, K, lda, ldb, ldc, nz, nz2, akc, bkc, act;
    float alpha, a_drop;
} iefvad_bwd_bgemm;
typedef struct iefvad_bwd_split_tn {
    const float* dY; const float* X; float* part; float* dW; float* colsum_part; float* db;
    int32_t rows, n_out, slices;
    float alpha;
} iefvad_bwd_split_tn;
typedef struct iefvad_bwd_softmax_dropout {
    float* S; const uint8_t* keep; uint64_t seed; int64_t rows; int32_t drop; float p;
} iefvad_bwd_softmax_dropout;
typedef struct iefvad_bwd_softmax_bwd {
    const float* Ps; float* dPd; int64_t rows; float scale;
} iefvad_bwd_softmax_bwd;
typedef struct iefvad_bwd_colsum {
    const float* Y; float* part; int32_t ld, rows, ncols;
} iefvad_bwd_colsum;
typedef struct iefvad_bwd_reduce {
    const float* part[5]; float* out[5]; uint64_t stride[5]; uint64_t n[5]; int32_t nparts[5]; float alpha[5]; int32_t count;
} iefvad_bwd_reduce;
typedef struct iefvad_bwd_scorer {
    const float* dlogit; const float* dfused; const float* z; const float* w; float* g; float* part_w; float* part_b; int32_t rows;
} iefvad_bwd_scorer;
typedef struct iefvad_bwd_fusion {
    const float* mu_i; const float* lv_i; const float* mu_e; const float* lv_e; const float* gz;
    const float* d_mu_i; const float* d_lv_i; const float* d_mu_e; const float* d_lv_e; const float* d_n_i; const float* d_n_e;
    float* dh_i; float* dh_e;
    int32_t rows; float factor, eps;
} iefvad_bwd_fusion;
typedef struct iefvad_bwd_layernorm {
    const float* x; const float* dy; const float* g; float* dx; float* part_g; float* part_b; int32_t rows; float eps;
} iefvad_bwd_layernorm;
int iefvad_backward_unit(int32_t kind, const void* args, size_t args_bytes, void* stream);

/* Batch-invariant mode of an IEFVAD_COMPUTE_BF16X6 handle (on != 0; off is the default).  By default a bf16x6 handle runs a
 * micro-batch's projections and attention in the split arithmetic only from 6 chunks on and in the f32 arithmetic below, so a
 * video's results differ at the 1e-7 level with what else is in the launch.  In this mode every projection and every attention of
 * the evaluation forward runs in the split arithmetic at every row count (the small tiling above takes the small launches): the
 * results of a chunk or a video are the same bits at B = 1 and B = 8192, on the padded and the valid-row routes, per video,
 * packed or from host lists.  The arithmetic stays fp32-accurate (the gates of the bf16x6 mode hold); a small call costs more than
 * in the default mode.  IEFVAD_COMPUTE_F32 and IEFVAD_COMPUTE_BF16 handles are already batch-invariant: the call succeeds and
 * changes nothing.  IEFVAD_COMPUTE_FP16X3 is refused: its operand scales are per chunk and per running maximum.  The call waits
 * for the device and releases the handle's cached hipGraphs, so a later small forward captures the new launches.  Training entries
 * keep their own kernel rule and are not affected.  Not thread-safe against calls on the same handle.  IEFVAD_ABI_VERSION stays. */
int iefvad_set_batch_invariant(iefvad_handle* h, int on);

/* Call-time step count: every EVALUATION entry of the handle (dense, scaled, perturbed, attn, the whole-video entries, the host
 * lists) runs refinement blocks 0 .. steps - 1 of the handle's cfg.num_steps, then the classifier.  0 <= steps <= cfg.num_steps;
 * the default is cfg.num_steps; a value outside the range is refused by name and changes nothing.  The results are, bit for bit,
 * those of a handle created with num_steps = steps that was given the first `steps` blocks -- both launch the same kernels on the
 * same data (IEFVAD_COMPUTE_BF16: the chain kernel reads a prefix of its packed stream; IEFVAD_COMPUTE_BF16X6: the folded scorer's
 * vector exists for every block).  Cached hipGraphs are keyed by the count.  iefvad_train_forward refuses a handle whose count is
 * not cfg.num_steps.  Makes no HIP call.  Not thread-safe against calls on the same handle.  IEFVAD_ABI_VERSION stays. */
int iefvad_set_steps(iefvad_handle* h, int32_t steps);

/* ---- the refinement trajectory -------------------------------------------------------------------------------------
 * One forward, and per snippet the whole K-step iteration z_{k+1} = z_k - lambda (W2_k relu(W1_k z_k + b1_k) + b2_k):
 *   logits_steps[k * stride + r] = c . z_k + b_c          k = 0 .. steps      (logits: the caller applies the sigmoid)
 *   delta_norm[k * stride + r]   = ||z_{k+1} - z_k||_2    k = 0 .. steps - 1  (= lambda ||r_k||, the convergence diagnostic)
 * with steps the handle's current count (iefvad_set_steps) and r the row of the call: b T + t (dense) or the packed row (whole
 * videos; valid rows only, no padding is computed or written).  `stride` is the number of ELEMENTS between two steps, at least the
 * call's rows.  Either pointer may be null, not both; device pointers, 4-byte aligned.  Row k of logits_steps is what a
 * steps = k call returns as `logits` (the same bits wherever that call uses the plain scorer; row `steps` is this call's logits).
 * Every other output of the call has the bits of the same call without a trajectory.  Cost: one HBM-bound row kernel per state
 * (iefvad_step_probe_kernel, csrc/trajectory.h) and a second [rows, D] fp32 state buffer behind the base workspace -- use the
 * _trajectory_workspace_bytes queries.  IEFVAD_COMPUTE_BF16 runs a trajectory pass on its launch-per-projection route (2 K GEMM
 * launches in place of the one chain kernel; the same bits, slower); IEFVAD_COMPUTE_BF16X6 stores h of the last step and forms
 * z_steps as a call that returns `fused` does.  Direct launches (no hipGraph).  Null-argument and range checks come before the
 * first launch.  Added without a change to any other entry: IEFVAD_ABI_VERSION stays. */
typedef struct iefvad_trajectory { float* logits_steps; float* delta_norm; size_t stride; } iefvad_trajectory;
size_t iefvad_trajectory_workspace_bytes(const iefvad_handle* h, int32_t B);
int iefvad_forward_trajectory(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B, void* workspace,
                              size_t workspace_bytes, const iefvad_outputs* out, const iefvad_trajectory* trajectory, void* stream);
/* Mirrors iefvad_forward_videos: [steps + 1, stride] and [steps, stride] in packed order. */
size_t iefvad_videos_trajectory_workspace_bytes(const iefvad_handle* h, const int32_t* lengths, int32_t nvideos);
int iefvad_forward_videos_trajectory(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype,
                                     const int32_t* lengths, int32_t nvideos, int32_t nan_to_num, void* workspace,
                                     size_t workspace_bytes, float* logits, float* w_i_mean, float* w_e_mean,
                                     const iefvad_trajectory* trajectory, void* stream);

/* ---- fusion ablations ------------------------------------------------------------------------------------------------
 * One forward, and per snippet the score the model gives when the precision-weighted fusion (imf_vad.py:130-144)
 *   w_i = f exp(-lv_i), w_e = f exp(-lv_e), den = w_i + w_e + eps, z0 = (w_i / den) mu_i + (w_e / den) mu_e
 * is altered by one substitution, followed by the unchanged refinement (the handle's current iefvad_set_steps count) and classifier:
 *   IEFVAD_VARIANT_FUSED  none: reproduces the call's `logits` (a self-check, and so that one result holds the whole table)
 *   IEFVAD_VARIANT_IMAGE  w_e := 0  (the event branch removed at the fusion: z0 = w_i / (w_i + eps) mu_i + 0 mu_e)
 *   IEFVAD_VARIANT_EVENT  w_i := 0
 *   IEFVAD_VARIANT_EQUAL  lv_i := lv_e := 0  (both precisions equal: w_i = w_e = f)
 * The operation order of the expression is kept, 0 mu and eps included, so NaN and inf behave as the substituted expression does.
 *   logits[v * stride + r], v in the order of kind[0 .. count - 1], r the row of the call: b T + t (dense) or the packed row (whole
 * videos; valid rows only, no padding is written).  Values are before the sigmoid.  `stride`: ELEMENTS between two variants, at
 * least the call's rows.  `logits`: a device pointer, 4-byte aligned.  1 <= count <= 4, every kind at most once.
 * Encoder and heads run once; behind the call's own tail one row kernel (iefvad_fusion_variants_kernel, csrc/variants.h) forms the
 * variants' z0 from the pass's mu / logvar and the refinement + scorer run once more on the stacked count x rows states, with the
 * kernels the unchanged selection rules pick for that row count.  IEFVAD_COMPUTE_F32 and IEFVAD_COMPUTE_BF16: the FUSED row has the
 * bits of the call's logits; IEFVAD_COMPUTE_BF16X6: within the arithmetic's tolerance (the stacked set may run on the split
 * kernels where the call's rows do not), the same bits with iefvad_set_batch_invariant.  Every other output of the call has the
 * bits of the same call without variants.  The stacked state, its scratch and logits live behind the base workspace: use the
 * _variants_workspace_bytes queries.  Direct launches (no hipGraph).  Refused by name before any launch: IEFVAD_COMPUTE_FP16X3
 * (not covered: its per-chunk running-max words have no home for the stacked states), a null struct or logits pointer, a
 * misaligned logits pointer, count outside 1..4, an unknown or repeated kind, a stride below the call's rows, a workspace smaller
 * than the query says.  Not covered: the host-list entries and training.  Added without a change to any other entry:
 * IEFVAD_ABI_VERSION stays. */
enum { IEFVAD_VARIANT_FUSED = 0, IEFVAD_VARIANT_IMAGE = 1, IEFVAD_VARIANT_EVENT = 2, IEFVAD_VARIANT_EQUAL = 3 };
typedef struct iefvad_variants { int32_t count; int32_t kind[4]; float* logits; size_t stride; } iefvad_variants;
size_t iefvad_variants_workspace_bytes(const iefvad_handle* h, int32_t B, int32_t count);
int iefvad_forward_variants(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B, void* workspace,
                            size_t workspace_bytes, const iefvad_outputs* out, const iefvad_variants* variants, void* stream);
/* Mirrors iefvad_forward_videos: [count, stride] in packed order. */
size_t iefvad_videos_variants_workspace_bytes(const iefvad_handle* h, const int32_t* lengths, int32_t nvideos, int32_t count);
int iefvad_forward_videos_variants(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype,
                                   const int32_t* lengths, int32_t nvideos, int32_t nan_to_num, void* workspace,
                                   size_t workspace_bytes, float* logits, float* w_i_mean, float* w_e_mean,
                                   const iefvad_variants* variants, void* stream);

/* ---- score samples ---------------------------------------------------------------------------------------------------
 * One forward, and per snippet S scores drawn from the model's own predictive spread: the heads predict a mean and a log-variance
 * per modality, and the fusion (imf_vad.py:130-144) collapses each Gaussian to its mean.  Here the means are sampled instead.  The
 * reference never samples, so these semantics are this library's own ("parity unpinned", as for the row noise above).  For sample
 * s = 0 .. samples - 1, modality m (0 image, 1 event), snippet id r, column c:
 *   seed_s = seed + s * 0x9E3779B97F4A7C15 (mod 2^64)
 *   eps    = the standard normal of the row noise (iefvad_perturb) for (seed_s, r, m, c)
 *   sd_m   = scale * exp(0.5 lv_m) / sqrt(f)        f: the Student-t factor (nu + 1) / nu, 1 for the Gaussian likelihood; so
 *                                                   sd_m^2 = scale^2 / w_m, the variance the fusion itself assigns to modality m
 *   mu~_m  = mu_m + eps * sd_m
 *   z0_s   = (w_i / den) mu~_i + (w_e / den) mu~_e  with the call's own w_i, w_e, den = w_i + w_e + epsilon
 * followed by the unchanged refinement (the handle's current iefvad_set_steps count) and classifier.  Literal fp32, no clamps: inf
 * and NaN behave as the expression does.  scale = 0 reproduces the call's logits in every sample (within the arithmetic's tolerance).
 * The snippet id is the one the row noise uses: sample_rows[row] (a DEVICE int32 vector over the call's rows, nullable), else the row
 * of the call -- b T + t (dense), the packed row (whole videos).  A snippet with the same id gets the same draws on either route, in
 * any batch composition and in any micro-batch pass.
 *   logits_samples[s * stride + row]   before the sigmoid; `stride`: ELEMENTS between two samples, at least the call's rows
 *   score_mean[row], score_std[row]    mean and population standard deviation (ddof = 0) over s of sigmoid(logits_samples[s]):
 *                                      formed on the device in fp32, samples in index order, two passes, no atomics -- the same call
 *                                      gives the same bits
 * All three are device fp32 pointers, 4-byte aligned; on the whole-video entry only valid rows are written.
 * Encoder and heads run once.  Behind the call's own tail, per group of up to 4 samples, one row kernel
 * (iefvad_sample_states_kernel, csrc/samples.h) forms the group's z0 from the pass's mu / logvar and the refinement + scorer run once
 * more on the stacked states with the kernels the unchanged selection rules pick for that row count; iefvad_samples_reduce_kernel
 * follows the last group.  Every other output of the call has the bits of the same call without samples.  One group's stacked state,
 * scratch and logits live behind the base workspace: use the _samples_workspace_bytes queries (they do not depend on S).  Direct
 * launches (no hipGraph).  Refused by name before any launch: IEFVAD_COMPUTE_FP16X3 (its per-chunk running-max words have no home for
 * the stacked states), a null struct, samples outside 1..64, a negative or non-finite scale, a null or misaligned result pointer, a
 * stride below the call's rows, a workspace smaller than the query says.  Not covered: the host-list entries and training.  Added
 * without a change to any other entry: IEFVAD_ABI_VERSION stays. */
typedef struct iefvad_samples {
    int32_t samples;                /* S, 1..64 */
    uint64_t seed;
    float scale;                    /* >= 0, finite; 1 = the heads' own spread */
    const int32_t* sample_rows;     /* device, nullable */
    float* logits_samples;          /* device [S, stride] */
    size_t stride;
    float* score_mean;              /* device [rows] */
    float* score_std;               /* device [rows] */
} iefvad_samples;
size_t iefvad_samples_workspace_bytes(const iefvad_handle* h, int32_t B);
int iefvad_forward_samples(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B, void* workspace,
                           size_t workspace_bytes, const iefvad_outputs* out, const iefvad_samples* samples, void* stream);
/* Mirrors iefvad_forward_videos: [S, stride] and the two vectors in packed order. */
size_t iefvad_videos_samples_workspace_bytes(const iefvad_handle* h, const int32_t* lengths, int32_t nvideos);
int iefvad_forward_videos_samples(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype,
                                  const int32_t* lengths, int32_t nvideos, int32_t nan_to_num, void* workspace,
                                  size_t workspace_bytes, float* logits, float* w_i_mean, float* w_e_mean,
                                  const iefvad_samples* samples, void* stream);

/* ---- online scores: trailing-window evaluation -------------------------------------------------------------------
 * iefvad_forward_videos and the reference's test() cut a video at fixed multiples of 256 snippets, and the temporal encoder attends
 * over the whole chunk (imf_vad.py:115, unmasked): the score of snippet t may depend on up to 255 FUTURE snippets.  This entry answers
 * what the model would have said live with a look-ahead below `stride` snippets.  The reference never does this, so these semantics
 * are this library's own ("parity unpinned", as for the row noise and the score samples); iefvad_forward on host-built windows pins
 * them exactly.  With 1 <= stride <= history <= 256, a video of n snippets has windows j = 1 .. ceil(n / stride):
 *   end_j = min(j stride, n)      start_j = max(0, end_j - history)      read0_j = (j - 1) stride
 * Window j is a 256-row chunk: rows [start_j, end_j) of the video, then zero rows (the chunker's convention for a short video).  It
 * goes through the unchanged model, and only snippets [read0_j, end_j) -- rows read0_j - start_j .. of the window -- are read out.
 * Every snippet belongs to exactly one window; its results depend on no snippet at or beyond end_j, so stride = 1 is strictly causal.
 * n = 300, stride = 128, history = 256: (start, end, read0) = (0,128,0) (0,256,128) (44,300,256).
 * nan_to_num (any non-zero value) is the per-video rule of iefvad_forward_videos, decided over the WHOLE video, once per video: a
 * NaN anywhere in a video changes how its earlier windows are loaded.  That one rule is NOT causal.
 * Arguments and results are those of iefvad_forward_videos: packed valid rows in, logits / w_i_mean / w_e_mean [sum(lengths)] out
 * (the latter two nullable).  The call's windows run in passes of at most micro_batch windows (csrc/window_plan.h); the encoder runs
 * on row-compressed windows (whole chunks with IEFVAD_DENSE_ENCODER=1); behind the last LayerNorm iefvad_readout_rows_kernel gathers
 * the read-out rows, and heads, fusion, refinement and scorer run on those alone, with the kernels the unchanged selection rules pick
 * for that row count.  Only the encoder's cost grows with the number of windows.  stride = history = 256 on videos whose lengths
 * are <= 256 or multiples of 256 builds the chunks of iefvad_forward_videos.
 * Refused by name before any launch: IEFVAD_COMPUTE_FP16X3 (its operand scales are per chunk and its tail keeps whole chunks), null
 * parameters, stride or history out of range, a workspace smaller than iefvad_videos_online_workspace_bytes says (0 for arguments no
 * call would accept).  Direct launches (no hipGraph).  Added without a change to any other entry: IEFVAD_ABI_VERSION stays. */
typedef struct iefvad_online {
    int32_t stride;                 /* 1..history: snippets read out per window; the look-ahead is below it */
    int32_t history;                /* stride..256: snippets a window holds at most */
} iefvad_online;
size_t iefvad_videos_online_workspace_bytes(const iefvad_handle* h, const int32_t* lengths, int32_t nvideos, const iefvad_online* online);
int iefvad_forward_videos_online(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype,
                                 const int32_t* lengths, int32_t nvideos, int32_t nan_to_num, const iefvad_online* online,
                                 void* workspace, size_t workspace_bytes, float* logits, float* w_i_mean, float* w_e_mean,
                                 void* stream);

/* The exact three-term bf16 split of n fp32 values (n % 4 == 0): planes[0..n) = bf16(x),
 * planes[n..2n) = bf16(x - p0), planes[2n..3n) = bf16(x - p0 - p1), round-to-nearest-even; x == p0 + p1 + p2
 * for finite x.  What iefvad_set_weights applies to every projection matrix in IEFVAD_COMPUTE_BF16X6. */
int iefvad_split_bf16x3(const float* src, void* planes, size_t n, void* stream);

/* The same for `count` matrices in ONE launch per 32 of them -- what iefvad_set_weights and the training backward use (a training
 * step re-splits every projection matrix and its transpose: 90 small launches before).  src / planes / n / rows are HOST arrays of
 * device pointers and sizes.  rows[i] == 0: planes[i] receives the split of src[i] as above (n[i] % 4 == 0).  rows[i] == R > 0:
 * src[i] is a row-major [R, n[i] / R] matrix and planes[i] receives the split of its TRANSPOSE [n[i] / R, R] (R % 64 == 0,
 * (n[i] / R) % 32 == 0) -- the operand of dX = dY W as an NT product.  Bit for bit the planes of iefvad_split_bf16x3. */
int iefvad_split_bf16x3_many(const float* const* src, void* const* planes, const size_t* n, const int32_t* rows, int32_t count,
                             void* stream);

/* ---- multi-GPU score gather ------------------------------------------------------------------
 * The reference has no collective at all (/root/reference/main.py:7 imports torch.distributed and never uses it);
 * what it fixes is the ORDER of the score vector: per-video scores are concatenated in test-list order and the
 * ground truth is indexed by the running snippet offset (/root/reference/test.py:123-129,153).  Videos shard across
 * ranks in contiguous ranges, so the rank-order concatenation of the ranks' score vectors is that order, and one
 * RCCL exchange over xGMI closes the evaluation.  librccl.so.1 is bound at run time (dlopen; a copy the process has
 * already loaded -- PyTorch's -- is preferred), so single-GPU users never load it.
 *
 * One process per GPU.  Rank 0 calls iefvad_comm_unique_id and hands the 128 bytes to the other ranks by any
 * host-side channel (the Python harness uses the torch.distributed store); every rank then calls
 * iefvad_comm_create with the device it will gather on current.  */
#define IEFVAD_COMM_ID_BYTES 128
typedef struct iefvad_comm iefvad_comm;

int iefvad_comm_unique_id(void* id_bytes /* host, IEFVAD_COMM_ID_BYTES */);
int iefvad_comm_create(const void* id_bytes, int32_t nranks, int32_t rank, iefvad_comm** out);
/* number of ranks RCCL itself reports for the communicator (ncclCommCount); 0 for a NULL handle */
int32_t iefvad_comm_nranks(const iefvad_comm* c);
void iefvad_comm_destroy(iefvad_comm* c);

/* RCCL's own version number (ncclGetVersion) once librccl is bound, 0 when it cannot be bound in this process.  Lets every
 * rank check -- and agree, over whatever host channel it has -- BEFORE the collective iefvad_comm_create that all ranks
 * will get through it. */
int32_t iefvad_rccl_version(void);

/* gathered[offset(r) .. offset(r) + counts[r]) = rank r's `local[0 .. counts[r])`, for every r, on every rank;
 * offset(r) = counts[0] + ... + counts[r-1].  `local`, `gathered` are device pointers to fp32; `counts` is a HOST
 * array of nranks element counts that every rank passes identically (shards are cut from the shared, ordered test
 * list -- harness.partition_by_snippets -- so no count exchange is needed), or NULL when every rank contributes
 * `count` elements.  `gathered_capacity` = the number of fp32 elements `gathered` can hold; a call whose ranks
 * contribute more fails before anything is enqueued.  `local` may be this rank's own slot of `gathered` (in place);
 * any other overlap is an error.  Equal counts run as ONE ncclAllGather; unequal counts as one grouped
 * ncclSend/ncclRecv exchange (every pair has a direct xGMI link) plus a device-to-device copy of the rank's own slice.
 * Enqueued on `stream` (hipStream_t); returns without synchronising. */
int iefvad_gather_scores(iefvad_comm* c, const float* local, size_t count, const int64_t* counts, float* gathered,
                         size_t gathered_capacity, void* stream);

/* The exchange iefvad_gather_scores would enqueue for (nranks, rank, counts | count), as data -- host only, no GPU, no
 * communicator: summary[0..4] = {equal counts (one all-gather) ? 1 : 0, this rank's offset, this rank's count, total
 * elements, number of point-to-point steps}; steps[4 i ..] = {peer, elements sent to it, offset at which its slice is
 * received, elements received}, one entry per peer in rank order (unequal counts only; `steps` may be NULL, else it holds
 * 4 (nranks - 1) values).  Zero-length transfers are listed with count 0 and are not issued. */
int iefvad_gather_plan(int32_t nranks, int32_t rank, const int64_t* counts, int64_t count, int64_t* summary, int64_t* steps);

const char* iefvad_last_error(void);
void iefvad_destroy(iefvad_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* IEFVAD_H */

// libiefvad.so -- C ABI (include/iefvad.h) and launch orchestration of the IEF-VAD fusion forward
// on MI355X.  Replaces MMFMIL.forward -> MultiModal_Fusion_Attn_Iter.forward
// (/root/reference/model/imf_vad.py:40-44, :109-161).  gfx950 only; no host fallback.
#include "../../include/iefvad.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <exception>
#include <new>
#include <thread>
#include <utility>
#include <vector>

#include "attention_f32.h"
#include "attention_maps.h"
#include "attention_bf16.h"
#include "attention_pbf16.h"
#include "attention_split.h"
#include "common.h"
#include "launch_rules.h"
#include "workspace_tail.h"
#include "gather.h"
#include "gemm_f32.h"
#include "gemm_bf16.h"
#include "gemm_split.h"
#include "gemm_split_wide.h"
#include "gemm_split_small.h"
#include "rowops.h"
#include "refine_chain_bf16.h"
#include "outproj_ln_chain_bf16.h"
#include "outproj_ln_pchain_bf16.h"
#include "inproj_chain_bf16.h"
#include "heads_chain_bf16.h"
#include "heads_pchain_bf16.h"
#include "ragged.h"
#include "resample.h"
#include "loss.h"
#include "gemm_split_tn.h"
#include "backward.h"
#include "metrics.h"
#include "similarity.h"
#include "trajectory.h"
#include "variants.h"
#include "samples.h"

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                          __FILE__, __LINE__);                                   \
    } while (0)

// ------------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------------
// Every resident form of one projection matrix W [N, D] with its bias [N].  The fp32 pair lives in the handle's arena; each other
// form is filled only in the arithmetic that reads it, in an arena of its own, by a walk in for_each_proj's order.
struct ProjW {
    int N;                 // output features: 3 D (in_proj), D (out_proj, refinement), 2 D (mu.weight stacked over logvar.weight)
    float* w;
    float* b;
    bf16_t* wb;            // IEFVAD_COMPUTE_BF16: round-to-nearest-even copy
    bf16_t* ws;            // IEFVAD_COMPUTE_BF16X6: three-plane split [3][N][D]
    _Float16* wh;          // IEFVAD_COMPUTE_FP16X3: two scaled fp16 planes [2][N][D] ...
    const float* wa;       // ... and the matrix's running-max word (in [0, kAmaxActBase) of amax_dev)
    bf16_t* wst;           // bf16x6 training: three-plane split of the TRANSPOSE [3][D][N] (dX = dY W as an NT product; train.h)
};

struct iefvad_handle {
    iefvad_config cfg;
    int D, DH;             // embed dim and head dim: 768 / 96, or 512 / 64 (iefvad_create_ex: the f32 forward only)
    int device;
    bool weights_set;
    LaunchPolicy policy;   // the environment switches of kernel selection (launch_rules.h), read once at iefvad_create
    char* iproj_stream[2][IEFVAD_MAX_LAYERS];   // bf16 mode: in_proj weights in per-wave fragment order, q | k | v passes (inproj_chain_bf16.h)
    char* heads_stream;    // bf16 mode: the four head matrices in per-wave fragment order (heads_chain_bf16.h)
    char* oproj_stream[2][IEFVAD_MAX_LAYERS];   // bf16 mode: out_proj weights in per-wave fragment order (outproj_ln_chain_bf16.h)
    bool train_attn_unfused; // IEFVAD_TRAIN_ATTN=unfused: bf16x6 train-mode attention on the three-launch path (train.h)
    bool hostpipe_trace;   // IEFVAD_HOSTPIPE_TRACE=1: iefvad_forward_videos_host prints its per-pass timeline to stderr (hostpipe.h)
    char* chain_stream;    // bf16 mode: the refinement weights in the chain kernel's per-wave piece order (refine_chain_bf16.h)
    float* arena;          // one allocation holding every repacked weight
    size_t arena_floats;
    // the projection matrices, and the pointers of the other parameters into the arena
    ProjW in[2][IEFVAD_MAX_LAYERS], out[2][IEFVAD_MAX_LAYERS], head[2], ref1[IEFVAD_MAX_STEPS], ref2[IEFVAD_MAX_STEPS];
    float* norm_w[2][IEFVAD_MAX_LAYERS];
    float* norm_b[2][IEFVAD_MAX_LAYERS];
    float* whiten_w[2];
    float* whiten_b[2];
    float* cls_w;
    float* cls_b;
    int steps;             // refinement steps the evaluation entries run: cfg.num_steps unless iefvad_set_steps chose a prefix
    // bf16x6, K >= 1: per block k, v = -lambda W2_k^T c [D] and s0 = b_c - lambda (c . b2_k) [1] of the folded scorer (rowops.h), D + 4
    // floats apart; a forward of `steps` steps reads block steps - 1 (score_fold_of)
    float* score_fold;
    // the arenas of the ProjW forms: bf16 copies (BF16), three-plane splits (BF16X6), fp16 planes (FP16X3); amax_dev holds the
    // running-max words of the matrices (filled at set_weights) and, behind them, of the activations of the current micro-batch
    bf16_t* arena_b;
    bf16_t* arena_s;
    _Float16* arena_h;
    float* amax_dev;
    struct EventPool* events;   // hipEvents of iefvad_forward_timed, reused across calls
    struct GraphCache* graphs;  // hipGraphs of small-batch forwards (cfg.graph_chunks)
    struct MetaRing* meta;      // pinned / device metadata buffers of iefvad_forward_videos
    int num_cus;                // compute units of the device: grid size of the persistent row-block kernels
    // training in the bf16x6 arithmetic: the arena of ProjW::wst, rebuilt by the first backward after every iefvad_set_weights (train.h)
    bf16_t* arena_st; float* zero_bias; bool tplanes_valid;
    struct HostPipe* hostpipe;  // staging slots, copy stream and workspace of iefvad_forward_videos_host (hostpipe.h)
    struct TrainState* train;   // records of the train-mode forwards whose backward is outstanding (train.h)
};
static const int kAmaxActBase = 256;   // running-max slots of the projection matrices (multi-way words); behind them the activations'
static int amax_act_tensors(int L, int K) { return 2 + 6 * L + 2 * K + 1; }   // inputs, per layer att|x|qkv x 2 modalities, z_0..z_K, h_0..h_{K-1}
static size_t amax_words(int L, int K, int mb_chunks) {
    return (size_t)kAmaxActBase * IEF_AMAX_FLOATS + (size_t)amax_act_tensors(L, K) * mb_chunks * IEF_AMAX_PARTS;
}

// chunks per internal pass: 256 (65,536 rows, 2.8 GB of workspace) in fp32 mode; the bf16 kernels are ~100 us
// each at that size and gain another 7 % from 4x longer launches (1024 chunks, 11 GB of workspace)
// the split modes (bf16x6 / fp16x3) gain 2.4 % from 4x longer launches as well (fewer kernel-boundary tails)
static const int kDefaultMicroBatchF32 = 256;
static const int kDefaultMicroBatchBF16 = 1024;

static const float* score_fold_of(const iefvad_handle* h, int steps) {
    return h->score_fold && steps >= 1 ? h->score_fold + (size_t)(steps - 1) * (h->D + 4) : nullptr;
}

static int micro_batch(const iefvad_handle* h) {
    if (h->cfg.micro_batch > 0) return h->cfg.micro_batch < 16384 ? h->cfg.micro_batch : 16384;   // attention grid.z = 2 x chunks
    return h->cfg.compute == IEFVAD_COMPUTE_F32 ? kDefaultMicroBatchF32 : kDefaultMicroBatchBF16;
}

// The one walk over the projection matrices: modality -> layer -> {in, out}, then the heads; then step -> {W1, W2}.  Every derived
// arena (bf16, planes, fp16 planes, transposed planes) is carved in this order, so the order fixes each pointer's offset (the kernels
// assume 16-byte alignment), the fp16x3 running-max word of each matrix and the entry order of a SplitMany table.
template <typename F>
static int for_each_proj(iefvad_handle* h, F f) {
    for (int m = 0; m < 2; ++m) {
        for (int l = 0; l < h->cfg.num_layers; ++l) {
            if (int rc = f(h->in[m][l])) return rc;
            if (int rc = f(h->out[m][l])) return rc;
        }
        if (int rc = f(h->head[m])) return rc;
    }
    for (int k = 0; k < h->cfg.num_steps; ++k) {
        if (int rc = f(h->ref1[k])) return rc;
        if (int rc = f(h->ref2[k])) return rc;
    }
    return 0;
}
// elements of all the matrices for_each_proj visits
static size_t proj_elems(const iefvad_handle* h) {
    const size_t DD = (size_t)h->D * h->D;
    return 2 * (size_t)h->cfg.num_layers * (3 * DD + DD) + 2 * (2 * DD) + (size_t)h->cfg.num_steps * 2 * DD;
}

extern "C" int iefvad_abi_version(void) { return IEFVAD_ABI_VERSION; }

extern "C" const char* iefvad_last_error(void) { return g_err; }

// The D=512 (head dim 64) forward: ViT-B/16 features, the f32 arithmetic's kernels only
#define IEF_D512 512

// Every kernel launched with more dynamic LDS than the default limit allows, with its byte count.  fn == nullptr: raise the limit of
// all of them (iefvad_create); else of that kernel alone (the unit entries that run without a handle).  Returns the first error.
static hipError_t raise_lds_limit(const void* fn = nullptr) {
    static const struct { const void* fn; int bytes; } table[] = {
        {(const void*)iefvad_gemm_bf16_kernel, GB2_LDS_BYTES},
        {(const void*)iefvad_gemm_bf16_pipe_kernel, GB2_LDS_BYTES},
        {(const void*)iefvad_gemm_bf16_w256_kernel, GB3_LDS_BYTES},
        {(const void*)iefvad_refine_chain_bf16_kernel, RC_LDS_BYTES},
        {(const void*)iefvad_outproj_ln_chain_bf16_kernel, OC_LDS_BYTES},
        {(const void*)iefvad_outproj_ln_pchain_bf16_kernel<true, true>, OP_LDS_BYTES},
        {(const void*)iefvad_outproj_ln_pchain_bf16_kernel<true, false>, OP_LDS_BYTES},
        {(const void*)iefvad_outproj_ln_pchain_bf16_kernel<false, true>, OP_LDS_BYTES},
        {(const void*)iefvad_heads_pchain_bf16_kernel, HP_LDS_BYTES},
        {(const void*)iefvad_gemm_split_tn256_kernel, TN_LDS_BYTES_OF(4)},
        {(const void*)iefvad_attention_pbf16_kernel, APB_LDS_BYTES},
        {(const void*)iefvad_attention_pbf16_rows_kernel, APB_LDS_BYTES},
        {(const void*)iefvad_gemm_f32_t256_kernel, GB2_LDS_BYTES},
        {(const void*)iefvad_gemm_split_n128_kernel, GS_LDS_BYTES_OF(2)},
        {(const void*)iefvad_attention_split_kernel, ATS_LDS_BYTES},
        {(const void*)iefvad_attention_split_rows_kernel, ATS_LDS_BYTES},
        {(const void*)iefvad_attention_split_train_kernel, ATS_LDS_BYTES},
        {(const void*)iefvad_attention_split_ds_kernel, ATS_LDS_BYTES},
        {(const void*)iefvad_attention_split_train_mask_kernel, ATS_LDS_BYTES},
        {(const void*)iefvad_heads_chain_bf16_kernel, HC_LDS_BYTES},
        {(const void*)iefvad_inproj_chain_bf16_kernel, IC_LDS_BYTES},
        {(const void*)iefvad_inproj_chain_f32in_kernel, IC_LDS_BYTES},
        {(const void*)iefvad_attention_split_f16_kernel, ATS_LDS_BYTES},
        {(const void*)iefvad_gemm_split_f16_n128_kernel, GS_LDS_BYTES_OF(2)},
    };
    for (const auto& k : table)
        if (!fn || fn == k.fn)
            if (hipError_t e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes); e != hipSuccess) return e;
    // the 128 x 256 split tiling is one kernel per epilogue kind: fn = iefvad_gemm_split_n128x2_kernel stands for all of them
    if (!fn || fn == (const void*)iefvad_gemm_split_n128x2_kernel)
        for (const GemmSplitWideKernel k : kGemmSplitWideKernels)
            if (hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, GS_LDS_BYTES_OF(2)); e != hipSuccess) return e;
    return hipSuccess;
}

// iefvad_create (D = 768 only) and iefvad_create_ex (also D = 512 in the f32 arithmetic): every check before the first HIP call
static int create_impl(const char* who, bool allow_512, const iefvad_config* cfg, iefvad_handle** out) {
    if (!cfg || !out) return fail("%s: null argument", who);
    *out = nullptr;
    if (cfg->abi_version != IEFVAD_ABI_VERSION)
        return fail("%s: abi_version %d, library is %d", who, cfg->abi_version, IEFVAD_ABI_VERSION);
    const bool d512 = allow_512 && cfg->embed_dim == IEF_D512;
    if (d512) {
        if (cfg->seq_len != IEF_T || cfg->num_heads != IEF_D512 / 64)
            return fail("%s: D=512 is built for T=256, H=8 (head dim 64) (got T=%d H=%d)", who, cfg->seq_len, cfg->num_heads);
        if (cfg->compute != IEFVAD_COMPUTE_F32)
            return fail("%s: D=512 runs in the f32 arithmetic only (compute = %d; bf16, bf16x6 and fp16x3 are built for D=768)", who,
                        cfg->compute);
    } else if (cfg->embed_dim != IEF_D || cfg->seq_len != IEF_T || cfg->num_heads != IEF_H) {
        if (allow_512)
            return fail("%s: kernels are built for D=768, T=256, H=8, or D=512, T=256, H=8 in the f32 arithmetic (got D=%d T=%d H=%d)", who,
                        cfg->embed_dim, cfg->seq_len, cfg->num_heads);
        return fail("iefvad_create: kernels are built for D=768, T=256, H=8 (got D=%d T=%d H=%d)",
                    cfg->embed_dim, cfg->seq_len, cfg->num_heads);
    }
    if (cfg->num_layers < 1 || cfg->num_layers > IEFVAD_MAX_LAYERS)
        return fail("%s: num_layers %d outside 1..%d", who, cfg->num_layers, IEFVAD_MAX_LAYERS);
    if (cfg->num_steps < 0 || cfg->num_steps > IEFVAD_MAX_STEPS)
        return fail("%s: num_steps %d outside 0..%d", who, cfg->num_steps, IEFVAD_MAX_STEPS);
    if (cfg->noise_model != IEFVAD_NOISE_GAUSSIAN && cfg->noise_model != IEFVAD_NOISE_STUDENT_T)
        return fail("Unsupported noise_model. Choose 'Gaussian' or 'StudentT'.");   // imf_vad.py:138
    if (cfg->compute != IEFVAD_COMPUTE_F32 && cfg->compute != IEFVAD_COMPUTE_BF16 && cfg->compute != IEFVAD_COMPUTE_BF16X6 &&
        cfg->compute != IEFVAD_COMPUTE_FP16X3)
        return fail("%s: unknown compute mode %d", who, cfg->compute);
    if (cfg->noise_model == IEFVAD_NOISE_STUDENT_T && !(cfg->nu != 0.f))
        return fail("%s: nu must be non-zero for StudentT", who);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail("%s: no HIP device", who);
    iefvad_handle* h = new (std::nothrow) iefvad_handle();
    if (!h) return fail("%s: out of host memory", who);
    memset(h, 0, sizeof(*h));
    h->cfg = *cfg;
    h->steps = cfg->num_steps;
    h->D = d512 ? IEF_D512 : IEF_D;
    h->DH = h->D / IEF_H;
    // The library's only environment switches: alternative paths that tests compare the default against, and a trace
    {
        auto num = [](const char* name) { const char* v = getenv(name); return v ? atoi(v) : 0; };
        auto first = [](const char* name) { const char* v = getenv(name); return v ? v[0] : '\0'; };
        h->policy = launch_policy(num("IEFVAD_ROWBLOCK_OFF"), num("IEFVAD_ROWBLOCK_MIN_WGS"), num("IEFVAD_CHAIN_MIN_BLOCKS"), first("IEFVAD_PERSIST") != '0',
                                  num("IEFVAD_SPLIT_TILE"), first("IEFVAD_DENSE_ENCODER") == '1');
        h->train_attn_unfused = first("IEFVAD_TRAIN_ATTN") == 'u';
        h->hostpipe_trace = first("IEFVAD_HOSTPIPE_TRACE") == '1';
    }
    hipError_t e = hipGetDevice(&h->device);
    if (e == hipSuccess) e = raise_lds_limit();
    if (e == hipSuccess) {
        hipDeviceProp_t prop;
        e = hipGetDeviceProperties(&prop, h->device);
        h->num_cus = e == hipSuccess ? prop.multiProcessorCount : 256;
        g_num_cus = h->num_cus;
    }
    if (e == hipSuccess && cfg->compute == IEFVAD_COMPUTE_FP16X3) e = hipMalloc((void**)&h->amax_dev, amax_words(cfg->num_layers, cfg->num_steps, micro_batch(h)) * sizeof(float));
    if (e != hipSuccess) {
        delete h;
        return fail("%s: %s", who, hipGetErrorString(e));
    }
    *out = h;
    return 0;
}

extern "C" int iefvad_create(const iefvad_config* cfg, iefvad_handle** out) { return create_impl("iefvad_create", false, cfg, out); }

extern "C" int iefvad_create_ex(const iefvad_config* cfg, iefvad_handle** out) { return create_impl("iefvad_create_ex", true, cfg, out); }

static void release_events(iefvad_handle* h);
static void release_graphs(iefvad_handle* h);
static void release_meta(iefvad_handle* h);
static void release_train(iefvad_handle* h);
static void release_hostpipe(iefvad_handle* h);

extern "C" void iefvad_destroy(iefvad_handle* h) {
    if (!h) return;
    if (h->arena) (void)hipFree(h->arena);
    if (h->arena_b) (void)hipFree(h->arena_b);
    if (h->chain_stream) (void)hipFree(h->chain_stream);
    if (h->heads_stream) (void)hipFree(h->heads_stream);
    for (int m = 0; m < 2; ++m)
        for (int l = 0; l < IEFVAD_MAX_LAYERS; ++l) {
            if (h->oproj_stream[m][l]) (void)hipFree(h->oproj_stream[m][l]);
            if (h->iproj_stream[m][l]) (void)hipFree(h->iproj_stream[m][l]);
        }
    if (h->arena_s) (void)hipFree(h->arena_s);
    if (h->arena_st) (void)hipFree(h->arena_st);
    if (h->zero_bias) (void)hipFree(h->zero_bias);
    if (h->arena_h) (void)hipFree(h->arena_h);
    if (h->amax_dev) (void)hipFree(h->amax_dev);
    release_events(h);
    release_graphs(h);
    release_meta(h);
    release_train(h);
    release_hostpipe(h);
    delete h;
}

// The two run-time choices that pick template arguments, each made in one place.  dispatch_in calls f(element-type tag, width
// constant) for an (input dtype, embed dim) pair and returns f's status; dispatch_d calls f(width constant).  In the callable:
// `typename decltype(t)::type` is the element type, `decltype(w)::value` the row width.
template <typename T> struct InType { using type = T; };
template <int W> struct RowWidth { static constexpr int value = W; };
template <typename F>
static int dispatch_d(bool d512, F&& f) {      // f returns its launch's return code
    if (d512) return f(RowWidth<IEF_D512>{});
    return f(RowWidth<IEF_D>{});
}
template <typename F>
static int dispatch_in(int in_dtype, bool d512, F&& f) {
    return dispatch_d(d512, [&](auto w) {
        return in_dtype == IEFVAD_IN_F32 ? f(InType<float>{}, w) : in_dtype == IEFVAD_IN_F16 ? f(InType<__half>{}, w) : f(InType<__hip_bfloat16>{}, w);
    });
}

template <typename T>
static int launch_cast(const void* in0, const void* in1, float* o0, float* o1, bf16_t* b0, bf16_t* b1, size_t n, int nsrc,
                       hipStream_t stream) {
    size_t blocks = (n / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(iefvad_cast_kernel<T>, dim3((unsigned)blocks, nsrc), dim3(256), 0, stream, (const T*)in0,
                       (const T*)in1, o0, o1, b0, b1, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T, int W>
static int launch_cast_scaled(const void* in0, const void* in1, float* o0, float* o1, bf16_t* b0, bf16_t* b1, size_t n, const float* s0,
                              const float* s1, const RowNoise& nz, hipStream_t stream) {
    size_t blocks = (n / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    // an amplitude vector selects the noise instantiation; without one the kernel of iefvad_forward_scaled runs, as it always has
    if (nz.any())
        hipLaunchKernelGGL((iefvad_cast_scaled_kernel<T, W, RowNoise>), dim3((unsigned)blocks, 2), dim3(256), 0, stream, (const T*)in0, (const T*)in1,
                           o0, o1, b0, b1, n, s0, s1, nz);
    else
        hipLaunchKernelGGL((iefvad_cast_scaled_kernel<T, W>), dim3((unsigned)blocks, 2), dim3(256), 0, stream, (const T*)in0, (const T*)in1, o0, o1,
                           b0, b1, n, s0, s1);
    HIP_TRY(hipGetLastError());
    return 0;
}

// iefvad_perturb_rows: both modalities in one launch (a null source / destination pair is skipped by the kernel)
template <typename T, int W>
static int launch_perturb_rows(const void* in0, const void* in1, void* o0, void* o1, size_t n, const float* s0, const float* s1, int fix_all,
                               const RowNoise& nz, float big, hipStream_t stream) {
    size_t blocks = (n / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL((iefvad_perturb_rows_kernel<T, W>), dim3((unsigned)blocks, 2), dim3(256), 0, stream, (const T*)in0, (const T*)in1, (T*)o0,
                       (T*)o1, n, s0, s1, fix_all, nz, big);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int launch_split_planes(const float* src, bf16_t* planes, size_t n, hipStream_t stream) {
    if (n % 4) return fail("split_bf16x3: n = %zu is not a multiple of 4", n);
    size_t blocks = (n / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(iefvad_split_planes_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, src, planes, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

// batches of iefvad_split_planes_many_kernel launches (gemm_split.h): add() queues a matrix, flush() launches what is queued
struct SplitMany {
    SplitManyArgs a;
    hipStream_t stream;
    explicit SplitMany(hipStream_t s) : stream(s) { a.count = 0; }
    int flush() {
        if (a.count == 0) return 0;
        hipLaunchKernelGGL(iefvad_split_planes_many_kernel, dim3(96, a.count), dim3(256), 0, stream, a);
        a.count = 0;
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // rows = 0: planes of src [n]; rows = n_out: planes of the transpose of src [n_out, n / n_out]
    int add(const float* src, bf16_t* dst, size_t n, int rows) {
        if (n % 4 || n > 0xffffffffu) return fail("split_bf16x3: n = %zu is not a multiple of 4 below 2^32", n);
        if (rows && (rows % 64 || (n / rows) % 32 || n % rows)) return fail("split_bf16x3: transposed split of a [%d, %zu] matrix", rows, n / rows);
        a.src[a.count] = src; a.dst[a.count] = dst; a.n[a.count] = (unsigned)n; a.rows[a.count] = rows;
        if (++a.count == SPLIT_MANY_MAX) return flush();
        return 0;
    }
};

extern "C" int iefvad_split_bf16x3_many(const float* const* src, void* const* planes, const size_t* n, const int32_t* rows, int32_t count,
                                        void* stream) {
    if (!src || !planes || !n || !rows || count < 0) return fail("iefvad_split_bf16x3_many: null argument");
    SplitMany sm((hipStream_t)stream);
    for (int i = 0; i < count; ++i) {
        if (!src[i] || !planes[i] || rows[i] < 0) return fail("iefvad_split_bf16x3_many: entry %d is null or has negative rows", i);
        if (((uintptr_t)src[i] | (uintptr_t)planes[i]) & 15) return fail("iefvad_split_bf16x3_many: entry %d is not 16-byte aligned", i);
        if (int rc = sm.add(src[i], (bf16_t*)planes[i], n[i], rows[i])) return rc;
    }
    return sm.flush();
}

extern "C" int iefvad_split_bf16x3(const float* src, void* planes, size_t n, void* stream) {
    if (!src || !planes) return fail("iefvad_split_bf16x3: null argument");
    return launch_split_planes(src, (bf16_t*)planes, n, (hipStream_t)stream);
}

// up to COPY_MANY_MAX device-to-device copies in one launch: blockIdx.y = tensor, 32 workgroups stride over it (16-byte moves when
// both ends are 16-byte aligned)
#define COPY_MANY_MAX 96
struct CopyManyArgs {
    float* dst[COPY_MANY_MAX];
    const float* src[COPY_MANY_MAX];
    unsigned count[COPY_MANY_MAX];
    int n;
};
__global__ __launch_bounds__(256) void iefvad_copy_many_kernel(CopyManyArgs a) {
    float* d = a.dst[blockIdx.y];
    const float* s = a.src[blockIdx.y];
    const unsigned n = a.count[blockIdx.y];
    const unsigned tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
    if ((((uintptr_t)d | (uintptr_t)s) & 15) == 0) {
        const unsigned n4 = n >> 2;
        for (unsigned i = tid; i < n4; i += nth) ((f32x4*)d)[i] = ((const f32x4*)s)[i];
        for (unsigned i = (n4 << 2) + tid; i < n; i += nth) d[i] = s[i];
    } else {
        for (unsigned i = tid; i < n; i += nth) d[i] = s[i];
    }
}

extern "C" int iefvad_set_weights(iefvad_handle* h, const iefvad_weights* w, void* stream_) {
    if (!h || !w) return fail("iefvad_set_weights: null argument");
    hipStream_t stream = (hipStream_t)stream_;
    const int L = h->cfg.num_layers, K = h->cfg.num_steps;
    const size_t D = h->D, DD = D * D;
    // validate pointers first
    for (int m = 0; m < 2; ++m) {
        for (int l = 0; l < L; ++l)
            if (!w->in_proj_w[m][l] || !w->in_proj_b[m][l] || !w->out_proj_w[m][l] || !w->out_proj_b[m][l] ||
                !w->norm_w[m][l] || !w->norm_b[m][l])
                return fail("iefvad_set_weights: null encoder weight (modality %d layer %d)", m, l);
        if (!w->whiten_w[m] || !w->whiten_b[m] || !w->mu_w[m] || !w->mu_b[m] || !w->logvar_w[m] || !w->logvar_b[m])
            return fail("iefvad_set_weights: null head weight (modality %d)", m);
    }
    for (int k = 0; k < K; ++k)
        if (!w->ref_w1[k] || !w->ref_b1[k] || !w->ref_w2[k] || !w->ref_b2[k])
            return fail("iefvad_set_weights: null refinement weight (step %d)", k);
    if (!w->cls_w || !w->cls_b) return fail("iefvad_set_weights: null classifier weight");

    const size_t total = 2 * L * (3 * DD + 3 * D + DD + D + 2 * D) + 2 * (2 * D) + 2 * (2 * DD + 2 * D) +
                         (size_t)K * (2 * DD + 2 * D) + D + 4 + (size_t)(K > 1 ? K : 1) * (D + 4);
    if (!h->arena) {
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipMalloc((void**)&h->arena, total * sizeof(float)));
        h->arena_floats = total;
    }
    float* p = h->arena;
    // the 38 + 4 K tensors go into the arena in batches of one launch (a training step re-uploads every parameter: 78 copies of
    // 6 us each were 2 % of it)
    CopyManyArgs cm;
    cm.n = 0;
    auto flush = [&]() -> hipError_t {
        if (cm.n == 0) return hipSuccess;
        hipLaunchKernelGGL(iefvad_copy_many_kernel, dim3(32, cm.n), dim3(256), 0, stream, cm);
        cm.n = 0;
        return hipGetLastError();
    };
    auto put = [&](float** dst, const float* src, size_t n) -> hipError_t {
        *dst = p;
        p += n;
        cm.dst[cm.n] = *dst; cm.src[cm.n] = src; cm.count[cm.n] = (unsigned)n;
        if (++cm.n == COPY_MANY_MAX) return flush();
        return hipSuccess;
    };
    for (int m = 0; m < 2; ++m) {
        for (int l = 0; l < L; ++l) {
            ProjW& in = h->in[m][l];
            ProjW& out = h->out[m][l];
            in.N = 3 * (int)D; out.N = (int)D;
            HIP_TRY(put(&in.w, w->in_proj_w[m][l], 3 * DD));
            HIP_TRY(put(&in.b, w->in_proj_b[m][l], 3 * D));
            HIP_TRY(put(&out.w, w->out_proj_w[m][l], DD));
            HIP_TRY(put(&out.b, w->out_proj_b[m][l], D));
            HIP_TRY(put(&h->norm_w[m][l], w->norm_w[m][l], D));
            HIP_TRY(put(&h->norm_b[m][l], w->norm_b[m][l], D));
        }
        HIP_TRY(put(&h->whiten_w[m], w->whiten_w[m], D));
        HIP_TRY(put(&h->whiten_b[m], w->whiten_b[m], D));
        // mu | logvar heads share their A operand: stack them into one [1536, 768] projection
        h->head[m].N = 2 * (int)D;
        HIP_TRY(put(&h->head[m].w, w->mu_w[m], DD));
        float* dummy;
        HIP_TRY(put(&dummy, w->logvar_w[m], DD));
        HIP_TRY(put(&h->head[m].b, w->mu_b[m], D));
        HIP_TRY(put(&dummy, w->logvar_b[m], D));
    }
    for (int k = 0; k < K; ++k) {
        h->ref1[k].N = h->ref2[k].N = (int)D;
        HIP_TRY(put(&h->ref1[k].w, w->ref_w1[k], DD));
        HIP_TRY(put(&h->ref1[k].b, w->ref_b1[k], D));
        HIP_TRY(put(&h->ref2[k].w, w->ref_w2[k], DD));
        HIP_TRY(put(&h->ref2[k].b, w->ref_b2[k], D));
    }
    HIP_TRY(put(&h->cls_w, w->cls_w, D));
    HIP_TRY(put(&h->cls_b, w->cls_b, 1));
    HIP_TRY(flush());
    p += 3;                                      // back to a 16-byte boundary: the folded scorer's vector is read 16 bytes per lane
    h->score_fold = nullptr;
    if (h->cfg.compute == IEFVAD_COMPUTE_BF16X6 && K >= 1) {
        // the scores-only forward drops the last refinement projection: logits = c . z_{K-1} + v . h + s0 (forward_pass, step 4).  One
        // vector per block (one launch: grid.y = block; the blocks' W2 / b2 are 2 DD + 2 D floats apart in the arena, above), so that a
        // forward of any prefix of the steps (iefvad_set_steps) finds the one of its last block.
        h->score_fold = p;
        p += (size_t)K * (D + 4);
        hipLaunchKernelGGL(iefvad_scorer_fold_weights_kernel, dim3((unsigned)(D / 16 + 1), K), dim3(256), 0, stream, h->ref2[0].w, h->ref2[0].b,
                           h->cls_w, h->cls_b, h->cfg.lambda_ref, h->score_fold, (int)D, 2 * DD + 2 * D, (int)(D + 4));
        HIP_TRY(hipGetLastError());
    }
    if ((size_t)(p - h->arena) > h->arena_floats) return fail("iefvad_set_weights: arena overflow");
    // the other resident forms, each one walk over the records (for_each_proj) that carves the form's arena in visiting order;
    // biases, LayerNorm and the scorer stay fp32 in every arithmetic
    const size_t nb = proj_elems(h);
    if (h->cfg.compute == IEFVAD_COMPUTE_BF16) {
        // bf16 (round-to-nearest-even) copies
        if (!h->arena_b) HIP_TRY(hipMalloc((void**)&h->arena_b, nb * sizeof(bf16_t)));
        bf16_t* q = h->arena_b;
        if (int rc = for_each_proj(h, [&](ProjW& r) {
                const size_t n = r.N * D;
                r.wb = q;
                q += n;
                return launch_cast<float>(r.w, nullptr, nullptr, nullptr, r.wb, nullptr, n, 1, stream);
            })) return rc;
        for (int m = 0; m < 2; ++m)
            for (int l = 0; l < L; ++l) {
                if (!h->oproj_stream[m][l]) HIP_TRY(hipMalloc((void**)&h->oproj_stream[m][l], wstream_bytes()));
                hipLaunchKernelGGL(iefvad_wstream_pack_kernel, dim3(256), dim3(256), 0, stream, h->out[m][l].wb, h->oproj_stream[m][l], 1);
                HIP_TRY(hipGetLastError());
                if (!h->iproj_stream[m][l]) HIP_TRY(hipMalloc((void**)&h->iproj_stream[m][l], wstream_bytes(IC_NPASS)));
                hipLaunchKernelGGL(iefvad_wstream_pack_kernel, dim3(512), dim3(256), 0, stream, h->in[m][l].wb, h->iproj_stream[m][l], IC_NPASS);
                HIP_TRY(hipGetLastError());
            }
        if (!h->heads_stream) HIP_TRY(hipMalloc((void**)&h->heads_stream, heads_stream_bytes()));
        hipLaunchKernelGGL(iefvad_heads_pack_kernel, dim3(512), dim3(256), 0, stream, h->head[0].wb, h->head[1].wb, h->heads_stream);
        HIP_TRY(hipGetLastError());
        if (K > 0) {
            // the same bf16 matrices (and the fp32 biases) once more, in the chain kernel's per-wave piece order
            if (!h->chain_stream) HIP_TRY(hipMalloc((void**)&h->chain_stream, chain_stream_bytes(K)));
            ChainPackArgs pa;
            memset(&pa, 0, sizeof(pa));
            for (int k = 0; k < K; ++k) {
                pa.W[2 * k] = h->ref1[k].wb; pa.bias[2 * k] = h->ref1[k].b;
                pa.W[2 * k + 1] = h->ref2[k].wb; pa.bias[2 * k + 1] = h->ref2[k].b;
            }
            pa.stream = h->chain_stream;
            pa.K = K;
            hipLaunchKernelGGL(iefvad_chain_pack_kernel, dim3(2048), dim3(256), 0, stream, pa);
            HIP_TRY(hipGetLastError());
        }
    }
    if (h->cfg.compute == IEFVAD_COMPUTE_BF16X6) {
        // exact three-term bf16 split (gemm_split.h)
        if (!h->arena_s) HIP_TRY(hipMalloc((void**)&h->arena_s, 3 * nb * sizeof(bf16_t)));
        bf16_t* q = h->arena_s;
        SplitMany sm(stream);                 // all 10 + 2 K matrices in one launch (two from K = 12 on)
        if (int rc = for_each_proj(h, [&](ProjW& r) {
                const size_t n = r.N * D;
                r.ws = q;
                q += 3 * n;
                return sm.add(r.w, r.ws, n, 0);
            })) return rc;
        if (int rc = sm.flush()) return rc;
    }
    if (h->cfg.compute == IEFVAD_COMPUTE_FP16X3) {
        // two fp16 planes, scaled by a power of two from the matrix's max |w| (gemm_split.h, F16)
        if (!h->arena_h) HIP_TRY(hipMalloc((void**)&h->arena_h, 2 * nb * sizeof(_Float16)));
        HIP_TRY(hipMemsetAsync(h->amax_dev, 0, kAmaxActBase * IEF_AMAX_FLOATS * sizeof(float), stream));
        _Float16* q = h->arena_h;
        int widx = 0;
        if (int rc = for_each_proj(h, [&](ProjW& r) -> int {
                if (widx >= kAmaxActBase) return fail("iefvad_set_weights: too many projection matrices");
                const size_t n = r.N * D;
                r.wh = q;
                q += 2 * n;
                float* word = h->amax_dev + IEF_AMAX_FLOATS * widx++;
                r.wa = word;
                size_t blocks = (n / 4 + 255) / 256;
                if (blocks > 1024) blocks = 1024;
                hipLaunchKernelGGL(iefvad_amax_kernel, dim3((unsigned)blocks, 1), dim3(256), 0, stream, r.w, r.w, word, word, n);
                hipLaunchKernelGGL(iefvad_split_planes_f16_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, r.w, r.wh, n,
                                   (const float*)word);
                HIP_TRY(hipGetLastError());
                return 0;
            })) return rc;
    }
    h->weights_set = true;
    h->tplanes_valid = false;
    return 0;
}

// workspace, in floats per row: xin(2) + qkv(6) + att(2) + y(2) + x(2) = 14 * D, + 1 (logits scratch).
// mu_i, lv_i, mu_e, lv_e, z, h alias the qkv region (6 * D), which is dead once the encoder is done.
static size_t ws_floats_per_row(const iefvad_handle* h) { return 14 * (size_t)h->D + 4; }

extern "C" size_t iefvad_workspace_bytes(const iefvad_handle* h, int32_t B) {
    if (!h || B <= 0) return 0;
    const int mb = micro_batch(h);
    const size_t rows = (size_t)(B < mb ? B : mb) * IEF_T;
    return rows * ws_floats_per_row(h) * sizeof(float) + 256;
}

// ------------------------------------------------------------------------------------------------
// stage timing
// ------------------------------------------------------------------------------------------------
enum Stage { ST_QKV = 0, ST_ATT, ST_OUT, ST_LN, ST_HEAD, ST_FUSION, ST_REFINE, ST_SCORER, ST_CAST, ST_COUNT };

// hipEvents are pooled on the handle and reused by every timed call (a timed forward of one micro-batch brackets ~35
// launches; creating and destroying 70 events per call would sit inside bench.py's timed region).
struct EventPool {
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    hipError_t err = hipSuccess;
    hipEvent_t take() {
        if (used == ev.size()) {
            hipEvent_t e = nullptr;
            hipError_t r = hipEventCreate(&e);
            if (r != hipSuccess) {
                if (err == hipSuccess) err = r;
                return nullptr;
            }
            ev.push_back(e);
        }
        return ev[used++];
    }
    void release_all() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        ev.clear();
        used = 0;
    }
};

struct Timer {
    bool on = false;
    hipStream_t stream = nullptr;
    EventPool* pool = nullptr;
    struct Span { int stage; hipEvent_t a, b; };
    std::vector<Span> spans;
    int gemm_launches = 0;
    hipEvent_t begin(int stage) {
        if (!on) return nullptr;
        Span s;
        s.stage = stage;
        s.a = pool->take();
        s.b = pool->take();
        if (!s.a || !s.b) return nullptr;          // pool->err is reported by iefvad_forward_timed
        (void)hipEventRecord(s.a, stream);
        spans.push_back(s);
        return s.b;
    }
    void end(hipEvent_t b) {
        if (on && b) (void)hipEventRecord(b, stream);
    }
};

// One checked launch: the launch, then hipGetLastError through `fail`.  With a timer and a stage, the launch sits in a span of that stage.
template <typename... P, typename... A>
static int launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, A&&... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, std::forward<A>(args)...);
    HIP_TRY(hipGetLastError());
    return 0;
}
template <typename... P, typename... A>
static int launch(Timer& tm, int stage, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, A&&... args) {
    hipEvent_t e = tm.begin(stage);
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, std::forward<A>(args)...);
    tm.end(e);
    HIP_TRY(hipGetLastError());
    return 0;
}

static void release_events(iefvad_handle* h) {
    if (h->events) {
        h->events->release_all();
        delete h->events;
        h->events = nullptr;
    }
}

// The projection launches: the plan (launch_rules.h) names the kernel and the grid, the code here fills the argument block and launches it
static int launch_gemm(const GemmArgs& a, int nz, hipStream_t stream, Timer& tm, int stage) {
    const GemmPlan pl = plan_gemm_f32(a.M, a.N, a.K, nz);
    if (pl.reject)
        return fail("gemm: shape M=%d N=%d K=%d not a multiple of the %dx%dx%d tile", a.M, a.N, a.K, GEMM_BM, GEMM_BN,
                    GEMM_BK);
    const dim3 grid(pl.wgs, 1, nz);
    tm.gemm_launches += 1;
    switch (pl.kernel) {
    case GEMM_F32_TINY: return launch(tm, stage, iefvad_gemm_f32_tiny_kernel, grid, dim3(256), 0, stream, a);
    case GEMM_F32_SMALL: return launch(tm, stage, iefvad_gemm_f32_small_kernel, grid, dim3(256), 0, stream, a);
    case GEMM_F32_128: return launch(tm, stage, iefvad_gemm_f32_kernel, grid, dim3(256), 0, stream, a);
    case GEMM_F32_T256: {
        GemmBArgs b;
        memset(&b, 0, sizeof(b));
        b.M = a.M; b.N = a.N; b.K = a.K; b.lda = a.lda; b.ldc = a.ldc; b.epi = a.epi; b.alpha = a.alpha; b.qcols = a.qcols;
        for (int m = 0; m < nz; ++m) {
            b.p[m].A = (const bf16_t*)a.p[m].A; b.p[m].W = (const bf16_t*)a.p[m].W;     // fp32 data behind the typed pointer
            b.p[m].bias = a.p[m].bias; b.p[m].C = a.p[m].C; b.p[m].R = a.p[m].R; b.p[m].C2 = a.p[m].C2;
        }
        return launch(tm, stage, iefvad_gemm_f32_t256_kernel, grid, dim3(256), GB2_LDS_BYTES, stream, b);
    }
    default: return fail("gemm: the plan names no fp32 kernel");
    }
}

static int launch_gemm_b(const GemmBArgs& a, int nz, hipStream_t stream, Timer& tm, int stage) {
    const GemmPlan pl = plan_gemm_bf16(a.M, a.N, a.K, nz, a.epi == EPI_REFINE);
    if (pl.reject)
        return fail("gemm(bf16): shape M=%d N=%d K=%d not a multiple of the %dx%dx%d tile", a.M, a.N, a.K, GEMM_BM,
                    GEMM_BN, GEMMB_BK);
    const dim3 grid(pl.wgs, 1, nz);
    tm.gemm_launches += 1;
    switch (pl.kernel) {
    case GEMM_BF16_W256: return launch(tm, stage, iefvad_gemm_bf16_w256_kernel, grid, dim3(512), GB3_LDS_BYTES, stream, a);
    case GEMM_BF16_PIPE: return launch(tm, stage, iefvad_gemm_bf16_pipe_kernel, grid, dim3(256), GB2_LDS_BYTES, stream, a);
    case GEMM_BF16_V1: return launch(tm, stage, iefvad_gemm_bf16_v1_kernel, grid, dim3(256), 0, stream, a);
    default: return fail("gemm(bf16): the plan names no bf16 kernel");
    }
}

static std::atomic<unsigned long long> g_split_wide_launches{0};     // iefvad_gemm_split_wide_launches: which tiling ran is otherwise invisible
static std::atomic<unsigned long long> g_split_small_launches{0};    // iefvad_gemm_split_small_launches
// the small tiling of the bf16x6 arithmetic (gemm_split_small.h): the batch-invariant mode below the split kernels' crossover, and its unit entry
static int launch_gemm_split_small(const GemmBArgs& a, int nz, hipStream_t stream, Timer& tm, int stage) {
    const GemmSmallPlan pl = plan_gemm_split_small(a.M, a.N, a.K, nz, a.epi == EPI_BIAS_RELU_DOT, a.p[0].R && a.p[0].C2);
    if (!pl.ok) {
        if (pl.why == GEMM_BAD_DOT_EPILOGUE)
            return fail("gemm(bf16x6, small): the dot-product epilogue takes one problem with its vector (R) and its partial sums (C2)");
        return fail("gemm(bf16x6, small): shape M=%d N=%d K=%d nz=%d not a multiple of the %dx%dx64 tile", a.M, a.N, a.K, nz, kSplitSmallBM, kSplitBN);
    }
    g_split_small_launches.fetch_add(1, std::memory_order_relaxed);
    tm.gemm_launches += 1;
    return launch(tm, stage, iefvad_gemm_split_small_kernel, dim3(pl.wgs, 1, nz), dim3(256), GSS_LDS_BYTES, stream, a);
}

// invariant: the handle is in the batch-invariant mode (LaunchPolicy::split_always): what the default mode would have left to the fp32
// kernels runs on the small tiling (an IEFVAD_SPLIT_TILE preference still forces its tiling; all three give the same bits)
static int launch_gemm_split(const GemmBArgs& a, int nz, hipStream_t stream, Timer& tm, int stage, bool f16 = false, int tile_n = 0,
                             bool invariant = false) {
    if (invariant && !f16 && tile_n == 0 && split_small_preferred(a.M, a.N, a.K, nz)) return launch_gemm_split_small(a, nz, stream, tm, stage);
    const GemmPlan pl = plan_gemm_split(a.M, a.N, a.K, nz, f16, tile_n, a.epi == EPI_BIAS_RELU_DOT, a.p[0].R && a.p[0].C2);
    switch (pl.reject) {
    case GEMM_OK: break;
    case GEMM_BAD_SHAPE: return fail("gemm(bf16x6): shape M=%d N=%d K=%d not a multiple of the %dx%dx64 tile", a.M, a.N, a.K, GS_BM, kSplitBN);
    case GEMM_BAD_TILE_N: return fail("gemm(bf16x6): tile_n = %d (128, 256 or 0 for the launch rule)", tile_n);
    case GEMM_NO_WIDE_TILING:
        return fail("gemm(bf16x6): the 128 x 256 tiling takes bf16x6 problems with N %% 256 == 0 (N = %d%s)", a.N, f16 ? ", fp16x3" : "");
    case GEMM_BAD_DOT_EPILOGUE:
        return fail("gemm(bf16x6): the dot-product epilogue takes one bf16x6 problem with its vector (R) and its partial sums (C2)");
    }
    const dim3 grid(pl.wgs, 1, nz);
    // the 128 x 256 tiling has one kernel per epilogue kind, whose stores are unconditional: every problem brings the outputs of its kind
    GemmSplitWideKernel wide = nullptr;
    if (pl.kernel == GEMM_SPLIT_N128X2) {
        const bool dot = a.epi == EPI_BIAS_RELU_DOT;
        const bool resid = a.epi == EPI_BIAS_RESID || a.epi == EPI_REFINE || a.epi == EPI_GATE;
        wide = gemm_split_wide_kernel(a.epi, a.p[0].C != nullptr);
        if (!wide) return fail("gemm(bf16x6): unknown epilogue %d", a.epi);
        if (a.epi == EPI_HEADS && a.ldc % 128) return fail("gemm(bf16x6): the heads epilogue needs ldc %% 128 == 0 (ldc = %d)", a.ldc);
        for (int m = 0; m < nz; ++m)
            if (!a.p[m].bias || (!dot && !a.p[m].C) || ((resid || dot) && !a.p[m].R) || ((dot || a.epi == EPI_HEADS) && !a.p[m].C2))
                return fail("gemm(bf16x6): problem %d lacks an operand of epilogue %d", m, a.epi);
    }
    void (*kernel)(GemmBArgs) = nullptr;
    switch (pl.kernel) {
    case GEMM_SPLIT_N128X2:
        kernel = wide;
        g_split_wide_launches.fetch_add(1, std::memory_order_relaxed);
        break;
    case GEMM_SPLIT_F16_N128: kernel = iefvad_gemm_split_f16_n128_kernel; break;
    case GEMM_SPLIT_N128: kernel = iefvad_gemm_split_n128_kernel; break;
    default: return fail("gemm(bf16x6): the plan names no split kernel");
    }
    tm.gemm_launches += 1;
    return launch(tm, stage, kernel, grid, dim3(256), GS_LDS_BYTES_OF(2), stream, a);
}

static size_t in_elem_bytes(int in_dtype) { return in_dtype == IEFVAD_IN_F32 ? 4 : 2; }

// One projection in either arithmetic: fills the fp32 or the bf16 argument block from the same description.
struct Proj {
    const float* A32[2];      // fp32 A operand (IEFVAD_COMPUTE_F32)
    const bf16_t* A16[2];     // bf16 A operand (IEFVAD_COMPUTE_BF16)
    const float* W32[2];
    const bf16_t* W16[2];
    const bf16_t* Ws[2];      // three-plane split of W (IEFVAD_COMPUTE_BF16X6)
    const _Float16* Wh[2];    // two scaled fp16 planes of W + the running-max words (IEFVAD_COMPUTE_FP16X3)
    const float* amaxW[2];
    const float* amaxA[2];
    float* amaxC[2];
    const float* bias[2];
    float* C[2];              // fp32 result (nullable in bf16 mode)
    bf16_t* Cb[2];            // bf16 copy of the result (bf16 mode only, nullable)
    const float* R[2];
    float* C2[2];
    int N, ldc, epi, nz;
    float alpha;
    int qcols;
    // problem m takes its weight, in every resident form, and its bias from one record
    void set_w(int m, const ProjW& r) {
        W32[m] = r.w; W16[m] = r.wb; Ws[m] = r.ws; Wh[m] = r.wh; amaxW[m] = r.wa; bias[m] = r.b;
    }
    // the shape half: one problem (w0) or one per modality (w0, w1); operands, alpha, qcols and the amax words are the caller's
    static Proj of(int epi, int N, int ldc, const ProjW& w0, const ProjW* w1 = nullptr) {
        Proj p;
        memset(&p, 0, sizeof(p));
        p.N = N; p.ldc = ldc; p.epi = epi; p.nz = w1 ? 2 : 1;
        p.set_w(0, w0);
        if (w1) p.set_w(1, *w1);
        return p;
    }
};

// What every projection of one forward shares.  D: the contraction length (the row width of A), the handle's embed dim;
// invariant: the batch-invariant mode (launch_gemm_split)
struct ProjCtx {
    int compute;
    bool use_split;
    int D, rows;
    hipStream_t stream;
    Timer* tm;
    int split_tile;
    bool invariant;
};

static float precision_factor(const iefvad_config& c) {      // the Student-t factor of the precision weights (imf_vad.py:134)
    return (c.noise_model == IEFVAD_NOISE_STUDENT_T) ? (c.nu + 1.0f) / c.nu : 1.0f;
}

static int launch_proj(const ProjCtx& x, const Proj& p, int stage) {
    const bool bf16 = (x.compute == IEFVAD_COMPUTE_BF16);
    if (p.epi == EPI_BIAS_RELU_DOT && !(x.use_split && x.compute == IEFVAD_COMPUTE_BF16X6))
        return fail("gemm: the dot-product epilogue exists in the bf16x6 split kernel only");
    if (x.use_split) {   // one rule for every projection of a micro-batch: the 768-wide, single-problem grid fills the chip
        const bool f16 = (x.compute == IEFVAD_COMPUTE_FP16X3);
        GemmBArgs g;
        memset(&g, 0, sizeof(g));
        g.M = x.rows; g.N = p.N; g.K = IEF_D; g.lda = IEF_D; g.ldc = p.ldc; g.epi = p.epi; g.alpha = p.alpha; g.qcols = p.qcols;
        g.wplane = p.N * IEF_D * 2;
        for (int m = 0; m < p.nz; ++m) {
            g.p[m].A = (const bf16_t*)p.A32[m];          // fp32 data behind the typed pointer
            g.p[m].W = f16 ? (const bf16_t*)p.Wh[m] : p.Ws[m];
            g.p[m].bias = p.bias[m]; g.p[m].C = p.C[m]; g.p[m].R = p.R[m]; g.p[m].C2 = p.C2[m];
            if (f16) {
                if (!p.amaxA[m] || !p.amaxW[m]) return fail("gemm(fp16x3): missing running-max word");
                g.p[m].amaxA = p.amaxA[m]; g.p[m].amaxW = p.amaxW[m]; g.p[m].amaxC = p.amaxC[m];
            }
        }
        return launch_gemm_split(g, p.nz, x.stream, *x.tm, stage, f16, split_tile_for(x.split_tile, p.N, f16), x.invariant);
    }
    if (!bf16) {
        GemmArgs g;
        memset(&g, 0, sizeof(g));
        g.M = x.rows; g.N = p.N; g.K = x.D; g.lda = x.D; g.ldc = p.ldc; g.epi = p.epi; g.alpha = p.alpha; g.qcols = p.qcols;
        for (int m = 0; m < p.nz; ++m) {
            g.p[m].A = p.A32[m]; g.p[m].W = p.W32[m]; g.p[m].bias = p.bias[m]; g.p[m].C = p.C[m]; g.p[m].R = p.R[m];
            g.p[m].C2 = p.C2[m];
        }
        return launch_gemm(g, p.nz, x.stream, *x.tm, stage);
    }
    GemmBArgs g;
    memset(&g, 0, sizeof(g));
    g.M = x.rows; g.N = p.N; g.K = IEF_D; g.lda = IEF_D; g.ldc = p.ldc; g.epi = p.epi; g.alpha = p.alpha; g.qcols = p.qcols;
    for (int m = 0; m < p.nz; ++m) {
        g.p[m].A = p.A16[m]; g.p[m].W = p.W16[m]; g.p[m].bias = p.bias[m]; g.p[m].C = p.C[m]; g.p[m].Cb = p.Cb[m];
        g.p[m].R = p.R[m]; g.p[m].C2 = p.C2[m];
    }
    return launch_gemm_b(g, p.nz, x.stream, *x.tm, stage);
}

// ---- the four row-block launches of the bf16 mode: shared by forward_pass and by the unit entry iefvad_rowblock_unit, so a unit test
// runs the very kernel symbol, grid and LDS size the forward uses at that row count
static int launch_inproj_chain(iefvad_handle* h, int l, const void* const A[2], bool a_fp32, bf16_t* const C[2], int rows, hipStream_t stream, Timer& tm) {
    InProjChainArgs ia;
    memset(&ia, 0, sizeof(ia));
    for (int m = 0; m < 2; ++m) {
        ia.p[m].A = A[m];
        ia.p[m].stream = h->iproj_stream[m][l]; ia.p[m].bias = h->in[m][l].b; ia.p[m].C = C[m];
    }
    // q is pre-scaled for the softmax by log2(e)/sqrt(96): both attention kernels use exp2
    ia.M = rows; ia.alpha = (1.0f / sqrtf((float)IEF_DH)) * 1.4426950408889634f; ia.wave_stride = (unsigned)wstream_wave_stride_bytes(IC_NPASS);
    tm.gemm_launches += 1;
    return launch(tm, ST_QKV, a_fp32 ? iefvad_inproj_chain_f32in_kernel : iefvad_inproj_chain_bf16_kernel, dim3(rows / IC_BM, 2), dim3(512), IC_LDS_BYTES,
                  stream, ia);
}

static int launch_outproj_ln_chain(iefvad_handle* h, int l, bool whiten, const bf16_t* const A[2], const float* const R[2], float* const y[2],
                                   bf16_t* const yb[2], int rows, hipStream_t stream, Timer& tm) {
    OutLnChainArgs oa;
    memset(&oa, 0, sizeof(oa));
    for (int m = 0; m < 2; ++m) {
        OutLnChainProblem& q = oa.p[m];
        q.A = A[m]; q.stream = h->oproj_stream[m][l]; q.bias = h->out[m][l].b; q.R = R[m];
        q.g1 = h->norm_w[m][l]; q.b1 = h->norm_b[m][l];
        if (whiten) { q.g2 = h->whiten_w[m]; q.b2 = h->whiten_b[m]; }
        q.y = y[m];
        q.yb = yb[m];
    }
    oa.M = rows; oa.eps = 1e-5f; oa.wave_stride = (unsigned)wstream_wave_stride_bytes();
    const bool uniform = (y[0] != nullptr) == (y[1] != nullptr) && (yb[0] != nullptr) == (yb[1] != nullptr) && (y[0] || yb[0]);
    const StagePlan pl = plan_outproj_ln(h->policy, h->num_cus, rows, uniform);
    const dim3 grid(pl.gx, pl.gy);
    tm.gemm_launches += 1;
    if (pl.kernel != STAGE_OUTLN_PCHAIN) return launch(tm, ST_OUT, iefvad_outproj_ln_chain_bf16_kernel, grid, dim3(512), OC_LDS_BYTES, stream, oa);
    // the persistent kernel is compiled per set of stored results
    void (*const kernel)(OutLnChainArgs) = (y[0] && yb[0]) ? iefvad_outproj_ln_pchain_bf16_kernel<true, true>
                                           : y[0]          ? iefvad_outproj_ln_pchain_bf16_kernel<true, false>
                                                           : iefvad_outproj_ln_pchain_bf16_kernel<false, true>;
    return launch(tm, ST_OUT, kernel, grid, dim3(512), OP_LDS_BYTES, stream, oa);
}

// bf16-mode attention over `nb` chunks per modality; `chunks` != nullptr: the row-compressed chunks of a whole-video pass (`_rows` kernels)
static int launch_attention_bf16(iefvad_handle* h, const bf16_t* const qkv[2], bf16_t* const out[2], int nb, const RaggedChunk* chunks,
                                 bool head_major, int rows, hipStream_t stream, Timer& tm) {
    AttnBArgs ab;
    for (int m = 0; m < 2; ++m) { ab.qkv[m] = qkv[m]; ab.out[m] = out[m]; }
    ab.nchunks = nb;
    ab.chunks = chunks;
    ab.head_major = head_major ? 1 : 0;
    ab.nrows = rows;
    const StagePlan pl = plan_attention_bf16(h->policy, h->num_cus, nb, chunks != nullptr);
    const dim3 grid(pl.gx, pl.gy, pl.gz);
    switch (pl.kernel) {
    case STAGE_ATTN_PBF16_ROWS: return launch(tm, ST_ATT, iefvad_attention_pbf16_rows_kernel, grid, dim3(512), APB_LDS_BYTES, stream, ab);
    case STAGE_ATTN_PBF16: return launch(tm, ST_ATT, iefvad_attention_pbf16_kernel, grid, dim3(512), APB_LDS_BYTES, stream, ab);
    case STAGE_ATTN_BF16_ROWS: return launch(tm, ST_ATT, iefvad_attention_bf16_rows_kernel, grid, dim3(256), 0, stream, ab);
    case STAGE_ATTN_BF16: return launch(tm, ST_ATT, iefvad_attention_bf16_kernel, grid, dim3(256), 0, stream, ab);
    default: return fail("attention(bf16): the plan names no kernel");
    }
}

// `ha` arrives with its tensors filled in; the stream, scalars and the kernel choice are set here
static int launch_heads_chain(iefvad_handle* h, HeadsChainArgs& ha, int rows, float factor, hipStream_t stream, Timer& tm) {
    for (int m = 0; m < 2; ++m) ha.bias[m] = h->head[m].b;
    ha.stream = h->heads_stream;
    ha.M = rows; ha.factor = factor; ha.eps = h->cfg.epsilon; ha.wave_stride = (unsigned)heads_stream_wave_stride_bytes();
    const StagePlan pl = plan_heads(h->policy, h->num_cus, rows);
    const dim3 grid(pl.gx, pl.gy);
    tm.gemm_launches += 1;
    if (pl.kernel == STAGE_HEADS_PCHAIN) return launch(tm, ST_HEAD, iefvad_heads_pchain_bf16_kernel, grid, dim3(512), HP_LDS_BYTES, stream, ha);
    return launch(tm, ST_HEAD, iefvad_heads_chain_bf16_kernel, grid, dim3(512), HC_LDS_BYTES, stream, ha);
}

static int launch_refine_chain(iefvad_handle* h, const float* z_in, float* z_out, float* logits, int rows, hipStream_t stream, Timer& tm) {
    const int K = h->steps;                // a prefix of the packed stream, which is in step order; the waves' streams stay cfg.num_steps long
    ChainArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.z_in = z_in; ca.stream = h->chain_stream; ca.cls_w = h->cls_w; ca.cls_b = h->cls_b;
    ca.z_out = z_out;           // may be z_in (in place): a workgroup reads its 64 rows before it writes them
    ca.logits = logits;
    ca.M = rows; ca.K = K; ca.lambda = h->cfg.lambda_ref; ca.wave_stride = (unsigned)chain_wave_stride_bytes(h->cfg.num_steps);
    tm.gemm_launches += 1;
    return launch(tm, ST_REFINE, iefvad_refine_chain_bf16_kernel, dim3(rows / RC_BM), dim3(64 * RC_NW), RC_LDS_BYTES, stream, ca);
}

// The feature rows a call or a pass reads, both modalities in one element type: [B, 256, D] blocks (dense) or packed valid rows
struct RowsIn {
    const void* img;
    const void* ev;
    int32_t in_dtype;
    RowsIn at(size_t rows, int D) const {
        const size_t o = rows * D * in_elem_bytes(in_dtype);
        return RowsIn{(const char*)img + o, (const char*)ev + o, in_dtype};
    }
};

// The head-averaged attention maps a call asked for (include/iefvad.h, csrc/attention_maps.h): [rows, 256] fp32 per modality and layer,
// null where not asked for.  `at` moves every map to a later first row.
struct AttnMaps {
    float* p[2][IEFVAD_MAX_LAYERS];
    bool any() const {
        for (int m = 0; m < 2; ++m)
            for (int l = 0; l < IEFVAD_MAX_LAYERS; ++l)
                if (p[m][l]) return true;
        return false;
    }
    AttnMaps at(long long rows) const {
        AttnMaps o = *this;
        for (int m = 0; m < 2; ++m)
            for (int l = 0; l < IEFVAD_MAX_LAYERS; ++l)
                if (p[m][l]) o.p[m][l] += rows * IEF_T;
        return o;
    }
};

// The refinement trajectory a call asked for (include/iefvad.h, csrc/trajectory.h): the [steps + 1, stride] logits and the
// [steps, stride] update norms of the whole CALL, either nullable; a pass writes columns row0 + packed row of the pass.  z_prev: the
// pass's second state buffer (workspace_tail.h), set by Extras::place.
struct TrajOut {
    float* logits_steps;
    float* delta_norm;
    long long stride, row0;
    float* z_prev;
    bool any() const { return logits_steps || delta_norm; }
    TrajOut at(long long rows) const {
        TrajOut o = *this;
        o.row0 += rows;
        return o;
    }
};

// The fusion ablations a call asked for (include/iefvad.h, csrc/variants.h): the [count, stride] logits of the whole CALL; a pass writes
// columns row0 + packed row of the pass.  ws: the stacked state [count, R, D], its h scratch of the same size and the [count, R]
// logits of a pass (workspace_tail.h), set by Extras::place.
struct VarOut {
    int count;
    int kind[IEF_MAX_VARIANTS];
    float* logits;
    long long stride, row0;
    float* ws;
    bool any() const { return logits != nullptr; }
    VarOut at(long long rows) const {
        VarOut o = *this;
        o.row0 += rows;
        return o;
    }
};

// The score samples a call asked for (include/iefvad.h, csrc/samples.h): the [count, stride] logits and the per-snippet mean / standard
// deviation of the scores of the whole CALL; a pass writes columns row0 + packed row of the pass.  ids: the snippet ids at the pass's
// first packed row (nullable: row0 + packed row).  ws: the workspace of a group of IEF_MAX_VARIANTS stacked states (workspace_tail.h),
// set by Extras::place.
struct SampleOut {
    int count;
    unsigned long long seed;
    float scale;
    const int* ids;
    float* logits;
    float* mean;
    float* stdev;
    long long stride, row0;
    float* ws;
    bool any() const { return logits != nullptr; }
    SampleOut at(long long rows) const {
        SampleOut o = *this;
        if (ids) o.ids += rows;
        o.row0 += rows;
        return o;
    }
};

// What a call asks for beyond its base outputs, on either route: filled by the entry, value-initialised = nothing.  `at` is the one place
// that moves it to a later first row of the call (the series keep their base pointers and take their column from row0); `place` the
// one place that gives the members their homes behind the base workspace (workspace_tail.h, which carries its own copies of two sizes).
static_assert(kTailChunkRows == IEF_T && kTailSampleGroup == IEF_MAX_VARIANTS, "workspace_tail.h is out of step with common.h / variants.h");
struct Extras {
    const float* scale[2];           // the scaled / perturbed entries: per-row input scales (image, event), [rows] each
    RowNoise noise;                  // the perturbed entries: per-row noise amplitudes, ids and seed (common.h)
    AttnMaps attn;                   // the attn entries: [rows, 256] maps, written inside the encoder (pass_encoder_layer)
    TrajOut traj;                    // the trajectory entries
    VarOut var;                      // the variants entries
    SampleOut smp;                   // the samples entries
    bool keep_heads() const { return var.any() || smp.any(); }      // both re-form z0 from all four head tensors
    TailWants wants() const { return TailWants{false, false, traj.any(), var.any() ? var.count : 0, smp.any()}; }
    Extras at(long long rows) const {
        Extras o = *this;
        for (int m = 0; m < 2; ++m)
            if (scale[m]) o.scale[m] += rows;
        o.noise = noise.at(rows);        // ids default to the row of the CALL
        o.attn = attn.at(rows);
        o.traj = traj.at(rows);
        o.var = var.at(rows);
        o.smp = smp.at(rows);
        return o;
    }
    void place(void* workspace, const WorkspaceTail& t) {
        if (traj.any()) traj.z_prev = (float*)((char*)workspace + t.z_prev);
        if (var.any()) var.ws = (float*)((char*)workspace + t.var);
        if (smp.any()) smp.ws = (float*)((char*)workspace + t.smp);
    }
};

// The row perturbation of a call as the kernels take it (common.h): the caller's amplitudes, ids and seed at row 0 of the call
static RowNoise row_noise(const iefvad_perturb& p) {
    RowNoise nz = {};
    nz.amp[0] = p.noise_amp[0]; nz.amp[1] = p.noise_amp[1];
    nz.id = p.noise_row;
    nz.seed = p.seed;
    return nz;
}
// ... and with its scales, as the record of a call that asks for nothing else
static Extras perturb_extras(const iefvad_perturb& p) {
    Extras x = {};
    x.scale[0] = p.scale[0]; x.scale[1] = p.scale[1];
    x.noise = row_noise(p);
    return x;
}

// Where the results of a whole-video call go: one record per call, filled by the entry (csrc/videos.h, csrc/hostpipe.h); it is defined
// here because a pass (RaggedPass, below) holds the view of it at its own first packed row.  `at` is the one place where row offsets
// are added: it advances the vectors, the [rows, D] tensors and the extras; the series keeps its base pointer and takes its column
// from row0, which `at` advances by the same rows.  Everything is nullable except logits.
enum { kWideFused = 0, kWideMuI, kWideMuE, kWideLvI, kWideLvE, kWideWi, kWideWe };
struct VideosOut {
    float* logits;                   // [rows] each
    float* w_i_mean;
    float* w_e_mean;
    double* w_colsum;                // iefvad_forward_videos_scaled: [2, D], the call's column sums of w_i / w_e over its valid rows
    // the similarity entries: the [4, sim_stride] series; packed row r of this view is column row0 + r.  With it the tail keeps fused
    // (= z_K) and both mu of its row set (tail_keep).
    float* similarity;
    long long sim_stride;
    // the full entries: the caller's packed [rows, D] tensors in the order of kWideFused .. kWideWe.  The tail keeps the asked-for
    // tensors of its row set (mu / lv / z in the workspace aliases of pass_buffers, the weights in w_rows) and
    // iefvad_rows_out_wide_kernel copies the valid rows out (pass_rows_out).
    float* wide[ROWS_OUT_WIDE_MAX];
    Extras x;                        // the scaled, perturbed, attn, trajectory, variants and samples entries: what they add, in packed rows
    long long row0;                  // packed row of the call's list (the host entries: of the whole list) that this view's first row is
    int nan_mode;                    // 0 = rows as they are, 1 = the per-video rule of test.py:90-95, 2 = every video and modality (test2.py:59-60)
    bool sweep_codes;                // the scaled entry: nan_mode outside 0..2 is refused (the other entries read any non-zero value as 1)

    bool wants_w_rows() const { return w_colsum || wide[kWideWi] || wide[kWideWe]; }      // the fusion stage must store its weights
    TailWants wants() const {
        TailWants w = x.wants();
        w.w_rows = wants_w_rows(); w.colsum = w_colsum != nullptr;
        return w;
    }
    VideosOut at(long long rows, int D) const {
        VideosOut o = *this;
        o.logits += rows;
        if (w_i_mean) o.w_i_mean += rows;
        if (w_e_mean) o.w_e_mean += rows;
        for (int t = 0; t < ROWS_OUT_WIDE_MAX; ++t)
            if (wide[t]) o.wide[t] += rows * D;
        o.x = x.at(rows);
        o.row0 += rows;
        return o;
    }
};

// One pass of the valid rows of whole videos (forward_videos_impl, csrc/videos.h): the pass's packed rows are forward_pass's `in`
struct RaggedPass {
    const RaggedChunk* d_chunks;     // device: the pass's chunks (src_row relative to the pass's first packed row)
    const int* d_flags;              // device: NaN flag per (video, modality); nullptr unless out.nan_mode == 1
    int valid_rows;                  // packed rows of the pass (an online pass: its read-out rows)
    int enc_used_rows;               // rows of the compressed set that belong to chunks
    int enc_rows;                    // > 0: the encoder's row set is row-compressed (RaggedChunk, common.h) and has this many rows (a multiple of 256)
    int first_pass;                  // the pass overwrites out.w_colsum, later ones add to it
    float* w_rows[2];                // home of the pass's w_i / w_e rows ([R, D] each, behind the base workspace); set if out.wants_w_rows()
    double* colsum_part;             // [nb, 2, D] slab partials of the pass; set with out.w_colsum
    VideosOut out;                   // the call's destinations at the pass's first packed row
    // an online pass (csrc/online.h): the chunks are overlapping trailing windows, src_row relative to the pass's source base, and
    // only rows skip .. skip + count of window c are read out, to packed row dst of the pass (window_plan.h); nullptr otherwise
    const OnlineRead* d_reads;
    int read_slices;                 // workgroups per (window, modality) of the read-out gather: one per 16 rows of the pass's largest count
};

// The workspace of one micro-batch carved into its tensors, with the pass's row set and the kernel choices that depend on it
// (PassFlags from pass_buffers on, TailFlags from pass_compact_rows on: launch_rules.h).
struct PassBuffers : PassFlags, TailFlags {
    int nb, rows;             // chunks; rows of the current row set (the compaction step shrinks it)
    size_t R;                 // region stride in rows: the dense capacity nb * 256
    bool enc_rows_mode;       // row-compressed chunks: valid rows + one pad row each
    bool compacted;           // the tail runs on the gathered valid rows (pass_compact_rows)
    // workspace regions, in units of R*D floats: xin 0..2 | qkv 2..8 | att 8..10 | y 10..12 | x 12..14 | logits
    float *xin[2], *qkv[2], *att[2], *ybuf[2], *xbuf[2];
    bf16_t *qkvb[2], *attb[2], *xb[2];      // bf16 mode: q|k|v as bf16 in the qkv region; the att region holds attb | xb
    float* lg_scratch;        // R floats; the 3 R behind it (ws_floats_per_row) hold the ragged path's row means
    // tail buffers: the caller's tensors, else aliases of the (dead by then) qkv region: mu_i lv_i mu_e lv_e z | h  (bf16 mode: hb, zb in h's slot)
    float *mu_i, *lv_i, *mu_e, *lv_e, *z, *hbuf, *n_i, *n_e, *logits, *wim_out, *wem_out;
    bf16_t *hb, *zb;
    const float* cur[2];      // the encoder's current fp32 rows: the inputs, then each layer's output
    const float* xt[2];       // the tail's fp32 / bf16 A operands
    const bf16_t* xtb[2];
    // fp16x3: the running-max words of this micro-batch's activations (one word per tensor that feeds a projection); activation
    // tensor t owns IEF_AMAX_PARTS words per chunk of the micro-batch
    float* am; size_t mbs; int L, K;
    float* am_t(int t) const { return f16mb ? am + mbs * t : nullptr; }
    float* am_in(int m) const { return am_t(m); }
    float* am_att(int l, int m) const { return am_t(2 + 6 * l + m); }
    float* am_x(int l, int m) const { return am_t(2 + 6 * l + 2 + m); }
    float* am_qkv(int l, int m) const { return am_t(2 + 6 * l + 4 + m); }
    float* am_z(int k) const { return am_t(2 + 6 * L + k); }
    float* am_h(int k) const { return am_t(2 + 6 * L + (K + 1) + k); }
};

static PassBuffers pass_buffers(const iefvad_handle* h, int nb, size_t row0, void* workspace, const iefvad_outputs* out, const RaggedPass* rg) {
    const iefvad_config& c = h->cfg;
    const size_t D = h->D, R = (size_t)nb * IEF_T;
    PassBuffers b;
    memset(&b, 0, sizeof(b));
    b.nb = nb; b.R = R;
    b.enc_rows_mode = rg && rg->enc_rows > 0;
    b.rows = b.enc_rows_mode ? rg->enc_rows : nb * IEF_T;
    float* ws = (float*)workspace;
    float* t0 = ws + 2 * R * D;
    for (int m = 0; m < 2; ++m) {
        b.xin[m] = ws + m * R * D;
        b.qkv[m] = t0 + 3 * m * R * D;
        b.qkvb[m] = (bf16_t*)t0 + 3 * m * R * D;
        b.att[m] = ws + (8 + m) * R * D;
        b.attb[m] = (bf16_t*)(ws + 8 * R * D) + m * R * D;
        b.xb[m] = (bf16_t*)(ws + 9 * R * D) + m * R * D;
        b.ybuf[m] = ws + (10 + m) * R * D;
        b.xbuf[m] = ws + (12 + m) * R * D;
        b.xt[m] = b.xbuf[m];
        b.xtb[m] = b.xb[m];
    }
    b.lg_scratch = ws + 14 * R * D;
    b.mu_i = out->image_mu ? out->image_mu + row0 * D : t0;
    b.lv_i = out->image_logvar ? out->image_logvar + row0 * D : t0 + R * D;
    b.mu_e = out->event_mu ? out->event_mu + row0 * D : t0 + 2 * R * D;
    b.lv_e = out->event_logvar ? out->event_logvar + row0 * D : t0 + 3 * R * D;
    b.z = out->fused ? out->fused + row0 * D : t0 + 4 * R * D;
    b.hbuf = t0 + 5 * R * D;
    b.hb = (bf16_t*)b.hbuf; b.zb = b.hb + R * D;
    b.n_i = out->w_i ? out->w_i + row0 * D : nullptr;
    b.n_e = out->w_e ? out->w_e + row0 * D : nullptr;
    b.logits = out->logits ? out->logits + row0 : b.lg_scratch;
    b.wim_out = out->w_i_mean ? out->w_i_mean + row0 : nullptr;
    b.wem_out = out->w_e_mean ? out->w_e_mean + row0 : nullptr;
    if (rg) {                                     // per-row results of the pass land in scratch, then in rg's packed vectors
        b.logits = b.lg_scratch;
        b.wim_out = rg->out.w_i_mean ? b.lg_scratch + R : nullptr;
        b.wem_out = rg->out.w_e_mean ? b.lg_scratch + 2 * R : nullptr;
        b.n_i = rg->w_rows[0];                    // only with w_colsum or a wide w_i / w_e: the fusion stage stores its weights there
        b.n_e = rg->w_rows[1];
    }
    static_cast<PassFlags&>(b) = plan_pass(h->policy, c.compute, b.rows);
    b.am = h->amax_dev ? h->amax_dev + kAmaxActBase * IEF_AMAX_FLOATS : nullptr;
    b.mbs = (size_t)micro_batch(h) * IEF_AMAX_PARTS;
    b.L = c.num_layers; b.K = c.num_steps;
    return b;
}

// the projections of a pass on its current row set (pass_tail: with use_split = b.tail_split)
static ProjCtx proj_ctx(const iefvad_handle* h, const PassBuffers& b, hipStream_t stream, Timer& tm) {
    return ProjCtx{h->cfg.compute, b.splitmb, h->D, b.rows, stream, &tm, h->policy.split_tile, h->policy.split_always};
}

// 0. inputs: `.to(torch.float)` (imf_vad.py:41-42) into b.cur; bf16 mode also gets the bf16 operand copy (b.need_xb0)
static int pass_load_inputs(iefvad_handle* h, PassBuffers& b, const RowsIn& in, const Extras& x, const RaggedPass* rg, hipStream_t stream, Timer& tm) {
    const size_t D = h->D, n = b.R * D;
    const void* const pi = in.img;
    const void* const pe = in.ev;
    const int32_t in_dtype = in.in_dtype;
    const bool d512 = h->D == IEF_D512;
    bf16_t* const b0p = b.need_xb0 ? b.xb[0] : nullptr;
    bf16_t* const b1p = b.need_xb0 ? b.xb[1] : nullptr;
    b.cur[0] = b.xin[0]; b.cur[1] = b.xin[1];
    if (rg) {
        // the chunker (tools.py:100-114) and the conditional nan_to_num (test.py:90-95) on the device: ragged.h
        if (b.enc_rows_mode && rg->enc_used_rows < b.rows) {     // the zero rows that round the set up to whole 256-row tiles
            const size_t o = (size_t)rg->enc_used_rows * D, nz = (size_t)(b.rows - rg->enc_used_rows) * D;
            for (int m = 0; m < 2; ++m) {
                HIP_TRY(hipMemsetAsync(b.xin[m] + o, 0, nz * sizeof(float), stream));
                if (b.need_xb0) HIP_TRY(hipMemsetAsync(b.xb[m] + o, 0, nz * sizeof(bf16_t), stream));
            }
        }
        // (the NaN flags of ALL the call's videos are already set: forward_videos_impl scans every pass's chunks before the
        // first pass runs, because test.py:90-95 decides per whole video and a video may straddle passes)
        const int nan_all = rg->out.nan_mode == 2;
        const bool scaled = x.scale[0] || x.scale[1] || nan_all;
        const bool noisy = x.noise.any();       // an amplitude vector selects the noise instantiation; every other call launches what it always has
        if (int rc = dispatch_in(in_dtype, d512, [&](auto t, auto w) {
                using T = typename decltype(t)::type;
                constexpr int W = decltype(w)::value;
                const dim3 grid(b.nb, 2, IEF_RAGGED_SLICES);
                const int nrows = b.enc_rows_mode ? 0 : IEF_T;
                if (noisy)
                    return launch(tm, ST_CAST, iefvad_scatter_rows_kernel<T, W, true, RowNoise>, grid, dim3(256), 0, stream, (const T*)pi, (const T*)pe,
                                  rg->d_chunks, rg->d_flags, b.xin[0], b.xin[1], b0p, b1p, nrows, x.scale[0], x.scale[1], nan_all, x.noise);
                return launch(tm, ST_CAST, scaled ? iefvad_scatter_rows_kernel<T, W, true> : iefvad_scatter_rows_kernel<T, W, false>, grid, dim3(256), 0,
                              stream, (const T*)pi, (const T*)pe, rg->d_chunks, rg->d_flags, b.xin[0], b.xin[1], b0p, b1p, nrows, x.scale[0], x.scale[1],
                              nan_all);
            })) return rc;
    } else if (x.scale[0] || x.scale[1] || x.noise.any()) {
        // iefvad_forward_scaled / _perturbed: the rows pass through the cast kernel whatever their type, scaled and perturbed on the way (rowops.h)
        hipEvent_t e = tm.begin(ST_CAST);
        const int rc = dispatch_in(in_dtype, d512, [&](auto t, auto w) {
            return launch_cast_scaled<typename decltype(t)::type, decltype(w)::value>(pi, pe, b.xin[0], b.xin[1], b0p, b1p, n, x.scale[0], x.scale[1], x.noise, stream);
        });
        tm.end(e);
        if (rc) return rc;
    } else if (in_dtype == IEFVAD_IN_F32) {
        b.cur[0] = (const float*)pi; b.cur[1] = (const float*)pe;
        if (b.need_xb0) {
            hipEvent_t e = tm.begin(ST_CAST);
            const int rc = launch_cast<float>(pi, pe, nullptr, nullptr, b.xb[0], b.xb[1], n, 2, stream);
            tm.end(e);
            if (rc) return rc;
        }
    } else {
        hipEvent_t e = tm.begin(ST_CAST);
        const int rc = dispatch_in(in_dtype, d512, [&](auto t, auto) {
            return launch_cast<typename decltype(t)::type>(pi, pe, b.xin[0], b.xin[1], b0p, b1p, n, 2, stream);
        });
        tm.end(e);
        if (rc) return rc;
    }
    if (b.f16mb) {
        // every (tensor, chunk) of this micro-batch starts from zero words; a kernel node, not a memset node, when captured (rowops.h)
        const unsigned words = (unsigned)b.nb * IEF_AMAX_PARTS;
        const dim3 zero_grid((words / 4 + 255) / 256, amax_act_tensors(b.L, b.K));
        if (int rc = launch(iefvad_amax_zero_kernel, zero_grid, dim3(256), 0, stream, b.am, b.mbs, words)) return rc;
        if (int rc = launch(tm, ST_CAST, iefvad_amax_chunk_kernel, dim3(b.nb, 2), dim3(256), 0, stream, b.cur[0], b.cur[1], b.am_in(0), b.am_in(1))) return rc;
    }
    return 0;
}

// 1. one layer of the temporal encoder (imf_vad.py:113-123): in_proj, attention, out_proj + residual, LayerNorm; b.cur moves to its output
static int pass_encoder_layer(iefvad_handle* h, PassBuffers& b, int l, const RaggedPass* rg, const AttnMaps& maps, hipStream_t stream, Timer& tm) {
    const iefvad_config& c = h->cfg;
    const bool bf = (c.compute == IEFVAD_COMPUTE_BF16);
    const int D = h->D, L = c.num_layers, rows = b.rows, nb = b.nb;
    const bool d512 = h->D == IEF_D512;      // iefvad_create_ex: f32 arithmetic only, so every bf16 / split branch below is 768-wide
    const RaggedChunk* enc_chunks = b.enc_rows_mode ? rg->d_chunks : nullptr;
    const ProjCtx px = proj_ctx(h, b, stream, tm);
    if (b.ip_chain) {
        const void* ipA[2] = {(l == 0) ? (const void*)b.cur[0] : (const void*)b.xb[0], (l == 0) ? (const void*)b.cur[1] : (const void*)b.xb[1]};
        if (int rc = launch_inproj_chain(h, l, ipA, l == 0, b.qkvb, rows, stream, tm)) return rc;
    } else {
        Proj p = Proj::of(EPI_QKV, 3 * D, 3 * D, h->in[0][l], &h->in[1][l]);
        p.qcols = D;
        // q is pre-scaled for the softmax by log2(e)/sqrt(d_h): both attention kernels use exp2
        p.alpha = 1.0f / sqrtf((float)h->DH) * 1.4426950408889634f;
        for (int m = 0; m < 2; ++m) {
            p.A32[m] = b.cur[m]; p.A16[m] = b.xb[m]; p.amaxA[m] = l == 0 ? b.am_in(m) : b.am_x(l - 1, m);
            p.amaxC[m] = b.am_qkv(l, m);
            if (bf) p.Cb[m] = b.qkvb[m]; else p.C[m] = b.qkv[m];
        }
        if (int rc = launch_proj(px, p, ST_QKV)) return rc;
    }

    if (bf) {
        if (int rc = launch_attention_bf16(h, b.qkvb, b.attb, nb, enc_chunks, b.ip_chain, rows, stream, tm)) return rc;
    } else {
        AttnArgs aa;
        memset(&aa, 0, sizeof(aa));
        for (int m = 0; m < 2; ++m) { aa.qkv[m] = b.qkv[m]; aa.out[m] = b.att[m]; }
        aa.nchunks = nb;
        aa.chunks = enc_chunks;
        // bf16x6: the split attention kernel goes with the split projections (same batch-size rule), so a small
        // batch is computed exactly as in the f32 mode
        for (int m = 0; m < 2; ++m) { aa.amax[m] = b.am_att(l, m); aa.amax_in[m] = b.am_qkv(l, m); }
        void (*const kernel)(AttnArgs) = b.f16mb    ? iefvad_attention_split_f16_kernel
                                         : b.splitmb ? (enc_chunks ? iefvad_attention_split_rows_kernel : iefvad_attention_split_kernel)
                                         : d512      ? (enc_chunks ? iefvad_attention_f32_rows_d64_kernel : iefvad_attention_f32_d64_kernel)
                                                     : (enc_chunks ? iefvad_attention_f32_rows_kernel : iefvad_attention_f32_kernel);
        if (int rc = launch(tm, ST_ATT, kernel, dim3(IEF_H, 2, 2 * nb), dim3(256), b.splitmb ? ATS_LDS_BYTES : 0, stream, aa)) return rc;
    }

    if (maps.p[0][l] || maps.p[1][l]) {
        // the layer's head-averaged attention weights, from q | k | v while they are alive (attention_maps.h).  The entries refuse
        // the bf16 arithmetic, whose q | k | v are bf16 planes in another layout.
        if (bf) return fail("attention maps: compute = BF16 is not supported");
        AttnMapArgs ma;
        memset(&ma, 0, sizeof(ma));
        for (int m = 0; m < 2; ++m) { ma.qkv[m] = b.qkv[m]; ma.out[m] = maps.p[m][l]; }
        ma.nchunks = nb;
        ma.chunks = rg ? rg->d_chunks : nullptr;
        void (*const kernel)(AttnMapArgs) = d512 ? (enc_chunks ? iefvad_attention_maps_kernel<true, 64> : iefvad_attention_maps_kernel<false, 64>)
                                                 : (enc_chunks ? iefvad_attention_maps_kernel<true, IEF_DH> : iefvad_attention_maps_kernel<false, IEF_DH>);
        if (int rc = launch(tm, ST_ATT, kernel, dim3(2, 2 * nb), dim3(256), 0, stream, ma)) return rc;
    }

    if (b.ln_fused) {      // out_proj + residual + LayerNorm(s) in one row-owning kernel
        float* oy[2] = {(l < L - 1) ? b.xbuf[0] : nullptr, (l < L - 1) ? b.xbuf[1] : nullptr};      // fp32 rows are only the next layer's residual
        if (int rc = launch_outproj_ln_chain(h, l, l == L - 1, b.attb, b.cur, oy, b.xb, rows, stream, tm)) return rc;
    } else {
        Proj p = Proj::of(EPI_BIAS_RESID, D, D, h->out[0][l], &h->out[1][l]);
        for (int m = 0; m < 2; ++m) {
            p.A32[m] = b.att[m]; p.A16[m] = b.attb[m]; p.amaxA[m] = b.am_att(l, m);
            p.C[m] = b.ybuf[m]; p.R[m] = b.cur[m];
        }
        if (int rc = launch_proj(px, p, ST_OUT)) return rc;

        LnArgs la;
        memset(&la, 0, sizeof(la));
        la.nrows = rows; la.eps = 1e-5f;
        for (int m = 0; m < 2; ++m) {
            la.x[m] = b.ybuf[m]; la.g1[m] = h->norm_w[m][l]; la.b1[m] = h->norm_b[m][l];
            if (l == L - 1) { la.g2[m] = h->whiten_w[m]; la.b2[m] = h->whiten_b[m]; }   // whitening LN, :117,:123
            // fp32 mode: x feeds both the next projection and the next residual; bf16 mode: the bf16 copy feeds the
            // projection, the fp32 tensor is only the next layer's residual (not needed after the last layer)
            la.y[m] = (!bf || l < L - 1) ? b.xbuf[m] : nullptr;
            la.yb[m] = bf ? b.xb[m] : nullptr;
            la.amax[m] = b.am_x(l, m);
        }
        const dim3 grid((rows + ROW_WAVES - 1) / ROW_WAVES, 2);
        if (int rc = dispatch_d(d512, [&](auto w) { return launch(tm, ST_LN, iefvad_layernorm_kernel<decltype(w)::value>, grid, dim3(256), 0, stream, la); }))
            return rc;
    }
    b.cur[0] = b.xbuf[0]; b.cur[1] = b.xbuf[1];
    return 0;
}

// Ragged pass with whole chunks in the encoder (IEFVAD_DENSE_ENCODER=1): everything behind the encoder is row-wise
// (imf_vad.py:125-150) and the reference slices the pad rows away (test.py:121), so the valid rows of the last
// LayerNorm's output are gathered (packed order, padded with zero rows to whole 256-row tiles) and b.rows shrinks to
// that count from here on.  fp16x3 keeps whole chunks: its operand scales are per chunk.  The compact operands live in
// the attention-output region, dead by now.  (Row-compressed chunks, the default: the tail runs on the encoder's row set.)
static int pass_compact_rows(iefvad_handle* h, PassBuffers& b, const RaggedPass* rg, hipStream_t stream, Timer& tm) {
    const bool bf = (h->cfg.compute == IEFVAD_COMPUTE_BF16);
    const size_t D = h->D;
    if (rg && rg->d_reads) {
        // an online pass, row-compressed windows or whole chunks: the windows' read-out rows are gathered in packed order and the
        // tail runs on them alone, as on a compacted set (the entry refuses fp16x3)
        const int mc = (rg->valid_rows + 255) / 256 * 256;        // <= b.rows: a window contributes at most its valid rows
        const size_t tail0 = (size_t)rg->valid_rows * D, tailn = (size_t)(mc - rg->valid_rows) * D;
        const dim3 grid(b.nb, 2, rg->read_slices);
        const bool d512 = h->D == IEF_D512;
        if (bf) {
            ReadoutArgs<bf16_t> ra;
            memset(&ra, 0, sizeof(ra));
            for (int m = 0; m < 2; ++m) { ra.src[m] = b.xb[m]; ra.dst[m] = b.attb[m]; b.xtb[m] = b.attb[m]; }
            ra.chunks = rg->d_chunks; ra.reads = rg->d_reads;
            if (tailn)
                for (int m = 0; m < 2; ++m) HIP_TRY(hipMemsetAsync(b.attb[m] + tail0, 0, tailn * sizeof(bf16_t), stream));
            if (int rc = dispatch_d(d512, [&](auto w) {
                    return launch(tm, ST_CAST, iefvad_readout_rows_kernel<bf16_t, decltype(w)::value>, grid, dim3(256), 0, stream, ra);
                })) return rc;
        } else {
            ReadoutArgs<float> ra;
            memset(&ra, 0, sizeof(ra));
            for (int m = 0; m < 2; ++m) { ra.src[m] = b.xbuf[m]; ra.dst[m] = b.att[m]; b.xt[m] = b.att[m]; }
            ra.chunks = rg->d_chunks; ra.reads = rg->d_reads;
            if (tailn)
                for (int m = 0; m < 2; ++m) HIP_TRY(hipMemsetAsync(b.att[m] + tail0, 0, tailn * sizeof(float), stream));
            if (int rc = dispatch_d(d512, [&](auto w) {
                    return launch(tm, ST_CAST, iefvad_readout_rows_kernel<float, decltype(w)::value>, grid, dim3(256), 0, stream, ra);
                })) return rc;
        }
        b.rows = mc;
        b.compacted = true;
    } else if (rg && !b.enc_rows_mode && h->cfg.compute != IEFVAD_COMPUTE_FP16X3) {
        const int mc = (rg->valid_rows + 255) / 256 * 256;
        if (mc < b.rows) {
            CompactArgs ca;
            memset(&ca, 0, sizeof(ca));
            for (int m = 0; m < 2; ++m) {
                if (bf) { ca.xb[m] = b.xb[m]; ca.xcb[m] = b.attb[m]; b.xtb[m] = b.attb[m]; }
                else { ca.x[m] = b.xbuf[m]; ca.xc[m] = b.att[m]; b.xt[m] = b.att[m]; }
            }
            ca.chunks = rg->d_chunks;
            const size_t tail0 = (size_t)rg->valid_rows * D, tailn = (size_t)(mc - rg->valid_rows) * D;
            if (tailn)
                for (int m = 0; m < 2; ++m)
                    HIP_TRY(bf ? hipMemsetAsync(b.attb[m] + tail0, 0, tailn * sizeof(bf16_t), stream)
                               : hipMemsetAsync(b.att[m] + tail0, 0, tailn * sizeof(float), stream));
            if (int rc = dispatch_d(h->D == IEF_D512, [&](auto w) {
                    return launch(tm, ST_CAST, iefvad_compact_rows_kernel<decltype(w)::value>, dim3(b.nb, 2), dim3(256), 0, stream, ca);
                })) return rc;
            b.rows = mc;
            b.compacted = true;
        }
    }
    static_cast<TailFlags&>(b) = plan_tail(h->policy, h->cfg.compute, b.rows, h->steps, b.splitmb, b.compacted, h->heads_stream != nullptr,
                                           h->chain_stream != nullptr);
    return 0;
}

// What the tail stores of its row set: the caller of a dense pass asked for the tensor, or a ragged pass copies it out (the full
// entries) or reduces it to the similarity series (fused and both mu) before it ends -- then it stays in the workspace alias of
// pass_buffers.  Kernel selection does not look at these.
struct TailKeep { bool fused, mu_i, mu_e, lv_i, lv_e; };
static TailKeep tail_keep(const iefvad_outputs* out, const RaggedPass* rg, bool heads) {
    auto rows = [&](int t, bool in_series) { return rg && (rg->out.wide[t] || (in_series && rg->out.similarity)); };
    // heads: the ablations / the score samples re-form z0 from all four head tensors (pass_variants, pass_samples)
    return TailKeep{out->fused || rows(kWideFused, true), out->image_mu || rows(kWideMuI, true) || heads, out->event_mu || rows(kWideMuE, true) || heads,
                    out->image_logvar || rows(kWideLvI, false) || heads, out->event_logvar || rows(kWideLvE, false) || heads};
}

// The rows of a pass that carry results, as the kernels behind the tail take them: the chunk table on the row-compressed / whole-chunk
// set (one slab per chunk), or no table on a dense or a compacted set, which is in packed order already (256-row slabs of it).
struct RowSet { const RaggedChunk* chunks; int valid_rows, nslabs; };
static RowSet row_set(const PassBuffers& b, const RaggedPass* rg) {
    const RaggedChunk* const chunks = (rg && !b.compacted) ? rg->d_chunks : nullptr;
    const int valid_rows = rg ? rg->valid_rows : b.rows;
    return RowSet{chunks, valid_rows, chunks ? b.nb : (valid_rows + 255) / 256};
}

// The probe of state z_k of a trajectory pass (trajectory.h): k = 0 behind the fusion, k = j + 1 behind step j.  `copy_logits`: entry k
// is the pass's logits, already in b.logits (the folded scorer).
static int pass_step_probe(iefvad_handle* h, const PassBuffers& b, const RaggedPass* rg, const TrajOut& tj, int k, int steps, bool copy_logits,
                           hipStream_t stream, Timer& tm) {
    float* const lo = tj.logits_steps ? tj.logits_steps + (long long)k * tj.stride : nullptr;
    float* const dn = (tj.delta_norm && k > 0) ? tj.delta_norm + (long long)(k - 1) * tj.stride : nullptr;
    const int store_prev = tj.delta_norm && k < steps;
    if (!lo && !dn && !store_prev) return 0;
    const RowSet rs = row_set(b, rg);
    const RaggedChunk* const chunks = rs.chunks;
    const int valid_rows = rs.valid_rows, nslabs = rs.nslabs;
    return dispatch_d(h->D == IEF_D512, [&](auto w) {
        return launch(tm, ST_SCORER, iefvad_step_probe_kernel<decltype(w)::value>, dim3(nslabs, TRAJ_SLICES), dim3(256), 0, stream, (const float*)b.z, tj.z_prev,
                      (const float*)h->cls_w, (const float*)h->cls_b, copy_logits ? (const float*)b.logits : (const float*)nullptr, chunks, valid_rows, lo, dn,
                      tj.row0, k == 0 ? 1 : 0, store_prev);
    });
}

// 4 - 5 of the tail on the state b.z of b.rows rows (scratch b.hbuf / b.hb / b.zb, partial sums in the y region, logits to b.logits),
// with the kernels b's TailFlags name: the call's own tail (pass_tail), and once more the stacked states of its fusion ablations
// and score samples (pass_stacked).  chain: the bf16 chain kernel takes steps and scorer; keep_fused: z_K is wanted, not the logits alone.
static int pass_refine_score(iefvad_handle* h, PassBuffers& b, const RaggedPass* rg, const TrajOut* tj, bool chain, bool keep_fused, hipStream_t stream,
                             Timer& tm) {
    const iefvad_config& c = h->cfg;
    const bool bf = (c.compute == IEFVAD_COMPUTE_BF16);
    const int D = h->D, K = h->steps, rows = b.rows;
    const bool d512 = h->D == IEF_D512;
    const dim3 row_grid((rows + ROW_WAVES - 1) / ROW_WAVES);
    float* const z = b.z;
    ProjCtx px = proj_ctx(h, b, stream, tm);
    px.use_split = b.tail_split;
    const bool fold = b.fold;
    const float* const score_fold = score_fold_of(h, K);

    if (chain)
        if (int rc = launch_refine_chain(h, z, keep_fused ? z : nullptr, b.logits, rows, stream, tm)) return rc;

    // bf16x6 on the split kernels: the last step's second projection is folded into the scorer,
    //   logits = c . z_K + b_c = c . z_{K-1} + v . h + s0     (v, s0: iefvad_set_weights; rowops.h),
    // v . h taken in the epilogue of the last step's FIRST projection (EPI_BIAS_RELU_DOT: six partial sums per row, into the y
    // region, dead since the last LayerNorm).  Without `fused` in the outputs (and no similarity reduction behind the pass:
    // keep_fused) that projection stores no h and the last W2 launch does not run; with it, h is stored and z_K is formed as always,
    // after the scorer has read z_{K-1} (EPI_REFINE updates z in place) -- so the logits of both output sets are the same bits.
    float* const fold_part = b.ybuf[0];

    // 4. K refinement steps z <- z - lambda * (W2 relu(W1 z + b1) + b2) (imf_vad.py:146-149); the state z stays fp32
    for (int k = 0; k < K && !chain; ++k) {
        const bool dot = fold && k == K - 1;
        Proj p = Proj::of(EPI_BIAS_RELU, D, D, h->ref1[k]);
        p.A32[0] = z; p.A16[0] = b.zb; p.amaxA[0] = b.am_z(k); p.amaxC[0] = b.am_h(k);
        p.C[0] = bf ? nullptr : b.hbuf; p.Cb[0] = bf ? b.hb : nullptr;
        if (dot) {
            p.epi = EPI_BIAS_RELU_DOT; p.R[0] = score_fold; p.C2[0] = fold_part;
            if (!keep_fused) p.C[0] = nullptr;
        }
        if (int rc = launch_proj(px, p, ST_REFINE)) return rc;
        if (dot) {
            if (int rc = launch(tm, ST_SCORER, iefvad_scorer_fold_kernel<IEF_D, IEF_D / kSplitBN>, row_grid, dim3(256), 0, stream, z, h->cls_w, fold_part,
                                score_fold, b.logits, rows)) return rc;
            if (!keep_fused) break;
        }
        p = Proj::of(EPI_REFINE, D, D, h->ref2[k]);
        p.alpha = c.lambda_ref;
        p.A32[0] = b.hbuf; p.A16[0] = b.hb; p.amaxA[0] = b.am_h(k); p.amaxC[0] = b.am_z(k + 1);
        p.C[0] = z; p.R[0] = z; p.Cb[0] = (bf && k + 1 < K) ? b.zb : nullptr;
        if (int rc = launch_proj(px, p, ST_REFINE)) return rc;
        if (tj)
            if (int rc = pass_step_probe(h, b, rg, *tj, k + 1, K, dot, stream, tm)) return rc;
    }

    // 5. scorer (imf_vad.py:150)
    if (!chain && !fold)
        return dispatch_d(d512, [&](auto w) {
            return launch(tm, ST_SCORER, iefvad_scorer_kernel<decltype(w)::value>, row_grid, dim3(256), 0, stream, z, h->cls_w, h->cls_b, b.logits, rows);
        });
    return 0;
}

// 2 - 5. everything behind the encoder, row-wise: heads, fusion, refinement, scorer.  K is the handle's current step count
// (iefvad_set_steps): blocks 0 .. K - 1 run.  `tj` (nullable): the pass records its trajectory -- a probe launch behind the fusion and
// behind every step; the state must then pass through HBM between steps, so the bf16 arithmetic takes its launch-per-projection
// route (bit-identical to the chain kernel) and the folded bf16x6 tail forms z_K as a pass that keeps `fused` does.
static int pass_tail(iefvad_handle* h, PassBuffers& b, const iefvad_outputs* out, const RaggedPass* rg, const TrajOut* tj, bool keep_heads,
                     hipStream_t stream, Timer& tm) {
    const iefvad_config& c = h->cfg;
    const bool bf = (c.compute == IEFVAD_COMPUTE_BF16);
    const int D = h->D, L = c.num_layers, K = h->steps, rows = b.rows;
    const bool d512 = h->D == IEF_D512;
    const float factor = precision_factor(c);
    const dim3 row_grid((rows + ROW_WAVES - 1) / ROW_WAVES);
    float* const z = b.z;
    ProjCtx px = proj_ctx(h, b, stream, tm);
    px.use_split = b.tail_split;

    const bool chain = b.chain && !tj;
    const TailKeep keep = tail_keep(out, rg, keep_heads);
    const bool keep_fused = keep.fused || tj;
    // 2 + 3 in one kernel (b.heads_rows): the four head tensors are stored only if the caller asked for them.
    if (b.heads_rows) {
        HeadsChainArgs ha;
        memset(&ha, 0, sizeof(ha));
        for (int m = 0; m < 2; ++m) ha.A[m] = b.xtb[m];
        ha.mu[0] = keep.mu_i ? b.mu_i : nullptr; ha.lv[0] = keep.lv_i ? b.lv_i : nullptr;
        ha.mu[1] = keep.mu_e ? b.mu_e : nullptr; ha.lv[1] = keep.lv_e ? b.lv_e : nullptr;
        ha.n[0] = b.n_i; ha.n[1] = b.n_e;
        ha.z = z;
        ha.zb = chain ? nullptr : b.zb;
        const bool means = b.wim_out || b.wem_out;
        ha.nsum_part = means ? b.ybuf[0] : nullptr;        // y is dead after the last LayerNorm: 48 of its 768 floats per row
        if (int rc = launch_heads_chain(h, ha, rows, factor, stream, tm)) return rc;
        if (means)
            if (int rc = launch(tm, ST_FUSION, iefvad_rowmean_finish_kernel, dim3((2 * rows + 255) / 256), dim3(256), 0, stream, ha.nsum_part, b.wim_out,
                                b.wem_out, rows, HC_NPART)) return rc;
    } else {
        // 2. mu / logvar heads (imf_vad.py:125-128): one [768 -> 1536] projection per modality
        Proj p = Proj::of(EPI_HEADS, 2 * D, D, h->head[0], &h->head[1]);
        for (int m = 0; m < 2; ++m) {
            p.A32[m] = b.xt[m]; p.A16[m] = b.xtb[m]; p.amaxA[m] = b.am_x(L - 1, m);
        }
        p.C[0] = b.mu_i; p.C2[0] = b.lv_i; p.C[1] = b.mu_e; p.C2[1] = b.lv_e;
        if (int rc = launch_proj(px, p, ST_HEAD)) return rc;

        // 3. precision weights + fusion (imf_vad.py:130-144), fp32 in both modes
        FusionArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.mu_i = b.mu_i; fa.lv_i = b.lv_i; fa.mu_e = b.mu_e; fa.lv_e = b.lv_e;
        fa.n_i = b.n_i; fa.n_e = b.n_e; fa.n_i_mean = b.wim_out; fa.n_e_mean = b.wem_out;
        fa.z = z;
        fa.zb = (bf && !chain) ? b.zb : nullptr;
        fa.nrows = rows; fa.factor = factor; fa.eps = c.epsilon;
        fa.z_amax = b.am_z(0);
        if (int rc = dispatch_d(d512, [&](auto w) { return launch(tm, ST_FUSION, iefvad_fusion_kernel<decltype(w)::value>, row_grid, dim3(256), 0, stream, fa); }))
            return rc;
    }

    if (tj)
        if (int rc = pass_step_probe(h, b, rg, *tj, 0, K, false, stream, tm)) return rc;
    return pass_refine_score(h, b, rg, tj, chain, keep_fused, stream, tm);
}

// 6. a ragged pass: the valid rows' results -> the caller's packed vectors and tensors (test.py:119-121: logits1[0:len_cur]), from
// where the tail left them, by the pass's row set (row_set).
static int pass_rows_out(iefvad_handle* h, const PassBuffers& b, const RaggedPass* rg, hipStream_t stream, Timer& tm) {
    const VideosOut& o = rg->out;
    const bool d512 = h->D == IEF_D512;
    const RowSet rs = row_set(b, rg);
    const RaggedChunk* const chunks = rs.chunks;
    const int valid_rows = rs.valid_rows, nslabs = rs.nslabs;
    if (int rc = launch(tm, ST_SCORER, iefvad_rows_out_kernel, dim3(nslabs), dim3(256), 0, stream, b.logits, b.wim_out, b.wem_out, o.logits, o.w_i_mean,
                        o.w_e_mean, chunks, valid_rows)) return rc;
    if (o.similarity)      // the four series of the pass's valid rows from z_K / mu_i / mu_e (similarity.h)
        if (int rc = dispatch_d(d512, [&](auto w) {
                return launch(tm, ST_SCORER, iefvad_similarity_rowset_kernel<decltype(w)::value>, dim3(nslabs, SIM_SLICES), dim3(256), 0, stream, b.z, b.mu_i,
                              b.mu_e, chunks, valid_rows, o.similarity, o.sim_stride, o.row0);
            })) return rc;
    // the full entries: the valid rows of the kept tensors -> the caller's packed tensors
    RowsOutWideArgs wa;
    memset(&wa, 0, sizeof(wa));
    const float* const home[ROWS_OUT_WIDE_MAX] = {b.z, b.mu_i, b.mu_e, b.lv_i, b.lv_e, b.n_i, b.n_e};
    int nt = 0;
    for (int t = 0; t < ROWS_OUT_WIDE_MAX; ++t)
        if (o.wide[t]) { wa.src[nt] = home[t]; wa.dst[nt] = o.wide[t]; ++nt; }
    if (nt) {
        wa.chunks = chunks;
        wa.valid_rows = valid_rows;
        if (int rc = dispatch_d(d512, [&](auto w) {
                return launch(tm, ST_SCORER, iefvad_rows_out_wide_kernel<decltype(w)::value>, dim3(nslabs, nt, IEF_RAGGED_SLICES), dim3(256), 0, stream, wa);
            })) return rc;
    }
    if (o.w_colsum) {
        // column sums of the stored weights over the valid rows (ragged.h)
        hipEvent_t e = tm.begin(ST_FUSION);      // one span over both launches
        int rc = dispatch_d(d512, [&](auto w) {
            return launch(iefvad_colsum_rows_kernel<decltype(w)::value>, dim3(nslabs, 2), dim3(256), 0, stream, b.n_i, b.n_e, chunks, valid_rows, rg->colsum_part);
        });
        if (!rc) rc = launch(iefvad_colsum_finish_kernel, dim3(2 * h->D / 16), dim3(256), 0, stream, rg->colsum_part, nslabs, 2 * h->D, rg->first_pass, o.w_colsum);
        tm.end(e);
        if (rc) return rc;
    }
    return 0;
}

// What the fusion ablations and the score samples share: V states of the pass's row set stacked as ONE row set of V x rows rows in
// `ws` (the state [V, rows, D], its h scratch at V R D floats, the [V, rows] logits at 2 V R D: variants_bytes), with the kernels
// plan_tail names for that row count (bf16: one chain launch where the rule says chain; bf16x6 on the split kernels: a scores-only
// tail with the folded scorer; f32: the fp32 tilings, bit-identical to each other) ...
static PassBuffers stacked_buffers(const iefvad_handle* h, const PassBuffers& b, float* ws, int V) {
    const size_t n = (size_t)V * b.R * h->D;
    PassBuffers s = b;
    s.rows = V * b.rows;
    s.z = ws;
    s.hbuf = ws + n;
    s.hb = (bf16_t*)s.hbuf; s.zb = s.hb + (size_t)V * b.rows * h->D;
    s.logits = ws + 2 * n;
    static_cast<TailFlags&>(s) = plan_tail(h->policy, h->cfg.compute, s.rows, h->steps, b.splitmb, b.compacted, h->heads_stream != nullptr,
                                           h->chain_stream != nullptr);
    return s;
}
// ... and, behind steps 4 - 5 on the stacked set, the valid rows' logits to rows 0 .. V - 1 of a [V, stride] result at `dst`
static int pass_stacked_out(const PassBuffers& b, const PassBuffers& s, const RaggedPass* rg, int V, float* dst, long long stride, long long row0,
                            hipStream_t stream, Timer& tm) {
    const RowSet rs = row_set(b, rg);
    const RaggedChunk* const chunks = rs.chunks;
    const int valid_rows = rs.valid_rows, nslabs = rs.nslabs;
    return launch(tm, ST_SCORER, iefvad_variants_out_kernel, dim3(nslabs, V), dim3(256), 0, stream, (const float*)s.logits, b.rows, chunks, valid_rows, dst,
                  stride, row0);
}
// The four steps on V stacked states: their buffers in `ws`, `fill(s, zb)` writes the V z0 (zb: the bf16 copy, null where the tail
// does not read it), steps 4 - 5, the valid rows' logits to `dst`
template <typename Fill>
static int pass_stacked(iefvad_handle* h, const PassBuffers& b, const RaggedPass* rg, float* ws, int V, float* dst, long long stride, long long row0,
                        hipStream_t stream, Timer& tm, Fill&& fill) {
    PassBuffers s = stacked_buffers(h, b, ws, V);
    if (int rc = fill(s, (h->cfg.compute == IEFVAD_COMPUTE_BF16 && !s.chain) ? s.zb : nullptr)) return rc;
    if (int rc = pass_refine_score(h, s, rg, nullptr, s.chain, false, stream, tm)) return rc;
    return pass_stacked_out(b, s, rg, V, dst, stride, row0, stream, tm);
}

// 7. the fusion ablations of a pass (variants.h), behind its own results: the variants' z0 from the kept mu / logvar of the row set,
// stacked behind the workspace, then steps 4 - 5 on it, then the valid rows' logits to the call's [count, stride] result.
static int pass_variants(iefvad_handle* h, const PassBuffers& b, const RaggedPass* rg, const VarOut& vo, hipStream_t stream, Timer& tm) {
    const iefvad_config& c = h->cfg;
    const bool d512 = h->D == IEF_D512;
    const int V = vo.count, rows = b.rows;
    return pass_stacked(h, b, rg, vo.ws, V, vo.logits, vo.stride, vo.row0, stream, tm, [&](const PassBuffers& s, bf16_t* zb) {
        VariantArgs va;
        memset(&va, 0, sizeof(va));
        va.mu_i = b.mu_i; va.lv_i = b.lv_i; va.mu_e = b.mu_e; va.lv_e = b.lv_e;
        va.z = s.z;
        va.zb = zb;
        va.nrows = rows; va.count = V;
        for (int v = 0; v < V; ++v) va.kind[v] = vo.kind[v];
        va.factor = precision_factor(c); va.eps = c.epsilon;
        return dispatch_d(d512, [&](auto w) {
            return launch(tm, ST_FUSION, iefvad_fusion_variants_kernel<decltype(w)::value>, dim3((rows + ROW_WAVES - 1) / ROW_WAVES), dim3(256), 0, stream, va);
        });
    });
}

// 7'. the score samples of a pass (samples.h), behind its own results: groups of up to IEF_MAX_VARIANTS samples, each the sampled z0
// of the row set stacked in the group's workspace, steps 4 - 5 on it and the valid rows' logits to rows s0 .. of the call's
// [count, stride] result; behind the last group the per-snippet mean and standard deviation of the scores from those rows.
static unsigned long long sample_seed(unsigned long long seed, int s) { return seed + (unsigned long long)s * 0x9E3779B97F4A7C15ull; }
static int pass_samples(iefvad_handle* h, const PassBuffers& b, const RaggedPass* rg, const SampleOut& so, hipStream_t stream, Timer& tm) {
    const iefvad_config& c = h->cfg;
    const bool d512 = h->D == IEF_D512;
    const RowSet rs = row_set(b, rg);
    const RaggedChunk* const chunks = rs.chunks;
    const int valid_rows = rs.valid_rows, nslabs = rs.nslabs;
    for (int s0 = 0; s0 < so.count; s0 += IEF_MAX_VARIANTS) {
        const int G = so.count - s0 < IEF_MAX_VARIANTS ? so.count - s0 : IEF_MAX_VARIANTS;
        if (int rc = pass_stacked(h, b, rg, so.ws, G, so.logits + (long long)s0 * so.stride, so.stride, so.row0, stream, tm, [&](const PassBuffers& s, bf16_t* zb) {
                SampleArgs sa;
                memset(&sa, 0, sizeof(sa));
                sa.mu_i = b.mu_i; sa.lv_i = b.lv_i; sa.mu_e = b.mu_e; sa.lv_e = b.lv_e;
                sa.z = s.z;
                sa.zb = zb;
                sa.chunks = chunks; sa.ids = so.ids; sa.row0 = so.row0;
                sa.nrows = b.rows; sa.valid_rows = valid_rows;
                sa.used_rows = (chunks && b.enc_rows_mode) ? rg->enc_used_rows : b.rows;
                sa.chunk_rows = b.enc_rows_mode ? 0 : IEF_T;
                sa.count = G;
                for (int g = 0; g < G; ++g) sa.seed[g] = sample_seed(so.seed, s0 + g);
                sa.factor = precision_factor(c); sa.eps = c.epsilon; sa.scale = so.scale;
                const dim3 grid(chunks ? b.nb + 1 : (b.rows + 255) / 256, SAMPLE_SLICES);
                return dispatch_d(d512, [&](auto w) {
                    return launch(tm, ST_FUSION, iefvad_sample_states_kernel<decltype(w)::value>, grid, dim3(256), 0, stream, sa);
                });
            })) return rc;
    }
    return launch(tm, ST_SCORER, iefvad_samples_reduce_kernel, dim3(nslabs), dim3(256), 0, stream, (const float*)so.logits, so.stride, so.count, chunks,
                  valid_rows, so.row0, so.mean, so.stdev);
}

// One micro-batch of `nb` chunks; `x`: what the call asks for beyond its base outputs, at the pass's first row.  Dense (rg == nullptr):
// `in` holds the pass's [nb, 256, 768] blocks, results go to `out` at row offset row0.  Ragged: `in` holds the pass's packed rows, the
// chunks are built from them on the device, everything behind the encoder runs on the valid rows only, results go to rg->out (`out`
// must be all-null, `x` is rg->out.x).
static int forward_pass(iefvad_handle* h, const RowsIn& in, const Extras& x, int nb, size_t row0, void* workspace, const iefvad_outputs* out,
                        const RaggedPass* rg, hipStream_t stream, Timer& tm) {
    PassBuffers b = pass_buffers(h, nb, row0, workspace, out, rg);
    if (int rc = pass_load_inputs(h, b, in, x, rg, stream, tm)) return rc;
    for (int l = 0; l < h->cfg.num_layers; ++l)
        if (int rc = pass_encoder_layer(h, b, l, rg, x.attn, stream, tm)) return rc;
    if (int rc = pass_compact_rows(h, b, rg, stream, tm)) return rc;
    if (int rc = pass_tail(h, b, out, rg, x.traj.any() ? &x.traj : nullptr, x.keep_heads(), stream, tm)) return rc;
    if (rg)
        if (int rc = pass_rows_out(h, b, rg, stream, tm)) return rc;
    if (x.var.any())
        if (int rc = pass_variants(h, b, rg, x.var, stream, tm)) return rc;
    return x.smp.any() ? pass_samples(h, b, rg, x.smp, stream, tm) : 0;
}

// the layout behind the base workspace of a dense call of B chunks
static WorkspaceTail dense_tail(const iefvad_handle* h, int32_t B, const TailWants& w) {
    const int mb = micro_batch(h);
    return workspace_tail(iefvad_workspace_bytes(h, B), (size_t)(B < mb ? B : mb), h->D, w);
}
// the public workspace queries of the dense entries with an extra: 0 for arguments no call would accept
static size_t dense_workspace_bytes(const iefvad_handle* h, int32_t B, const TailWants& w) {
    return iefvad_workspace_bytes(h, B) ? dense_tail(h, B, w).total : 0;
}

static int forward_impl(iefvad_handle* h, const RowsIn& in, const Extras& x, int32_t B, void* workspace, size_t workspace_bytes,
                        const iefvad_outputs* out, hipStream_t stream, Timer& tm) {
    const void* const img = in.img;
    const void* const ev = in.ev;
    const int32_t in_dtype = in.in_dtype;
    if (!h || !img || !ev || !out) return fail("iefvad_forward: null argument");
    if (!h->weights_set) return fail("iefvad_forward: weights not set");
    if (B <= 0) return fail("iefvad_forward: B must be positive (got %d)", B);
    if (in_dtype != IEFVAD_IN_F32 && in_dtype != IEFVAD_IN_F16 && in_dtype != IEFVAD_IN_BF16)
        return fail("iefvad_forward: unknown in_dtype %d", in_dtype);
    const WorkspaceTail tail = dense_tail(h, B, x.wants());
    if (!workspace || workspace_bytes < tail.total)
        return fail("iefvad_forward: workspace too small (%zu < %zu bytes)", workspace_bytes, tail.total);
    if (((uintptr_t)workspace & 15) || ((uintptr_t)img & 15) || ((uintptr_t)ev & 15))
        return fail("iefvad_forward: buffers must be 16-byte aligned");
    Extras call = x;
    call.place(workspace, tail);
    const int mb = micro_batch(h);
    for (int b0 = 0; b0 < B; b0 += mb) {
        const int nb = (B - b0 < mb) ? (B - b0) : mb;
        const size_t row0 = (size_t)b0 * IEF_T;
        if (int rc = forward_pass(h, in.at(row0, h->D), call.at((long long)row0), nb, row0, workspace, out, nullptr, stream, tm)) return rc;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// whole videos: valid rows in, per-snippet results out (include/iefvad.h, csrc/ragged.h)
// ------------------------------------------------------------------------------------------------
static int attn_maps_args(const char* who, const iefvad_handle* h, const iefvad_attn_maps* maps, AttnMaps* am);   // the maps entries' checks, below
#include "videos.h"
#include "online.h"

// ------------------------------------------------------------------------------------------------
// small batches: replay a captured hipGraph of the forward
// ------------------------------------------------------------------------------------------------
// The reference calls the model once per video (test.py:76-117): B = 1 .. a few chunks, ~31 kernels of a few microseconds
// each.  Launched one by one they are host-bound (3-5 us of enqueue per launch).  For B <= cfg.graph_chunks the library
// captures forward_impl once per (B, in_dtype, output set, workspace) on a private stream, with every caller-owned
// pointer replaced by a library-owned staging buffer, and a call becomes: two device-to-device copies of the inputs,
// ONE hipGraphLaunch on the caller's stream, and one copy per requested output.  Same kernels, same order: same bits.
static const int kGraphDefaultChunks = 8, kGraphMaxChunks = 32, kGraphMaxEntries = 48;

struct GraphEntry {
    int B, in_dtype;
    unsigned outmask;
    void* workspace;
    size_t workspace_bytes;
    hipGraphExec_t exec;
    unsigned long long last_use;
    int steps;                   // the handle's step count at capture (iefvad_set_steps): a graph of K steps never replays for k
};

struct GraphCache {
    hipStream_t cap_stream = nullptr;
    char* in_buf = nullptr;      // img | ev staging, sized for max_chunks at 4 bytes per element
    float* small_buf = nullptr;  // logits | w_i_mean | w_e_mean, max_chunks * T floats each
    float* big_buf = nullptr;    // the seven [B*T, D] outputs (allocated on the first call that asks for one)
    int max_chunks = 0;
    unsigned long long clock = 0;
    bool disabled = false;       // capture or instantiation failed once: every later call launches directly
    std::vector<GraphEntry> entries;
};

static void release_graphs(iefvad_handle* h) {
    if (!h->graphs) return;
    for (auto& e : h->graphs->entries) (void)hipGraphExecDestroy(e.exec);
    if (h->graphs->cap_stream) (void)hipStreamDestroy(h->graphs->cap_stream);
    if (h->graphs->in_buf) (void)hipFree(h->graphs->in_buf);
    if (h->graphs->small_buf) (void)hipFree(h->graphs->small_buf);
    if (h->graphs->big_buf) (void)hipFree(h->graphs->big_buf);
    delete h->graphs;
    h->graphs = nullptr;
}

static int graph_limit(const iefvad_handle* h) {
    const int g = h->cfg.graph_chunks;
    if (g < 0) return 0;
    const int lim = g == 0 ? kGraphDefaultChunks : (g < kGraphMaxChunks ? g : kGraphMaxChunks);
    const int mb = micro_batch(h);
    return lim < mb ? lim : mb;          // a graphed call is a single micro-batch
}

static int forward_graphed(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B, void* workspace,
                           size_t workspace_bytes, const iefvad_outputs* out, hipStream_t stream) {
    static_assert(sizeof(iefvad_outputs) == 10 * sizeof(float*), "iefvad_outputs is ten pointers");
    const size_t D = h->D, T = IEF_T;
    if (!h->graphs) {
        h->graphs = new (std::nothrow) GraphCache();
        if (!h->graphs) return fail("iefvad_forward: out of host memory");
    }
    GraphCache& gc = *h->graphs;
    if (!gc.cap_stream) {
        HIP_TRY(hipSetDevice(h->device));
        gc.max_chunks = graph_limit(h);
        HIP_TRY(hipStreamCreateWithFlags(&gc.cap_stream, hipStreamNonBlocking));
        HIP_TRY(hipMalloc((void**)&gc.in_buf, 2 * (size_t)gc.max_chunks * T * D * 4));
        HIP_TRY(hipMalloc((void**)&gc.small_buf, 3 * (size_t)gc.max_chunks * T * sizeof(float)));
    }
    const size_t rows = (size_t)B * T, mrows = (size_t)gc.max_chunks * T;
    float* const* of = (float* const*)out;               // fused logits image_mu event_mu image_logvar event_logvar w_i w_e w_i_mean w_e_mean
    static const bool kBig[10] = {true, false, true, true, true, true, true, true, false, false};
    unsigned outmask = 0;
    bool any_big = false;
    for (int i = 0; i < 10; ++i)
        if (of[i]) { outmask |= 1u << i; any_big |= kBig[i]; }
    if (any_big && !gc.big_buf) HIP_TRY(hipMalloc((void**)&gc.big_buf, 7 * mrows * D * sizeof(float)));
    // staging addresses (fixed for the life of the handle, so every captured graph stays valid)
    char* s_img = gc.in_buf;
    char* s_ev = gc.in_buf + mrows * D * 4;
    float* s_out[10];
    {
        int big = 0, small = 0;
        for (int i = 0; i < 10; ++i)
            s_out[i] = kBig[i] ? gc.big_buf + (size_t)(big++) * mrows * D : gc.small_buf + (size_t)(small++) * mrows;
    }
    GraphEntry* hit = nullptr;
    for (auto& e : gc.entries)
        if (e.B == B && e.in_dtype == in_dtype && e.outmask == outmask && e.workspace == workspace && e.workspace_bytes == workspace_bytes && e.steps == h->steps) hit = &e;
    if (!hit) {
        iefvad_outputs so;
        float** sf = (float**)&so;
        for (int i = 0; i < 10; ++i) sf[i] = of[i] ? s_out[i] : nullptr;
        // The graph is an optimisation: if capture or instantiation is refused (a capture already active on this thread, an
        // exhausted graph pool ...), remember it and let the caller's direct path run instead.
        Timer tm;
        if (hipStreamBeginCapture(gc.cap_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
            (void)hipGetLastError();
            gc.disabled = true;
            return -1;
        }
        const int rc = forward_impl(h, RowsIn{s_img, s_ev, in_dtype}, Extras{}, B, workspace, workspace_bytes, &so, gc.cap_stream, tm);
        hipGraph_t graph = nullptr;
        const hipError_t ce = hipStreamEndCapture(gc.cap_stream, &graph);      // always end the capture, also after a failed launch
        if (rc) {
            if (graph) (void)hipGraphDestroy(graph);
            return rc;
        }
        hipGraphExec_t exec = nullptr;
        hipError_t ie = (ce == hipSuccess && graph) ? hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) : hipErrorUnknown;
        if (graph) (void)hipGraphDestroy(graph);
        if (ie != hipSuccess) {
            (void)hipGetLastError();
            gc.disabled = true;
            return -1;
        }
        if ((int)gc.entries.size() >= kGraphMaxEntries) {                      // evict the least recently used graph
            size_t lru = 0;
            for (size_t i = 1; i < gc.entries.size(); ++i)
                if (gc.entries[i].last_use < gc.entries[lru].last_use) lru = i;
            (void)hipGraphExecDestroy(gc.entries[lru].exec);
            gc.entries.erase(gc.entries.begin() + (long)lru);
        }
        gc.entries.push_back(GraphEntry{B, in_dtype, outmask, workspace, workspace_bytes, exec, 0, h->steps});
        hit = &gc.entries.back();
    }
    hit->last_use = ++gc.clock;
    const size_t in_bytes = rows * D * in_elem_bytes(in_dtype);
    HIP_TRY(hipMemcpyAsync(s_img, img, in_bytes, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(s_ev, ev, in_bytes, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipGraphLaunch(hit->exec, stream));
    for (int i = 0; i < 10; ++i)
        if (of[i]) HIP_TRY(hipMemcpyAsync(of[i], s_out[i], rows * (kBig[i] ? D : 1) * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return 0;
}

extern "C" int iefvad_forward(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B, void* workspace,
                              size_t workspace_bytes, const iefvad_outputs* out, void* stream) {
    if (h && out && img && ev && h->weights_set && B > 0 && B <= graph_limit(h) && workspace &&
        workspace_bytes >= iefvad_workspace_bytes(h, B) && !(((uintptr_t)workspace | (uintptr_t)img | (uintptr_t)ev) & 15) &&
        (in_dtype == IEFVAD_IN_F32 || in_dtype == IEFVAD_IN_F16 || in_dtype == IEFVAD_IN_BF16))
    {
        if (!(h->graphs && h->graphs->disabled)) {
            const int rc = forward_graphed(h, img, ev, in_dtype, B, workspace, workspace_bytes, out, (hipStream_t)stream);
            if (rc >= 0) return rc;            // -1: graphs unavailable, fall through to direct launches
        }
    }
    Timer tm;      // everything else, and every invalid argument (reported by forward_impl), takes the direct path
    return forward_impl(h, RowsIn{img, ev, in_dtype}, Extras{}, B, workspace, workspace_bytes, out, (hipStream_t)stream, tm);
}

// The checks of a maps request that need no device: something is asked for, only at layers the model has, 16-byte aligned, and
// not in the bf16 arithmetic (whose q | k | v are bf16 planes)
static int attn_maps_args(const char* who, const iefvad_handle* h, const iefvad_attn_maps* maps, AttnMaps* am) {
    if (!h) return fail("%s: null handle", who);
    if (!maps) return fail("%s: null maps", who);
    memset(am, 0, sizeof(*am));
    int top = -1;        // the last layer asked for; the pointers are looked at before the handle is
    for (int l = 0; l < IEFVAD_MAX_LAYERS; ++l) {
        float* const p[2] = {maps->image[l], maps->event[l]};
        for (int m = 0; m < 2; ++m) {
            if (!p[m]) continue;
            if ((uintptr_t)p[m] & 15) return fail("%s: the attention maps must be 16-byte aligned", who);
            am->p[m][l] = p[m];
            top = l;
        }
    }
    if (top < 0) return fail("%s: every map is null (nothing is asked for)", who);
    if (top >= h->cfg.num_layers) return fail("%s: a map is asked for at layer %d, the model has %d layers", who, top, h->cfg.num_layers);
    if (h->cfg.compute == IEFVAD_COMPUTE_BF16)
        return fail("%s: attention maps are not available with compute = BF16 (q | k | v are bf16 planes there); use F32, BF16X6 or FP16X3", who);
    return 0;
}

extern "C" int iefvad_forward_attn(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B, void* workspace,
                                   size_t workspace_bytes, const iefvad_outputs* out, const iefvad_attn_maps* maps, void* stream) {
    Extras x = {};
    if (int rc = attn_maps_args("iefvad_forward_attn", h, maps, &x.attn)) return rc;
    Timer tm;      // direct launches: the map pointers are per call, a cached graph would pin their addresses
    return forward_impl(h, RowsIn{img, ev, in_dtype}, x, B, workspace, workspace_bytes, out, (hipStream_t)stream, tm);
}

static int perturb_aligned(const char* who, const iefvad_perturb& p) {
    if (((uintptr_t)p.noise_amp[0] | (uintptr_t)p.noise_amp[1] | (uintptr_t)p.noise_row) & 3)
        return fail("%s: noise amplitude and noise row vectors must be 4-byte aligned", who);
    return 0;
}

extern "C" int iefvad_forward_perturbed(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B, const iefvad_perturb* p,
                                        void* workspace, size_t workspace_bytes, const iefvad_outputs* out, void* stream) {
    if (!h) return fail("iefvad_forward_perturbed: null argument");
    if (!p) return fail("iefvad_forward_perturbed: null perturbation");
    if (int rc = perturb_aligned("iefvad_forward_perturbed", *p)) return rc;
    const Extras x = perturb_extras(*p);
    if (!x.scale[0] && !x.scale[1] && !x.noise.any()) return iefvad_forward(h, img, ev, in_dtype, B, workspace, workspace_bytes, out, stream);
    Timer tm;      // direct launches: vectors and seed are per call, a cached graph would pin them
    return forward_impl(h, RowsIn{img, ev, in_dtype}, x, B, workspace, workspace_bytes, out, (hipStream_t)stream, tm);
}

extern "C" int iefvad_forward_scaled(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B, const float* img_row_scale,
                                     const float* ev_row_scale, void* workspace, size_t workspace_bytes, const iefvad_outputs* out, void* stream) {
    if (!h) return fail("iefvad_forward_scaled: null argument");
    iefvad_perturb p = {};
    p.scale[0] = img_row_scale; p.scale[1] = ev_row_scale;
    return iefvad_forward_perturbed(h, img, ev, in_dtype, B, &p, workspace, workspace_bytes, out, stream);
}

extern "C" int iefvad_perturb_rows(const void* img_rows, const void* ev_rows, int32_t in_dtype, int32_t D, int64_t rows, int32_t nan_to_num_all,
                                   const iefvad_perturb* p, void* out_img, void* out_ev, void* stream) {
    static const char* const who = "iefvad_perturb_rows";
    if (!p) return fail("%s: null perturbation", who);
    if (in_dtype != IEFVAD_IN_F32 && in_dtype != IEFVAD_IN_F16 && in_dtype != IEFVAD_IN_BF16) return fail("%s: unknown in_dtype %d", who, in_dtype);
    if (D != IEF_D && D != IEF_D512) return fail("%s: D must be %d or %d (got %d)", who, IEF_D, IEF_D512, D);
    if (rows <= 0 || rows > 0x7fffffffLL) return fail("%s: rows must be in 1 .. 2^31 - 1 (got %lld)", who, (long long)rows);
    if ((!img_rows && out_img) || (!ev_rows && out_ev)) return fail("%s: an output without its source rows", who);
    if (!out_img && !out_ev) return fail("%s: null outputs (nothing is asked for)", who);
    if (((uintptr_t)img_rows | (uintptr_t)ev_rows | (uintptr_t)out_img | (uintptr_t)out_ev) & 15) return fail("%s: buffers must be 16-byte aligned", who);
    if (((uintptr_t)p->scale[0] | (uintptr_t)p->scale[1]) & 3) return fail("%s: row scale vectors must be 4-byte aligned", who);
    if (int rc = perturb_aligned(who, *p)) return rc;
    const RowNoise nz = row_noise(*p);
    const float big = in_dtype == IEFVAD_IN_F32 ? 3.40282347e38f : in_dtype == IEFVAD_IN_F16 ? 65504.f : 3.38953139e38f;     // RaggedLimits (ragged.h)
    return dispatch_in(in_dtype, D == IEF_D512, [&](auto t, auto w) {
        return launch_perturb_rows<typename decltype(t)::type, decltype(w)::value>(out_img ? img_rows : nullptr, out_ev ? ev_rows : nullptr, out_img, out_ev,
                                                                                  (size_t)rows * D, p->scale[0], p->scale[1], nan_to_num_all != 0, nz,
                                                                                  big, (hipStream_t)stream);
    });
}

extern "C" int iefvad_forward_timed(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B,
                                    void* workspace, size_t workspace_bytes, const iefvad_outputs* out, void* stream_,
                                    iefvad_stage_times* times) {
    if (!times) return fail("iefvad_forward_timed: null times");
    hipStream_t stream = (hipStream_t)stream_;
    if (!h) return fail("iefvad_forward_timed: null handle");
    if (!h->events) h->events = new (std::nothrow) EventPool();
    if (!h->events) return fail("iefvad_forward_timed: out of host memory");
    EventPool& pool = *h->events;
    pool.used = 0;
    pool.err = hipSuccess;
    Timer tm;
    tm.on = true;
    tm.stream = stream;
    tm.pool = &pool;
    hipEvent_t t0 = pool.take(), t1 = pool.take();
    if (!t0 || !t1) return fail("iefvad_forward_timed: hipEventCreate: %s", hipGetErrorString(pool.err));
    HIP_TRY(hipEventRecord(t0, stream));
    int rc = forward_impl(h, RowsIn{img, ev, in_dtype}, Extras{}, B, workspace, workspace_bytes, out, stream, tm);
    (void)hipEventRecord(t1, stream);
    hipError_t se = hipStreamSynchronize(stream);
    if (rc) return rc;
    if (pool.err != hipSuccess) return fail("iefvad_forward_timed: hipEventCreate: %s", hipGetErrorString(pool.err));
    if (se != hipSuccess) return fail("iefvad_forward_timed: %s", hipGetErrorString(se));
    float acc[ST_COUNT] = {0};
    for (auto& s : tm.spans) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s.a, s.b));
        acc[s.stage] += ms;
    }
    float total = 0.f;
    HIP_TRY(hipEventElapsedTime(&total, t0, t1));
    memset(times, 0, sizeof(*times));
    times->total_ms = total;
    times->qkv_gemm_ms = acc[ST_QKV];
    times->attention_ms = acc[ST_ATT];
    times->out_gemm_ms = acc[ST_OUT];
    times->layernorm_ms = acc[ST_LN];
    times->head_gemm_ms = acc[ST_HEAD];
    times->fusion_ms = acc[ST_FUSION];
    times->refine_gemm_ms = acc[ST_REFINE];
    times->scorer_ms = acc[ST_SCORER];
    times->cast_ms = acc[ST_CAST];
    times->gemm_launches = tm.gemm_launches;
    return 0;
}


// ------------------------------------------------------------------------------------------------
// training: train-mode forward and the model's backward pass
// ------------------------------------------------------------------------------------------------
#include "train.h"

// ------------------------------------------------------------------------------------------------
// multi-GPU score gather (include/iefvad.h; csrc/gather.h binds librccl at run time)
// ------------------------------------------------------------------------------------------------
#define RCCL_TRY(api, expr)                                                                                   \
    do {                                                                                                      \
        ncclResult_t r_ = (expr);                                                                             \
        if (r_ != ncclSuccess) return fail("%s failed: %s (%s:%d)", #expr, (api)->GetErrorString(r_), __FILE__, __LINE__); \
    } while (0)

extern "C" int iefvad_comm_unique_id(void* id_bytes) {
    if (!id_bytes) return fail("iefvad_comm_unique_id: null argument");
    static_assert(sizeof(ncclUniqueId) == IEFVAD_COMM_ID_BYTES, "ncclUniqueId size");
    const char* why = "";
    const RcclApi* api = rccl_api(&why);
    if (!api) return fail("iefvad_comm_unique_id: %s", why);
    ncclUniqueId id;
    RCCL_TRY(api, api->GetUniqueId(&id));
    memcpy(id_bytes, &id, sizeof(id));
    return 0;
}

extern "C" int iefvad_comm_create(const void* id_bytes, int32_t nranks, int32_t rank, iefvad_comm** out) {
    if (!id_bytes || !out) return fail("iefvad_comm_create: null argument");
    *out = nullptr;
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail("iefvad_comm_create: rank %d of %d", rank, nranks);
    const char* why = "";
    const RcclApi* api = rccl_api(&why);
    if (!api) return fail("iefvad_comm_create: %s", why);
    iefvad_comm* c = new (std::nothrow) iefvad_comm();
    if (!c) return fail("iefvad_comm_create: out of host memory");
    memset(c, 0, sizeof(*c));
    c->rank = rank;
    hipError_t e = hipGetDevice(&c->device);
    if (e != hipSuccess) {
        delete c;
        return fail("iefvad_comm_create: %s", hipGetErrorString(e));
    }
    ncclUniqueId id;
    memcpy(&id, id_bytes, sizeof(id));
    ncclResult_t r = api->CommInitRank(&c->comm, nranks, id, rank);
    if (r == ncclSuccess) r = api->CommCount(c->comm, &c->nranks);
    if (r != ncclSuccess) {
        if (c->comm) (void)api->CommDestroy(c->comm);
        delete c;
        return fail("iefvad_comm_create: %s", api->GetErrorString(r));
    }
    if (c->nranks != nranks) {
        const int got = c->nranks;
        (void)api->CommDestroy(c->comm);
        delete c;
        return fail("iefvad_comm_create: RCCL reports %d ranks, caller said %d", got, nranks);
    }
    *out = c;
    return 0;
}

extern "C" int32_t iefvad_comm_nranks(const iefvad_comm* c) { return c ? c->nranks : 0; }

extern "C" void iefvad_comm_destroy(iefvad_comm* c) {
    if (!c) return;
    const RcclApi* api = rccl_api(nullptr);
    if (api && c->comm) (void)api->CommDestroy(c->comm);
    delete c;
}

extern "C" int32_t iefvad_rccl_version(void) {
    const RcclApi* api = rccl_api(nullptr);
    int v = 0;
    if (!api || api->GetVersion(&v) != ncclSuccess) return 0;
    return v;
}

extern "C" int iefvad_gather_plan(int32_t nranks, int32_t rank, const int64_t* counts, int64_t count, int64_t* summary,
                                  int64_t* steps) {
    if (!summary) return fail("iefvad_gather_plan: null summary");
    if (!counts && count < 0) return fail("iefvad_gather_plan: count = %lld", (long long)count);
    GatherPlan plan;
    if (const char* why = gather_plan(nranks, rank, counts, (size_t)count, &plan)) return fail("iefvad_gather_plan: %s", why);
    summary[0] = plan.equal ? 1 : 0;
    summary[1] = (int64_t)plan.my_offset;
    summary[2] = (int64_t)plan.my_count;
    summary[3] = (int64_t)plan.total;
    summary[4] = (int64_t)plan.steps.size();
    if (steps)
        for (size_t i = 0; i < plan.steps.size(); ++i) {
            steps[4 * i + 0] = plan.steps[i].peer;
            steps[4 * i + 1] = (int64_t)plan.steps[i].send_count;
            steps[4 * i + 2] = (int64_t)plan.steps[i].recv_offset;
            steps[4 * i + 3] = (int64_t)plan.steps[i].recv_count;
        }
    return 0;
}

extern "C" int iefvad_gather_scores(iefvad_comm* c, const float* local, size_t count, const int64_t* counts, float* gathered,
                                    size_t gathered_capacity, void* stream_) {
    if (!c || !gathered) return fail("iefvad_gather_scores: null argument");
    const RcclApi* api = rccl_api(nullptr);
    if (!api) return fail("iefvad_gather_scores: librccl not bound");
    hipStream_t stream = (hipStream_t)stream_;
    GatherPlan plan;
    if (const char* why = gather_plan(c->nranks, c->rank, counts, count, &plan)) return fail("iefvad_gather_scores: %s", why);
    if (plan.total > gathered_capacity)
        return fail("iefvad_gather_scores: the ranks contribute %zu elements, `gathered` holds %zu", plan.total, gathered_capacity);
    if (plan.my_count > 0 && !local) return fail("iefvad_gather_scores: null local buffer");
    // `local` may BE its own slot of `gathered` (in place, as ncclAllGather allows); any other overlap would be overwritten
    // by a peer's slice while it is still being sent
    if (plan.my_count > 0 && local != gathered + plan.my_offset && local < gathered + plan.total && gathered < local + plan.my_count)
        return fail("iefvad_gather_scores: `local` overlaps `gathered` outside its own slot");
    if (plan.total == 0) return 0;
    if (plan.equal) {   // the common case (bench, balanced shards): ONE collective
        RCCL_TRY(api, api->AllGather(local, gathered, plan.my_count, ncclFloat32, c->comm, stream));
        return 0;
    }
    // unequal shards: one grouped point-to-point exchange -- rank r's slice lands at its running offset on every peer
    RCCL_TRY(api, api->GroupStart());
    ncclResult_t first_bad = ncclSuccess;
    for (const GatherStep& s : plan.steps) {
        ncclResult_t a = s.send_count ? api->Send(local, s.send_count, ncclFloat32, s.peer, c->comm, stream) : ncclSuccess;
        ncclResult_t b = s.recv_count ? api->Recv(gathered + s.recv_offset, s.recv_count, ncclFloat32, s.peer, c->comm, stream) : ncclSuccess;
        if (first_bad == ncclSuccess) first_bad = (a != ncclSuccess) ? a : b;
    }
    ncclResult_t ge = api->GroupEnd();      // always close the group, even after a failed enqueue
    if (first_bad != ncclSuccess) return fail("iefvad_gather_scores: %s", api->GetErrorString(first_bad));
    if (ge != ncclSuccess) return fail("iefvad_gather_scores: ncclGroupEnd: %s", api->GetErrorString(ge));
    if (plan.my_count && gathered + plan.my_offset != local)
        HIP_TRY(hipMemcpyAsync(gathered + plan.my_offset, local, plan.my_count * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// training-side loss head: forward and the gradients with respect to the model's outputs (csrc/loss.h)
// ------------------------------------------------------------------------------------------------
extern "C" size_t iefvad_loss_workspace_bytes(int32_t B, int32_t T) {
    if (B <= 0 || T <= 0) return 0;
    return ((size_t)B * T * 4 + (size_t)B) * sizeof(float) + 256;
}

extern "C" int iefvad_loss_forward(const float* logits, const float* image_mu, const float* event_mu, const float* image_logvar,
                                   const float* event_logvar, const int32_t* lengths, const float* targets, int32_t B, int32_t T,
                                   int32_t noise_model, float nu, float lambda_reg, float lambda_kl, float* out, void* workspace,
                                   size_t workspace_bytes, void* stream_) {
    if (!logits || !lengths || !targets || !out || !workspace) return fail("iefvad_loss_forward: null argument");
    const bool heads = image_mu || event_mu || image_logvar || event_logvar;      // all four or none (none: CLAS2 alone)
    if (heads && !(image_mu && event_mu && image_logvar && event_logvar))
        return fail("iefvad_loss_forward: image_mu, event_mu, image_logvar, event_logvar must be given together");
    if (B <= 0) return fail("iefvad_loss_forward: B must be positive (got %d)", B);
    if (T != IEF_T) return fail("iefvad_loss_forward: kernels are built for T = %d (got %d)", IEF_T, T);
    if (noise_model != IEFVAD_NOISE_GAUSSIAN && noise_model != IEFVAD_NOISE_STUDENT_T)
        return fail("Unsupported noise_model. Choose 'Gaussian' or 'StudentT'.");
    if (noise_model == IEFVAD_NOISE_STUDENT_T && !(nu > 0.f)) return fail("iefvad_loss_forward: nu must be positive for StudentT");
    if (workspace_bytes < iefvad_loss_workspace_bytes(B, T)) return fail("iefvad_loss_forward: workspace too small");
    if ((uintptr_t)workspace & 15) return fail("iefvad_loss_forward: the workspace must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const int rows = heads ? B * T : 0;
    float* part = (float*)workspace;
    float* inst = part + (size_t)B * T * 4;
    hipLaunchKernelGGL(iefvad_mil_topk_kernel, dim3(B), dim3(256), 0, stream, logits, (const int*)lengths, inst, T);
    LossRowArgs ra;
    ra.mu_i = image_mu; ra.mu_e = event_mu; ra.lv_i = image_logvar; ra.lv_e = event_logvar; ra.part = part; ra.rows = rows;
    ra.lv_shift = noise_model == IEFVAD_NOISE_STUDENT_T ? logf(nu / (nu + 1.0f)) : 0.f;       // ucf_train.py:94-95
    if (heads) hipLaunchKernelGGL(iefvad_loss_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, ra);
    LossFinishArgs fa;
    fa.inst = inst; fa.targets = targets; fa.part = part; fa.out = out; fa.B = B; fa.rows = rows; fa.lambda_reg = lambda_reg;
    fa.lambda_kl = lambda_kl;
    hipLaunchKernelGGL(iefvad_loss_finish_kernel, dim3(1), dim3(256), 0, stream, fa);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int iefvad_loss_backward(const float* logits, const float* image_mu, const float* event_mu, const float* image_logvar,
                                    const float* event_logvar, const int32_t* lengths, const float* targets, int32_t B, int32_t T,
                                    int32_t noise_model, float nu, float lambda_reg, float lambda_kl, float grad_scale,
                                    float* d_logits, float* d_image_mu, float* d_event_mu, float* d_image_logvar,
                                    float* d_event_logvar, const float* grad_scale_dev, void* stream_) {
    if (!logits || !lengths || !targets) return fail("iefvad_loss_backward: null argument");
    const bool heads = d_image_mu || d_event_mu || d_image_logvar || d_event_logvar;
    if (heads && !(image_mu && event_mu && image_logvar && event_logvar))
        return fail("iefvad_loss_backward: image_mu, event_mu, image_logvar, event_logvar are needed for their gradients");
    if (B <= 0) return fail("iefvad_loss_backward: B must be positive (got %d)", B);
    if (T != IEF_T) return fail("iefvad_loss_backward: kernels are built for T = %d (got %d)", IEF_T, T);
    if (noise_model != IEFVAD_NOISE_GAUSSIAN && noise_model != IEFVAD_NOISE_STUDENT_T)
        return fail("Unsupported noise_model. Choose 'Gaussian' or 'StudentT'.");
    if (noise_model == IEFVAD_NOISE_STUDENT_T && !(nu > 0.f)) return fail("iefvad_loss_backward: nu must be positive for StudentT");
    hipStream_t stream = (hipStream_t)stream_;
    if (d_logits)
        hipLaunchKernelGGL(iefvad_mil_topk_grad_kernel, dim3(B), dim3(256), 0, stream, logits, (const int*)lengths, targets, d_logits, T,
                           grad_scale / (float)B, grad_scale_dev);
    if (heads) {
        LossRowGradArgs ga;
        ga.mu_i = image_mu; ga.mu_e = event_mu; ga.lv_i = image_logvar; ga.lv_e = event_logvar;
        ga.d_mu_i = d_image_mu; ga.d_mu_e = d_event_mu; ga.d_lv_i = d_image_logvar; ga.d_lv_e = d_event_logvar;
        ga.rows = B * T;
        ga.lv_shift = noise_model == IEFVAD_NOISE_STUDENT_T ? logf(nu / (nu + 1.0f)) : 0.f;
        ga.lambda_reg = lambda_reg; ga.lambda_kl = lambda_kl; ga.scale = grad_scale; ga.scale_dev = grad_scale_dev;
        hipLaunchKernelGGL(iefvad_loss_rows_grad_kernel, dim3((ga.rows + 3) / 4), dim3(256), 0, stream, ga);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int iefvad_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                                 double beta2, double eps, double weight_decay, int32_t step, void* stream_) {
    if (!param || !grad || !exp_avg || !exp_avg_sq) return fail("iefvad_adamw_step: null argument");
    if (step < 1) return fail("iefvad_adamw_step: step counts from 1 (got %d)", step);
    if (n == 0) return 0;
    AdamWArgs a;
    a.p = param; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq; a.n = n;
    // torch forms these in Python floats (doubles) and rounds once when they meet the fp32 tensors
    a.decay = (float)(1.0 - lr * weight_decay);
    a.w1 = (float)(1.0 - beta1);
    a.beta2 = (float)beta2;
    a.w2 = (float)(1.0 - beta2);
    a.step_size = (float)(lr / (1.0 - pow(beta1, (double)step)));
    a.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)step));
    a.eps = (float)eps;
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(iefvad_adamw_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, (hipStream_t)stream_, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int iefvad_adamw_step_multi(const iefvad_adamw_tensor* table_dev, int32_t count, uint64_t total_chunks, double lr, double beta1, double beta2,
                                       double eps, double weight_decay, int32_t step, void* stream_) {
    if (!table_dev) return fail("iefvad_adamw_step_multi: null argument");
    if (step < 1) return fail("iefvad_adamw_step_multi: step counts from 1 (got %d)", step);
    if (count <= 0 || total_chunks == 0) return 0;
    if (total_chunks > 0x7fffffffull) return fail("iefvad_adamw_step_multi: too many chunks");
    AdamWMultiArgs a;
    a.table = table_dev; a.count = count;
    a.decay = (float)(1.0 - lr * weight_decay);       // the scalars of iefvad_adamw_step, formed the same way
    a.w1 = (float)(1.0 - beta1);
    a.beta2 = (float)beta2;
    a.w2 = (float)(1.0 - beta2);
    a.step_size = (float)(lr / (1.0 - pow(beta1, (double)step)));
    a.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)step));
    a.eps = (float)eps;
    hipLaunchKernelGGL(iefvad_adamw_multi_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream_, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// metric tail of the evaluation loop (metrics.h)
// ------------------------------------------------------------------------------------------------
static size_t mt_align(size_t x) { return (x + 255) & ~(size_t)255; }
// ngroups = 0: the layout of iefvad_auc_ap; ngroups >= 1: iefvad_auc_ap_grouped's (one AP partial per (group, tile), 64 numerators and the
// NaN mask in the tail, the group table)
static size_t metric_layout(int64_t n, int ngroups, char* base, MetricWs* w) {
    const size_t tiles = (size_t)((n + MT_TILE - 1) / MT_TILE);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += mt_align(bytes); return p; };
    char* a = take((size_t)n * 8);
    char* b = take((size_t)n * 8);
    char* hist = take(tiles * MT_RADIX * 4);
    char* bsum = take(tiles * 4);
    char* bstart = take(tiles * 4);
    char* ap_part = take(tiles * 8 * (size_t)(ngroups > 0 ? ngroups : 1));
    const size_t tail_bytes = ngroups > 0 ? 8 * (size_t)(MT_MAXG + 1) : 16;
    char* tail = take(tail_bytes);
    char* dtotal = take(MT_RADIX * 4);
    char* tab = ngroups > 0 ? take(sizeof(MetricGroupTab)) : nullptr;
    if (w) {
        w->dtotal = (unsigned*)dtotal;
        w->a = (unsigned long long*)a; w->b = (unsigned long long*)b; w->hist = (unsigned*)hist; w->bsum = (unsigned*)bsum;
        w->bstart = (unsigned*)bstart; w->ap_part = (double*)ap_part; w->auc_num = (unsigned long long*)tail;
        w->flags = (unsigned*)(tail + tail_bytes - 8);
        w->tab = (MetricGroupTab*)tab;
    }
    return off;
}

// the LSD sort of the pairs in w.a: four 8-bit digits of the key (the upper word of a pair), then, in the grouped format, the group byte.
// Returns the buffer the sorted pairs end up in (w.a after four passes, w.b after five); the other one is free afterwards.
static const unsigned long long* metric_sort(const MetricWs& w, int64_t n, int tiles, bool grouped, hipStream_t stream) {
    unsigned long long* src = w.a;
    unsigned long long* dst = w.b;
    for (int pass = 0; pass < (grouped ? 5 : 4); ++pass) {
        const int shift = pass < 4 ? 32 + 8 * pass : MT_POS_BITS;
        hipLaunchKernelGGL(iefvad_metric_hist_kernel, dim3(tiles), dim3(MT_THREADS), 0, stream, src, (long long)n, shift, w.hist, tiles);
        hipLaunchKernelGGL(iefvad_metric_digit_scan_kernel, dim3(MT_RADIX), dim3(256), 0, stream, w.hist, tiles, w.dtotal);
        hipLaunchKernelGGL(iefvad_metric_scatter_kernel, dim3(tiles), dim3(MT_THREADS), 0, stream, src, dst, (long long)n, shift, w.hist, tiles, w.dtotal);
        unsigned long long* t = src; src = dst; dst = t;
    }
    return src;
}

extern "C" size_t iefvad_auc_ap_workspace_bytes(int64_t n) {
    if (n <= 0) return 0;
    return metric_layout(n, 0, nullptr, nullptr);
}

extern "C" int iefvad_auc_ap(const float* scores, const uint8_t* gt_frames, int64_t n, int32_t repeat, double* auc, double* ap,
                             void* workspace, size_t workspace_bytes, void* stream_) {
    if (!scores || !gt_frames || !workspace || (!auc && !ap)) return fail("iefvad_auc_ap: null argument");
    if (n <= 0 || repeat <= 0) return fail("iefvad_auc_ap: n = %lld, repeat = %d", (long long)n, repeat);
    if ((unsigned long long)n * (unsigned long long)repeat >= (1ull << 32))
        return fail("iefvad_auc_ap: n * repeat = %llu frames do not fit the 32-bit frame counters", (unsigned long long)n * (unsigned long long)repeat);
    if (((uintptr_t)workspace & 255) != 0) return fail("iefvad_auc_ap: the workspace must be 256-byte aligned");
    MetricWs w;
    const size_t need = metric_layout(n, 0, (char*)workspace, &w);
    if (workspace_bytes < need) return fail("iefvad_auc_ap: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t stream = (hipStream_t)stream_;
    const int tiles = (int)((n + MT_TILE - 1) / MT_TILE);
    HIP_TRY(hipMemsetAsync(w.auc_num, 0, 16, stream));
    hipLaunchKernelGGL(iefvad_metric_pairs_kernel, dim3((unsigned)((n + MT_THREADS - 1) / MT_THREADS)), dim3(MT_THREADS), 0, stream, scores,
                       (const unsigned char*)gt_frames, (long long)n, (int)repeat, w.a, w.flags);
    const unsigned long long* src = metric_sort(w, n, tiles, false, stream);          // back in w.a: w.b is free for the two scanned columns
    unsigned* tp_incl = (unsigned*)w.b;
    unsigned* gstart = tp_incl + n;
    hipLaunchKernelGGL(iefvad_metric_tile_sums_kernel<false>, dim3(tiles), dim3(MT_THREADS), 0, stream, src, (long long)n, w.bsum, w.bstart);
    hipLaunchKernelGGL(iefvad_metric_tile_scan_kernel, dim3(1), dim3(1024), 0, stream, w.bsum, w.bstart, tiles);
    hipLaunchKernelGGL(iefvad_metric_tile_apply_kernel<false>, dim3(tiles), dim3(MT_THREADS), 0, stream, src, (long long)n, w.bsum, w.bstart, tp_incl, gstart);
    hipLaunchKernelGGL(iefvad_metric_groups_kernel, dim3(tiles), dim3(MT_THREADS), 0, stream, src, (long long)n, (int)repeat, tp_incl, gstart, w.auc_num,
                       w.ap_part);
    hipLaunchKernelGGL(iefvad_metric_finish_kernel, dim3(1), dim3(256), 0, stream, tp_incl, (long long)n, (int)repeat, w.auc_num, w.ap_part, tiles, w.flags,
                       auc, ap);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" size_t iefvad_auc_ap_grouped_workspace_bytes(int64_t n, int32_t ngroups) {
    if (n <= 0 || ngroups < 1 || ngroups > MT_MAXG) return 0;
    return metric_layout(n, ngroups, nullptr, nullptr);
}

extern "C" int iefvad_auc_ap_grouped(const float* scores, const uint8_t* gt_frames, const uint8_t* group, int64_t n, int32_t repeat, int32_t ngroups,
                                     double* auc, double* ap, int64_t* frames, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!scores) return fail("iefvad_auc_ap_grouped: scores is null");
    if (!gt_frames) return fail("iefvad_auc_ap_grouped: gt_frames is null");
    if (!group) return fail("iefvad_auc_ap_grouped: group is null");
    if (!auc && !ap) return fail("iefvad_auc_ap_grouped: auc and ap are both null");
    if (!workspace) return fail("iefvad_auc_ap_grouped: workspace is null");
    if (ngroups < 1 || ngroups > MT_MAXG) return fail("iefvad_auc_ap_grouped: ngroups = %d, 1 .. %d groups per call", ngroups, MT_MAXG);
    if (n <= 0) return fail("iefvad_auc_ap_grouped: n = %lld", (long long)n);
    if (repeat <= 0 || repeat > (int32_t)MT_POS_MASK)       // a snippet's positives share the payload word with the group byte
        return fail("iefvad_auc_ap_grouped: repeat = %d, 1 .. %u frames per snippet", repeat, MT_POS_MASK);
    if ((unsigned long long)n * (unsigned long long)repeat >= (1ull << 32))
        return fail("iefvad_auc_ap_grouped: n * repeat = %llu frames do not fit the 32-bit frame counters", (unsigned long long)n * (unsigned long long)repeat);
    if (((uintptr_t)workspace & 255) != 0) return fail("iefvad_auc_ap_grouped: the workspace must be 256-byte aligned");
    MetricWs w;
    const size_t need = metric_layout(n, ngroups, (char*)workspace, &w);
    if (workspace_bytes < need) return fail("iefvad_auc_ap_grouped: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t stream = (hipStream_t)stream_;
    const int tiles = (int)((n + MT_TILE - 1) / MT_TILE);
    unsigned long long* nanmask = (unsigned long long*)w.flags;
    HIP_TRY(hipMemsetAsync(w.auc_num, 0, 8 * (MT_MAXG + 1), stream));          // the numerators and, behind them, the NaN mask
    hipLaunchKernelGGL(iefvad_metric_pairs_grouped_kernel, dim3((unsigned)((n + MT_THREADS - 1) / MT_THREADS)), dim3(MT_THREADS), 0, stream, scores,
                       (const unsigned char*)gt_frames, (const unsigned char*)group, (long long)n, (int)repeat, (int)ngroups, w.a, nanmask);
    // ordered by (group, key); w.dtotal keeps the last digit's totals = the pairs per group.  The other buffer takes the scanned columns
    const unsigned long long* src = metric_sort(w, n, tiles, true, stream);
    unsigned* tp_incl = (unsigned*)(src == w.a ? w.b : w.a);
    unsigned* gstart = tp_incl + n;
    hipLaunchKernelGGL(iefvad_metric_tile_sums_kernel<true>, dim3(tiles), dim3(MT_THREADS), 0, stream, src, (long long)n, w.bsum, w.bstart);
    hipLaunchKernelGGL(iefvad_metric_tile_scan_kernel, dim3(1), dim3(1024), 0, stream, w.bsum, w.bstart, tiles);
    hipLaunchKernelGGL(iefvad_metric_tile_apply_kernel<true>, dim3(tiles), dim3(MT_THREADS), 0, stream, src, (long long)n, w.bsum, w.bstart, tp_incl, gstart);
    hipLaunchKernelGGL(iefvad_metric_group_table_kernel, dim3(1), dim3(128), 0, stream, w.dtotal, tp_incl, (int)ngroups, w.tab);
    hipLaunchKernelGGL(iefvad_metric_groups_grouped_kernel, dim3(tiles), dim3(MT_THREADS), 0, stream, src, (long long)n, (int)repeat, (int)ngroups, tp_incl,
                       gstart, w.tab, w.auc_num, w.ap_part, tiles);
    hipLaunchKernelGGL(iefvad_metric_finish_grouped_kernel, dim3(ngroups), dim3(256), 0, stream, w.tab, (int)repeat, w.auc_num, w.ap_part, tiles, nanmask,
                       auc, ap, (long long*)frames);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// training input pipeline: ragged rows -> 256-segment windows, and a step's batch out of the cached windows (resample.h)
// ------------------------------------------------------------------------------------------------
extern "C" size_t iefvad_resample_workspace_bytes(int32_t nvideos) {
    if (nvideos <= 0) return 0;
    return ((size_t)nvideos * sizeof(ResampleVideo) + 255) & ~(size_t)255;
}

extern "C" int iefvad_resample_videos(const void* rows, int32_t in_dtype, const int32_t* lengths, int32_t nvideos, int32_t T, int32_t D,
                                      void* workspace, size_t workspace_bytes, float* out, int32_t* out_lengths, void* stream_) {
    if (!rows || !lengths || !workspace || !out || !out_lengths) return fail("iefvad_resample_videos: null argument");
    if (nvideos <= 0) return fail("iefvad_resample_videos: nvideos must be positive (got %d)", nvideos);
    if (T != IEF_T) return fail("iefvad_resample_videos: T = %d, the window is %d segments", T, IEF_T);
    if (D <= 0 || D % 8) return fail("iefvad_resample_videos: D = %d must be a positive multiple of 8", D);
    if (in_dtype != IEFVAD_IN_F32 && in_dtype != IEFVAD_IN_F16)
        return fail("iefvad_resample_videos: in_dtype %d (fp32 and fp16 feature files only)", in_dtype);
    const size_t need = iefvad_resample_workspace_bytes(nvideos);
    if (workspace_bytes < need) return fail("iefvad_resample_videos: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    if (((uintptr_t)rows & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)out & 15) || ((uintptr_t)out_lengths & 3))
        return fail("iefvad_resample_videos: rows, workspace and out must be 16-byte aligned, out_lengths 4-byte");
    const int groups = D / (in_dtype == IEFVAD_IN_F32 ? 4 : 8);
    if ((long long)nvideos * groups > 0xffffffffLL / 256)       // grid.x * block.x of one launch stays below 2^32
        return fail("iefvad_resample_videos: %d videos of D = %d exceed one launch (%lld at this width)", nvideos, D, 0xffffffffLL / 256 / groups);
    std::vector<ResampleVideo> table;
    try {
        table.resize((size_t)nvideos);
    } catch (const std::exception&) {
        return fail("iefvad_resample_videos: out of host memory");
    }
    long long row = 0;
    for (int v = 0; v < nvideos; ++v) {
        if (lengths[v] < 1) return fail("iefvad_resample_videos: lengths[%d] = %d (every video has at least one row)", v, lengths[v]);
        table[v].src_row = row;
        table[v].n = lengths[v];
        table[v].out = v;
        row += lengths[v];
    }
    // longest video first (resample.h); ties in list order, so the table is a function of the lengths alone
    std::stable_sort(table.begin(), table.end(), [](const ResampleVideo& a, const ResampleVideo& b) { return a.n > b.n; });
    hipStream_t stream = (hipStream_t)stream_;
    // the table is host memory of this call: the copy is ordered on `stream` behind whatever still reads the workspace, and waited for
    HIP_TRY(hipMemcpyAsync(workspace, table.data(), (size_t)nvideos * sizeof(ResampleVideo), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const dim3 grid((unsigned)((long long)nvideos * groups));
    if (in_dtype == IEFVAD_IN_F32)
        hipLaunchKernelGGL(iefvad_resample_rows_kernel<float>, grid, dim3(256), 0, stream, (const float*)rows, (const ResampleVideo*)workspace, (int)D, out,
                           (int*)out_lengths);
    else
        hipLaunchKernelGGL(iefvad_resample_rows_kernel<__half>, grid, dim3(256), 0, stream, (const __half*)rows, (const ResampleVideo*)workspace, (int)D, out,
                           (int*)out_lengths);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int iefvad_gather_windows(const float* img_set, const float* ev_set, const int32_t* set_lengths, int32_t nset, const int32_t* index,
                                     int32_t B, int32_t T, int32_t D, float* img_out, float* ev_out, int32_t* len_out, void* stream_) {
    if (!img_set || !ev_set || !set_lengths || !index || !img_out || !ev_out || !len_out) return fail("iefvad_gather_windows: null argument");
    if (nset <= 0 || B <= 0) return fail("iefvad_gather_windows: nset = %d, B = %d must be positive", nset, B);
    if (B > 65535) return fail("iefvad_gather_windows: B = %d exceeds one launch (65535 windows)", B);
    if (T != IEF_T) return fail("iefvad_gather_windows: T = %d, the window is %d segments", T, IEF_T);
    if (D <= 0 || D % 8) return fail("iefvad_gather_windows: D = %d must be a positive multiple of 8", D);
    if (((uintptr_t)img_set & 15) || ((uintptr_t)ev_set & 15) || ((uintptr_t)img_out & 15) || ((uintptr_t)ev_out & 15) ||
        ((uintptr_t)set_lengths & 3) || ((uintptr_t)index & 3) || ((uintptr_t)len_out & 3))
        return fail("iefvad_gather_windows: the window tensors must be 16-byte aligned, the int32 vectors 4-byte");
    const int nvec = IEF_T * D / 4, per_wg = 256 * IEF_GW_VEC;
    hipLaunchKernelGGL(iefvad_gather_windows_kernel, dim3((nvec + per_wg - 1) / per_wg, B, 2), dim3(256), 0, (hipStream_t)stream_, img_set, ev_set,
                       (const int*)set_lengths, (int)nset, (const int*)index, (int)D, img_out, ev_out, (int*)len_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// the similarity series of the vis=True plots (similarity.h)
// ------------------------------------------------------------------------------------------------
extern "C" int iefvad_similarity_rows(const float* fused, const float* image_mu, const float* event_mu, int64_t rows, int32_t D,
                                      const int32_t* src_rows, int64_t nout, float* out, void* stream_) {
    if (!fused || !image_mu || !event_mu) return fail("iefvad_similarity_rows: null tensor (fused, image_mu, event_mu)");
    if (!out) return fail("iefvad_similarity_rows: null out");
    if (rows <= 0) return fail("iefvad_similarity_rows: rows = %lld must be positive", (long long)rows);
    if (nout < 0) return fail("iefvad_similarity_rows: nout = %lld is negative", (long long)nout);
    if (D != 768 && D != 512) return fail("iefvad_similarity_rows: D = %d (768 and 512 are built)", D);
    if (!src_rows && nout > rows) return fail("iefvad_similarity_rows: nout = %lld exceeds rows = %lld without src_rows", (long long)nout, (long long)rows);
    if (nout > 0x7fffffffLL) return fail("iefvad_similarity_rows: nout = %lld exceeds one launch (2^31 - 1 rows)", (long long)nout);
    if (((uintptr_t)fused & 15) || ((uintptr_t)image_mu & 15) || ((uintptr_t)event_mu & 15) || ((uintptr_t)out & 15) || ((uintptr_t)src_rows & 3))
        return fail("iefvad_similarity_rows: misaligned pointer (the tensors and out 16-byte, src_rows 4-byte)");
    if (nout == 0) return 0;
    const dim3 grid((unsigned)((nout + ROW_WAVES - 1) / ROW_WAVES));
    if (D == 768)
        hipLaunchKernelGGL(iefvad_similarity_rows_kernel<768>, grid, dim3(256), 0, (hipStream_t)stream_, fused, image_mu, event_mu, (long long)rows,
                           (const int*)src_rows, (long long)nout, out);
    else
        hipLaunchKernelGGL(iefvad_similarity_rows_kernel<512>, grid, dim3(256), 0, (hipStream_t)stream_, fused, image_mu, event_mu, (long long)rows,
                           (const int*)src_rows, (long long)nout, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

#include "vadclip.h"
#include "hostgather.h"
#include "hostpipe.h"

// One production row-block kernel of the bf16 mode on caller-supplied rows (include/iefvad.h): the launch helpers forward_pass uses.
extern "C" int iefvad_rowblock_unit(iefvad_handle* h, int32_t stage, int32_t layer, int32_t rows, const iefvad_unit_io* io, void* stream_) {
    if (!h || !io) return fail("iefvad_rowblock_unit: null argument");
    if (!h->weights_set) return fail("iefvad_rowblock_unit: weights not set");
    if (h->D != IEF_D) return fail("iefvad_rowblock_unit: the row-block kernels are built for D=768 (this handle has D=%d)", h->D);
    if (h->cfg.compute != IEFVAD_COMPUTE_BF16) return fail("iefvad_rowblock_unit: the row-block kernels belong to compute = BF16 (got %d)", h->cfg.compute);
    if (rows <= 0 || rows % 64) return fail("iefvad_rowblock_unit: rows = %d must be a positive multiple of 64", rows);
    if (stage == IEFVAD_UNIT_ATTENTION && rows % IEF_T) return fail("iefvad_rowblock_unit: ATTENTION runs whole chunks, rows = %d must be a multiple of %d", rows, IEF_T);
    hipStream_t stream = (hipStream_t)stream_;
    const int L = h->cfg.num_layers, K = h->cfg.num_steps;
    Timer tm;
    auto aligned = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
    switch (stage) {
    case IEFVAD_UNIT_INPROJ: {
        if (layer < 0 || layer >= L) return fail("iefvad_rowblock_unit: layer %d of %d", layer, L);
        if (!h->iproj_stream[0][layer]) return fail("iefvad_rowblock_unit: in_proj streams are not packed on this handle");
        const void* A[2] = {io->x[0], io->x[1]};
        bf16_t* C[2] = {(bf16_t*)io->y[0], (bf16_t*)io->y[1]};
        for (int m = 0; m < 2; ++m)
            if (!A[m] || !C[m] || !aligned(A[m]) || !aligned(C[m])) return fail("iefvad_rowblock_unit: INPROJ needs x[m] and y[m], 16-byte aligned");
        return launch_inproj_chain(h, layer, A, layer == 0, C, rows, stream, tm);
    }
    case IEFVAD_UNIT_OUTPROJ_LN: {
        if (layer < 0 || layer >= L) return fail("iefvad_rowblock_unit: layer %d of %d", layer, L);
        if (!h->oproj_stream[0][layer]) return fail("iefvad_rowblock_unit: out_proj streams are not packed on this handle");
        const bf16_t* A[2] = {(const bf16_t*)io->x[0], (const bf16_t*)io->x[1]};
        const float* R[2] = {io->resid[0], io->resid[1]};
        float* y[2] = {(float*)io->y[0], (float*)io->y[1]};
        bf16_t* yb[2] = {(bf16_t*)io->yb[0], (bf16_t*)io->yb[1]};
        for (int m = 0; m < 2; ++m)
            if (!A[m] || !R[m] || (!y[m] && !yb[m]) || !aligned(A[m]) || !aligned(R[m]) || !aligned(y[m]) || !aligned(yb[m]))
                return fail("iefvad_rowblock_unit: OUTPROJ_LN needs x[m], resid[m] and y[m] or yb[m], 16-byte aligned");
        return launch_outproj_ln_chain(h, layer, layer == L - 1, A, R, y, yb, rows, stream, tm);
    }
    case IEFVAD_UNIT_HEADS: {
        if (!h->heads_stream) return fail("iefvad_rowblock_unit: the heads stream is not packed on this handle");
        if (!io->x[0] || !io->x[1] || !io->z || !aligned(io->x[0]) || !aligned(io->x[1]) || !aligned(io->z))
            return fail("iefvad_rowblock_unit: HEADS needs x[0], x[1] and z, 16-byte aligned");
        HeadsChainArgs ha;
        memset(&ha, 0, sizeof(ha));
        for (int m = 0; m < 2; ++m) {
            ha.A[m] = (const bf16_t*)io->x[m];
            ha.mu[m] = io->mu[m]; ha.lv[m] = io->logvar[m]; ha.n[m] = io->w[m];
        }
        ha.z = io->z;
        return launch_heads_chain(h, ha, rows, precision_factor(h->cfg), stream, tm);
    }
    case IEFVAD_UNIT_REFINE: {
        if (K < 1 || !h->chain_stream) return fail("iefvad_rowblock_unit: the refinement chain needs K >= 1 (K = %d)", K);
        if (!io->x[0] || !io->logits || !aligned(io->x[0]) || !aligned(io->z)) return fail("iefvad_rowblock_unit: REFINE needs x[0] (z_0) and logits");
        return launch_refine_chain(h, (const float*)io->x[0], io->z, io->logits, rows, stream, tm);
    }
    case IEFVAD_UNIT_ATTENTION: {
        const bf16_t* qkv[2] = {(const bf16_t*)io->x[0], (const bf16_t*)io->x[1]};
        bf16_t* out[2] = {(bf16_t*)io->yb[0], (bf16_t*)io->yb[1]};
        for (int m = 0; m < 2; ++m)
            if (!qkv[m] || !out[m] || !aligned(qkv[m]) || !aligned(out[m])) return fail("iefvad_rowblock_unit: ATTENTION needs x[m] and yb[m], 16-byte aligned");
        return launch_attention_bf16(h, qkv, out, rows / IEF_T, nullptr, true, rows, stream, tm);
    }
    default:
        return fail("iefvad_rowblock_unit: unknown stage %d", stage);
    }
}

extern "C" int iefvad_gemm_bias(const void* A, const void* W, const float* bias, float* C, int32_t M, int32_t N, int32_t K,
                                int32_t compute, void* stream) {
    if (!A || !W || !bias || !C) return fail("iefvad_gemm_bias: null argument");
    Timer tm;
    if (compute == IEFVAD_COMPUTE_F32) {
        GemmArgs g;
        memset(&g, 0, sizeof(g));
        g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N; g.epi = EPI_BIAS;
        g.p[0].A = (const float*)A; g.p[0].W = (const float*)W; g.p[0].bias = bias; g.p[0].C = C;
        return launch_gemm(g, 1, (hipStream_t)stream, tm, ST_QKV);
    }
    if (compute == IEFVAD_COMPUTE_BF16) {
        GemmBArgs g;
        memset(&g, 0, sizeof(g));
        g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N; g.epi = EPI_BIAS;
        g.p[0].A = (const bf16_t*)A; g.p[0].W = (const bf16_t*)W; g.p[0].bias = bias; g.p[0].C = C;
        return launch_gemm_b(g, 1, (hipStream_t)stream, tm, ST_QKV);
    }
    if (compute == IEFVAD_COMPUTE_BF16X6) {
        GemmBArgs g;
        memset(&g, 0, sizeof(g));
        g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N; g.epi = EPI_BIAS; g.wplane = N * K * 2;
        g.p[0].A = (const bf16_t*)A; g.p[0].W = (const bf16_t*)W; g.p[0].bias = bias; g.p[0].C = C;
        hipError_t e = raise_lds_limit((const void*)iefvad_gemm_split_n128_kernel);
        if (e == hipSuccess) e = raise_lds_limit((const void*)iefvad_gemm_split_n128x2_kernel);
        if (e != hipSuccess) return fail("iefvad_gemm_bias: %s", hipGetErrorString(e));
        return launch_gemm_split(g, 1, (hipStream_t)stream, tm, ST_QKV);
    }
    return fail("iefvad_gemm_bias: unknown compute mode %d", compute);
}

extern "C" uint64_t iefvad_gemm_split_wide_launches(void) { return g_split_wide_launches.load(std::memory_order_relaxed); }

// the argument block of the two split unit entries from their common arguments; bm x bn: the tile the shape must fit
static int gemm_split_unit_args(const char* who, const iefvad_gemm_split_io* io, int32_t M, int32_t N, int32_t K, int32_t ldc, int32_t epilogue,
                                int32_t qcols, float alpha, int32_t nz, int bm, int bn, GemmBArgs& g) {
    static const int epi_of[] = {EPI_BIAS, EPI_QKV, EPI_BIAS_RELU, EPI_BIAS_RESID, EPI_REFINE, EPI_HEADS, EPI_BIAS_RELU_DOT};
    auto aligned = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
    if (M <= 0 || N <= 0 || K < 64 || M % bm || N % bn || K % 64)
        return fail("%s: shape M=%d N=%d K=%d not a multiple of the %dx%dx64 tile", who, M, N, K, bm, bn);
    const int epi = epi_of[epilogue];
    const bool heads = epi == EPI_HEADS, dot = epi == EPI_BIAS_RELU_DOT;
    const bool resid = epi == EPI_BIAS_RESID || epi == EPI_REFINE;
    if (heads ? (N != 2 * ldc || ldc % 128) : (ldc < N || ldc % 4)) return fail("%s: ldc = %d does not fit N = %d", who, ldc, N);
    if (epi == EPI_QKV && (qcols < 0 || qcols > N || qcols % 8)) return fail("%s: qcols = %d", who, qcols);
    memset(&g, 0, sizeof(g));
    g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = ldc; g.epi = epi; g.alpha = alpha; g.qcols = qcols;
    g.wplane = N * K * 2;
    for (int m = 0; m < nz; ++m) {
        if (!io->A[m] || !io->W[m] || !io->bias[m] || (!io->C[m] && !dot) || ((resid || dot) && !io->R[m]) || ((heads || dot) && !io->C2[m]))
            return fail("%s: problem %d lacks an operand of epilogue %d", who, m, epilogue);
        if (!aligned(io->A[m]) || !aligned(io->W[m]) || !aligned(io->bias[m]) || !aligned(io->C[m]) || !aligned(io->R[m]) || !aligned(io->C2[m]))
            return fail("%s: operands must be 16-byte aligned", who);
        g.p[m].A = (const bf16_t*)io->A[m]; g.p[m].W = (const bf16_t*)io->W[m]; g.p[m].bias = io->bias[m]; g.p[m].C = io->C[m];
        g.p[m].R = (resid || dot) ? io->R[m] : nullptr;
        g.p[m].C2 = (heads || dot) ? io->C2[m] : nullptr;
    }
    return 0;
}

extern "C" int iefvad_gemm_split_unit(const iefvad_gemm_split_io* io, int32_t M, int32_t N, int32_t K, int32_t ldc, int32_t epilogue,
                                      int32_t qcols, float alpha, int32_t nz, int32_t tile_n, void* stream) {
    if (!io) return fail("iefvad_gemm_split_unit: null argument");
    if (epilogue < 0 || epilogue > IEFVAD_SPLIT_EPI_BIAS_RELU_DOT) return fail("iefvad_gemm_split_unit: unknown epilogue %d", epilogue);
    if (nz < 1 || nz > 2) return fail("iefvad_gemm_split_unit: nz = %d (1 or 2)", nz);
    if (tile_n != 128 && tile_n != 256) return fail("iefvad_gemm_split_unit: tile_n = %d (128 or 256)", tile_n);
    GemmBArgs g;
    if (int rc = gemm_split_unit_args("iefvad_gemm_split_unit", io, M, N, K, ldc, epilogue, qcols, alpha, nz, GS_BM, tile_n, g)) return rc;
    hipError_t e = raise_lds_limit((const void*)iefvad_gemm_split_n128_kernel);
    if (e == hipSuccess) e = raise_lds_limit((const void*)iefvad_gemm_split_n128x2_kernel);
    if (e != hipSuccess) return fail("iefvad_gemm_split_unit: %s", hipGetErrorString(e));
    Timer tm;
    return launch_gemm_split(g, nz, (hipStream_t)stream, tm, ST_QKV, false, tile_n);
}

extern "C" uint64_t iefvad_gemm_split_small_launches(void) { return g_split_small_launches.load(std::memory_order_relaxed); }

extern "C" int iefvad_gemm_split_small_unit(const iefvad_gemm_split_io* io, int32_t M, int32_t N, int32_t K, int32_t ldc, int32_t epilogue,
                                            int32_t qcols, float alpha, int32_t nz, void* stream) {
    if (!io) return fail("iefvad_gemm_split_small_unit: null argument");
    if (epilogue < 0 || epilogue > IEFVAD_SPLIT_EPI_BIAS_RELU_DOT) return fail("iefvad_gemm_split_small_unit: unknown epilogue %d", epilogue);
    if (nz < 1 || nz > 2) return fail("iefvad_gemm_split_small_unit: nz = %d (1 or 2)", nz);
    GemmBArgs g;
    if (int rc = gemm_split_unit_args("iefvad_gemm_split_small_unit", io, M, N, K, ldc, epilogue, qcols, alpha, nz, kSplitSmallBM, kSplitBN, g)) return rc;
    Timer tm;
    return launch_gemm_split_small(g, nz, (hipStream_t)stream, tm, ST_QKV);
}

// One kernel of the backward pass on the caller's buffers (include/iefvad.h), through train.h's own launch helpers
extern "C" int iefvad_backward_unit(int32_t kind, const void* args, size_t args_bytes, void* stream_) {
    static const char* const who = "iefvad_backward_unit";
    if (!args) return fail("%s: null argument", who);
    hipStream_t stream = (hipStream_t)stream_;
    auto al = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
    auto sized = [&](size_t want) { return args_bytes == want ? 0 : fail("%s: kind %d takes an argument block of %zu bytes (got %zu)", who, kind, want, args_bytes); };
    switch (kind) {
    case IEFVAD_BWD_BGEMM: {
        if (int rc = sized(sizeof(iefvad_bwd_bgemm))) return rc;
        const iefvad_bwd_bgemm& u = *(const iefvad_bwd_bgemm*)args;
        if (!u.A || !u.B || !u.C) return fail("%s: BGEMM needs A, B and C", who);
        if (!al(u.A) || !al(u.B) || ((u.a1 | u.a2 | u.b1 | u.b2) & 3)) return fail("%s: BGEMM reads A and B 16 bytes at a time: pointers and batch strides must be aligned", who);
        if (u.act < 0 || u.act > 2) return fail("%s: BGEMM act = %d (0, 1 or 2)", who, u.act);
        BgemmArgs a;
        memset(&a, 0, sizeof(a));
        a.A = u.A; a.B = u.B; a.C = u.C; a.R = u.R; a.G = u.G; a.bias = u.bias;
        a.M = u.M; a.N = u.N; a.K = u.K; a.lda = u.lda; a.ldb = u.ldb; a.ldc = u.ldc;
        a.a1 = u.a1; a.a2 = u.a2; a.b1 = u.b1; a.b2 = u.b2; a.c1 = u.c1; a.c2 = u.c2;
        a.nz2 = u.nz2; a.alpha = u.alpha; a.act = u.act; a.a_drop = u.a_drop;
        return launch_bgemm(a, u.akc != 0, u.bkc != 0, u.nz, stream);
    }
    case IEFVAD_BWD_SPLIT_TN: {
        if (int rc = sized(sizeof(iefvad_bwd_split_tn))) return rc;
        const iefvad_bwd_split_tn& u = *(const iefvad_bwd_split_tn*)args;
        if (!u.dY || !u.X || !u.part || !u.dW || (u.colsum_part && !u.db)) return fail("%s: SPLIT_TN needs dY, X, part and dW (and db with colsum_part)", who);
        if (!al(u.dY) || !al(u.X) || !al(u.part) || !al(u.colsum_part)) return fail("%s: SPLIT_TN operands must be 16-byte aligned", who);
        if (u.rows <= 0 || u.rows % TN_BK || u.n_out <= 0 || u.n_out % 128)
            return fail("%s: SPLIT_TN rows = %d must be a multiple of %d and n_out = %d of 128", who, u.rows, TN_BK, u.n_out);
        const int nk_total = u.rows / TN_BK;
        if (u.slices < 1 || u.slices > nk_total / 8) return fail("%s: SPLIT_TN slices = %d outside 1..%d (eight 16-row tiles per slice at least)", who, u.slices, nk_total / 8);
        hipError_t e = raise_lds_limit((const void*)iefvad_gemm_split_tn256_kernel);
        if (e != hipSuccess) return fail("%s: %s", who, hipGetErrorString(e));
        return launch_dw_split_tn(u.dY, u.X, u.rows, u.n_out, u.slices, u.part, u.colsum_part, u.n_out, u.alpha, u.dW, nullptr, u.db, nullptr, stream);
    }
    case IEFVAD_BWD_SOFTMAX_DROPOUT: {
        if (int rc = sized(sizeof(iefvad_bwd_softmax_dropout))) return rc;
        const iefvad_bwd_softmax_dropout& u = *(const iefvad_bwd_softmax_dropout*)args;
        if (!u.S || !al(u.S) || u.rows <= 0) return fail("%s: SOFTMAX_DROPOUT needs S, 16-byte aligned, and rows > 0", who);
        SoftmaxDropArgs a;
        a.S = u.S; a.drop = u.drop ? 1 : 0; a.keep = u.keep; a.seed = u.seed; a.p = u.p; a.rows = u.rows;
        return launch_softmax_dropout(a, stream);
    }
    case IEFVAD_BWD_SOFTMAX_BWD: {
        if (int rc = sized(sizeof(iefvad_bwd_softmax_bwd))) return rc;
        const iefvad_bwd_softmax_bwd& u = *(const iefvad_bwd_softmax_bwd*)args;
        if (!u.Ps || !u.dPd || !al(u.Ps) || !al(u.dPd) || u.rows <= 0) return fail("%s: SOFTMAX_BWD needs Ps and dPd, 16-byte aligned, and rows > 0", who);
        return launch_softmax_bwd(u.Ps, u.scale, u.dPd, u.rows, stream);
    }
    case IEFVAD_BWD_COLSUM: {
        if (int rc = sized(sizeof(iefvad_bwd_colsum))) return rc;
        const iefvad_bwd_colsum& u = *(const iefvad_bwd_colsum*)args;
        if (!u.Y || !u.part || u.rows <= 0 || u.ncols <= 0 || u.ld < u.ncols) return fail("%s: COLSUM needs Y and part, rows > 0 and 0 < ncols <= ld", who);
        return launch_colsum(u.Y, u.ld, u.rows, u.ncols, u.part, stream);
    }
    case IEFVAD_BWD_REDUCE_PARTS:
    case IEFVAD_BWD_REDUCE_PARTS_MULTI: {
        if (int rc = sized(sizeof(iefvad_bwd_reduce))) return rc;
        const iefvad_bwd_reduce& u = *(const iefvad_bwd_reduce*)args;
        if (u.count < 1 || u.count > 5) return fail("%s: REDUCE_PARTS count = %d (1..5)", who, u.count);
        for (int j = 0; j < u.count; ++j)
            if (!u.part[j] || u.nparts[j] < 1) return fail("%s: REDUCE_PARTS job %d needs part and nparts >= 1", who, j);
        if (kind == IEFVAD_BWD_REDUCE_PARTS) return reduce_parts(u.part[0], (size_t)u.stride[0], u.nparts[0], (size_t)u.n[0], u.out[0], u.alpha[0], stream);
        ReduceBatch rb;
        for (int j = 0; j < u.count; ++j) rb.add(u.part[j], (size_t)u.stride[j], u.nparts[j], (size_t)u.n[j], u.out[j], u.alpha[j]);
        return rb.launch(stream);
    }
    case IEFVAD_BWD_SCORER: {
        if (int rc = sized(sizeof(iefvad_bwd_scorer))) return rc;
        const iefvad_bwd_scorer& u = *(const iefvad_bwd_scorer*)args;
        if (!u.z || !u.w || !u.g || !u.part_w || !u.part_b || u.rows <= 0) return fail("%s: SCORER needs z, w, g, part_w, part_b and rows > 0", who);
        if (!al(u.z) || !al(u.w) || !al(u.g) || !al(u.dfused)) return fail("%s: SCORER operands must be 16-byte aligned", who);
        ScorerBwdArgs a;
        a.dlogit = u.dlogit; a.dfused = u.dfused; a.z = u.z; a.w = u.w; a.g = u.g; a.part_w = u.part_w; a.part_b = u.part_b; a.rows = u.rows;
        return launch_scorer_bwd(a, stream);
    }
    case IEFVAD_BWD_FUSION: {
        if (int rc = sized(sizeof(iefvad_bwd_fusion))) return rc;
        const iefvad_bwd_fusion& u = *(const iefvad_bwd_fusion*)args;
        if (!u.mu_i || !u.lv_i || !u.mu_e || !u.lv_e || !u.gz || !u.dh_i || !u.dh_e || u.rows <= 0)
            return fail("%s: FUSION needs mu, logvar of both modalities, gz, dh_i, dh_e and rows > 0", who);
        for (const void* p : {(const void*)u.mu_i, (const void*)u.lv_i, (const void*)u.mu_e, (const void*)u.lv_e, (const void*)u.gz, (const void*)u.d_mu_i,
                              (const void*)u.d_lv_i, (const void*)u.d_mu_e, (const void*)u.d_lv_e, (const void*)u.dh_i, (const void*)u.dh_e})
            if (!al(p)) return fail("%s: FUSION operands must be 16-byte aligned", who);
        FusionBwdArgs a;
        memset(&a, 0, sizeof(a));
        a.mu_i = u.mu_i; a.lv_i = u.lv_i; a.mu_e = u.mu_e; a.lv_e = u.lv_e; a.gz = u.gz;
        a.d_mu_i = u.d_mu_i; a.d_lv_i = u.d_lv_i; a.d_mu_e = u.d_mu_e; a.d_lv_e = u.d_lv_e; a.d_n_i = u.d_n_i; a.d_n_e = u.d_n_e;
        a.dh_i = u.dh_i; a.dh_e = u.dh_e; a.rows = u.rows; a.factor = u.factor; a.eps = u.eps;
        return launch_fusion_bwd(a, stream);
    }
    case IEFVAD_BWD_LAYERNORM: {
        if (int rc = sized(sizeof(iefvad_bwd_layernorm))) return rc;
        const iefvad_bwd_layernorm& u = *(const iefvad_bwd_layernorm*)args;
        if (!u.x || !u.dy || !u.g || !u.dx || !u.part_g || !u.part_b || u.rows <= 0) return fail("%s: LAYERNORM needs x, dy, g, dx, part_g, part_b and rows > 0", who);
        if (!al(u.x) || !al(u.dy) || !al(u.g) || !al(u.dx)) return fail("%s: LAYERNORM operands must be 16-byte aligned", who);
        LnBwdArgs a;
        a.x = u.x; a.dy = u.dy; a.g = u.g; a.dx = u.dx; a.part_g = u.part_g; a.part_b = u.part_b; a.rows = u.rows; a.eps = u.eps;
        return launch_layernorm_bwd(a, stream);
    }
    }
    return fail("%s: unknown kind %d", who, kind);
}

// Batch-invariant mode (include/iefvad.h): flips LaunchPolicy::split_always.  The cached hipGraphs hold the other mode's launches, so
// they go (after the device has finished with their staging buffers).  train.h never reads the flag: training keeps its own rule.
extern "C" int iefvad_set_batch_invariant(iefvad_handle* h, int on) {
    if (!h) return fail("iefvad_set_batch_invariant: null argument");
    if (h->cfg.compute == IEFVAD_COMPUTE_FP16X3)
        return fail("iefvad_set_batch_invariant: compute = FP16X3 has no batch-invariant mode (its operand scales are per chunk and per running maximum)");
    if (h->cfg.compute != IEFVAD_COMPUTE_BF16X6) return 0;      // f32 and bf16 are batch-invariant as they are
    const bool want = on != 0;
    if (h->policy.split_always == want) return 0;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    release_graphs(h);
    h->policy.split_always = want;
    return 0;
}

// Call-time step count (include/iefvad.h): the evaluation entries run refinement blocks 0 .. steps - 1.  Nothing resident depends on
// the count (every block's folded-scorer vector is there since iefvad_set_weights, the chain's stream is in step order), and the
// graph cache is keyed by it, so this only records the number.
extern "C" int iefvad_set_steps(iefvad_handle* h, int32_t steps) {
    if (!h) return fail("iefvad_set_steps: null argument");
    if (steps < 0 || steps > h->cfg.num_steps) return fail("iefvad_set_steps: steps %d outside 0..%d (the handle's num_steps)", steps, h->cfg.num_steps);
    h->steps = steps;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// the entries that add one extra to a forward: trajectory, fusion ablations, score samples (include/iefvad.h)
// ------------------------------------------------------------------------------------------------
// A dense entry: its null and B checks, `args(x, rows of the call)` -- the extra's own checks, into the record --, its workspace check
// under its own name, then the forward.  Direct launches: the results' pointers are per call, a cached graph would pin their addresses.
template <typename Args>
static int forward_extra(const char* who, iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B, void* workspace,
                         size_t workspace_bytes, const iefvad_outputs* out, void* stream, Args&& args) {
    if (!h) return fail("%s: null handle", who);
    if (!img || !ev || !out) return fail("%s: null argument", who);
    if (B <= 0) return fail("%s: B must be positive (got %d)", who, B);
    Extras x = {};
    if (int rc = args(x, (long long)B * IEF_T)) return rc;
    const size_t need = dense_workspace_bytes(h, B, x.wants());
    if (!workspace || workspace_bytes < need) return fail("%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, need);
    Timer tm;
    return forward_impl(h, RowsIn{img, ev, in_dtype}, x, B, workspace, workspace_bytes, out, (hipStream_t)stream, tm);
}
// A whole-video entry: the same, on the call's packed rows; forward_videos_impl makes the remaining checks
template <typename Args>
static int forward_videos_extra(const char* who, iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype, const int32_t* lengths,
                                int32_t nvideos, int32_t nan_to_num, void* workspace, size_t workspace_bytes, float* logits, float* w_i_mean,
                                float* w_e_mean, void* stream, Args&& args) {
    if (!h) return fail("%s: null handle", who);
    if (!lengths) return fail("%s: null argument", who);
    if (nvideos <= 0) return fail("%s: nvideos must be positive (got %d)", who, nvideos);
    long long rows, chunks;
    if (int rc = videos_layout(lengths, nvideos, &rows, &chunks, who)) return rc;
    VideosOut out = videos_out(logits, w_i_mean, w_e_mean, nan_to_num);
    if (int rc = args(out.x, rows)) return rc;
    Timer tm;
    return forward_videos_impl(h, RowsIn{img_rows, ev_rows, in_dtype}, lengths, nvideos, workspace, workspace_bytes, out, (hipStream_t)stream, tm, who);
}
static TailWants want_traj() { TailWants w = {}; w.traj = true; return w; }
static TailWants want_variants(int count) { TailWants w = {}; w.variants = count; return w; }
static TailWants want_samples() { TailWants w = {}; w.samples = true; return w; }

// The checks of a trajectory request that need no device: something is asked for, 4-byte aligned, a stride that holds the call's rows
static int trajectory_args(const char* who, const iefvad_trajectory* t, long long rows, TrajOut* tj) {
    if (!t) return fail("%s: null trajectory", who);
    if (!t->logits_steps && !t->delta_norm) return fail("%s: logits_steps and delta_norm are both null (nothing is asked for)", who);
    if (((uintptr_t)t->logits_steps | (uintptr_t)t->delta_norm) & 3) return fail("%s: logits_steps and delta_norm must be 4-byte aligned", who);
    if ((long long)t->stride < rows) return fail("%s: stride %zu is less than the call's %lld rows", who, t->stride, rows);
    *tj = TrajOut{t->logits_steps, t->delta_norm, (long long)t->stride, 0, nullptr};
    return 0;
}

extern "C" size_t iefvad_trajectory_workspace_bytes(const iefvad_handle* h, int32_t B) { return dense_workspace_bytes(h, B, want_traj()); }
extern "C" size_t iefvad_videos_trajectory_workspace_bytes(const iefvad_handle* h, const int32_t* lengths, int32_t nvideos) {
    return videos_workspace_bytes(h, lengths, nvideos, want_traj());
}

extern "C" int iefvad_forward_trajectory(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B, void* workspace,
                                         size_t workspace_bytes, const iefvad_outputs* out, const iefvad_trajectory* trajectory, void* stream) {
    static const char* const who = "iefvad_forward_trajectory";
    return forward_extra(who, h, img, ev, in_dtype, B, workspace, workspace_bytes, out, stream,
                         [&](Extras& x, long long rows) { return trajectory_args(who, trajectory, rows, &x.traj); });
}

extern "C" int iefvad_forward_videos_trajectory(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype,
                                                const int32_t* lengths, int32_t nvideos, int32_t nan_to_num, void* workspace,
                                                size_t workspace_bytes, float* logits, float* w_i_mean, float* w_e_mean,
                                                const iefvad_trajectory* trajectory, void* stream) {
    static const char* const who = "iefvad_forward_videos_trajectory";
    return forward_videos_extra(who, h, img_rows, ev_rows, in_dtype, lengths, nvideos, nan_to_num, workspace, workspace_bytes, logits, w_i_mean, w_e_mean,
                                stream, [&](Extras& x, long long rows) { return trajectory_args(who, trajectory, rows, &x.traj); });
}

// The checks of a variants request that need no device
static int variants_args(const char* who, const iefvad_handle* h, const iefvad_variants* v, long long rows, VarOut* vo) {
    if (h->cfg.compute == IEFVAD_COMPUTE_FP16X3) return fail("%s: compute = FP16X3 is not supported (IEFVAD_COMPUTE_FP16X3 has no fusion variants)", who);
    if (!v) return fail("%s: null variants", who);
    if (!v->logits) return fail("%s: null variants logits", who);
    if ((uintptr_t)v->logits & 3) return fail("%s: variants logits must be 4-byte aligned", who);
    if (v->count < 1 || v->count > IEF_MAX_VARIANTS) return fail("%s: count %d outside 1..%d", who, v->count, IEF_MAX_VARIANTS);
    *vo = VarOut{};
    for (int i = 0; i < v->count; ++i) {
        if (v->kind[i] < IEFVAD_VARIANT_FUSED || v->kind[i] > IEFVAD_VARIANT_EQUAL) return fail("%s: unknown variant kind %d at %d", who, v->kind[i], i);
        for (int j = 0; j < i; ++j)
            if (v->kind[j] == v->kind[i]) return fail("%s: variant kind %d is repeated (at %d and %d)", who, v->kind[i], j, i);
        vo->kind[i] = v->kind[i];
    }
    if ((long long)v->stride < rows) return fail("%s: stride %zu is less than the call's %lld rows", who, v->stride, rows);
    vo->count = v->count; vo->logits = v->logits; vo->stride = (long long)v->stride;
    return 0;
}

static bool variants_count_ok(int32_t count) { return count >= 1 && count <= IEF_MAX_VARIANTS; }
extern "C" size_t iefvad_variants_workspace_bytes(const iefvad_handle* h, int32_t B, int32_t count) {
    return variants_count_ok(count) ? dense_workspace_bytes(h, B, want_variants(count)) : 0;
}
extern "C" size_t iefvad_videos_variants_workspace_bytes(const iefvad_handle* h, const int32_t* lengths, int32_t nvideos, int32_t count) {
    return variants_count_ok(count) ? videos_workspace_bytes(h, lengths, nvideos, want_variants(count)) : 0;
}

extern "C" int iefvad_forward_variants(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B, void* workspace,
                                       size_t workspace_bytes, const iefvad_outputs* out, const iefvad_variants* variants, void* stream) {
    static const char* const who = "iefvad_forward_variants";
    return forward_extra(who, h, img, ev, in_dtype, B, workspace, workspace_bytes, out, stream,
                         [&](Extras& x, long long rows) { return variants_args(who, h, variants, rows, &x.var); });
}

extern "C" int iefvad_forward_videos_variants(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype,
                                              const int32_t* lengths, int32_t nvideos, int32_t nan_to_num, void* workspace,
                                              size_t workspace_bytes, float* logits, float* w_i_mean, float* w_e_mean,
                                              const iefvad_variants* variants, void* stream) {
    static const char* const who = "iefvad_forward_videos_variants";
    return forward_videos_extra(who, h, img_rows, ev_rows, in_dtype, lengths, nvideos, nan_to_num, workspace, workspace_bytes, logits, w_i_mean, w_e_mean,
                                stream, [&](Extras& x, long long rows) { return variants_args(who, h, variants, rows, &x.var); });
}

// The checks of a samples request that need no device
static int samples_args(const char* who, const iefvad_handle* h, const iefvad_samples* p, long long rows, SampleOut* so) {
    if (h->cfg.compute == IEFVAD_COMPUTE_FP16X3) return fail("%s: compute = FP16X3 is not supported (IEFVAD_COMPUTE_FP16X3 has no score samples)", who);
    if (!p) return fail("%s: null samples", who);
    if (p->samples < 1 || p->samples > IEF_MAX_SAMPLES) return fail("%s: samples %d outside 1..%d", who, p->samples, IEF_MAX_SAMPLES);
    if (!(p->scale >= 0.f) || p->scale > 3.40282347e38f) return fail("%s: scale must be finite and >= 0 (got %g)", who, (double)p->scale);
    if (!p->logits_samples) return fail("%s: null logits_samples", who);
    if (!p->score_mean) return fail("%s: null score_mean", who);
    if (!p->score_std) return fail("%s: null score_std", who);
    if (((uintptr_t)p->logits_samples | (uintptr_t)p->score_mean | (uintptr_t)p->score_std | (uintptr_t)p->sample_rows) & 3)
        return fail("%s: logits_samples, score_mean, score_std and sample_rows must be 4-byte aligned", who);
    if ((long long)p->stride < rows) return fail("%s: stride %zu is less than the call's %lld rows", who, p->stride, rows);
    *so = SampleOut{};
    so->count = p->samples; so->seed = p->seed; so->scale = p->scale; so->ids = p->sample_rows;
    so->logits = p->logits_samples; so->mean = p->score_mean; so->stdev = p->score_std; so->stride = (long long)p->stride;
    return 0;
}

// one group of stacked states, whatever the sample count
extern "C" size_t iefvad_samples_workspace_bytes(const iefvad_handle* h, int32_t B) { return dense_workspace_bytes(h, B, want_samples()); }
extern "C" size_t iefvad_videos_samples_workspace_bytes(const iefvad_handle* h, const int32_t* lengths, int32_t nvideos) {
    return videos_workspace_bytes(h, lengths, nvideos, want_samples());
}

extern "C" int iefvad_forward_samples(iefvad_handle* h, const void* img, const void* ev, int32_t in_dtype, int32_t B, void* workspace,
                                      size_t workspace_bytes, const iefvad_outputs* out, const iefvad_samples* samples, void* stream) {
    static const char* const who = "iefvad_forward_samples";
    return forward_extra(who, h, img, ev, in_dtype, B, workspace, workspace_bytes, out, stream,
                         [&](Extras& x, long long rows) { return samples_args(who, h, samples, rows, &x.smp); });
}

extern "C" int iefvad_forward_videos_samples(iefvad_handle* h, const void* img_rows, const void* ev_rows, int32_t in_dtype,
                                             const int32_t* lengths, int32_t nvideos, int32_t nan_to_num, void* workspace,
                                             size_t workspace_bytes, float* logits, float* w_i_mean, float* w_e_mean,
                                             const iefvad_samples* samples, void* stream) {
    static const char* const who = "iefvad_forward_videos_samples";
    return forward_videos_extra(who, h, img_rows, ev_rows, in_dtype, lengths, nvideos, nan_to_num, workspace, workspace_bytes, logits, w_i_mean, w_e_mean,
                                stream, [&](Extras& x, long long rows) { return samples_args(who, h, samples, rows, &x.smp); });
}

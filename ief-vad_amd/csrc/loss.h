// Training-side loss head, forward only: the three terms the reference's trainers add up
// (/root/reference/train/ucf_train.py:68-101, train/xd_train.py:60-75), as device reductions over tensors the forward
// already produces (logits, image_mu, event_mu, image_logvar, event_logvar):
//   * CLAS2 (/root/reference/train/loss.py:18-30): per video i, p_i = mean of the k = int(len_i / 16 + 1) largest
//     sigmoid(logit[i, 0:len_i]); binary cross entropy of p against (1 - labels[:, 0]), mean over the batch
//     (torch's BCE clamps the logarithms at -100);
//   * the regulariser (ucf_train.py:75-82): mean over all B*T rows of 1 - cosine_similarity(normalize(mu_i), normalize(mu_e))
//     plus the mean of | ||mu_i|| - ||mu_e|| |;
//   * the KL terms (ucf_train.py:84-98): -0.5 mean(1 + l - mu^2 - exp(l)) per modality, with l = logvar for the Gaussian
//     noise model and logvar + log(nu / (nu + 1)) for Student-t.
// No atomics: per-video and per-row partial results land in a workspace and ONE workgroup combines them in a fixed order,
// so the losses are bit-reproducible from run to run.
// Backward of the loss head (iefvad_loss_backward): the gradients of the total with respect to the five tensors above, i.e.
// what autograd hands to the model's outputs; the model's own backward pass is not part of this library.
#pragma once
#include "common.h"

#define LOSS_T IEF_T

// one workgroup (256 threads = the T snippets) per video: top-k mean of the sigmoid scores over the valid prefix
// rank order of torch.topk(largest=True): NaN counts as larger than every number; equal keys are ordered by index (any choice among
// equal VALUES gives the same mean; among NaNs the mean is NaN anyway)
__device__ __forceinline__ bool topk_before(float y, int u, float x, int t) {
    const bool ny = y != y, nx = x != x;
    if (ny || nx) return ny && (!nx || u < t);
    return (y > x) || (y == x && u < t);
}

__global__ __launch_bounds__(256) void iefvad_mil_topk_kernel(const float* logits, const int* lengths, float* inst, int T) {
    __shared__ float s[LOSS_T];
    const int v = blockIdx.x, t = threadIdx.x;
    const int len_raw = lengths[v];
    const int len = len_raw < 0 ? 0 : (len_raw > T ? T : len_raw);
    const int k = len_raw / 16 + 1;                              // int(lengths[i] / 16 + 1), loss.py:26 -- from the length as given
    const float x = (t < len) ? 1.0f / (1.0f + expf(-logits[(size_t)v * T + t])) : -1.0f;     // sigmoid is in (0, 1): -1 never wins
    s[t] = x;
    __syncthreads();
    int rank = 0;
    for (int u = 0; u < T; ++u) rank += topk_before(s[u], u, x, t);
    float part = (t < len && rank < k) ? x : 0.f;
    part = wave_sum(part);
    __shared__ float w[4];
    if ((t & 63) == 0) w[t >> 6] = part;
    __syncthreads();
    // torch.topk raises for k > len (a length beyond T, or <= 0): no exception can leave a kernel, the video's score is NaN instead
    if (t == 0) inst[v] = (k <= len) ? ((w[0] + w[1]) + (w[2] + w[3])) / (float)k : __builtin_nanf("");
}

// one wavefront per row: cosine / norm regulariser terms and the two KL sums of the row -> part[row][4]
struct LossRowArgs {
    const float* mu_i; const float* mu_e; const float* lv_i; const float* lv_e;     // [rows, 768]
    float* part;                 // [rows][4]: 1 - cos, |norm_i - norm_e|, KL sum image, KL sum event
    int rows;
    float lv_shift;              // 0 (Gaussian) or log(nu / (nu + 1)) (StudentT)
};
__global__ __launch_bounds__(256) void iefvad_loss_rows_kernel(LossRowArgs a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const size_t base = (size_t)row * IEF_D + 4 * lane;
    f32x4 mi[3], me[3];
    float sii = 0.f, see = 0.f, kli = 0.f, kle = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        mi[j] = *(const f32x4*)(a.mu_i + base + 256 * j);
        me[j] = *(const f32x4*)(a.mu_e + base + 256 * j);
        const f32x4 li = *(const f32x4*)(a.lv_i + base + 256 * j), le = *(const f32x4*)(a.lv_e + base + 256 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sii += mi[j][e] * mi[j][e];
            see += me[j][e] * me[j][e];
            const float l1 = li[e] + a.lv_shift, l2 = le[e] + a.lv_shift;
            kli += 1.0f + l1 - mi[j][e] * mi[j][e] - expf(l1);
            kle += 1.0f + l2 - me[j][e] * me[j][e] - expf(l2);
        }
    }
    const float ni = sqrtf(wave_sum(sii)), ne = sqrtf(wave_sum(see));
    kli = wave_sum(kli);
    kle = wave_sum(kle);
    // F.normalize (x / max(||x||, 1e-12)), then F.cosine_similarity of the normalised rows (each again divided by
    // max(its norm, 1e-8)): ucf_train.py:75-77
    const float ri = 1.0f / fmaxf(ni, 1e-12f), re = 1.0f / fmaxf(ne, 1e-12f);
    float s2i = 0.f, s2e = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            mi[j][e] *= ri;
            me[j][e] *= re;
            s2i += mi[j][e] * mi[j][e];
            s2e += me[j][e] * me[j][e];
        }
    const float qi = 1.0f / fmaxf(sqrtf(wave_sum(s2i)), 1e-8f), qe = 1.0f / fmaxf(sqrtf(wave_sum(s2e)), 1e-8f);
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) dot += (mi[j][e] * qi) * (me[j][e] * qe);
    dot = wave_sum(dot);
    if (lane == 0) {
        float* p = a.part + (size_t)row * 4;
        p[0] = 1.0f - dot;
        p[1] = fabsf(ni - ne);
        p[2] = kli;
        p[3] = kle;
    }
}

// F.binary_cross_entropy's clamp of a logarithm at -100, NaN kept: fmaxf(NaN, -100) is -100, which turned the NaN score of a video
// (a length <= 0, a k beyond T, a NaN logit in its prefix) into a finite classification loss
__device__ __forceinline__ float bce_log(float x) {
    const float l = logf(x);
    return l < -100.f ? -100.f : l;
}

// ONE workgroup: fixed-order sums of the partials -> out[8] = classification, reg, cos, norm, kl, kl_image, kl_event, total
struct LossFinishArgs {
    const float* inst;           // [B] instance scores
    const float* targets;        // [B] 1 = abnormal (1 - labels[:, 0]), loss.py:20
    const float* part;           // [rows][4]
    float* out;                  // [8]
    int B, rows;
    float lambda_reg, lambda_kl;
};
__global__ __launch_bounds__(256) void iefvad_loss_finish_kernel(LossFinishArgs a) {
    __shared__ double red[5][256];
    const int t = threadIdx.x;
    double acc[5] = {0, 0, 0, 0, 0};
    for (int v = t; v < a.B; v += 256) {
        const float p = a.inst[v], y = a.targets[v];
        const float lp = bce_log(p), lq = bce_log(1.0f - p);
        acc[0] += (double)(-(y * lp + (1.0f - y) * lq));
    }
    // eight rows requested ahead, added in row order (the order of the one-row-at-a-time loop: same bits; that loop was 128 dependent
    // memory round trips per thread at the UCF batch, 46 us for 512 KB)
    int r = t;
    for (; r + 7 * 256 < a.rows; r += 8 * 256) {
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = *(const f32x4*)(a.part + (size_t)(r + 256 * u) * 4);
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[1 + j] += (double)v[u][j];
    }
    for (; r < a.rows; r += 256)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[1 + j] += (double)a.part[(size_t)r * 4 + j];
#pragma unroll
    for (int j = 0; j < 5; ++j) red[j][t] = acc[j];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s)
#pragma unroll
            for (int j = 0; j < 5; ++j) red[j][t] += red[j][t + s];
        __syncthreads();
    }
    if (t == 0) {
        const double cls = red[0][0] / a.B;
        const double nr = a.rows > 0 ? (double)a.rows : 1.0;       // rows == 0: the classification term alone was asked for
        const double lcos = red[1][0] / nr, lnorm = red[2][0] / nr;
        const double n = nr * IEF_D;
        const double kli = -0.5 * red[3][0] / n, kle = -0.5 * red[4][0] / n;
        a.out[0] = (float)cls;
        a.out[1] = (float)(lcos + lnorm);
        a.out[2] = (float)lcos;
        a.out[3] = (float)lnorm;
        a.out[4] = (float)(kli + kle);
        a.out[5] = (float)kli;
        a.out[6] = (float)kle;
        a.out[7] = (float)(cls + a.lambda_reg * (lcos + lnorm) + a.lambda_kl * (kli + kle));
    }
}

// ---- backward of the loss head ------------------------------------------------------------------------------------------
// d total / d logits: one workgroup per video.  p = top-k mean as in the forward; BCE'(p) as torch's binary_cross_entropy
// backward evaluates it, (p - y) / max((1 - p) p, 1e-12); each of the k selected snippets gets sigma'(x) / k of it.
__global__ __launch_bounds__(256) void iefvad_mil_topk_grad_kernel(const float* logits, const int* lengths, const float* targets,
                                                                   float* d_logits, int T, float scale_over_B, const float* scale_dev) {
    __shared__ float s[LOSS_T];
    __shared__ float w[4];
    const int v = blockIdx.x, t = threadIdx.x;
    const int len_raw = lengths[v];
    const int len = len_raw < 0 ? 0 : (len_raw > T ? T : len_raw);
    const int k = len_raw / 16 + 1;
    const float x = (t < len) ? 1.0f / (1.0f + expf(-logits[(size_t)v * T + t])) : -1.0f;
    s[t] = x;
    __syncthreads();
    int rank = 0;
    for (int u = 0; u < T; ++u) rank += topk_before(s[u], u, x, t);
    const bool sel = t < len && rank < k;
    float part = sel ? x : 0.f;
    part = wave_sum(part);
    if ((t & 63) == 0) w[t >> 6] = part;
    __syncthreads();
    const float p = (k <= len) ? ((w[0] + w[1]) + (w[2] + w[3])) / (float)k : __builtin_nanf("");
    const float y = targets[v];
    const float sc = scale_dev ? scale_over_B * scale_dev[0] : scale_over_B;
    const float dp = (p - y) / fmaxf((1.0f - p) * p, 1e-12f) * sc;
    d_logits[(size_t)v * T + t] = sel ? dp * (x * (1.0f - x)) / (float)k : 0.f;
}

// d total / d (mu_i, mu_e, logvar_i, logvar_e): one wavefront per row.
//   cosine term  (1/R) (1 - cos):  d/da = -(b^ - cos a^) / |a|   (a^ = a / |a|; F.normalize then F.cosine_similarity, clamps inactive)
//   norm term    (1/R) ||a| - |b||: d/da = sign(|a| - |b|) a^
//   KL           -0.5 / (R D) sum(1 + l - mu^2 - e^l): d/dmu = mu / (R D), d/dlogvar = -0.5 (1 - e^l) / (R D)
struct LossRowGradArgs {
    const float* mu_i; const float* mu_e; const float* lv_i; const float* lv_e;     // [rows, 768]
    float* d_mu_i; float* d_mu_e; float* d_lv_i; float* d_lv_e;                     // [rows, 768], nullable each
    int rows;
    float lv_shift, lambda_reg, lambda_kl, scale;
    const float* scale_dev;      // nullable: the upstream gradient as a device scalar (multiplies `scale`; no host read of it)
};
__global__ __launch_bounds__(256) void iefvad_loss_rows_grad_kernel(LossRowGradArgs a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const size_t base = (size_t)row * IEF_D + 4 * lane;
    f32x4 mi[3], me[3];
    float sii = 0.f, see = 0.f, sie = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        mi[j] = *(const f32x4*)(a.mu_i + base + 256 * j);
        me[j] = *(const f32x4*)(a.mu_e + base + 256 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sii += mi[j][e] * mi[j][e];
            see += me[j][e] * me[j][e];
            sie += mi[j][e] * me[j][e];
        }
    }
    // F.normalize (x / max(|x|, 1e-12)) then F.cosine_similarity (each factor / max(its norm, 1e-8)), differentiated WITH their
    // clamp branches, so that a zero row gets what autograd gives it (a 1e20-scale value: meaningless, but the same)
    // Not covered: a nonzero row whose norm is below 1e-19.  Its squares are fp32 subnormals, and in the second clamp's branch
    // (hi <= 1e-8) this formula differs from torch's fp64 autograd by 1.3e-2 relative there (tests/test_gpu_loss_units.py leaves
    // such rows out; the heads' rows have norms of order 1 to 10).
    const float rni = sqrtf(wave_sum(sii)), rne = sqrtf(wave_sum(see));
    const float ni = fmaxf(rni, 1e-12f), ne = fmaxf(rne, 1e-12f);
    const float hi = rni / ni, he = rne / ne;                       // norms of the normalised rows: 1, or |x| 1e12 below the clamp
    const float qi = fmaxf(hi, 1e-8f), qe = fmaxf(he, 1e-8f);
    const float dh = wave_sum(sie) / (ni * ne);                     // u_i . u_e
    const float cs = dh / (qi * qe);
    const float al = 1.0f / (qi * qe);
    const float bi = hi > 1e-8f ? cs / (hi * qi) : 0.f, be = he > 1e-8f ? cs / (he * qe) : 0.f;
    // d cos / d a = c1 u_e + c2 u_i (u = normalised row), through the Jacobian of the normalisation
    float c1i, c2i, c1e, c2e;
    if (rni > 1e-12f) { c1i = al / rni; c2i = -(bi + al * dh - bi * hi * hi) / rni; } else { c1i = al * 1e12f; c2i = -bi * 1e12f; }
    if (rne > 1e-12f) { c1e = al / rne; c2e = -(be + al * dh - be * he * he) / rne; } else { c1e = al * 1e12f; c2e = -be * 1e12f; }
    const float invR = (a.scale_dev ? a.scale * a.scale_dev[0] : a.scale) / (float)a.rows, invRD = invR / (float)IEF_D;
    const float sg = rni > rne ? 1.f : (rni < rne ? -1.f : 0.f);
    const float cr = a.lambda_reg * invR, ck = a.lambda_kl * invRD;
    const float gni = rni > 0.f ? sg / rni : 0.f, gne = rne > 0.f ? -sg / rne : 0.f;      // d | |a| - |b| |: torch.norm's backward is 0 at 0
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        f32x4 gi, ge;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ui = mi[j][e] / ni, ue = me[j][e] / ne;
            gi[e] = cr * (-(c1i * ue + c2i * ui) + gni * mi[j][e]) + ck * mi[j][e];
            ge[e] = cr * (-(c1e * ui + c2e * ue) + gne * me[j][e]) + ck * me[j][e];
        }
        if (a.d_mu_i) *(f32x4*)(a.d_mu_i + base + 256 * j) = gi;
        if (a.d_mu_e) *(f32x4*)(a.d_mu_e + base + 256 * j) = ge;
        if (a.d_lv_i) {
            const f32x4 l = *(const f32x4*)(a.lv_i + base + 256 * j);
            f32x4 g;
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = -0.5f * ck * (1.0f - expf(l[e] + a.lv_shift));
            *(f32x4*)(a.d_lv_i + base + 256 * j) = g;
        }
        if (a.d_lv_e) {
            const f32x4 l = *(const f32x4*)(a.lv_e + base + 256 * j);
            f32x4 g;
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = -0.5f * ck * (1.0f - expf(l[e] + a.lv_shift));
            *(f32x4*)(a.d_lv_e + base + 256 * j) = g;
        }
    }
}

// ---- optimiser step: torch.optim.AdamW as the trainers construct it (/root/reference/train/ucf_train.py:28, xd_train.py:25:
// lr from the arguments, betas (0.9, 0.999), eps 1e-8, weight_decay 0.01, no amsgrad), single-tensor form, torch's operation order:
//   p *= 1 - lr wd;  m = lerp(m, g, 1 - b1);  v = b2 v + ((1 - b2) g) g;  p += -(lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
// Every scalar (1 - lr wd, 1 - b1, 1 - b2, lr / (1 - b1^t), sqrt(1 - b2^t)) is formed on the HOST in double and rounded to fp32
// once, as torch forms them in Python floats before they meet the fp32 tensors (1.0f - 0.999f would be 0.00099998713, torch
// multiplies by fp32(0.001) = 0.0010000000475).
struct AdamWArgs {
    float* p; const float* g; float* m; float* v;
    size_t n;
    float decay, w1, beta2, w2, step_size, bc2_sqrt, eps;
};
__global__ __launch_bounds__(256) void iefvad_adamw_kernel(AdamWArgs a) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (size_t)gridDim.x * blockDim.x) {
        const float g = a.g[i];
        float p = a.p[i];
        p = p * a.decay;                                                           // mul_(1 - lr * weight_decay)
        const float m = a.m[i] + a.w1 * (g - a.m[i]);                              // lerp_(grad, 1 - beta1)
        const float v = a.beta2 * a.v[i] + (a.w2 * g) * g;                         // mul_(beta2).addcmul_(grad, grad, value = 1 - beta2):
                                                                                   // addcmul forms (value grad) grad, finite up to |g| 1.8e20
        const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
        a.m[i] = m;
        a.v[i] = v;
        a.p[i] = p - a.step_size * (m / denom);                                    // addcdiv_(exp_avg, denom, value = -step_size)
    }
}

// The same update for MANY tensors in one launch (iefvad_adamw_step_multi): the reference's model has 78 parameter tensors, 46 of them
// 768-element vectors, and one launch each was 0.40 ms of a 30 ms training step for 0.13 ms worth of memory traffic.  `table` is a
// DEVICE array; a workgroup owns ADAMW_CHUNK consecutive elements of one tensor and finds it by bisection over first_chunk.
#define ADAMW_CHUNK 4096
struct AdamWMultiArgs {
    const iefvad_adamw_tensor* table;
    int count;
    float decay, w1, beta2, w2, step_size, bc2_sqrt, eps;
};
__global__ __launch_bounds__(256) void iefvad_adamw_multi_kernel(AdamWMultiArgs a) {
    const unsigned long long chunk = blockIdx.x;
    int lo = 0, hi = a.count - 1;
    while (lo < hi) {                                       // the last tensor whose first_chunk <= chunk
        const int mid = (lo + hi + 1) >> 1;
        if (a.table[mid].first_chunk <= chunk) lo = mid; else hi = mid - 1;
    }
    const iefvad_adamw_tensor t = a.table[lo];
    const size_t i0 = (size_t)(chunk - t.first_chunk) * ADAMW_CHUNK;
    const size_t i1 = i0 + ADAMW_CHUNK < t.n ? i0 + ADAMW_CHUNK : (size_t)t.n;
    for (size_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const float g = t.grad[i];
        float p = t.param[i];
        p = p * a.decay;
        const float m = t.exp_avg[i] + a.w1 * (g - t.exp_avg[i]);
        const float v = a.beta2 * t.exp_avg_sq[i] + (a.w2 * g) * g;
        const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
        t.exp_avg[i] = m;
        t.exp_avg_sq[i] = v;
        t.param[i] = p - a.step_size * (m / denom);
    }
}

// The optimiser step (reference utils/runner.py:162-180: clip_grad_norm_, Adam, the KL rule of the learning rate, plus this build's bookkeeping of the
// loss statistics and the copies of the weights it keeps current), written once for its three forms:
//   bg_adam_step + bg_adapt_lr  (bg_ppo.hip: sqnorm_kernel, adam_kernel, adapt_lr_kernel; the supervised updates, the first step after a restore)
//   bg_optimizer_step           (bg_ppo.hip: optimizer_step_kernel, 64 workgroups that each take the norm of the whole gradient)
//   bg_update_tail              (bg_tail.hip: tail_adam_kernel, 256 workgroups that add the norm slots of tail_sums_kernel)
// A fused kernel is how the squared norm reaches its workgroups, then opt_block_total, clip_coef, opt_slice, opt_last_ticket; the host side of both is
// opt_args_fill.  A change to the step (an epsilon rule, weight decay, another learning-rate rule) is made here.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "bg_common.h"
#include "bg_reduce.h"

// ------------------------------------------------------------------ the copies of a weight matrix that the fused launches keep current while they
// update the parameters (bg_param_mirror, include/booster_gym_amd.h): element (r, c) of the [rows][cols] matrix, new value pn
constexpr int OPT_MAX_MIRRORS = 16;
struct ParamMirrors { int n; bg_param_mirror m[OPT_MAX_MIRRORS]; };

__device__ __forceinline__ void bg_mirror_write(const bg_param_mirror& mm, int r, int c, float pn) {
    if (mm.transpose < 2) {
        mm.dst[mm.transpose ? (size_t)c * mm.ld + r : (size_t)r * mm.ld + c] = pn;
    } else {
        // the three bf16 planes of bg_mlp_split_weights (hi + mid + lo == pn exactly), [n][ld / 32][3][32] with the chained kernels' k order inside
        // a 32-chunk; 2: planes of W (n = r, k = c), 3: planes of W^T (n = c, k = r)
        const int n = mm.transpose == 2 ? r : c, k = mm.transpose == 2 ? c : r;
        const unsigned u = __float_as_uint(pn);
        const float r1 = pn - __uint_as_float(u & 0xffff0000u);
        const unsigned v = __float_as_uint(r1);
        const float r2 = r1 - __uint_as_float(v & 0xffff0000u);
        const int kin = k & 31, s = kin >> 3, hh = (kin >> 2) & 1, q = kin & 3;
        unsigned short* d = reinterpret_cast<unsigned short*>(mm.dst) + ((size_t)n * (mm.ld >> 5) + (k >> 5)) * 96 + (s >> 1) * 16 + hh * 8 + (s & 1) * 4 + q;
        d[0] = (unsigned short)(u >> 16);
        d[32] = (unsigned short)(v >> 16);
        d[64] = (unsigned short)(__float_as_uint(r2) >> 16);
        if (mm.pad > 0) {  // ... and the planes of -W, mm.pad uint16 behind (bg_mlp_split_weights_pm's layout)
            d += mm.pad;
            d[0] = (unsigned short)((u >> 16) ^ 0x8000u);
            d[32] = (unsigned short)((v >> 16) ^ 0x8000u);
            d[64] = (unsigned short)((__float_as_uint(r2) >> 16) ^ 0x8000u);
        }
    }
}
// host-side check of a descriptor against a flat buffer of n floats
inline bool bg_mirror_ok(const bg_param_mirror& q, int64_t n) {
    if (!q.dst || q.rows <= 0 || q.cols <= 0 || q.offset < 0 || (int64_t)q.offset + (int64_t)q.rows * q.cols > n || q.transpose < 0 || q.transpose > 3) return false;
    if (q.ld < ((q.transpose & 1) ? q.rows : q.cols)) return false;
    if (q.transpose >= 2 && ((q.ld & 31) != 0 || ((uintptr_t)q.dst & 15) != 0)) return false;
    return true;
}

// ------------------------------------------------------------------ the step
constexpr int OPT_THREADS = 1024;  // threads of a workgroup of either fused kernel (16 waves: opt_block_total)
// what the fused kernels take from their entry points (bg_optimizer_step's and bg_update_tail's arguments from `n` to `lr_max`, the step as its two
// bias corrections)
struct OptArgs {
    int n; float *p, *g, *m, *v, *lr_dev; float bc1, bc2_sqrt, beta1, beta2, eps, max_norm;
    double* grad_logstd; int ls_off, ls_n;
    double *stats, *stats_acc, *stats_last; int n_stats, kl_index; float kl_count, desired_kl, lr_min, lr_max;
};

// Adam's bias corrections of step `step` (1-based): 1 - beta1^step and sqrt(1 - beta2^step)
inline void adam_bias_corrections(float beta1, float beta2, int step, float& bc1, float& bc2_sqrt) {
    bc1 = 1.0f - powf(beta1, (float)step);
    bc2_sqrt = sqrtf(1.0f - powf(beta2, (float)step));
}
// the factor on every gradient element, from the squared global norm (torch.nn.utils.clip_grad_norm_); max_norm <= 0: no clipping
__device__ __forceinline__ float clip_coef(double sqnorm, float max_norm) {
    const float total = (float)sqrt(sqnorm);
    return max_norm > 0.f ? fminf(max_norm / (total + 1e-6f), 1.0f) : 1.0f;
}
// the KL rule (reference utils/runner.py:174-180): the learning rate behind a step whose mean KL divergence was `kl`
__device__ __forceinline__ float kl_rule(float lr, float kl, float desired, float lr_min, float lr_max) {
    if (kl > desired * 2.0f) return fmaxf(lr_min, lr / 1.5f);
    if (kl < desired / 2.0f) return fminf(lr_max, lr * 1.5f);
    return lr;
}
// element i: gradient times coef into the moments, the new parameter stored and returned
__device__ __forceinline__ float adam_element(float* p, const float* g, float* m, float* v, int i, float coef, float step_size, float beta1, float beta2,
                                              float bc2_sqrt, float eps) {
    const float gi = g[i] * coef;
    const float mi = beta1 * m[i] + (1.0f - beta1) * gi;
    const float vi = beta2 * v[i] + (1.0f - beta2) * gi * gi;
    m[i] = mi; v[i] = vi;
    const float pn = p[i] - step_size * mi / (sqrtf(vi) / bc2_sqrt + eps);
    p[i] = pn;
    return pn;
}
// The total over a workgroup of OPT_THREADS threads' float64 partial sums, in every thread: a butterfly per wave, then one thread adds the 16 wave
// totals in wave order.  The same order in every workgroup: workgroups that start from the same partial sums hold the same bits.
__device__ __forceinline__ double opt_block_total(double acc) {
    __shared__ double s_part[OPT_THREADS / 64];
    __shared__ double s_total;
    const int t = threadIdx.x;
    acc = wave_sum_d(acc);
    if ((t & 63) == 0) s_part[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        double tot = 0.0;
        for (int w = 0; w < OPT_THREADS / 64; w++) tot += s_part[w];
        s_total = tot;
    }
    __syncthreads();
    return s_total;
}
// clip + Adam on slice blockIdx.x of G, every new parameter inside one of the mirrored matrices also written to that matrix's copy
__device__ __forceinline__ void opt_slice(const OptArgs& o, const ParamMirrors& mir, int G, float lr, float coef) {
    const float step_size = lr / o.bc1;
    const int per = (o.n + G - 1) / G, i0 = blockIdx.x * per, i1 = min(o.n, i0 + per);
    for (int i = i0 + threadIdx.x; i < i1; i += OPT_THREADS) {
        const float pn = adam_element(o.p, o.g, o.m, o.v, i, coef, step_size, o.beta1, o.beta2, o.bc2_sqrt, o.eps);
        for (int k = 0; k < mir.n; k++) {
            const bg_param_mirror& mm = mir.m[k];
            const int j = i - mm.offset;
            if (j >= 0 && j < mm.rows * mm.cols) {
                const int r = j / mm.cols, c = j - r * mm.cols;
                bg_mirror_write(mm, r, c, pn);
            }
        }
    }
}
// Behind the slice: the last workgroup to take a ticket applies the KL rule to the learning rate (`lr`: its value at the kernel's start, which every
// thread has read), publishes / accumulates the loss statistics and zeroes the accumulators and the ticket for the next mini-epoch.
__device__ __forceinline__ void opt_last_ticket(const OptArgs& o, float lr, unsigned* ticket) {
    __syncthreads();
    if (threadIdx.x != 0) return;
    // No fence in front of the ticket: the last workgroup needs nothing the others WROTE, only that they have READ lr and the log-std gradient --
    // and those loads have returned (their values went into every thread's arithmetic in front of the barrier above).  An agent-scope
    // release here writes back the XCD's whole L2, once per workgroup.
    const unsigned k = atomicAdd(ticket, 1u);
    if (k != gridDim.x - 1u) return;
    if (o.stats) {
        *o.lr_dev = kl_rule(lr, (float)(o.stats[o.kl_index] / (double)o.kl_count), o.desired_kl, o.lr_min, o.lr_max);
        for (int j = 0; j < o.n_stats; j++) {
            const double sj = o.stats[j];
            o.stats_last[j] = sj;
            o.stats_acc[j] += sj;
            o.stats[j] = 0.0;
        }
    }
    if (o.grad_logstd) for (int j = 0; j < o.ls_n; j++) o.grad_logstd[j] = 0.0;
    *ticket = 0u;
}

// host side of the two fused entry points: the checks they share (`who` prefixes the messages), the mirrors and the kernels' arguments
inline int opt_args_fill(const char* who, int32_t n, float* params, float* grads, float* exp_avg, float* exp_avg_sq, float* lr_device, int32_t step,
                         float beta1, float beta2, float eps, float max_grad_norm, double* grad_logstd, int32_t ls_off, int32_t ls_n, double* stats,
                         double* stats_acc, double* stats_last, int32_t n_stats, int32_t kl_index, float kl_count, float desired_kl, float lr_min,
                         float lr_max, const uint32_t* ticket, const bg_param_mirror* mirrors, int32_t n_mirrors, OptArgs& o, ParamMirrors& mir) {
    if (n <= 0 || !params || !grads || !exp_avg || !exp_avg_sq || !lr_device || !ticket || step < 1) return bg_fail(who, -1, "bad argument");
    if (grad_logstd && (ls_n <= 0 || ls_n > OPT_THREADS || ls_off < 0 || ls_off + ls_n > n)) return bg_fail(who, -1, "log-std slice outside the buffer");
    if (stats && (!stats_acc || !stats_last || n_stats <= 0 || kl_index < 0 || kl_index >= n_stats || !(kl_count > 0.f)))
        return bg_fail(who, -1, "statistics arguments");
    if (n_mirrors < 0 || n_mirrors > OPT_MAX_MIRRORS || (n_mirrors > 0 && !mirrors)) return bg_fail(who, -1, "at most 16 weight mirrors");
    mir.n = n_mirrors;
    for (int k = 0; k < n_mirrors; k++) {
        if (!bg_mirror_ok(mirrors[k], n)) return bg_fail(who, -1, "bad weight mirror");
        mir.m[k] = mirrors[k];
    }
    o.n = n; o.p = params; o.g = grads; o.m = exp_avg; o.v = exp_avg_sq; o.lr_dev = lr_device;
    adam_bias_corrections(beta1, beta2, step, o.bc1, o.bc2_sqrt);
    o.beta1 = beta1; o.beta2 = beta2; o.eps = eps; o.max_norm = max_grad_norm;
    o.grad_logstd = grad_logstd; o.ls_off = ls_off; o.ls_n = ls_n;
    o.stats = stats; o.stats_acc = stats_acc; o.stats_last = stats_last; o.n_stats = n_stats; o.kl_index = kl_index; o.kl_count = kl_count;
    o.desired_kl = desired_kl; o.lr_min = lr_min; o.lr_max = lr_max;
    return 0;
}

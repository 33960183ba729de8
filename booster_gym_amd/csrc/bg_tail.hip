// The tail of a mini-epoch (reference utils/runner.py:162-180: loss.backward()'s last sums, clip_grad_norm_, optimizer.step(), the KL rule) as TWO
// launches behind the main weight-gradient kernel, where rounds 2-3 had three around it: reduce_group_kernel (bg_head.hip) in front of the weight
// gradients, mlp_wgrad_group_finish_kernel (bg_wgrad.hip) behind them and optimizer_step_kernel (bg_ppo.hip), 5.3 + 5.6 + 20.4 us of kernels and three
// launch-to-launch gaps of 7-8 us on the critical path of every mini-epoch (tools/timeline.py on the round-3 trace).
//
//   tail_sums_kernel   one workgroup per block of either kernel's work -- the weight gradients' fixed-order sums over their slices and the deferred
//                      reductions (head / bias gradients, float64 loss statistics), through the block functions the two kernels named above run
//                      themselves (bg_wgrad.h, bg_reduce.h): the gradients are the same bits -- and, while the finished values are in registers, the block's sum
//                      of their squares (float64) into one slot of norm_partial.  Every element of the flat gradient except the log-std's is
//                      written by exactly one block, so the slots add up to the squared global norm;
//   tail_adam_kernel   every workgroup adds the slots in slot order (+ the log-std's squares): the same total everywhere, deterministic, no
//                      atomics -- optimizer_step_kernel spends half of its 20 us re-reading the whole gradient in each of its 64 workgroups for this --
//                      then clip + Adam + weight mirrors on its slice, the KL rule and the statistics' bookkeeping by the last workgroup to take a ticket.
// (First form of this file: ONE launch with two grid-wide barriers between the three phases.  Correct, and 35 us per mini-epoch SLOWER than the three
// launches it replaced (update 21.7 against 21.0 ms, tools/ab_env.sh): an agent-scope fence on this part writes back and invalidates the XCD's whole
// L2, 256 workgroups did that twice each while the others were reading.  Launch boundaries are the cheaper grid barrier.)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "bg_optim.h"
#include "bg_reduce.h"
#include "bg_wgrad.h"

namespace {
// ADAM_GRID: one workgroup per CU.  Every workgroup adds the ~2,900 norm slots itself (23 KB out of L2, the same order everywhere: the same total), so
// the count changes no bit; with the weight copies the launch writes since round 6 (bf16 planes of W, -W, W^T, -W^T: up to 12 two-byte stores per
// parameter, the transposed ones a cache line each) 256 workgroups instead of 64 are worth 0.1 ms per iteration (21.82-21.90 against 21.95-22.00 ms).
constexpr int ADAM_GRID = 256, TAIL_THREADS = 256, TAIL_MAX_ITEMS = BG_TAIL_MAX_BLOCKS;
#define BG_STR_(x) #x
#define BG_STR(x) BG_STR_(x)  // the value of a macro as text

// one workgroup per block of the weight gradients' finish (wgrad_finish_block, bg_wgrad.h) or of the deferred reductions (reduce_block, bg_reduce.h)
__global__ __launch_bounds__(TAIL_THREADS) void tail_sums_kernel(WgradGroup wg, ReduceGroup rg, int rg_blocks, double* __restrict__ norm_partial) {
    __shared__ f32x4 sm4[16][16];
    __shared__ float smf[16][17];
    __shared__ double sd[4];
    const int item = blockIdx.x;
    double q = item < rg_blocks ? reduce_block(rg, item, smf, sd) : wgrad_finish_block(wg, item - rg_blocks, sm4);
    // the writers are threads 0..15 = the first lanes of wave 0: a butterfly over that wave (zeros elsewhere) in a fixed order
    if (threadIdx.x < 64) {
        q = wave_sum_d(q);
        if (threadIdx.x == 0) norm_partial[item] = q;
    }
}

// (the norm from the slots; the rest of the step: bg_optim.h)
__global__ __launch_bounds__(OPT_THREADS) void tail_adam_kernel(OptArgs o, ParamMirrors mir, const double* __restrict__ norm_partial, int n_partial,
                                                                unsigned* __restrict__ ticket) {
    const int t = threadIdx.x;
    const float lr = *o.lr_dev;  // read by every thread before this workgroup takes its ticket
    // the log-std gradient arrives in float64 from the heads: put it into the flat buffer (every workgroup writes the same values) ...
    double acc = 0.0;
    if (o.grad_logstd && t < o.ls_n) {
        const float gl = (float)o.grad_logstd[t];
        o.g[o.ls_off + t] = gl;
        acc = (double)gl * (double)gl;  // ... and its share of the norm, the only elements tail_sums_kernel has not squared
    }
    for (int i = t; i < n_partial; i += OPT_THREADS) acc += norm_partial[i];
    opt_slice(o, mir, gridDim.x, lr, clip_coef(opt_block_total(acc), o.max_norm));
    opt_last_ticket(o, lr, ticket);
}
}  // namespace

// the work list of tail_sums_kernel from the two descriptor lists (shared by bg_update_tail and bg_update_tail_sums)
static int tail_sums_fill(const bg_wgrad_problem* wgrad, int32_t n_wgrad, const bg_reduce_problem* reduce, int32_t n_reduce, WgradGroup& wg, ReduceGroup& rg,
                          int& blocks, int& fin, const char* who) {
    wg.np = 0;
    int wgs = 0;
    fin = 0;
    if (n_wgrad > 0) {
        const int rc = bg_wgrad_group_fill(wgrad, n_wgrad, wg, wgs, fin, who);
        if (rc) return rc;
    }
    if (const int rc = reduce_group_fill(reduce, n_reduce, 0, rg, blocks, who)) return rc;
    if (blocks + fin > TAIL_MAX_ITEMS) return bg_set_error(-4, "bg_update_tail: more than " BG_STR(BG_TAIL_MAX_BLOCKS) " blocks of sums (norm_scratch holds one slot per block)");
    return 0;
}
// Launch (1) of bg_update_tail alone: the sums.  For the ranks of a multi-GPU job, whose gradient is averaged over the ranks between the sums and the
// optimiser: bg_update_tail_sums, the all-reduce, bg_optimizer_step (which takes the norm of the AVERAGED gradient itself).
extern "C" int bg_update_tail_sums(const bg_wgrad_problem* wgrad, int32_t n_wgrad, const bg_reduce_problem* reduce, int32_t n_reduce, double* norm_scratch,
                                   void* stream) {
    if (!norm_scratch) return bg_set_error(-1, "bg_update_tail_sums: bad argument");
    WgradGroup wg;
    ReduceGroup rg;
    int blocks = 0, fin = 0;
    const int rc = tail_sums_fill(wgrad, n_wgrad, reduce, n_reduce, wg, rg, blocks, fin, "bg_update_tail_sums");
    if (rc) return rc;
    if (blocks + fin > 0) hipLaunchKernelGGL(tail_sums_kernel, dim3(blocks + fin), dim3(TAIL_THREADS), 0, (hipStream_t)stream, wg, rg, blocks, norm_scratch);
    if (hipGetLastError() != hipSuccess) return bg_set_error(-2, "bg_update_tail_sums: launch failed");
    return 0;
}
extern "C" int bg_update_tail(const bg_wgrad_problem* wgrad, int32_t n_wgrad, const bg_reduce_problem* reduce, int32_t n_reduce, int32_t n, float* params,
                              float* grads, float* exp_avg, float* exp_avg_sq, float* lr_device, int32_t step, float beta1, float beta2, float eps,
                              float max_grad_norm, double* grad_logstd, int32_t ls_off, int32_t ls_n, double* stats, double* stats_acc, double* stats_last,
                              int32_t n_stats, int32_t kl_index, float kl_count, float desired_kl, float lr_min, float lr_max, uint32_t* sync,
                              double* norm_scratch, const bg_param_mirror* mirrors, int32_t n_mirrors, void* stream) {
    if (!norm_scratch) return bg_set_error(-1, "bg_update_tail: bad argument");
    OptArgs o;
    ParamMirrors mir;
    if (const int rc = opt_args_fill("bg_update_tail", n, params, grads, exp_avg, exp_avg_sq, lr_device, step, beta1, beta2, eps, max_grad_norm, grad_logstd,
                                     ls_off, ls_n, stats, stats_acc, stats_last, n_stats, kl_index, kl_count, desired_kl, lr_min, lr_max, sync, mirrors,
                                     n_mirrors, o, mir))
        return rc;
    WgradGroup wg;
    ReduceGroup rg;
    int blocks = 0, fin = 0;
    if (const int rc = tail_sums_fill(wgrad, n_wgrad, reduce, n_reduce, wg, rg, blocks, fin, "bg_update_tail")) return rc;
    if (blocks + fin > 0) hipLaunchKernelGGL(tail_sums_kernel, dim3(blocks + fin), dim3(TAIL_THREADS), 0, (hipStream_t)stream, wg, rg, blocks, norm_scratch);
    hipLaunchKernelGGL(tail_adam_kernel, dim3(ADAM_GRID), dim3(OPT_THREADS), 0, (hipStream_t)stream, o, mir, (const double*)norm_scratch, blocks + fin, (unsigned*)sync);
    if (hipGetLastError() != hipSuccess) return bg_set_error(-2, "bg_update_tail: launch failed");
    return 0;
}

// The deferred fixed-order reductions (include/booster_gym_amd.h: bg_reduce_problem): the sums over the workgroups' records that the head kernels and
// the backward layers leave (head: output-layer weight / bias gradients, last hidden layer's bias gradient, float64 loss statistics; backward layer:
// the bias gradient of the layer below), for up to 8 descriptors in one launch.  ONE block, run by reduce_group_kernel (bg_head.hip: bg_reduce_group and
// the heads' immediate forms) and by tail_sums_kernel (bg_tail.hip: the default plan), so that every plan of the update adds the same terms in the same
// order.  Workgroups [begin_k, begin_k + nblk_k) serve descriptor k: 16 outputs x 16 record slices each, followed by one workgroup per float64
// statistic of the descriptor.
#pragma once
#include "bg_common.h"

namespace {
constexpr int RG_MAX = 8;
struct ReduceGroup { int np; int begin[RG_MAX]; bg_reduce_problem p[RG_MAX]; };

__device__ __forceinline__ double wave_sum_d(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// Block blk of the group.  An output block: out[i] = sum_g partial[g][i] for 16 outputs; returns (threads 0..15: the others 0) the square of the value
// this thread wrote.  A statistics block: row ks of the stat-major [n_stat][groups] block added up in a fixed order, then ONE atomic: ks < n_ls goes to
// grad_logstd[ks] (+ entropy_coef: d(entropy.mean())/dlogstd = 1), the rest to stats[ks - n_ls]; a statistic whose stat_skip bit is set is skipped.
// (One workgroup PER statistic: a single workgroup walking the 17 statistics of the actor head one after the other -- a load, a butterfly and two
// barriers each -- was a 66 us launch on the actor's chain of every mini-epoch.)
__device__ __forceinline__ double reduce_block(const ReduceGroup& grp, int blk, float (*sm)[17], double* sd) {
    int k = 0;
#pragma unroll
    for (int j = 1; j < RG_MAX; j++)
        if (j < grp.np && blk >= grp.begin[j]) k = j;
    const bg_reduce_problem& pr = grp.p[k];
    const int b = blk - grp.begin[k], nsum = (pr.n_out + 15) / 16;
    if (b >= nsum) {
        const int ks = b - nsum;
        if ((pr.stat_skip >> ks) & 1u) return 0.0;
        const double* sp = reinterpret_cast<const double*>(pr.partial + pr.stat_base);
        double s = 0.0;
#pragma unroll 4
        for (int g = threadIdx.x; g < pr.groups; g += 256) s += sp[(size_t)ks * pr.groups + g];
        s = wave_sum_d(s);
        if ((threadIdx.x & 63) == 0) sd[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            const double v = sd[0] + sd[1] + sd[2] + sd[3];
            if (ks < pr.n_ls) atomicAdd(&pr.grad_logstd[ks], v + pr.entropy_coef);
            else atomicAdd(&pr.stats[ks - pr.n_ls], v);
        }
        return 0.0;  // (statistics are not gradients; the log-std's gradient is squared by tail_adam_kernel, once every statistic has been added)
    }
    const int o = threadIdx.x & 15, gs = threadIdx.x >> 4, i = b * 16 + o;
    float s = 0.f;
    if (i < pr.n_out) {
#pragma unroll 8  // 8 loads in flight: the 48 dependent adds of a thread were a chain of 48 L2 round trips
        for (int g = gs; g < pr.groups; g += 16) s += pr.partial[(size_t)g * pr.record + i];
    }
    sm[gs][o] = s;
    __syncthreads();
    if (threadIdx.x < 16 && i < pr.n_out) {
        float v = 0.f;
        for (int j = 0; j < 16; j++) v += sm[j][o];
        if (i < pr.n[0]) pr.out[0][i] = v;
        else if (i < pr.n[0] + pr.n[1]) pr.out[1][i - pr.n[0]] = v;
        else pr.out[2][i - pr.n[0] - pr.n[1]] = v;
        return (double)v * (double)v;
    }
    return 0.0;
}

// validation of `lo` (0 or 1) to 8 descriptors + the work list of their blocks (`blocks`: their count); `who` prefixes the error messages
inline int reduce_group_fill(const bg_reduce_problem* problems, int32_t count, int lo, ReduceGroup& grp, int& blocks, const char* who) {
    if (count < lo || count > RG_MAX || (count > 0 && !problems)) return bg_fail(who, -1, lo ? "1 to 8 reductions" : "at most 8 reductions");
    grp.np = count;
    blocks = 0;
    for (int k = 0; k < count; k++) {
        const bg_reduce_problem& q = problems[k];
        if (!q.partial || q.groups <= 0 || q.record <= 0 || q.n_out <= 0 || q.n_out > q.record || !q.out[0] || q.n[0] <= 0 ||
            q.n[0] + q.n[1] + q.n[2] != q.n_out || (q.n[1] > 0 && !q.out[1]) || (q.n[2] > 0 && !q.out[2]))
            return bg_fail(who, -1, "bad reduction descriptor");
        if (q.n_stat < 0 || q.n_stat > 32 || (q.n_stat > 0 && (!q.stats || (q.n_ls > 0 && !q.grad_logstd) || (q.stat_base & 1))))
            return bg_fail(who, -1, "bad statistics descriptor");
        grp.begin[k] = blocks;
        grp.p[k] = q;
        blocks += (q.n_out + 15) / 16 + q.n_stat;
    }
    for (int k = count; k < RG_MAX; k++) grp.begin[k] = blocks;
    return 0;
}
}  // namespace

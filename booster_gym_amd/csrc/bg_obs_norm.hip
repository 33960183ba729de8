// Empirical observation normalisation (algorithm.empirical_normalization; rsl_rl's EmpiricalNormalization restated in utils/obs_norm.py): the two
// launches the feature adds beside the hot path.  Neither is part of an env-step, sampling, chain, head or tail kernel.
//
//   bg_obs_moments     column sums and sums of squares of the iteration's T x N observation rows, float64, in a fixed order (no floating-point
//                      atomics): what the ranks exchange and what the host merges into the running mean / variance once per PPO iteration.
//   bg_obs_normalize   dst = (src - mean) * inv_std on a block of columns, zero in the destination's padded columns: where rows enter a network
//                      (the rollout's scratch for bg_actor_sample*, the update's _critic_in / _actor_in, the forward-ahead's row ranges, the
//                      symmetry loss's mirrored rows).
//
// This file is compiled without the value-changing FP relaxations of the other translation units and with -ffp-contract=off (Makefile): the
// normalised value is the fp32 subtract rounded, then the fp32 multiply rounded, in every call site, so the rollout and the update produce the
// same bits for the same row.

#include "bg_common.h"

// ------------------------------------------------------------------ moments
// The matrix is [rows][cols_a + cols_b], given as two column blocks with their own row strides (the observation block and the privileged block of
// the experience buffer: no concatenated copy).  A wave reads one row at a time, its 64 lanes on 64 consecutive columns (whole lines), NK chunks of
// 64 columns per row and RU rows in flight; wave w of workgroup g takes rows (g * 4 + w) * RU + j, j < RU, then strides by grid * 4 * RU.  A lane
// owns its columns: it adds the rows it meets in ascending order into float64 registers, so there is no cross-lane step at all.  Per workgroup ONE
// LDS step: waves 1 .. 3 leave their sums in LDS, wave 0 adds them in wave order and writes the workgroup's record [2][C] to `scratch`; the second
// launch adds the records in a fixed order (obs_moments_finish_kernel).  The grid is a function of `rows` alone (never of the device), so the same
// input gives the same bits anywhere.
constexpr int MOM_WAVES = 4;
constexpr int MOM_BLOCK = MOM_WAVES * 64;
constexpr int MOM_MAX_COLS_A = 512, MOM_MAX_COLS_B = 201;

struct MomArgs {
    const float *a, *b;
    int cols_a, cols_b;
    size_t stride_a, stride_b;
    int rows;
};

template <int NK, int RU>
__global__ __launch_bounds__(MOM_BLOCK) void obs_moments_kernel(MomArgs q, double* __restrict__ scratch) {
    __shared__ double s_part[MOM_WAVES - 1][2][NK * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C = q.cols_a + q.cols_b;
    double s[NK], ss[NK];
    const float* base[NK];  // this lane's column k * 64 + lane: its address in row 0 and its row stride; nullptr beyond the last column
    size_t stride[NK];
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const int c = k * 64 + lane;
        s[k] = 0.0; ss[k] = 0.0;
        base[k] = c < q.cols_a ? q.a + c : c < C ? q.b + (c - q.cols_a) : nullptr;
        stride[k] = c < q.cols_a ? q.stride_a : q.stride_b;
    }
    const int step = (int)gridDim.x * MOM_WAVES * RU;
    for (int r0 = ((int)blockIdx.x * MOM_WAVES + wave) * RU; r0 < q.rows; r0 += step) {
        float x[RU][NK];
#pragma unroll
        for (int j = 0; j < RU; j++)
#pragma unroll
            for (int k = 0; k < NK; k++) x[j][k] = (base[k] && r0 + j < q.rows) ? base[k][(size_t)(r0 + j) * stride[k]] : 0.f;
#pragma unroll
        for (int j = 0; j < RU; j++)
#pragma unroll
            for (int k = 0; k < NK; k++) {
                const double v = (double)x[j][k];
                s[k] += v;
                ss[k] += v * v;
            }
    }
    if (wave > 0) {
#pragma unroll
        for (int k = 0; k < NK; k++) {
            s_part[wave - 1][0][k * 64 + lane] = s[k];
            s_part[wave - 1][1][k * 64 + lane] = ss[k];
        }
    }
    __syncthreads();
    if (wave == 0) {
        double* rec = scratch + (size_t)blockIdx.x * 2 * C;
#pragma unroll
        for (int k = 0; k < NK; k++) {
            const int c = k * 64 + lane;
            for (int w = 0; w < MOM_WAVES - 1; w++) {
                s[k] += s_part[w][0][c];
                ss[k] += s_part[w][1][c];
            }
            if (c < C) {
                rec[c] = s[k];
                rec[C + c] = ss[k];
            }
        }
    }
}

// out[i] = the records' element i added in a fixed order: i < C the sums, C <= i < 2C the sums of squares.  A workgroup owns 16 outputs (16
// consecutive doubles of a record: one 128-byte line per load); 16 segments of threads each add a contiguous run of ceil(groups / 16) records in
// slot order, eight loads in flight, and thread (output, segment 0) adds the 16 segment sums in segment order through LDS.
constexpr int FIN_OUT = 16, FIN_SEG = 16;
__global__ __launch_bounds__(FIN_OUT * FIN_SEG) void obs_moments_finish_kernel(int groups, int C, const double* __restrict__ scratch, double* __restrict__ sum,
                                                                               double* __restrict__ sumsq) {
    __shared__ double s_seg[FIN_SEG][FIN_OUT];
    const int o = threadIdx.x % FIN_OUT, seg = threadIdx.x / FIN_OUT;
    const int i = blockIdx.x * FIN_OUT + o;
    const int per = (groups + FIN_SEG - 1) / FIN_SEG;
    const int g0 = seg * per, g1 = min(groups, g0 + per);
    double acc = 0.0;
    if (i < 2 * C) {
        const double* p = scratch + i;
        const size_t rec = (size_t)2 * C;
        int g = g0;
        for (; g + 8 <= g1; g += 8) {
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = p[(size_t)(g + k) * rec];
#pragma unroll
            for (int k = 0; k < 8; k++) acc += v[k];
        }
        for (; g < g1; g++) acc += p[(size_t)g * rec];
    }
    s_seg[seg][o] = acc;
    __syncthreads();
    if (seg == 0 && i < 2 * C) {
        double t = s_seg[0][o];
        for (int k = 1; k < FIN_SEG; k++) t += s_seg[k][o];
        if (i < C) sum[i] = t;
        else sumsq[i - C] = t;
    }
}

static int moments_groups(int rows) {
    int g = (rows + 31) / 32;
    return g < 1 ? 1 : g > BG_OBS_MOMENTS_MAX_GROUPS ? BG_OBS_MOMENTS_MAX_GROUPS : g;
}

extern "C" int bg_obs_moments(int32_t rows, const float* a, int32_t cols_a, int32_t stride_a, const float* b, int32_t cols_b, int32_t stride_b, double* sum,
                              double* sumsq, double* scratch, void* stream) {
    if (rows <= 0 || !a || !sum || !sumsq || !scratch) return bg_set_error(-1, "bg_obs_moments: bad argument");
    if (cols_a <= 0 || cols_a > MOM_MAX_COLS_A || cols_b < 0 || cols_b > MOM_MAX_COLS_B)
        return bg_set_error(-1, "bg_obs_moments: unsupported columns (first block 1 to 512, second block 0 to 201)");
    if (stride_a < cols_a || (cols_b > 0 && (!b || stride_b < cols_b))) return bg_set_error(-1, "bg_obs_moments: bad argument (a block's row stride is below its columns)");
    const int C = cols_a + cols_b, groups = moments_groups(rows);
    const MomArgs q{a, cols_b > 0 ? b : nullptr, cols_a, cols_b, (size_t)stride_a, (size_t)stride_b, rows};
    const dim3 grid((unsigned)groups), block(MOM_BLOCK);
    hipStream_t st = (hipStream_t)stream;
    // (chunks of 64 columns per row) x (rows in flight per wave): 8 to 12 loads in flight per lane
    if (C <= 64) hipLaunchKernelGGL((obs_moments_kernel<1, 8>), grid, block, 0, st, q, scratch);
    else if (C <= 128) hipLaunchKernelGGL((obs_moments_kernel<2, 4>), grid, block, 0, st, q, scratch);
    else if (C <= 256) hipLaunchKernelGGL((obs_moments_kernel<4, 2>), grid, block, 0, st, q, scratch);
    else if (C <= 384) hipLaunchKernelGGL((obs_moments_kernel<6, 2>), grid, block, 0, st, q, scratch);
    else if (C <= 512) hipLaunchKernelGGL((obs_moments_kernel<8, 1>), grid, block, 0, st, q, scratch);
    else hipLaunchKernelGGL((obs_moments_kernel<12, 1>), grid, block, 0, st, q, scratch);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(obs_moments_finish_kernel, dim3((2 * C + FIN_OUT - 1) / FIN_OUT), dim3(FIN_OUT * FIN_SEG), 0, st, groups, C, (const double*)scratch, sum, sumsq);
    HIP_OK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ normalise
// One thread per destination element of the [rows][dst_cols] block, a row's elements on consecutive lanes (as bg_obs_stack): the destination goes
// out in whole lines.  Columns [cols, dst_cols) are the zero padding of a network input.
constexpr int NORM_BLOCK = 256;
__global__ __launch_bounds__(NORM_BLOCK) void obs_normalize_kernel(unsigned total, unsigned cols, unsigned dst_cols, const float* __restrict__ src, size_t src_stride,
                                                                   float* __restrict__ dst, size_t dst_stride, const float* __restrict__ mean,
                                                                   const float* __restrict__ inv_std) {
    const unsigned t = blockIdx.x * NORM_BLOCK + threadIdx.x;
    if (t >= total) return;
    const unsigned r = t / dst_cols, c = t - r * dst_cols;
    float y = 0.f;
    if (c < cols) {
        const float d = src[(size_t)r * src_stride + c] - mean[c];
        y = d * inv_std[c];
    }
    dst[(size_t)r * dst_stride + c] = y;
}

extern "C" int bg_obs_normalize(int32_t rows, int32_t cols, const float* src, int32_t src_stride, float* dst, int32_t dst_cols, int32_t dst_stride,
                                const float* mean, const float* inv_std, int32_t col0, void* stream) {
    if (rows <= 0 || !src || !dst || !mean || !inv_std) return bg_set_error(-1, "bg_obs_normalize: bad argument");
    if (cols <= 0 || col0 < 0 || col0 + cols > MOM_MAX_COLS_A + MOM_MAX_COLS_B || dst_cols > 512)
        return bg_set_error(-1, "bg_obs_normalize: unsupported columns (col0 + cols at most 713, dst_cols at most 512)");
    if (src_stride < cols || dst_cols < cols || dst_stride < dst_cols) return bg_set_error(-1, "bg_obs_normalize: bad argument (cols <= src_stride, cols <= dst_cols <= dst_stride)");
    const size_t total = (size_t)rows * dst_cols;
    if (total >= (1ull << 31)) return bg_set_error(-1, "bg_obs_normalize: bad argument (rows x dst_cols must stay below 2^31)");
    const float *se = src + ((size_t)rows - 1) * src_stride + cols, *de = dst + ((size_t)rows - 1) * dst_stride + dst_cols;
    if (src < de && dst < se) return bg_set_error(-1, "bg_obs_normalize: src and dst overlap");
    hipLaunchKernelGGL(obs_normalize_kernel, dim3((unsigned)((total + NORM_BLOCK - 1) / NORM_BLOCK)), dim3(NORM_BLOCK), 0, (hipStream_t)stream, (unsigned)total,
                       (unsigned)cols, (unsigned)dst_cols, src, (size_t)src_stride, dst, (size_t)dst_stride, mean + col0, inv_std + col0);
    HIP_OK(hipGetLastError());
    return 0;
}

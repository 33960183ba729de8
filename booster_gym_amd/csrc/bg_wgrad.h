// Descriptors of the grouped weight-gradient launch, shared by bg_wgrad.hip (fp32 MFMA) and bg_wgrad_split.hip (split bf16 MFMA), and the block of
// their fixed-order finish over the slices, shared by mlp_wgrad_group_finish_kernel (bg_wgrad.hip) and tail_sums_kernel (bg_tail.hip).
#pragma once
#include "bg_common.h"

constexpr int WG_MAX_PROBLEMS = 8;
struct WgradProblem {
    const float* G; const float* A; float* P; float* dW;
    int M, Cout, Cin, Cin_real, tci, ntile_ci, ntiles, tw, slices, wg_begin, fin_begin, n4;
};
struct WgradGroup { int np; WgradProblem p[WG_MAX_PROBLEMS]; };

namespace {
// dW[co][ci < Cin_real] = sum over slices of P[s][co][ci], slices added in a fixed order; block b of the group's finish: 16 float4 columns x 16 slice
// groups per workgroup (the slice loop is a chain of dependent-address loads: many short chains, not few long ones)
// returns (threads 0..15: the others 0) the squares of the values this thread wrote
__device__ __forceinline__ double wgrad_finish_block(const WgradGroup& grp, int b, f32x4 (*sm)[16]) {
    int k = 0;
#pragma unroll
    for (int j = 1; j < WG_MAX_PROBLEMS; j++)
        if (j < grp.np && b >= grp.p[j].fin_begin) k = j;
    const WgradProblem& pr = grp.p[k];
    const int c = threadIdx.x & 15, sg = threadIdx.x >> 4, e4 = (b - pr.fin_begin) * 16 + c, n4 = pr.n4, S = pr.slices, Cin = pr.Cin, Cin_real = pr.Cin_real;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (e4 < n4)
        for (int s = sg; s < S; s += 16) acc += *reinterpret_cast<const f32x4*>(pr.P + ((size_t)s * n4 + e4) * 4);
    sm[sg][c] = acc;
    __syncthreads();
    if (sg == 0 && e4 < n4) {
        f32x4 v = sm[0][c];
#pragma unroll
        for (int j = 1; j < 16; j++) v += sm[j][c];
        const int row = (e4 * 4) / Cin, col = (e4 * 4) % Cin;
        double q = 0.0;
        if (Cin_real == Cin) {
            *reinterpret_cast<f32x4*>(pr.dW + (size_t)row * Cin + col) = v;
            q = (double)v[0] * (double)v[0] + (double)v[1] * (double)v[1] + (double)v[2] * (double)v[2] + (double)v[3] * (double)v[3];
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (col + j < Cin_real) { pr.dW[(size_t)row * Cin_real + col + j] = v[j]; q += (double)v[j] * (double)v[j]; }
        }
        return q;
    }
    return 0.0;
}
}  // namespace

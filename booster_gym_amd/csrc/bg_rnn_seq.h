// What the sequence kernels of the two recurrent cells share (bg_gru.hip, bg_lstm.hip), written once: the rows a workgroup owns, the 32-MFMA step and
// the two ways a lane fetches W_hh.  A workgroup (4 waves) owns MR = 16 envs, keeps their state tile [16][H + 4] in LDS and walks the T steps itself; the
// MFMA operands are bg_actor_mlp.hip's `layer`'s (v_mfma_f32_16x16x4_f32: A from LDS, one ds_read_b128 feeds 4 MFMAs; B = W_hh from global memory / L2).
// Each of the two files includes this under its own build flags (bg_lstm.o: no packed fp32 forms).
// The gate arithmetic, the state-tile loops, the backward GEMM's flat loop and the LSTM's gate gradients stay per kernel: under -fassociative-math the
// order of their float operations depends on the code around them, and as functions of this header they compiled to other instructions
// (profiles/rnn_seq_isa.txt).  Internal to those two translation units; gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include "bg_common.h"

namespace {

constexpr int MR = 16;  // envs per workgroup

// 32 MFMAs: the k-chunk of 128 columns at AROW (this lane's row of an LDS tile, at its k-group) times the 8 weight vectors WV, even k-groups of 16 into
// ACC0 and odd ones into ACC1 (two chains: neither waits on its own dependent latency)
#define BG_RNN_MFMA32(ACC0, ACC1, AROW, WV)                                                                                            \
    _Pragma("unroll") for (int u = 0; u < 8; u += 2) {                                                                                 \
        const f32x4 a0 = *reinterpret_cast<const f32x4*>((AROW) + 16 * u), a1 = *reinterpret_cast<const f32x4*>((AROW) + 16 * (u + 1)); \
        ACC0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, WV[u].x, ACC0, 0, 0, 0);                                                      \
        ACC1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, WV[u + 1].x, ACC1, 0, 0, 0);                                                  \
        ACC0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, WV[u].y, ACC0, 0, 0, 0);                                                      \
        ACC1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, WV[u + 1].y, ACC1, 0, 0, 0);                                                  \
        ACC0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, WV[u].z, ACC0, 0, 0, 0);                                                      \
        ACC1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, WV[u + 1].z, ACC1, 0, 0, 0);                                                  \
        ACC0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, WV[u].w, ACC0, 0, 0, 0);                                                      \
        ACC1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, WV[u + 1].w, ACC1, 0, 0, 0);                                                  \
    }

// Forward, along k: the 8 weight vectors of gate g, column tile j, k-chunk c for the lane (r = lane & 15, kg = lane >> 4): row g H + 16 j + r of W_hh,
// columns 128 c + 16 u + 4 kg + [0, 4): 16-byte loads
template <int H>
__device__ __forceinline__ void seq_fetch_along_k(f32x4 (&w)[8], const float* __restrict__ W, int g, int j, int c, int r, int kg) {
    const float* wrow = W + (size_t)(g * H + j * 16 + r) * H + c * 128 + 4 * kg;
#pragma unroll
    for (int u = 0; u < 8; u++) w[u] = *reinterpret_cast<const f32x4*>(wrow + 16 * u);
}

// Backward, down the rows: the 32 weights of column tile j, k-chunk c for the lane: W_hh[row0 + 128 c + 16 u + 4 kg + e][16 j + r], u = 0 .. 7,
// e = 0 .. 3, scalar loads (16 lanes = one 64-byte segment).  row0: the first row of the pass (the LSTM's wide form runs K in two passes).
template <int H>
__device__ __forceinline__ void seq_fetch_down_rows(f32x4 (&w)[8], const float* __restrict__ W, int row0, int j, int c, int r, int kg) {
    const float* wcol = W + (size_t)(row0 + c * 128 + 4 * kg) * H + j * 16 + r;
#pragma unroll
    for (int u = 0; u < 8; u++) w[u] = f32x4{wcol[(size_t)(16 * u) * H], wcol[(size_t)(16 * u + 1) * H], wcol[(size_t)(16 * u + 2) * H], wcol[(size_t)(16 * u + 3) * H]};
}

}  // namespace

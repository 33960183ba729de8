// The recurrence of a GRU student's update (utils/distill.py, distillation.student_memory; rsl_rl's recurrent student of `Distillation`, which
// back-propagates through the T = horizon_length steps of an iteration from the stored hidden state): bg_gru_sequence_forward and
// bg_gru_sequence_backward, ONE launch each for all T steps, fp32 MFMA, gfx950 only.
//
// The x-side of the cell, gi = X W_ih^T + b_ih, has no dependence on the state and runs on all T N rows at once (bg_mlp_layer_forward).  What is
// left is sequential in t and independent over the envs, so a workgroup (4 waves) owns 16 envs, keeps their state tile [16][H + 4] in LDS and walks
// the steps itself: no launch and no trip of the state through memory between steps.  Operands as in bg_actor_mlp.hip's `layer`
// (v_mfma_f32_16x16x4_f32, exact fp32):
//     A[i = lane & 15][k = lane >> 4]  the state (forward) / dgh (backward) from LDS, one ds_read_b128 feeds 4 MFMAs
//     B[k = lane >> 4][j = lane & 15]  W_hh from global memory / L2: 196 kB at H = 128, 786 kB at H = 256, more than LDS holds beside the tiles
//     C/D: column j = lane & 15, row i = (lane >> 4) * 4 + reg
// Forward: gh = h_prev W_hh^T + b_hh.  A wave owns the column tiles wave, wave + 4, ... of H and accumulates the r, z and n tile of those columns (rows
// j, H + j, 2H + j of W_hh: 16-byte loads along k), so the gate arithmetic (bg_gru.h, the rollout's) runs in its registers; the new state goes to the
// second LDS tile, which the next step reads.  Three weight buffers rotate: the loads of the next gate's 128-wide k-chunk fly under this one's 32 MFMAs.
// Backward: carry = dh z + dgh W_hh, K = 3H; the contraction runs over the ROWS of W_hh, so B is read with scalar loads (16 lanes = one 64-byte
// segment), double-buffered per k-chunk as `layer` does.  Both write every value they produce once and add in a fixed order: deterministic.
// A step is a chain of dependent round trips (operands from memory, barrier, MFMAs, gates, barrier), one wave per SIMD, so what a step reads from
// memory is requested in front of MFMAs that do not need it: the forward loads a tile's gi in front of the tile's MFMAs, the backward loads step
// t - 1's dh_ext, gates and h_prev into registers in front of step t's GEMM.
#include <hip/hip_runtime.h>

#include "bg_common.h"
#include "bg_gru.h"

namespace {

constexpr int MR = 16;  // envs per workgroup

#define BG_GRU_MFMA32(ACC0, ACC1, AROW, WV)                                                                                            \
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

// The forward recurrence of the 16 envs [16 block, 16 block + 16) of one problem: the one body of bg_gru_sequence_forward's kernel (block = blockIdx.x)
// and of the grouped launch's (block = the workgroup's place among its problem's).
template <int H>
__device__ __forceinline__ void gru_sequence_forward_body(float (&tile)[2][MR * (H + 4)], unsigned block, int T, int N, const float* __restrict__ gi, const float* __restrict__ h0,
                                                          const uint8_t* __restrict__ reset, const float* __restrict__ W, const float* __restrict__ bh,
                                                          float* __restrict__ h_prev, float* __restrict__ h, float* __restrict__ gates) {
    constexpr int LDH = H + 4, TPW = H / 64, CPT = H / 128;  // row stride of the state tiles; column tiles per wave; 128-wide k-chunks
    const int r0 = block * MR, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, kg = lane >> 4;
    for (int k = threadIdx.x; k < MR * H; k += blockDim.x) {
        const int rr = k / H, c = k - rr * H, row = r0 + rr;
        tile[0][rr * LDH + c] = (h0 && row < N) ? h0[(size_t)row * H + c] : 0.f;
    }
    __syncthreads();
    // the 8 weight vectors of gate g, column tile j, k-chunk c for this lane: row g H + 16 j + r of W_hh, columns 128 c + 16 u + 4 kg + [0, 4)
    auto fetch = [&](f32x4 (&w)[8], int g, int j, int c) {
        const float* wrow = W + (size_t)(g * H + j * 16 + r) * H + c * 128 + 4 * kg;
#pragma unroll
        for (int u = 0; u < 8; u++) w[u] = *reinterpret_cast<const f32x4*>(wrow + 16 * u);
    };
    int cur = 0;
    for (int t = 0; t < T; t++) {
        float *hc = tile[cur], *hn = tile[cur ^ 1];
        const size_t tn = (size_t)t * N;
        // the state entering the step: zero behind a reset; it is the operand of W_hh's weight gradient
        for (int k = threadIdx.x; k < MR * H; k += blockDim.x) {
            const int rr = k / H, c = k - rr * H, row = r0 + rr;
            if (row < N) {
                float v = hc[rr * LDH + c];
                if (reset && reset[tn + row]) hc[rr * LDH + c] = v = 0.f;
                h_prev[(tn + row) * H + c] = v;
            }
        }
        __syncthreads();
        f32x4 w0[8], w1[8], w2[8];
        fetch(w0, 0, wave, 0);
        f32x4 acc[3][2];
#pragma unroll 1
        for (int jt = 0; jt < TPW; jt++) {
            const int j = wave + 4 * jt, col = j * 16 + r;
            float giv[4][3] = {};  // the tile's x-side pre-activations, in flight under its MFMAs
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int row = r0 + kg * 4 + q;
                if (row < N) {
                    const float* g = gi + (tn + row) * (3 * H) + col;
                    giv[q][0] = g[0]; giv[q][1] = g[H]; giv[q][2] = g[2 * H];
                }
            }
#pragma unroll 1
            for (int c = 0; c < CPT; c++) {
                if (c == 0) {
#pragma unroll
                    for (int g = 0; g < 3; g++) {
                        const float b = bh[g * H + col];
                        acc[g][0] = f32x4{b, b, b, b};
                        acc[g][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                }
                const float* arow = hc + r * LDH + c * 128 + 4 * kg;
                fetch(w1, 1, j, c);
                BG_GRU_MFMA32(acc[0][0], acc[0][1], arow, w0)
                fetch(w2, 2, j, c);
                BG_GRU_MFMA32(acc[1][0], acc[1][1], arow, w1)
                if (c + 1 < CPT) fetch(w0, 0, j, c + 1);
                else if (jt + 1 < TPW) fetch(w0, 0, j + 4, 0);
                BG_GRU_MFMA32(acc[2][0], acc[2][1], arow, w2)
            }
            // gh = acc0 + acc1 first, then gru_gates adds gi: (acc0 + acc1) + gi, the association bg_gru_sequence_forward has always run.  Under this
            // file's -fassociative-math the optimiser is free to split the sum as (acc0 + gi) + acc1, and whether it does depends on the code around
            // the body (it did once the body was a function); a sum without the reassociation flag cannot be taken apart
            f32x4 ghr, ghz, ghn;
            {
#pragma clang fp reassociate(off)
                ghr = acc[0][0] + acc[0][1];
                ghz = acc[1][0] + acc[1][1];
                ghn = acc[2][0] + acc[2][1];
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int rr = kg * 4 + q, row = r0 + rr;
                const bg::GruGates g = bg::gru_gates(giv[q][0], giv[q][1], giv[q][2], ghr[q], ghz[q], ghn[q], hc[rr * LDH + col]);
                hn[rr * LDH + col] = g.h;
                if (row < N) {
                    h[(tn + row) * H + col] = g.h;
                    float* go = gates + (tn + row) * (4 * H) + col;
                    go[0] = g.r; go[H] = g.z; go[2 * H] = g.n; go[3 * H] = ghn[q];
                }
            }
        }
        __syncthreads();
        cur ^= 1;
    }
}

template <int H>
__global__ __launch_bounds__(256) void gru_sequence_forward_kernel(int T, int N, const float* __restrict__ gi, const float* __restrict__ h0,
                                                                   const uint8_t* __restrict__ reset, const float* __restrict__ W, const float* __restrict__ bh,
                                                                   float* __restrict__ h_prev, float* __restrict__ h, float* __restrict__ gates) {
    __shared__ __attribute__((aligned(16))) float tile[2][MR * (H + 4)];
    gru_sequence_forward_body<H>(tile, blockIdx.x, T, N, gi, h0, reset, W, bh, h_prev, h, gates);
}

// ... and the backward recurrence of those envs, likewise the one body of both launches.
template <int H>
__device__ __forceinline__ void gru_sequence_backward_body(float (&gt)[MR * (3 * H + 4)], float (&carry)[MR * (H + 4)], unsigned block, int T, int N, const float* __restrict__ dh_ext, const float* __restrict__ gates,
                                                           const float* __restrict__ h_prev, const uint8_t* __restrict__ reset,
                                                           const float* __restrict__ W, float* __restrict__ dgi, float* __restrict__ dgh,
                                                           float* __restrict__ dh0) {
    constexpr int LDH = H + 4, LDG = 3 * H + 4, TPW = H / 64, CPT = 3 * H / 128;
    const int r0 = block * MR, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, kg = lane >> 4;
    for (int k = threadIdx.x; k < MR * LDH; k += blockDim.x) carry[k] = 0.f;
    __syncthreads();
    // the 32 weights of column tile j, k-chunk c for this lane: W_hh[128 c + 16 u + 4 kg + e][16 j + r], u = 0 .. 7, e = 0 .. 3
    auto fetch = [&](f32x4 (&w)[8], int s) {
        const int j = wave + 4 * (s / CPT), c = s % CPT;
        const float* wcol = W + (size_t)(c * 128 + 4 * kg) * H + j * 16 + r;
#pragma unroll
        for (int u = 0; u < 8; u++) w[u] = f32x4{wcol[(size_t)(16 * u) * H], wcol[(size_t)(16 * u + 1) * H], wcol[(size_t)(16 * u + 2) * H], wcol[(size_t)(16 * u + 3) * H]};
    };
    // a thread's elements of a step's operands (dh_ext, r, z, n, gh_n, h_prev): those of step t - 1 are loaded under step t's GEMM
    constexpr int EPT = MR * H / 256;
    float in[EPT][6];
    auto load = [&](int t) {
        const size_t tn = (size_t)t * N;
#pragma unroll
        for (int e = 0; e < EPT; e++) {
            const int k = threadIdx.x + 256 * e, rr = k / H, c = k - rr * H, row = r0 + rr;
            if (row < N) {
                const float* g = gates + (tn + row) * (4 * H) + c;
                in[e][0] = dh_ext[(tn + row) * H + c]; in[e][1] = g[0]; in[e][2] = g[H]; in[e][3] = g[2 * H]; in[e][4] = g[3 * H];
                in[e][5] = h_prev[(tn + row) * H + c];
            }
        }
    };
    load(T - 1);
    for (int t = T - 1; t >= 0; t--) {
        const size_t tn = (size_t)t * N;
#pragma unroll
        for (int e = 0; e < EPT; e++) {
            const int k = threadIdx.x + 256 * e, rr = k / H, c = k - rr * H, row = r0 + rr;
            float dr_pre = 0.f, dz_pre = 0.f, dn_pre = 0.f, dn_r = 0.f, dhz = 0.f;
            if (row < N) {
                // dn = dh (1 - z), dz = dh (h_prev - n), dn_pre = dn (1 - n^2), dz_pre = dz z (1 - z), dr_pre = dn_pre gh_n r (1 - r), each product and each
                // fused multiply-add written out and nothing left to contract or reassociate: which of the equivalent forms the compiler picks depends
                // on the code around the body.  These are the forms bg_gru_sequence_backward has always run (x (1 - y) as x - y x in one rounding), so
                // the single launch keeps its bits and the grouped one has the same
#pragma clang fp contract(off) reassociate(off)
                const float dh = in[e][0] + carry[rr * LDH + c];
                const float gr = in[e][1], gz = in[e][2], gn = in[e][3], ghn = in[e][4], hp = in[e][5];
                const float dn = __builtin_fmaf(-gz, dh, dh);
                dhz = gz * dh;
                dn_pre = __builtin_fmaf(-(gn * gn), dn, dn);
                dz_pre = __builtin_fmaf(-gz, dhz, dhz) * (hp - gn);
                dn_r = dn_pre * gr;
                dr_pre = __builtin_fmaf(-gr, dn_r, dn_r) * ghn;
                float *a = dgi + (tn + row) * (3 * H) + c, *b = dgh + (tn + row) * (3 * H) + c;
                a[0] = dr_pre; a[H] = dz_pre; a[2 * H] = dn_pre;
                b[0] = dr_pre; b[H] = dz_pre; b[2 * H] = dn_r;
            }
            float* gl = gt + rr * LDG + c;
            gl[0] = dr_pre; gl[H] = dz_pre; gl[2 * H] = dn_r;
            carry[rr * LDH + c] = dhz;
        }
        __syncthreads();
        if (t > 0) load(t - 1);
        constexpr int steps = TPW * CPT;
        f32x4 cur[8], nxt[8] = {};
        fetch(cur, 0);
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
        for (int s = 0; s < steps; s++) {
            if (s + 1 < steps) fetch(nxt, s + 1);
            const int j = wave + 4 * (s / CPT), c = s % CPT;
            if (c == 0) acc0 = acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
            const float* arow = gt + r * LDG + c * 128 + 4 * kg;
            BG_GRU_MFMA32(acc0, acc1, arow, cur)
            if (c == CPT - 1) {
                const f32x4 v = acc0 + acc1;
                const int col = j * 16 + r;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int rr = kg * 4 + q, row = r0 + rr;
                    float x = carry[rr * LDH + col] + v[q];  // (this lane alone reads and writes the element in this phase)
                    if (row >= N || (reset && reset[tn + row])) x = 0.f;
                    carry[rr * LDH + col] = x;
                }
            }
#pragma unroll
            for (int u = 0; u < 8; u++) cur[u] = nxt[u];
        }
        __syncthreads();
    }
    if (dh0) {
        for (int k = threadIdx.x; k < MR * H; k += blockDim.x) {
            const int rr = k / H, c = k - rr * H, row = r0 + rr;
            if (row < N) dh0[(size_t)row * H + c] = carry[rr * LDH + c];
        }
    }
}

template <int H>
__global__ __launch_bounds__(256) void gru_sequence_backward_kernel(int T, int N, const float* __restrict__ dh_ext, const float* __restrict__ gates,
                                                                    const float* __restrict__ h_prev, const uint8_t* __restrict__ reset,
                                                                    const float* __restrict__ W, float* __restrict__ dgi, float* __restrict__ dgh,
                                                                    float* __restrict__ dh0) {
    __shared__ __attribute__((aligned(16))) float gt[MR * (3 * H + 4)];  // dgh of the step: the GEMM's A operand
    __shared__ __attribute__((aligned(16))) float carry[MR * (H + 4)];   // dh carried to the step below
    gru_sequence_backward_body<H>(gt, carry, blockIdx.x, T, N, dh_ext, gates, h_prev, reset, W, dgi, dgh, dh0);
}

// Several recurrences in ONE grid (bg_gru_sequence_forward_group / _backward_group).  A recurrence is a chain of dependent round trips on one wave per
// SIMD, so its time hardly depends on its number of envs, and two of them launched one after the other on one stream cost twice that.  Here a workgroup
// serves one problem through the bodies above (the outputs are the single launches' bit for bit), and the workgroups of the problems ALTERNATE in
// dispatch order: round r of the grid holds workgroup r of every problem that has one, so that the problems share the CUs from the first workgroups on
// (two workgroups fit a CU's LDS at every H; two forward waves fit a SIMD's registers, two backward ones do not).  The grouped backward kernel at
// H = 128 compiles to the whole register file with spills where the single one takes 356 registers: the runner issues the
// backward recurrences as single launches unless BG_GRU_GROUP=2.
constexpr int GROUP_MAX = BG_GRU_GROUP_MAX;
static_assert(GROUP_MAX == 4, "the group kernels select among four problems");

// The problem that workgroup b of such a grid serves, and in `local` its place among that problem's workgroups; nb[p]: the problems' workgroup counts.
// At most n segments of rounds over a constant set of unfinished problems.  -1 for a b outside the grid (the sum of nb).
__device__ __forceinline__ int group_block(int nb0, int nb1, int nb2, int nb3, int n, int b, int& local) {
    const int nb[GROUP_MAX] = {nb0, nb1, nb2, nb3};
    int r = 0, rem = b;
#pragma unroll
    for (int seg = 0; seg < GROUP_MAX; seg++) {
        int active = 0, next = 0x7fffffff;
#pragma unroll
        for (int p = 0; p < GROUP_MAX; p++) {
            if (p < n && nb[p] > r) {
                active++;
                next = min(next, nb[p]);
            }
        }
        if (active == 0) break;
        const int span = (next - r) * active;
        if (rem < span) {
            const int k = rem % active;  // the k-th unfinished problem, in ascending order
            int found = 0, seen = 0;
#pragma unroll
            for (int p = 0; p < GROUP_MAX; p++) {
                if (p < n && nb[p] > r) {
                    if (seen == k) found = p;
                    seen++;
                }
            }
            local = r + rem / active;
            return found;
        }
        rem -= span;
        r = next;
    }
    local = -1;
    return -1;
}

// Field F of problem p of the kernel's one argument (a ForwardGroup / BackwardGroup by value, at the start of the kernel-argument segment): read from
// that segment at a workgroup-uniform offset, a scalar load, so that the pointers live in scalar registers as the single kernels' arguments do
// (indexing the by-value argument with p makes the compiler copy it to private memory; selecting among the four problems keeps all of them live).
// This reads offset 0 of the segment: the struct must stay the grouped kernels' ONLY explicit argument, nothing may be placed in front of `g`.
#define BG_GRU_PICK(GROUP, F) (((const __attribute__((address_space(4))) GROUP*)__builtin_amdgcn_kernarg_segment_ptr())->p[p].F)

struct ForwardGroup {
    bg_gru_forward_problem p[GROUP_MAX];
    int nb[GROUP_MAX];
    int n;
};

struct BackwardGroup {
    bg_gru_backward_problem p[GROUP_MAX];
    int nb[GROUP_MAX];
    int n;
};
static_assert(offsetof(ForwardGroup, p) == 0 && offsetof(BackwardGroup, p) == 0, "BG_GRU_PICK reads the problems at the start of the kernel-argument segment");

template <int H>
__global__ __launch_bounds__(256) void gru_sequence_forward_group_kernel(const ForwardGroup g) {
    int local;
    const int p = group_block(g.nb[0], g.nb[1], g.nb[2], g.nb[3], g.n, blockIdx.x, local);
    if (p < 0) return;
#define PICK(F) BG_GRU_PICK(ForwardGroup, F)
    __shared__ __attribute__((aligned(16))) float tile[2][MR * (H + 4)];
    gru_sequence_forward_body<H>(tile, local, PICK(T), PICK(N), PICK(gi), PICK(h0), PICK(reset), PICK(W_hh), PICK(b_hh), PICK(h_prev), PICK(h), PICK(gates));
#undef PICK
}

template <int H>
__global__ __launch_bounds__(256) void gru_sequence_backward_group_kernel(const BackwardGroup g) {
    int local;
    const int p = group_block(g.nb[0], g.nb[1], g.nb[2], g.nb[3], g.n, blockIdx.x, local);
    if (p < 0) return;
#define PICK(F) BG_GRU_PICK(BackwardGroup, F)
    __shared__ __attribute__((aligned(16))) float gt[MR * (3 * H + 4)];  // dgh of the step: the GEMM's A operand
    __shared__ __attribute__((aligned(16))) float carry[MR * (H + 4)];   // dh carried to the step below
    gru_sequence_backward_body<H>(gt, carry, local, PICK(T), PICK(N), PICK(dh_ext), PICK(gates), PICK(h_prev), PICK(reset), PICK(W_hh), PICK(dgi), PICK(dgh), PICK(dh0));
#undef PICK
}

// The cell's two bias gradients of the PPO update (algorithm.rnn_hidden_size): the column sums of dgi and dgh [B][3H] as ONE launch that leaves one
// record [6H] = dgi's sums | dgh's per 128-row block, for a bg_reduce_problem of the update's deferred group to add up (bg_reduce.h).  Memory-bound: a
// lane owns one 16-byte column of the joined row [dgi row | dgh row] per 64-lane group (3 groups at H = 128, 6 at H = 256: a wave reads 1 KiB, or two
// 512-byte runs where a group straddles the two tensors), a wave the rows wave, wave + 4, ... of the block in ascending order, its loads of four rows
// in flight; the four waves' sums meet in LDS and are added in wave order: every term once, a fixed order, no atomics.
constexpr int BP_ROWS = 128;  // rows per workgroup = per record

template <int H>
__global__ __launch_bounds__(256) void gru_bias_partial_kernel(int B, const float* __restrict__ dgi, const float* __restrict__ dgh, float* __restrict__ records) {
    constexpr int C = 3 * H, C4 = C / 4, G = 2 * C4 / 64;
    static_assert(2 * C4 % 64 == 0, "");
    __shared__ f32x4 sm[4][2 * C4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r0 = blockIdx.x * BP_ROWS, r1 = min(r0 + BP_ROWS, B);  // (rows at or beyond B are never read)
    const float* src[G];
    f32x4 acc[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        const int v = 64 * g + lane;
        src[g] = v < C4 ? dgi + 4 * v : dgh + 4 * (v - C4);
        acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll 4
    for (int r = r0 + wave; r < r1; r += 4) {
#pragma unroll
        for (int g = 0; g < G; g++) acc[g] += *reinterpret_cast<const f32x4*>(src[g] + (size_t)r * C);
    }
#pragma unroll
    for (int g = 0; g < G; g++) sm[wave][64 * g + lane] = acc[g];
    __syncthreads();
    f32x4* rec = reinterpret_cast<f32x4*>(records + (size_t)blockIdx.x * 2 * C);
    for (int v = threadIdx.x; v < 2 * C4; v += 256) rec[v] = ((sm[0][v] + sm[1][v]) + sm[2][v]) + sm[3][v];
}

int check_shape(const char* who, int32_t T, int32_t N, int32_t H) {
    if (T <= 0 || N <= 0) return bg_fail(who, -1, "bad argument (T, N: at least 1)");
    if (H != 128 && H != 256) return bg_fail(who, -4, "unsupported H (128 or 256)");
    return 0;
}

}  // namespace

extern "C" int bg_gru_sequence_forward(int32_t T, int32_t N, int32_t H, const float* gi, const float* h0, const uint8_t* reset, const float* W_hh,
                                       const float* b_hh, float* h_prev, float* h, float* gates, void* stream) {
    const char* who = "bg_gru_sequence_forward";
    if (const int rc = check_shape(who, T, N, H)) return rc;
    if (!gi || !W_hh || !b_hh || !h_prev || !h || !gates) return bg_fail(who, -1, "bad argument");
    if (!aligned16(W_hh)) return bg_fail(who, -1, "W_hh must be 16-byte aligned");
    const dim3 grid((N + MR - 1) / MR), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (H == 128) hipLaunchKernelGGL(gru_sequence_forward_kernel<128>, grid, block, 0, st, T, N, gi, h0, reset, W_hh, b_hh, h_prev, h, gates);
    else hipLaunchKernelGGL(gru_sequence_forward_kernel<256>, grid, block, 0, st, T, N, gi, h0, reset, W_hh, b_hh, h_prev, h, gates);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_gru_sequence_backward(int32_t T, int32_t N, int32_t H, const float* dh_ext, const float* gates, const float* h_prev, const uint8_t* reset,
                                        const float* W_hh, float* dgi, float* dgh, float* dh0, void* stream) {
    const char* who = "bg_gru_sequence_backward";
    if (const int rc = check_shape(who, T, N, H)) return rc;
    if (!dh_ext || !gates || !h_prev || !W_hh || !dgi || !dgh) return bg_fail(who, -1, "bad argument");
    const dim3 grid((N + MR - 1) / MR), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (H == 128) hipLaunchKernelGGL(gru_sequence_backward_kernel<128>, grid, block, 0, st, T, N, dh_ext, gates, h_prev, reset, W_hh, dgi, dgh, dh0);
    else hipLaunchKernelGGL(gru_sequence_backward_kernel<256>, grid, block, 0, st, T, N, dh_ext, gates, h_prev, reset, W_hh, dgi, dgh, dh0);
    HIP_OK(hipGetLastError());
    return 0;
}

namespace {

// The checks both grouped entry points share, before any launch: 1 to GROUP_MAX problems of one supported H.
int check_group(const char* who, const void* problems, int32_t n_problems, int32_t H) {
    if (!problems || n_problems < 1) return bg_fail(who, -1, "bad argument (no problem)");
    if (n_problems > GROUP_MAX) return bg_fail(who, -1, "bad argument (more than 4 problems)");
    if (H != 128 && H != 256) return bg_fail(who, -4, "unsupported H (128 or 256)");
    return 0;
}

}  // namespace

extern "C" int bg_gru_sequence_forward_group(const bg_gru_forward_problem* problems, int32_t n_problems, int32_t H, void* stream) {
    const char* who = "bg_gru_sequence_forward_group";
    if (const int rc = check_group(who, problems, n_problems, H)) return rc;
    ForwardGroup g = {};
    int blocks = 0;
    for (int k = 0; k < n_problems; k++) {
        const bg_gru_forward_problem& q = problems[k];
        if (const int rc = check_shape(who, q.T, q.N, H)) return rc;
        if (!q.gi || !q.W_hh || !q.b_hh || !q.h_prev || !q.h || !q.gates) return bg_fail(who, -1, "bad argument (a null pointer)");
        if (!aligned16(q.W_hh)) return bg_fail(who, -1, "W_hh must be 16-byte aligned");
        g.p[k] = q;
        g.nb[k] = (q.N + MR - 1) / MR;
        blocks += g.nb[k];
    }
    g.n = n_problems;
    const dim3 grid(blocks), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (H == 128) hipLaunchKernelGGL(gru_sequence_forward_group_kernel<128>, grid, block, 0, st, g);
    else hipLaunchKernelGGL(gru_sequence_forward_group_kernel<256>, grid, block, 0, st, g);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_gru_sequence_backward_group(const bg_gru_backward_problem* problems, int32_t n_problems, int32_t H, void* stream) {
    const char* who = "bg_gru_sequence_backward_group";
    if (const int rc = check_group(who, problems, n_problems, H)) return rc;
    BackwardGroup g = {};
    int blocks = 0;
    for (int k = 0; k < n_problems; k++) {
        const bg_gru_backward_problem& q = problems[k];
        if (const int rc = check_shape(who, q.T, q.N, H)) return rc;
        if (!q.dh_ext || !q.gates || !q.h_prev || !q.W_hh || !q.dgi || !q.dgh) return bg_fail(who, -1, "bad argument (a null pointer)");
        if (!aligned16(q.W_hh)) return bg_fail(who, -1, "W_hh must be 16-byte aligned");
        g.p[k] = q;
        g.nb[k] = (q.N + MR - 1) / MR;
        blocks += g.nb[k];
    }
    g.n = n_problems;
    const dim3 grid(blocks), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (H == 128) hipLaunchKernelGGL(gru_sequence_backward_group_kernel<128>, grid, block, 0, st, g);
    else hipLaunchKernelGGL(gru_sequence_backward_group_kernel<256>, grid, block, 0, st, g);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_gru_bias_partial(int32_t B, int32_t H, const float* dgi, const float* dgh, float* records, void* stream) {
    const char* who = "bg_gru_bias_partial";
    if (B <= 0) return bg_fail(who, -1, "bad argument (B: at least 1)");
    if (H != 128 && H != 256) return bg_fail(who, -4, "unsupported H (128 or 256)");
    if (!dgi || !dgh || !records) return bg_fail(who, -1, "bad argument");
    if (!aligned16(dgi) || !aligned16(dgh) || !aligned16(records)) return bg_fail(who, -1, "dgi, dgh and records must be 16-byte aligned");
    const dim3 grid((B + BP_ROWS - 1) / BP_ROWS), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (H == 128) hipLaunchKernelGGL(gru_bias_partial_kernel<128>, grid, block, 0, st, B, dgi, dgh, records);
    else hipLaunchKernelGGL(gru_bias_partial_kernel<256>, grid, block, 0, st, B, dgi, dgh, records);
    HIP_OK(hipGetLastError());
    return 0;
}

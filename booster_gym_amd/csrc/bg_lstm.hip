// The recurrence of an LSTM actor's PPO update (utils/model.py LSTMTrainer, algorithm.rnn_cell: "lstm"; legged_gym / rsl_rl's ActorCriticRecurrent with
// its default cell, back-propagation through the T = horizon_length steps of an iteration from the stored state): bg_lstm_sequence_forward and
// bg_lstm_sequence_backward, ONE launch each for all T steps, fp32 MFMA, gfx950 only; and bg_lstm_bias_partial, the cell's bias gradients.
//
// As in bg_gru.hip the x-side gi = X W_ih^T + b_ih runs on all T N rows at once (bg_mlp_layer_forward) and a workgroup (4 waves) owns 16 envs and walks the
// steps itself, the state tile [16][H + 4] in LDS, the operands of v_mfma_f32_16x16x4_f32 as there:
//     A[i = lane & 15][k = lane >> 4]  h (forward) / dg (backward) from LDS, one ds_read_b128 feeds 4 MFMAs
//     B[k = lane >> 4][j = lane & 15]  W_hh from global memory / L2: 262 kB at H = 128, 1 MB at H = 256, 4 MB at H = 512
//     C/D: column j = lane & 15, row i = (lane >> 4) * 4 + reg
// What the LSTM changes:
//   - the two sides of a pre-activation simply add, so the forward accumulators START from gi + b_hh and the gate arithmetic (bg_lstm.h, the rollout's)
//     takes the accumulated sums; backwards dgi == dgh, ONE tensor dg [T][N][4H] serves W_ih, W_hh and both biases;
//   - the second state c is elementwise.  Forward, a wave owns the column tiles wave, wave + 4, ... of H at EVERY step, so element (row, col) of c is the
//     same lane's for all T steps and stays in its registers (4 H / 64 floats per lane); only h goes through the double-buffered LDS tile.  Backward, dc
//     is carried in the registers of the elementwise thread mapping (16 H / 256 floats per thread); only dh goes through LDS;
//   - four gates: two weight buffers ping-pong through i, f, g, o, the next gate's 8 loads in flight under this gate's 32 MFMAs;
//   - the backward GEMM carry_h = dg W_hh has K = 4H, its B operand read down the rows of W_hh with scalar loads (16 lanes = one 64-byte segment).
// Both write every value they produce once and add in a fixed order: deterministic.  What a step reads from memory is requested in front of MFMAs that
// do not need it: the forward loads the next tile's (at a step's last tile: the next step's first tile's) gi under this tile's MFMAs, the backward
// loads step t - 1's dh_ext, gates and c_prev into registers under step t's GEMM.
// MR, the 32-MFMA step and the two fetches of W_hh are bg_rnn_seq.h's, shared with bg_gru.hip.
#include <hip/hip_runtime.h>

#include "bg_common.h"
#include "bg_lstm.h"
#include "bg_rnn_seq.h"

namespace {

// The forward recurrence of the 16 envs [16 blockIdx.x, 16 blockIdx.x + 16).
template <int H>
__global__ __launch_bounds__(256) void lstm_sequence_forward_kernel(int T, int N, const float* __restrict__ gi, const float* __restrict__ h0,
                                                                    const float* __restrict__ c0, const uint8_t* __restrict__ reset,
                                                                    const float* __restrict__ W, const float* __restrict__ bh, float* __restrict__ h_prev,
                                                                    float* __restrict__ c_prev, float* __restrict__ h, float* __restrict__ c,
                                                                    float* __restrict__ gates) {
    constexpr int LDH = H + 4, TPW = H / 64, CPT = H / 128;  // row stride of the state tiles; column tiles per wave; 128-wide k-chunks
    __shared__ __attribute__((aligned(16))) float tile[2][MR * LDH];
    const int r0 = blockIdx.x * MR, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, kg = lane >> 4;
    for (int k = threadIdx.x; k < MR * H; k += blockDim.x) {
        const int rr = k / H, cc = k - rr * H, row = r0 + rr;
        tile[0][rr * LDH + cc] = (h0 && row < N) ? h0[(size_t)row * H + cc] : 0.f;
    }
    // this lane's elements of c and of b_hh: rows r0 + 4 kg + q, column 16 (wave + 4 jt) + r, for all T steps
    float cr[TPW][4], bias[TPW][4];
#pragma unroll
    for (int jt = 0; jt < TPW; jt++) {
        const int col = (wave + 4 * jt) * 16 + r;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int row = r0 + kg * 4 + q;
            cr[jt][q] = (c0 && row < N) ? c0[(size_t)row * H + col] : 0.f;
        }
#pragma unroll
        for (int g = 0; g < 4; g++) bias[jt][g] = bh[g * H + col];
    }
    __syncthreads();
    auto fetch = [&](f32x4 (&w)[8], int g, int j, int kc) { seq_fetch_along_k<H>(w, W, g, j, kc, r, kg); };
    // the x-side pre-activations of column tile j at step t: v[q][gate]
    auto load_gi = [&](float (&v)[4][4], int t, int j) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int row = r0 + kg * 4 + q;
#pragma unroll
            for (int g = 0; g < 4; g++) v[q][g] = 0.f;
            if (row < N) {
                const float* p = gi + ((size_t)t * N + row) * (4 * H) + j * 16 + r;
#pragma unroll
                for (int g = 0; g < 4; g++) v[q][g] = p[g * H];
            }
        }
    };
    float giv[4][4];
    load_gi(giv, 0, wave);
    int cur = 0;
    for (int t = 0; t < T; t++) {
        float *hc = tile[cur], *hn = tile[cur ^ 1];
        const size_t tn = (size_t)t * N;
        // the states entering the step: zero behind a reset.  h_prev is the operand of W_hh's weight gradient, c_prev of the backward recurrence
        for (int k = threadIdx.x; k < MR * H; k += blockDim.x) {
            const int rr = k / H, cc = k - rr * H, row = r0 + rr;
            if (row < N) {
                float v = hc[rr * LDH + cc];
                if (reset && reset[tn + row]) hc[rr * LDH + cc] = v = 0.f;
                h_prev[(tn + row) * H + cc] = v;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int row = r0 + kg * 4 + q;
            if (row < N) {
                const bool z = reset && reset[tn + row];
#pragma unroll
                for (int jt = 0; jt < TPW; jt++) {
                    if (z) cr[jt][q] = 0.f;
                    c_prev[(tn + row) * H + (wave + 4 * jt) * 16 + r] = cr[jt][q];
                }
            }
        }
        __syncthreads();
        f32x4 wa[8], wb[8];
        fetch(wa, 0, wave, 0);
        static_for<TPW>([&](auto JT) {
            constexpr int jt = decltype(JT)::value;
            const int j = wave + 4 * jt, col = j * 16 + r;
            f32x4 acc[4][2];
            {
                // gi + b_hh first, the MFMAs accumulate h W_hh^T onto it: without the reassociation flag of this file's build the sum cannot be taken apart
#pragma clang fp reassociate(off)
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    acc[g][0] = f32x4{giv[0][g] + bias[jt][g], giv[1][g] + bias[jt][g], giv[2][g] + bias[jt][g], giv[3][g] + bias[jt][g]};
                    acc[g][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
            if (jt + 1 < TPW) load_gi(giv, t, j + 4);  // (the accumulators hold this tile's values: the registers take the next tile's)
            else if (t + 1 < T) load_gi(giv, t + 1, wave);
#pragma unroll 1
            for (int kc = 0; kc < CPT; kc++) {
                const float* arow = hc + r * LDH + kc * 128 + 4 * kg;
                fetch(wb, 1, j, kc);
                BG_RNN_MFMA32(acc[0][0], acc[0][1], arow, wa)
                fetch(wa, 2, j, kc);
                BG_RNN_MFMA32(acc[1][0], acc[1][1], arow, wb)
                fetch(wb, 3, j, kc);
                BG_RNN_MFMA32(acc[2][0], acc[2][1], arow, wa)
                if (kc + 1 < CPT) fetch(wa, 0, j, kc + 1);
                else if (jt + 1 < TPW) fetch(wa, 0, j + 4, 0);
                BG_RNN_MFMA32(acc[3][0], acc[3][1], arow, wb)
            }
            float p[4][4];
            {
#pragma clang fp reassociate(off)
#pragma unroll
                for (int g = 0; g < 4; g++)
#pragma unroll
                    for (int q = 0; q < 4; q++) p[g][q] = acc[g][0][q] + acc[g][1][q];
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int rr = kg * 4 + q, row = r0 + rr;
                const bg::LstmGates s = bg::lstm_gates(p[0][q], p[1][q], p[2][q], p[3][q], cr[jt][q]);
                cr[jt][q] = s.c;
                hn[rr * LDH + col] = s.h;
                if (row < N) {
                    h[(tn + row) * H + col] = s.h;
                    c[(tn + row) * H + col] = s.c;
                    float* go = gates + (tn + row) * (5 * H) + col;
                    go[0] = s.i; go[H] = s.f; go[2 * H] = s.g; go[3 * H] = s.o; go[4 * H] = s.tanh_c;
                }
            }
        });
        __syncthreads();
        cur ^= 1;
    }
}

// ... and the backward recurrence of those envs.  Thread `tid` owns the elements k = tid + 256 e of the [16][H] tile (row k / H, column k % H) in the
// elementwise phase of every step: its dc never leaves its registers.
template <int H>
__global__ __launch_bounds__(256) void lstm_sequence_backward_kernel(int T, int N, const float* __restrict__ dh_ext, const float* __restrict__ gates,
                                                                     const float* __restrict__ c_prev, const uint8_t* __restrict__ reset,
                                                                     const float* __restrict__ W, float* __restrict__ dg, float* __restrict__ dh0,
                                                                     float* __restrict__ dc0) {
    constexpr int LDH = H + 4, LDG = 4 * H + 4, TPW = H / 64, CPT = 4 * H / 128;
    __shared__ __attribute__((aligned(16))) float gt[MR * LDG];     // dg of the step: the GEMM's A operand
    __shared__ __attribute__((aligned(16))) float carry[MR * LDH];  // dh carried to the step below
    const int r0 = blockIdx.x * MR, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, kg = lane >> 4;
    for (int k = threadIdx.x; k < MR * LDH; k += blockDim.x) carry[k] = 0.f;
    __syncthreads();
    // step s of the GEMM's flat loop over (column tile, k-chunk): tile wave + 4 (s / CPT), chunk s % CPT
    auto fetch = [&](f32x4 (&w)[8], int s) { seq_fetch_down_rows<H>(w, W, 0, wave + 4 * (s / CPT), s % CPT, r, kg); };
    // a thread's elements of a step's operands (dh_ext, i, f, g, o, tanh(c'), c_prev) and their rows' reset flags: those of step t - 1 are loaded under
    // step t's GEMM
    constexpr int EPT = MR * H / 256;
    float in[EPT][7], dcc[EPT];
    bool rs[EPT];
#pragma unroll
    for (int e = 0; e < EPT; e++) dcc[e] = 0.f;
    auto load = [&](int t) {
        const size_t tn = (size_t)t * N;
#pragma unroll
        for (int e = 0; e < EPT; e++) {
            const int k = threadIdx.x + 256 * e, rr = k / H, cc = k - rr * H, row = r0 + rr;
            rs[e] = false;
            if (row < N) {
                const float* g = gates + (tn + row) * (5 * H) + cc;
                in[e][0] = dh_ext[(tn + row) * H + cc];
                in[e][1] = g[0]; in[e][2] = g[H]; in[e][3] = g[2 * H]; in[e][4] = g[3 * H]; in[e][5] = g[4 * H];
                in[e][6] = c_prev[(tn + row) * H + cc];
                rs[e] = reset && reset[tn + row];
            }
        }
    };
    load(T - 1);
    for (int t = T - 1; t >= 0; t--) {
        const size_t tn = (size_t)t * N;
        bool rq[4];  // the reset flags of the rows this lane finishes behind the GEMM
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int row = r0 + kg * 4 + q;
            rq[q] = row >= N || (reset && reset[tn + row]);
        }
#pragma unroll
        for (int e = 0; e < EPT; e++) {
            const int k = threadIdx.x + 256 * e, rr = k / H, cc = k - rr * H, row = r0 + rr;
            float di = 0.f, df = 0.f, dgg = 0.f, dout = 0.f;
            if (row < N) {
                const float dh = in[e][0] + carry[rr * LDH + cc];
                const float gi_ = in[e][1], gf = in[e][2], gg = in[e][3], go = in[e][4], tc = in[e][5], cp = in[e][6];
                const float dc = dcc[e] + dh * go * (1.0f - tc * tc);
                dout = dh * tc * (go * (1.0f - go));
                di = dc * gg * (gi_ * (1.0f - gi_));
                df = dc * cp * (gf * (1.0f - gf));
                dgg = dc * gi_ * (1.0f - gg * gg);
                dcc[e] = rs[e] ? 0.f : dc * gf;
                float* o = dg + (tn + row) * (4 * H) + cc;
                o[0] = di; o[H] = df; o[2 * H] = dgg; o[3 * H] = dout;
            }
            float* gl = gt + rr * LDG + cc;
            gl[0] = di; gl[H] = df; gl[2 * H] = dgg; gl[3 * H] = dout;
        }
        __syncthreads();
        if (t > 0) load(t - 1);
        constexpr int steps = TPW * CPT;
        f32x4 cur[8], nxt[8] = {};
        fetch(cur, 0);
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
        for (int s = 0; s < steps; s++) {
            if (s + 1 < steps) fetch(nxt, s + 1);
            const int j = wave + 4 * (s / CPT), kc = s % CPT;
            if (kc == 0) acc0 = acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
            const float* arow = gt + r * LDG + kc * 128 + 4 * kg;
            BG_RNN_MFMA32(acc0, acc1, arow, cur)
            if (kc == CPT - 1) {
                const int col = j * 16 + r;
#pragma unroll
                for (int q = 0; q < 4; q++) carry[(kg * 4 + q) * LDH + col] = rq[q] ? 0.f : acc0[q] + acc1[q];  // (no thread reads the tile in this phase)
            }
#pragma unroll
            for (int u = 0; u < 8; u++) cur[u] = nxt[u];
        }
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < EPT; e++) {
        const int k = threadIdx.x + 256 * e, rr = k / H, cc = k - rr * H, row = r0 + rr;
        if (row < N) {
            if (dh0) dh0[(size_t)row * H + cc] = carry[rr * LDH + cc];
            if (dc0) dc0[(size_t)row * H + cc] = dcc[e];
        }
    }
}

// ---- H = 512 (legged_gym's rnn_hidden_size; algorithm.rnn_hidden_size: 512 with rnn_cell: "lstm").  The forward kernel and the bias sums above are
// instantiated at 512 as they are (the forward: c and b_hh in 32 + 32 registers of a lane, two h tiles = 66,048 B of LDS, no scratch).  The backward
// kernel above is not: its dg tile [16][4H + 4] and the dh tile come to 164,352 B, over the CU's 160 kB, and its seven prefetched operands of 32
// elements per thread to 224 registers.  This form runs the K = 4H GEMM carry_h = dg W_hh in TWO K PASSES over gate pairs, in this fixed order:
//   pass 0: K = the rows [0, 2H) of W_hh, the gates (i, f);   pass 1: K = the rows [2H, 4H), the gates (g, o).
// The elementwise phase of a step computes all four gate gradients of a thread's 32 elements, writes them to dg in memory, puts (di, df) into the ONE
// tile [16][2H + 4] and keeps (dg_g, do) in registers; the MFMAs of pass 0 consume the tile and park their sums in the dh tile (free in this phase: the
// carry was consumed by the elementwise phase), each lane its own elements; behind a barrier the tile takes (dg_g, do) and the MFMAs of pass 1 start
// their accumulator from the parked sums: an element is ((acc0 + acc1 of pass 0) + pass 1's even k-groups) + pass 1's odd k-groups, k ascending within
// each.  LDS 65,792 + 33,024 = 98,816 B.  dc stays in the elementwise mapping's 32 registers.  The operands of a step are loaded in its elementwise
// phase, eight elements' loads in flight at a time, not under the step above's GEMM (no registers for them beside dc, dg_g and do): per step that
// exposes a few memory round trips beside 2 x 2,048 MFMAs per wave.  dh0 / dc0 / reset may be NULL as above.
__global__ __launch_bounds__(256) void lstm_sequence_backward_wide_kernel(int T, int N, const float* __restrict__ dh_ext, const float* __restrict__ gates,
                                                                          const float* __restrict__ c_prev, const uint8_t* __restrict__ reset,
                                                                          const float* __restrict__ W, float* __restrict__ dg, float* __restrict__ dh0,
                                                                          float* __restrict__ dc0) {
    constexpr int H = 512, LDH = H + 4, LDG = 2 * H + 4, TPW = H / 64, CPT = 2 * H / 128, EPT = MR * H / 256, EB = 8;
    __shared__ __attribute__((aligned(16))) float gt[MR * LDG];     // dg of the step, one gate pair at a time: the GEMM's A operand
    __shared__ __attribute__((aligned(16))) float carry[MR * LDH];  // dh carried to the step below; between the passes: pass 0's sums
    static_assert(sizeof(float) * (MR * LDG + MR * LDH) <= 160 * 1024, "within the CU's LDS");
    const int r0 = blockIdx.x * MR, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, kg = lane >> 4;
    for (int k = threadIdx.x; k < MR * LDH; k += blockDim.x) carry[k] = 0.f;
    __syncthreads();
    // step s of pass `pass` of the GEMM: the rows [2H pass, 2H pass + 2H) of W_hh
    auto fetch = [&](f32x4 (&w)[8], int pass, int s) { seq_fetch_down_rows<H>(w, W, pass * 2 * H, wave + 4 * (s / CPT), s % CPT, r, kg); };
    float dcc[EPT], dgg[EPT], dout[EPT];
#pragma unroll
    for (int e = 0; e < EPT; e++) dcc[e] = 0.f;
    for (int t = T - 1; t >= 0; t--) {
        const size_t tn = (size_t)t * N;
        bool rq[4];  // the reset flags of the rows this lane finishes behind the GEMM
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int row = r0 + kg * 4 + q;
            rq[q] = row >= N || (reset && reset[tn + row]);
        }
#pragma unroll
        for (int eb = 0; eb < EPT; eb += EB) {
            float in[EB][7];
            bool rs[EB];
#pragma unroll
            for (int x = 0; x < EB; x++) {
                const int k = threadIdx.x + 256 * (eb + x), rr = k / H, cc = k - rr * H, row = r0 + rr;
                rs[x] = false;
                if (row < N) {
                    const float* g = gates + (tn + row) * (5 * H) + cc;
                    in[x][0] = dh_ext[(tn + row) * H + cc];
                    in[x][1] = g[0]; in[x][2] = g[H]; in[x][3] = g[2 * H]; in[x][4] = g[3 * H]; in[x][5] = g[4 * H];
                    in[x][6] = c_prev[(tn + row) * H + cc];
                    rs[x] = reset && reset[tn + row];
                }
            }
#pragma unroll
            for (int x = 0; x < EB; x++) {
                const int e = eb + x, k = threadIdx.x + 256 * e, rr = k / H, cc = k - rr * H, row = r0 + rr;
                float di = 0.f, df = 0.f;
                dgg[e] = dout[e] = 0.f;
                if (row < N) {
                    const float dh = in[x][0] + carry[rr * LDH + cc];
                    const float gi_ = in[x][1], gf = in[x][2], gg = in[x][3], go = in[x][4], tc = in[x][5], cp = in[x][6];
                    const float dc = dcc[e] + dh * go * (1.0f - tc * tc);
                    dout[e] = dh * tc * (go * (1.0f - go));
                    di = dc * gg * (gi_ * (1.0f - gi_));
                    df = dc * cp * (gf * (1.0f - gf));
                    dgg[e] = dc * gi_ * (1.0f - gg * gg);
                    dcc[e] = rs[x] ? 0.f : dc * gf;
                    float* o = dg + (tn + row) * (4 * H) + cc;
                    o[0] = di; o[H] = df; o[2 * H] = dgg[e]; o[3 * H] = dout[e];
                }
                float* gl = gt + rr * LDG + cc;
                gl[0] = di; gl[H] = df;
            }
            __builtin_amdgcn_sched_barrier(0);  // (the next eight elements' loads stay behind these eight's arithmetic: 56 operand registers, not 224)
        }
        __syncthreads();
        constexpr int steps = TPW * CPT;
#pragma unroll 1
        for (int pass = 0; pass < 2; pass++) {
            if (pass) {
                __syncthreads();  // every wave is through with the (i, f) tile
#pragma unroll
                for (int e = 0; e < EPT; e++) {
                    const int k = threadIdx.x + 256 * e, rr = k / H, cc = k - rr * H;
                    float* gl = gt + rr * LDG + cc;
                    gl[0] = dgg[e]; gl[H] = dout[e];
                }
                __syncthreads();
            }
            f32x4 cur[8], nxt[8] = {};
            fetch(cur, pass, 0);
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
            for (int s = 0; s < steps; s++) {
                if (s + 1 < steps) fetch(nxt, pass, s + 1);
                const int j = wave + 4 * (s / CPT), kc = s % CPT, col = j * 16 + r;
                if (kc == 0) {
                    acc0 = acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (pass) {  // pass 0's sums of this lane's own elements
#pragma unroll
                        for (int q = 0; q < 4; q++) acc0[q] = carry[(kg * 4 + q) * LDH + col];
                    }
                }
                const float* arow = gt + r * LDG + kc * 128 + 4 * kg;
                BG_RNN_MFMA32(acc0, acc1, arow, cur)
                if (kc == CPT - 1) {
#pragma unroll
                    for (int q = 0; q < 4; q++) carry[(kg * 4 + q) * LDH + col] = (pass && rq[q]) ? 0.f : acc0[q] + acc1[q];  // (no other thread reads the tile in this phase)
                }
#pragma unroll
                for (int u = 0; u < 8; u++) cur[u] = nxt[u];
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < EPT; e++) {
        const int k = threadIdx.x + 256 * e, rr = k / H, cc = k - rr * H, row = r0 + rr;
        if (row < N) {
            if (dh0) dh0[(size_t)row * H + cc] = carry[rr * LDH + cc];
            if (dc0) dc0[(size_t)row * H + cc] = dcc[e];
        }
    }
}

// The cell's bias gradients: the column sums of dg [B][4H] as ONE launch that leaves one record [4H] per 128-row block, for bg_reduce_problems of the
// update's deferred group to add up (bg_reduce.h): b_ih's and b_hh's gradients are the same sums, two finishes on the same records.  Memory-bound, the
// design of bg_gru_bias_partial on one tensor: a lane owns one 16-byte column per 64-lane group (H / 64 groups: a wave reads 1 KiB runs), a wave the
// rows wave, wave + 4, ... of the block in ascending order, its loads of four rows in flight; the four waves' sums meet in LDS and are added in wave
// order: every term once, a fixed order, no atomics.
constexpr int BP_ROWS = 128;  // rows per workgroup = per record

template <int H>
__global__ __launch_bounds__(256) void lstm_bias_partial_kernel(int B, const float* __restrict__ dg, float* __restrict__ records) {
    constexpr int C = 4 * H, C4 = C / 4, G = C4 / 64;
    __shared__ f32x4 sm[4][C4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r0 = blockIdx.x * BP_ROWS, r1 = min(r0 + BP_ROWS, B);  // (rows at or beyond B are never read)
    f32x4 acc[G];
#pragma unroll
    for (int g = 0; g < G; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int row = r0 + wave; row < r1; row += 4) {
#pragma unroll
        for (int g = 0; g < G; g++) acc[g] += *reinterpret_cast<const f32x4*>(dg + (size_t)row * C + 4 * (64 * g + lane));
    }
#pragma unroll
    for (int g = 0; g < G; g++) sm[wave][64 * g + lane] = acc[g];
    __syncthreads();
    f32x4* rec = reinterpret_cast<f32x4*>(records + (size_t)blockIdx.x * C);
    for (int v = threadIdx.x; v < C4; v += 256) rec[v] = ((sm[0][v] + sm[1][v]) + sm[2][v]) + sm[3][v];
}

int check_shape(const char* who, int32_t T, int32_t N, int32_t H) {
    if (T <= 0 || N <= 0) return bg_fail(who, -1, "bad argument (T, N: at least 1)");
    if (H != 128 && H != 256 && H != 512) return bg_fail(who, -4, "unsupported H (128, 256 or 512)");
    return 0;
}

}  // namespace

extern "C" int bg_lstm_sequence_forward(int32_t T, int32_t N, int32_t H, const float* gi, const float* h0, const float* c0, const uint8_t* reset,
                                        const float* W_hh, const float* b_hh, float* h_prev, float* c_prev, float* h, float* c, float* gates, void* stream) {
    const char* who = "bg_lstm_sequence_forward";
    if (const int rc = check_shape(who, T, N, H)) return rc;
    if (!gi || !W_hh || !b_hh || !h_prev || !c_prev || !h || !c || !gates) return bg_fail(who, -1, "bad argument");
    if (!aligned16(W_hh)) return bg_fail(who, -1, "W_hh must be 16-byte aligned");
    const dim3 grid((N + MR - 1) / MR), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (H == 128) hipLaunchKernelGGL(lstm_sequence_forward_kernel<128>, grid, block, 0, st, T, N, gi, h0, c0, reset, W_hh, b_hh, h_prev, c_prev, h, c, gates);
    else if (H == 512) hipLaunchKernelGGL(lstm_sequence_forward_kernel<512>, grid, block, 0, st, T, N, gi, h0, c0, reset, W_hh, b_hh, h_prev, c_prev, h, c, gates);
    else hipLaunchKernelGGL(lstm_sequence_forward_kernel<256>, grid, block, 0, st, T, N, gi, h0, c0, reset, W_hh, b_hh, h_prev, c_prev, h, c, gates);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_lstm_sequence_backward(int32_t T, int32_t N, int32_t H, const float* dh_ext, const float* gates, const float* c_prev, const uint8_t* reset,
                                         const float* W_hh, float* dg, float* dh0, float* dc0, void* stream) {
    const char* who = "bg_lstm_sequence_backward";
    if (const int rc = check_shape(who, T, N, H)) return rc;
    if (!dh_ext || !gates || !c_prev || !W_hh || !dg) return bg_fail(who, -1, "bad argument");
    const dim3 grid((N + MR - 1) / MR), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (H == 128) hipLaunchKernelGGL(lstm_sequence_backward_kernel<128>, grid, block, 0, st, T, N, dh_ext, gates, c_prev, reset, W_hh, dg, dh0, dc0);
    else if (H == 512) hipLaunchKernelGGL(lstm_sequence_backward_wide_kernel, grid, block, 0, st, T, N, dh_ext, gates, c_prev, reset, W_hh, dg, dh0, dc0);
    else hipLaunchKernelGGL(lstm_sequence_backward_kernel<256>, grid, block, 0, st, T, N, dh_ext, gates, c_prev, reset, W_hh, dg, dh0, dc0);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_lstm_bias_partial(int32_t B, int32_t H, const float* dg, float* records, void* stream) {
    const char* who = "bg_lstm_bias_partial";
    if (B <= 0) return bg_fail(who, -1, "bad argument (B: at least 1)");
    if (H != 128 && H != 256 && H != 512) return bg_fail(who, -4, "unsupported H (128, 256 or 512)");
    if (!dg || !records) return bg_fail(who, -1, "bad argument");
    if (!aligned16(dg) || !aligned16(records)) return bg_fail(who, -1, "dg and records must be 16-byte aligned");
    const dim3 grid((B + BP_ROWS - 1) / BP_ROWS), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (H == 128) hipLaunchKernelGGL(lstm_bias_partial_kernel<128>, grid, block, 0, st, B, dg, records);
    else if (H == 512) hipLaunchKernelGGL(lstm_bias_partial_kernel<512>, grid, block, 0, st, B, dg, records);
    else hipLaunchKernelGGL(lstm_bias_partial_kernel<256>, grid, block, 0, st, B, dg, records);
    HIP_OK(hipGetLastError());
    return 0;
}

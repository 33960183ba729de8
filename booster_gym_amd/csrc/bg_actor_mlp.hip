// Fused actor MLP + Gaussian sample for the rollout at any supported architecture (reference utils/model.py:8-25 with the widths a user sets,
// utils/runner.py:109-111: dist = model.act(obs); act = dist.sample()), fp32 MFMA, gfx950 only.  bg_actor_sample (bg_ppo.hip) keeps the
// reference's widths built into its kernel; this one reads them from descriptors: 47 H inputs (H = 1 .. 10 observation frames, env.frame_stack)
// and with terrain.actor_heights P more, the height scan (K = 47 H + P up to 480 = BG_ACTOR_MAX_INPUT: whole k-chunks within the 516-column LDS tile),
// 2 to 4 hidden ELU layers of widths a multiple of 128 up to 512, 12 outputs.
//
// One workgroup (4 waves) = 16 observation rows.  The activations ping-pong between two LDS tiles [16][MAXW + 4]; each wave owns the 16-neuron
// output tiles wave, wave + 4, ... of a layer and accumulates them with v_mfma_f32_16x16x4_f32 (exact fp32, D = A*B + C), operands as in
// bg_actor_sample:
//     A[i = lane & 15][k = lane >> 4] = X[row i][k]          (from LDS, one ds_read_b128 feeds 4 MFMAs)
//     B[k = lane >> 4][j = lane & 15] = W[neuron j][k]       (straight from global memory / L2: torch layout [out][in], one 16-byte load feeds 4 MFMAs)
//     C/D: neuron j = lane & 15, row i = (lane >> 4) * 4 + reg
// A wave walks its (tile, 128-wide k-chunk) steps in one flat loop and fetches the 8 weight vectors (+ the bias) of step s + 1 before it runs the
// 32 MFMAs of step s, so the L2 latency hides under them whatever the widths.  Two accumulators per tile (even / odd k groups) keep the MFMA chain
// from waiting on its own 40-cycle dependent latency.
// The first layer reads the torch-layout rows [out][47 H] (16-byte aligned only when H % 4 == 0) with scalar loads, straight from the parameters
// (no padded copy that could go stale), in k-chunks of 48 columns = 12 MFMAs, prefetched the same way; the input tile is zero beyond column 47 H.
// LDS: 2 x 16 x 516 floats = 66 kB at MAXW = 512 (two workgroups per CU), 33 kB at MAXW = 256; 16 rows per workgroup: 256 workgroups at 4,096 rows.
// The input tile [16][48 H] lives in the first activation tile, so 6 frames and more (288 columns and up) take the MAXW = 512 form.
// The noise is bg_actor_sample's: the same bg::rand4(seed, row, counter, RS_ACTOR + g) draw per (row, group of 4 actions), the same expression.
//
// bg_distill_act (teacher-student distillation, utils/distill.py) runs TWO such networks on the same rows in one launch: the grid is split, workgroups
// [0, nb) evaluate the teacher on all 47 H + P columns of their 16 rows and write its mean, workgroups [nb, 2 nb) the student on the first 47 H
// columns and sample.  Both kernels are one body, actor_rows, so a half computes what the stand-alone kernel does on the same operands, bit for bit.
// bg_distill_act_mix (distillation.teacher_action_prob, DAgger's mixing) is the same split grid in which the teacher's half acts on a row with
// probability beta: a Philox uniform per (row, step) on a stream of its own, evaluated by both halves, decides which half writes the row's action.
//
// bg_actor_sample_est (the learned state estimator, T1.yaml estimator.enabled; its targets are columns of the reference's privileged observation,
// envs/t1.py:593-602) runs two networks on the same rows one BEHIND the other in the same workgroup: the estimator 47 H -> hidden -> 12, whose
// means go to memory, then the actor on the tile [obs | the first E means | zeros] rebuilt in LDS.  Same pieces (load_tile, run_layers, sample), same
// two LDS tiles: the launch costs about the two stand-alone launches it replaces, without their two boundaries and the concatenation copy.
//
// bg_actor_sample_gru and bg_distill_act_gru (a recurrent student, T1.yaml distillation.student_memory; rsl_rl's recurrent `Distillation` student) put
// a GRU cell in front of the network, on the same 16 rows and the same layer code: gru_rows, below.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "bg_common.h"
#include "bg_gru.h"
#include "bg_rng.h"

namespace {

constexpr int MR = 16;         // rows per workgroup
constexpr int MAX_LAYERS = 5;  // 4 hidden + the output layer
constexpr int KC = 48;         // k-chunk of the first layer: one frame's 47 observations and a column more (47 H <= 48 H: H chunks cover H frames)

struct ActorNet {
    const float* W[MAX_LAYERS];
    const float* b[MAX_LAYERS];
    int in[MAX_LAYERS], out[MAX_LAYERS];
    int n;
};

__device__ __forceinline__ float elu(float x) { return x > 0.f ? x : expm1f(x); }  // = bg_ppo.hip's

// first layer: K = 47 H (+ P) inputs (rows not 16-byte aligned): scalar weight loads, k padded to a multiple of KC with zeros; OUT a multiple of 16.  A wave
// walks its (tile, k-chunk) steps in one flat loop, the weights of step s + 1 in flight under the 12 MFMAs of step s; with H = 1 one step per tile.
template <int LDA, int LDO = LDA, bool ACT = true>
__device__ __forceinline__ void first_layer(const float* __restrict__ W, const float* __restrict__ bv, int K, int OUT, const float* in, float* out,
                                            int wave, int lane) {
    constexpr int STEPS = KC / 4;
    const int r = lane & 15, kg = lane >> 4, tiles = OUT / 16, cpt = (K + KC - 1) / KC;
    if (wave >= tiles) return;
    const int steps = (tiles - wave + 3) / 4 * cpt;
    float cur[STEPS], nxt[STEPS] = {}, bc = 0.f, bn = 0.f;
    auto fetch = [&](float (&w)[STEPS], float& bias, int s) {
        const int tile = wave + 4 * (s / cpt), c = s % cpt, n = tile * 16 + r;
        const float* wrow = W + (size_t)n * K;
#pragma unroll
        for (int s2 = 0; s2 < STEPS; s2++) { const int k = c * KC + 4 * s2 + kg; w[s2] = k < K ? wrow[k] : 0.f; }
        if (c == 0) bias = bv[n];
    };
    fetch(cur, bc, 0);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < steps; s++) {
        if (s + 1 < steps) fetch(nxt, bn, s + 1);
        const int tile = wave + 4 * (s / cpt), c = s % cpt;
        if (c == 0) acc = f32x4{bc, bc, bc, bc};
        const float* arow = in + r * LDA + c * KC + kg;
#pragma unroll
        for (int s2 = 0; s2 < STEPS; s2++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[4 * s2], cur[s2], acc, 0, 0, 0);
        if (c == cpt - 1) {
#pragma unroll
            for (int q = 0; q < 4; q++) out[(kg * 4 + q) * LDO + tile * 16 + r] = ACT ? elu(acc[q]) : acc[q];
        }
#pragma unroll
        for (int s2 = 0; s2 < STEPS; s2++) cur[s2] = nxt[s2];
        if (c + 1 == cpt) bc = bn;
    }
}

// a layer of K inputs (a multiple of 128) and OUT outputs; neurons >= OUT (the 12-wide output layer's last tile) compute zeros that nobody reads
template <int LDA, int LDO = LDA>
__device__ __forceinline__ void layer(const float* __restrict__ W, const float* __restrict__ bv, int K, int OUT, bool act, const float* in, float* out,
                                      int wave, int lane) {
    const int r = lane & 15, kg = lane >> 4, tiles = (OUT + 15) / 16, cpt = K >> 7;
    if (wave >= tiles) return;
    const int steps = (tiles - wave + 3) / 4 * cpt;
    f32x4 cur[8], nxt[8] = {};
    float bc = 0.f, bn = 0.f;
    auto fetch = [&](f32x4 (&w)[8], float& bias, int s) {
        const int tile = wave + 4 * (s / cpt), c = s % cpt, n = tile * 16 + r;
        const bool nv = n < OUT;
        const float* wrow = W + (size_t)(nv ? n : 0) * K + c * 128 + 4 * kg;
#pragma unroll
        for (int u = 0; u < 8; u++) {
            w[u] = *reinterpret_cast<const f32x4*>(wrow + 16 * u);
            if (!nv) w[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (c == 0) bias = nv ? bv[n] : 0.f;
    };
    fetch(cur, bc, 0);
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    for (int s = 0; s < steps; s++) {
        if (s + 1 < steps) fetch(nxt, bn, s + 1);
        const int tile = wave + 4 * (s / cpt), c = s % cpt;
        if (c == 0) { acc0 = f32x4{bc, bc, bc, bc}; acc1 = f32x4{0.f, 0.f, 0.f, 0.f}; }
        const float* arow = in + r * LDA + c * 128 + 4 * kg;
#pragma unroll
        for (int u = 0; u < 8; u += 2) {
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(arow + 16 * u), a1 = *reinterpret_cast<const f32x4*>(arow + 16 * (u + 1));
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, cur[u].x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, cur[u + 1].x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, cur[u].y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, cur[u + 1].y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, cur[u].z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, cur[u + 1].z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, cur[u].w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, cur[u + 1].w, acc1, 0, 0, 0);
        }
        if (c == cpt - 1) {
            const f32x4 v = acc0 + acc1;
#pragma unroll
            for (int q = 0; q < 4; q++) out[(kg * 4 + q) * LDO + tile * 16 + r] = act ? elu(v[q]) : v[q];
        }
#pragma unroll
        for (int u = 0; u < 8; u++) cur[u] = nxt[u];
        if (c + 1 == cpt) bc = bn;
    }
}

// The pieces of a workgroup's pass over its 16 rows [r0, r0 + 16): load_tile, run_layers, sample.  actor_rows strings them together for one network,
// actor_est_sample_kernel for two networks back to back.

// The input tile [16][KP] (KP = K padded to whole k-chunks) into `tile`: columns [0, KO) from the rows of `obs`, `stride` floats apart, columns [KO, K)
// from `ext` (an LDS tile of row stride LDA: bg_actor_sample_est's estimates; nullptr with KO == K), zeros behind them and in the rows past N.
template <int LDA>
__device__ __forceinline__ void load_tile(float* tile, int N, int r0, const float* __restrict__ obs, int stride, int KO, const float* ext, int K) {
    const int KP = (K + KC - 1) / KC * KC;  // 47 H (+ P) columns; the tile's columns padded to whole k-chunks with zeros (KP <= LDA: host)
    for (int k = threadIdx.x; k < MR * KP; k += blockDim.x) {
        const int r = k / KP, c = k - r * KP;
        float v = 0.f;
        if (r0 + r < N) {
            if (c < KO) v = obs[(size_t)(r0 + r) * stride + c];
            else if (c < K) v = ext[r * LDA + c - KO];
        }
        tile[r * LDA + c] = v;
    }
    __syncthreads();
}

// Every layer of `net` on the input tile buf[in], the activations ping-ponging between the two tiles; returns the index of the tile that holds the
// 12 outputs of the 16 rows (columns [0, 12)).  Ends behind a barrier.
template <int LDA>
__device__ __forceinline__ int run_layers(const ActorNet& net, float (*buf)[MR * LDA], int in) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    first_layer<LDA>(net.W[0], net.b[0], net.in[0], net.out[0], buf[in], buf[in ^ 1], wave, lane);
    __syncthreads();
    int cur = in ^ 1;
    for (int l = 1; l < net.n; l++) {
        layer<LDA>(net.W[l], net.b[l], net.in[l], net.out[l], l + 1 < net.n, buf[cur], buf[cur ^ 1], wave, lane);
        __syncthreads();
        cur ^= 1;
    }
    return cur;
}

// run_layers on an input tile `x` of its own (row stride LDA) that stays as it is: the first layer writes buf[0] and the activations ping-pong between
// the two tiles of `buf` from there (bg_rnd_reward: two networks read the one tile).
template <int LDA>
__device__ __forceinline__ int run_layers_keep(const ActorNet& net, const float* x, float (*buf)[MR * LDA]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    first_layer<LDA>(net.W[0], net.b[0], net.in[0], net.out[0], x, buf[0], wave, lane);
    __syncthreads();
    int cur = 0;
    for (int l = 1; l < net.n; l++) {
        layer<LDA>(net.W[l], net.b[l], net.in[l], net.out[l], l + 1 < net.n, buf[cur], buf[cur ^ 1], wave, lane);
        __syncthreads();
        cur ^= 1;
    }
    return cur;
}

// sample: one thread per (row, group of 4 actions), as bg_actor_sample, from the means in `m` (an LDS tile of row stride LDA).  act_out == nullptr: the
// mean alone goes to mu_out and no noise is drawn (bg_distill_act's teacher, bg_actor_sample_est's estimator).
// MIX (bg_distill_act_mix, compiled into its kernel alone): the row's action comes from ONE of two calls on the same rows, the teacher's when
// u < beta and the student's otherwise, u = entry 0 of rand4_uniform(seed, row, counter, RS_DAGGER): both calls evaluate u and the one that acts
// writes act_out, with the noise draw the other would have used (the teacher without it when teacher_noise is 0: its mean alone).
template <int LDA, bool MIX>
__device__ __forceinline__ void sample(const float* m_tile, int N, int r0, const float* __restrict__ logstd, uint64_t seed, uint32_t counter,
                                       float* __restrict__ mu_out, float* __restrict__ act_out, bool teacher_half, float beta, int teacher_noise) {
    if (threadIdx.x < MR * 3) {
        const int r = threadIdx.x / 3, g = threadIdx.x % 3, row = r0 + r;
        if (row < N) {
            if constexpr (MIX) {
                float u[4];
                bg::rand4_uniform(seed, (uint32_t)row, counter, bg::RS_DAGGER, u);
                const bool acts = (u[0] < beta) == teacher_half, noise = acts && (!teacher_half || teacher_noise != 0);
                bg::Rand4 rn = {};
                if (noise) rn = bg::rand4(seed, (uint32_t)row, counter, bg::RS_ACTOR + g);
                for (int k = 0; k < 4; k++) {
                    const int a = g * 4 + k;
                    const float m = m_tile[r * LDA + a];
                    if (mu_out) mu_out[(size_t)row * BG_NUM_DOFS + a] = m;
                    if (noise) act_out[(size_t)row * BG_NUM_DOFS + a] = m + expf(logstd[a]) * rn.n[k];
                    else if (acts) act_out[(size_t)row * BG_NUM_DOFS + a] = m;
                }
            } else if (!act_out) {
                for (int k = 0; k < 4; k++) mu_out[(size_t)row * BG_NUM_DOFS + g * 4 + k] = m_tile[r * LDA + g * 4 + k];
            } else {
                bg::Rand4 rn = bg::rand4(seed, (uint32_t)row, counter, bg::RS_ACTOR + g);
                for (int k = 0; k < 4; k++) {
                    const int a = g * 4 + k;
                    const float m = m_tile[r * LDA + a];
                    if (mu_out) mu_out[(size_t)row * BG_NUM_DOFS + a] = m;
                    act_out[(size_t)row * BG_NUM_DOFS + a] = m + expf(logstd[a]) * rn.n[k];
                }
            }
        }
    }
}

// One workgroup's 16 rows [r0, r0 + 16) through one network: the body of the three kernels below.  The rows are `stride` floats apart and the network
// reads its own first net.in[0] columns of them.
template <int MAXW, bool MIX = false>
__device__ __forceinline__ void actor_rows(int N, int r0, const float* __restrict__ obs, int stride, const ActorNet& net, const float* __restrict__ logstd,
                                           uint64_t seed, uint32_t counter, float* __restrict__ mu_out, float* __restrict__ act_out, bool teacher_half = false,
                                           float beta = 0.f, int teacher_noise = 0) {
    constexpr int LDA = MAXW + 4;  // row stride (floats): = 4 mod 64 banks, as bg_actor_sample's 260
    __shared__ __attribute__((aligned(16))) float buf[2][MR * LDA];
    load_tile<LDA>(buf[0], N, r0, obs, stride, net.in[0], nullptr, net.in[0]);
    const int cur = run_layers<LDA>(net, buf, 0);
    sample<LDA, MIX>(buf[cur], N, r0, logstd, seed, counter, mu_out, act_out, teacher_half, beta, teacher_noise);
}

// bg_actor_sample_est: the estimator, then the actor on [obs | estimates], on the same 16 rows in one workgroup.  The estimator's 12 means go to est_out
// (sample's mean-only form); the actor's input tile is rebuilt in the activation tile the estimator's last layer read (free behind run_layers' last
// barrier): the 47 H observation columns from global memory again (L2-hot), columns [47 H, 47 H + E) from the tile that holds the estimator's means,
// zeros to the k-chunk boundary -- what load_tile builds from a contiguous row [obs | est_out[:E]], so the actor's half computes what
// bg_actor_sample_mlp_scan(scan_points = E) does on that row, bit for bit.  The tile of the means is overwritten only behind load_tile's barrier.
struct EstNets { ActorNet est, actor; };
template <int MAXW>
__global__ __launch_bounds__(256) void actor_est_sample_kernel(int N, const float* __restrict__ obs, EstNets nets, const float* __restrict__ logstd, uint64_t seed,
                                                               uint32_t counter, float* __restrict__ est_out, float* __restrict__ mu_out, float* __restrict__ act_out) {
    constexpr int LDA = MAXW + 4;
    __shared__ __attribute__((aligned(16))) float buf[2][MR * LDA];
    const int r0 = blockIdx.x * MR, KO = nets.est.in[0];
    load_tile<LDA>(buf[0], N, r0, obs, KO, KO, nullptr, KO);
    int cur = run_layers<LDA>(nets.est, buf, 0);
    sample<LDA, false>(buf[cur], N, r0, nullptr, seed, counter, est_out, nullptr, false, 0.f, 0);
    load_tile<LDA>(buf[cur ^ 1], N, r0, obs, KO, KO, buf[cur], nets.actor.in[0]);
    cur = run_layers<LDA>(nets.actor, buf, cur ^ 1);
    sample<LDA, false>(buf[cur], N, r0, logstd, seed, counter, mu_out, act_out, false, 0.f, 0);
}

template <int MAXW>
__global__ __launch_bounds__(256) void actor_mlp_sample_kernel(int N, const float* __restrict__ obs, ActorNet net, const float* __restrict__ logstd,
                                                               uint64_t seed, uint32_t counter, float* __restrict__ mu_out, float* __restrict__ act_out) {
    actor_rows<MAXW>(N, blockIdx.x * MR, obs, net.in[0], net, logstd, seed, counter, mu_out, act_out);  // contiguous rows; act_out != nullptr: host
}

// bg_distill_act: nets.n[0] = the teacher (workgroups [0, nb): the longer network first), nets.n[1] = the student (workgroups [nb, 2 nb)).  Both read
// rows of `stride` floats (the student's 47 H columns are a prefix of the teacher's 47 H + P); the teacher writes its mean, the student samples.
// bg_distill_act_hist: the student half reads its own rows `sobs` of `sstride` floats (its longer history [47 Hs]); bg_distill_act passes the teacher's.
struct DistillNets { ActorNet n[2]; };
template <int MAXW>
__global__ __launch_bounds__(256) void distill_act_kernel(int N, int nb, const float* __restrict__ obs, int stride, const float* __restrict__ sobs, int sstride,
                                                          DistillNets nets, const float* __restrict__ logstd, uint64_t seed, uint32_t counter, float* __restrict__ student_mu,
                                                          float* __restrict__ act_out, float* __restrict__ teacher_mu) {
    const bool teacher = (int)blockIdx.x < nb;
    const int r0 = (teacher ? blockIdx.x : blockIdx.x - nb) * MR;
    actor_rows<MAXW>(N, r0, teacher ? obs : sobs, teacher ? stride : sstride, nets.n[teacher ? 0 : 1], logstd, seed, counter, teacher ? teacher_mu : student_mu,
                     teacher ? nullptr : act_out);
}

// bg_distill_act_mix: distill_act_kernel's split grid with the DAgger choice per row (actor_rows' MIX form).  Both halves write their mean; `act_out`
// receives each row from the half that acts on it: the two sets of rows are disjoint, so no atomics and no second pass.
template <int MAXW>
__global__ __launch_bounds__(256) void distill_act_mix_kernel(int N, int nb, const float* __restrict__ obs, int stride, const float* __restrict__ sobs, int sstride,
                                                              DistillNets nets, const float* __restrict__ logstd, uint64_t seed, uint32_t counter, float beta,
                                                              int teacher_noise, float* __restrict__ student_mu, float* __restrict__ act_out,
                                                              float* __restrict__ teacher_mu) {
    const bool teacher = (int)blockIdx.x < nb;
    const int r0 = (teacher ? blockIdx.x : blockIdx.x - nb) * MR;
    actor_rows<MAXW, true>(N, r0, teacher ? obs : sobs, teacher ? stride : sstride, nets.n[teacher ? 0 : 1], logstd, seed, counter, teacher ? teacher_mu : student_mu,
                           act_out, teacher, beta, teacher_noise);
}

// bg_rnd_reward (random network distillation, T1.yaml rnd.enabled; rsl_rl's rnd_cfg): a fixed random target network and a trained predictor on the
// same 16 state rows, one BEHIND the other in the same workgroup, as bg_actor_sample_est runs its two.  The input tile [obs | priv | zeros] is built
// ONCE, from the two row blocks of the experience buffer (no concatenated copy in memory), in a third LDS tile that neither network's activations
// touch; both 16 x 12 embeddings stay on chip (the target's in `emb`, the predictor's in its last activation tile) and one thread per row adds the 12
// squared differences in ascending j.  Every layer is first_layer / layer on the operands bg_actor_sample_mlp_scan has on a contiguous copy of the
// rows, so both embeddings are that launch's means, bit for bit.  LDS: 3 x 16 x (MAXW + 4) floats + 768 B = 50 kB at MAXW = 256, 99 kB at 512.
// The in-place add runs in float64 ((double)rew + (double)weight * inv_sigma * rho, the product of three fp32 numbers rounded once at 2^-53) and is
// rounded to fp32 once, whatever the signs of the two terms.
struct RndNets { ActorNet target, pred; };
template <int MAXW>
__global__ __launch_bounds__(256) void rnd_reward_kernel(int N, const float* __restrict__ obs, int obs_cols, const float* __restrict__ priv, int priv_cols, RndNets nets,
                                                         const uint8_t* __restrict__ dones, const float* __restrict__ reward_stats, float weight,
                                                         float* __restrict__ target_out, float* __restrict__ intrinsic, float* __restrict__ rewards) {
    constexpr int LDA = MAXW + 4;
    __shared__ __attribute__((aligned(16))) float xt[MR * LDA];
    __shared__ __attribute__((aligned(16))) float buf[2][MR * LDA];
    __shared__ float emb[MR * BG_NUM_DOFS];
    const int r0 = blockIdx.x * MR, K = obs_cols + priv_cols, KP = (K + KC - 1) / KC * KC;  // (KP <= MAXW: host)
    for (int k = threadIdx.x; k < MR * KP; k += blockDim.x) {
        const int r = k / KP, c = k - r * KP;
        float v = 0.f;
        if (r0 + r < N) {
            if (c < obs_cols) v = obs[(size_t)(r0 + r) * obs_cols + c];
            else if (c < K) v = priv[(size_t)(r0 + r) * priv_cols + c - obs_cols];
        }
        xt[r * LDA + c] = v;
    }
    __syncthreads();
    int cur = run_layers_keep<LDA>(nets.target, xt, buf);
    if (threadIdx.x < MR * BG_NUM_DOFS) {
        const int r = threadIdx.x / BG_NUM_DOFS, j = threadIdx.x % BG_NUM_DOFS;
        const float v = buf[cur][r * LDA + j];
        emb[threadIdx.x] = v;
        if (r0 + r < N) target_out[(size_t)(r0 + r) * BG_NUM_DOFS + j] = v;
    }
    __syncthreads();  // (the predictor's first layer overwrites buf[0])
    cur = run_layers_keep<LDA>(nets.pred, xt, buf);
    if (threadIdx.x < MR && r0 + (int)threadIdx.x < N) {
        const int r = threadIdx.x, row = r0 + r;
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < BG_NUM_DOFS; j++) {
            const float d = buf[cur][r * LDA + j] - emb[r * BG_NUM_DOFS + j];
            ss = fmaf(d, d, ss);
        }
        const bool done = dones[row] != 0;  // the successor row opens the next episode: reaching a reset is not novelty
        const float rho = done ? 0.f : sqrtf(ss);
        intrinsic[row] = rho;
        if (weight != 0.f && !done) {
            const double scale = (double)weight * (double)(reward_stats ? reward_stats[2] : 1.f);
            rewards[row] = (float)((double)rewards[row] + scale * (double)rho);
        }
    }
}

// ---- a recurrent student (distillation.student_memory, torch.nn.GRUCell(47, H) in front of the trunk): bg_actor_sample_gru, bg_distill_act_gru.
// The same 16 rows per workgroup and the same pieces: the x-side gate pre-activations gi = x W_ih^T + b_ih [16][3H] are first_layer's scalar-load form
// without the ELU on the 48-column tile of the newest observation, the h-side gh = h W_hh^T + b_hh [16][3H] are layer's form on the LDS tile of h, the
// gate arithmetic (bg_gru.h) runs on the two tiles, h' goes to memory and, in place of h, is the input tile of the trunk, whose every layer is
// `layer` (its first takes H inputs, a multiple of 128).  LDS: gi | gh | h | x; the trunk's two activation tiles lie over gi once the gates are done.
//   floats: max(16 (3H + 4), 2 x 16 (MAXW + 4)) + 16 (3H + 4) + 16 (H + 4) + 16 x 52
//   H = 128: 68 kB (MAXW = 256), 100 kB (512); H = 256: 116 kB (256), 132 kB (512), of the CU's 160 kB: one workgroup per CU at H = 256, two at 128
//   with MAXW = 256.
struct GruCell { const float *W_ih, *W_hh, *b_ih, *b_hh; };

template <int H, int MAXW>
struct GruLds {
    static constexpr int LDA = MAXW + 4, LDG = 3 * H + 4, LDH = H + 4, LDX = KC + 4;  // row strides (floats), multiples of 4; the three wide ones = 4 mod 32 banks
    static constexpr int TRUNK = 2 * MR * LDA, GI = MR * LDG;
    static constexpr int A = GI > TRUNK ? GI : TRUNK, B = MR * LDG, HT = MR * LDH, X = MR * LDX;
    static constexpr int FLOATS = A + B + HT + X;
};

// One workgroup's 16 rows through the cell and the trunk.  h_in and h_out may be the same buffer: the rows are read here, in front of the first barrier,
// and written behind the second, and no other workgroup touches them.  reset (may be nullptr): a row with a non-zero entry reads h_in as zero.
template <int H, int MAXW, bool MIX>
__device__ __forceinline__ void gru_rows(float* lds, int N, int r0, const float* __restrict__ obs, int stride, const GruCell& cell, const ActorNet& net,
                                         const float* __restrict__ logstd, uint64_t seed, uint32_t counter, const uint8_t* __restrict__ reset, const float* h_in,
                                         float* h_out, float* __restrict__ mu_out, float* __restrict__ act_out, float beta, int teacher_noise) {
    using L = GruLds<H, MAXW>;
    float *gi = lds, *gh = lds + L::A, *ht = gh + L::B, *xt = ht + L::HT;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = threadIdx.x; k < MR * KC; k += blockDim.x) {
        const int r = k / KC, c = k - r * KC;
        xt[r * L::LDX + c] = (r0 + r < N && c < BG_NUM_OBS) ? obs[(size_t)(r0 + r) * stride + c] : 0.f;
    }
    for (int k = threadIdx.x; k < MR * H; k += blockDim.x) {
        const int r = k / H, c = k - r * H, row = r0 + r;
        float v = 0.f;
        if (row < N && !(reset && reset[row])) v = h_in[(size_t)row * H + c];
        ht[r * L::LDH + c] = v;
    }
    __syncthreads();
    first_layer<L::LDX, L::LDG, false>(cell.W_ih, cell.b_ih, BG_NUM_OBS, 3 * H, xt, gi, wave, lane);
    layer<L::LDH, L::LDG>(cell.W_hh, cell.b_hh, H, 3 * H, false, ht, gh, wave, lane);
    __syncthreads();
    for (int k = threadIdx.x; k < MR * H; k += blockDim.x) {
        const int r = k / H, c = k - r * H, row = r0 + r;
        const float *a = gi + r * L::LDG + c, *b = gh + r * L::LDG + c;
        const bg::GruGates g = bg::gru_gates(a[0], a[H], a[2 * H], b[0], b[H], b[2 * H], ht[r * L::LDH + c]);
        ht[r * L::LDH + c] = g.h;
        if (row < N) h_out[(size_t)row * H + c] = g.h;
    }
    __syncthreads();
    float(*buf)[MR * L::LDA] = reinterpret_cast<float(*)[MR * L::LDA]>(lds);  // (over gi, which nobody reads any more)
    layer<L::LDH, L::LDA>(net.W[0], net.b[0], H, net.out[0], true, ht, buf[0], wave, lane);
    __syncthreads();
    int cur = 0;
    for (int l = 1; l < net.n; l++) {
        layer<L::LDA>(net.W[l], net.b[l], net.in[l], net.out[l], l + 1 < net.n, buf[cur], buf[cur ^ 1], wave, lane);
        __syncthreads();
        cur ^= 1;
    }
    sample<L::LDA, MIX>(buf[cur], N, r0, logstd, seed, counter, mu_out, act_out, false, beta, teacher_noise);
}

template <int H, int MAXW>
__global__ __launch_bounds__(256) void actor_gru_sample_kernel(int N, const float* __restrict__ obs, int stride, GruCell cell, ActorNet net,
                                                               const float* __restrict__ logstd, uint64_t seed, uint32_t counter, const uint8_t* __restrict__ reset,
                                                               const float* h_in, float* h_out, float* __restrict__ mu_out, float* __restrict__ act_out) {
    __shared__ __attribute__((aligned(16))) float lds[GruLds<H, MAXW>::FLOATS];
    gru_rows<H, MAXW, false>(lds, N, blockIdx.x * MR, obs, stride, cell, net, logstd, seed, counter, reset, h_in, h_out, mu_out, act_out, 0.f, 0);
}

// bg_distill_act_gru: distill_act_mix_kernel's split grid (MIX = false: distill_act_kernel's) with the recurrent student in the second half.  The
// teacher's half is actor_rows' sequence of pieces on the front of the same LDS block.  sobs / sstride: the rows the cell reads its 47 inputs from: the
// teacher's own (bg_distill_act_gru) or the student's buffer (bg_distill_act_gru_own: a student row that is no prefix of the teacher's).
template <int H, int MAXW, bool MIX>
__global__ __launch_bounds__(256) void distill_act_gru_kernel(int N, int nb, const float* __restrict__ obs, int stride, const float* __restrict__ sobs, int sstride,
                                                              DistillNets nets, GruCell cell,
                                                              const float* __restrict__ logstd, uint64_t seed, uint32_t counter, float beta, int teacher_noise,
                                                              const uint8_t* __restrict__ reset, const float* h_in, float* h_out, float* __restrict__ student_mu,
                                                              float* __restrict__ act_out, float* __restrict__ teacher_mu) {
    using L = GruLds<H, MAXW>;
    __shared__ __attribute__((aligned(16))) float lds[L::FLOATS];
    if ((int)blockIdx.x < nb) {
        const int r0 = blockIdx.x * MR;
        float(*buf)[MR * L::LDA] = reinterpret_cast<float(*)[MR * L::LDA]>(lds);
        load_tile<L::LDA>(buf[0], N, r0, obs, stride, nets.n[0].in[0], nullptr, nets.n[0].in[0]);
        const int cur = run_layers<L::LDA>(nets.n[0], buf, 0);
        sample<L::LDA, MIX>(buf[cur], N, r0, logstd, seed, counter, teacher_mu, MIX ? act_out : nullptr, true, beta, teacher_noise);
    } else {
        gru_rows<H, MAXW, MIX>(lds, N, (blockIdx.x - nb) * MR, sobs, sstride, cell, nets.n[1], logstd, seed, counter, reset, h_in, h_out, student_mu, act_out, beta,
                               teacher_noise);
    }
}

}  // namespace

// The descriptors of one network -> ActorNet, with the width rules of the kernel; scan: the height-scan values behind the 47 H observations of a row
// (bg_env_cfg.actor_heights), 0 without them.  maxw: the widest hidden layer.  `who` heads the error messages.
// first_in > 0: the trunk behind a GRU cell, whose first layer takes the first_in = H values of the hidden state (a 16-byte aligned matrix as the others).
// any_in: a network on a state row (bg_rnd_reward), whose first layer takes any 1 to BG_ACTOR_MAX_INPUT columns.
static int fill_net(const char* who, int32_t n_layers, const bg_mlp_layer_desc* layers, int32_t scan, ActorNet& net, int& maxw, int32_t first_in = 0,
                    bool any_in = false) {
    const std::string w(who);
    if (n_layers < 3 || n_layers > MAX_LAYERS) return bg_set_error(-4, (w + ": 2 to 4 hidden layers (n_layers 3 to 5)").c_str());
    net = ActorNet{};
    net.n = n_layers;
    maxw = 0;
    for (int l = 0; l < n_layers; l++) {
        const bg_mlp_layer_desc& d = layers[l];
        if (!d.W || !d.b) return bg_set_error(-1, (w + ": bad argument (layer weights)").c_str());
        const bool last = l + 1 == n_layers;
        if (l == 0 && any_in ? (d.in < 1 || d.in > BG_ACTOR_MAX_INPUT) : l == 0 && first_in ? d.in != first_in : l == 0 ? (d.in - scan < BG_NUM_OBS || d.in - scan > BG_NUM_OBS * BG_MAX_FRAME_STACK || (d.in - scan) % BG_NUM_OBS != 0 || d.in > BG_ACTOR_MAX_INPUT)
                   : d.in != layers[l - 1].out)
            return bg_set_error(-4, (w + ": layer widths do not chain (first layer: 47 H inputs, H = 1 .. 10 observation frames, and the "
                                         "height scan's points behind them, BG_ACTOR_MAX_INPUT at most)").c_str());
        if (last ? d.out != BG_NUM_DOFS : (d.out % 128 != 0 || d.out < 128 || d.out > 512))
            return bg_set_error(-4, (w + ": unsupported widths (hidden: multiples of 128 up to 512; output: 12)").c_str());
        if ((l > 0 || first_in) && ((uintptr_t)d.W & 15)) return bg_set_error(-1, (w + ": weight matrices after the first must be 16-byte aligned").c_str());
        net.W[l] = d.W; net.b[l] = d.b; net.in[l] = d.in; net.out[l] = d.out;
        if (!last && d.out > maxw) maxw = d.out;
    }
    return 0;
}

static int sample_mlp(int32_t N, const float* obs, int32_t n_layers, const bg_mlp_layer_desc* layers, int32_t scan, const float* logstd, uint64_t seed,
                      uint64_t counter, float* mu, float* actions, void* stream) {
    if (N <= 0 || !obs || !layers || !logstd || !actions) return bg_set_error(-1, "bg_actor_sample_mlp: bad argument");
    ActorNet net;
    int maxw = 0;
    if (const int rc = fill_net("bg_actor_sample_mlp", n_layers, layers, scan, net, maxw)) return rc;
    const dim3 grid((N + MR - 1) / MR), block(256);
    hipStream_t st = (hipStream_t)stream;
    const int kp = (layers[0].in + KC - 1) / KC * KC;  // the input tile's columns: within the 256-wide form's LDS tile up to 5 frames (240)
    if (maxw <= 256 && kp <= 256) hipLaunchKernelGGL(actor_mlp_sample_kernel<256>, grid, block, 0, st, N, obs, net, logstd, seed, (uint32_t)counter, mu, actions);
    else hipLaunchKernelGGL(actor_mlp_sample_kernel<512>, grid, block, 0, st, N, obs, net, logstd, seed, (uint32_t)counter, mu, actions);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_actor_sample_mlp(int32_t N, const float* obs, int32_t n_layers, const bg_mlp_layer_desc* layers, const float* logstd, uint64_t seed,
                                   uint64_t counter, float* mu, float* actions, void* stream) {
    return sample_mlp(N, obs, n_layers, layers, 0, logstd, seed, counter, mu, actions, stream);
}

extern "C" int bg_actor_sample_mlp_scan(int32_t N, const float* obs, int32_t n_layers, const bg_mlp_layer_desc* layers, int32_t scan_points,
                                        const float* logstd, uint64_t seed, uint64_t counter, float* mu, float* actions, void* stream) {
    if (scan_points < 0 || scan_points > BG_MAX_HEIGHT_SCAN_POINTS) return bg_set_error(-1, "bg_actor_sample_mlp_scan: bad argument (scan_points)");
    return sample_mlp(N, obs, n_layers, layers, scan_points, logstd, seed, counter, mu, actions, stream);
}

extern "C" int bg_actor_sample_est(int32_t N, const float* obs, int32_t n_est, const bg_mlp_layer_desc* est, int32_t est_cols, int32_t n_actor,
                                   const bg_mlp_layer_desc* actor, const float* logstd, uint64_t seed, uint64_t counter, float* est_out, float* mu, float* actions,
                                   void* stream) {
    if (N <= 0 || !obs || !est || !actor || !logstd || !est_out || !actions) return bg_set_error(-1, "bg_actor_sample_est: bad argument");
    if (est_cols < 1 || est_cols > BG_NUM_DOFS) return bg_set_error(-1, "bg_actor_sample_est: bad argument (est_cols: 1 to 12 of the estimator's outputs)");
    EstNets nets;
    int maxw_e = 0, maxw_a = 0;
    if (const int rc = fill_net("bg_actor_sample_est (estimator)", n_est, est, 0, nets.est, maxw_e)) return rc;
    if (const int rc = fill_net("bg_actor_sample_est (actor)", n_actor, actor, est_cols, nets.actor, maxw_a)) return rc;
    if (actor[0].in != est[0].in + est_cols)
        return bg_set_error(-4, "bg_actor_sample_est (actor): the first layer takes the estimator's 47 H observation columns and est_cols estimates behind them");
    const dim3 grid((N + MR - 1) / MR), block(256);
    hipStream_t st = (hipStream_t)stream;
    // one LDS form for both networks: the wider hidden layer of the two and the actor's input tile (the wider of the two tiles)
    const int kp = (actor[0].in + KC - 1) / KC * KC, maxw = maxw_e > maxw_a ? maxw_e : maxw_a;
    if (maxw <= 256 && kp <= 256)
        hipLaunchKernelGGL(actor_est_sample_kernel<256>, grid, block, 0, st, N, obs, nets, logstd, seed, (uint32_t)counter, est_out, mu, actions);
    else
        hipLaunchKernelGGL(actor_est_sample_kernel<512>, grid, block, 0, st, N, obs, nets, logstd, seed, (uint32_t)counter, est_out, mu, actions);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_rnd_reward(int32_t N, const float* obs, int32_t obs_cols, const float* priv, int32_t priv_cols, int32_t n_target, const bg_mlp_layer_desc* target,
                             int32_t n_pred, const bg_mlp_layer_desc* predictor, const uint8_t* dones, const float* reward_stats, float weight, float* target_out,
                             float* intrinsic, float* rewards, void* stream) {
    if (N <= 0 || !obs || !target || !predictor || !dones || !target_out || !intrinsic || !rewards) return bg_set_error(-1, "bg_rnd_reward: bad argument");
    if (obs_cols < 1 || priv_cols < 0 || (priv_cols > 0) != (priv != nullptr))
        return bg_set_error(-1, "bg_rnd_reward: bad argument (obs_cols at least 1; priv NULL with priv_cols 0 and only then)");
    uint32_t wbits;
    memcpy(&wbits, &weight, sizeof wbits);  // (a bit test: this file is compiled with -ffinite-math-only)
    if ((wbits >> 31) ? wbits != 0x80000000u : (wbits & 0x7f800000u) == 0x7f800000u)
        return bg_set_error(-1, "bg_rnd_reward: bad argument (weight: a finite number >= 0)");
    const int64_t K = (int64_t)obs_cols + priv_cols;
    if (K > BG_ACTOR_MAX_INPUT) return bg_set_error(-4, "bg_rnd_reward: the state row obs_cols + priv_cols exceeds BG_ACTOR_MAX_INPUT");
    RndNets nets;
    int maxw_t = 0, maxw_p = 0;
    if (const int rc = fill_net("bg_rnd_reward (target)", n_target, target, 0, nets.target, maxw_t, 0, true)) return rc;
    if (const int rc = fill_net("bg_rnd_reward (predictor)", n_pred, predictor, 0, nets.pred, maxw_p, 0, true)) return rc;
    if (target[0].in != K) return bg_set_error(-4, "bg_rnd_reward (target): the first layer takes the obs_cols + priv_cols columns of the state row");
    if (predictor[0].in != K) return bg_set_error(-4, "bg_rnd_reward (predictor): the first layer takes the obs_cols + priv_cols columns of the state row");
    const dim3 grid((N + MR - 1) / MR), block(256);
    hipStream_t st = (hipStream_t)stream;
    // one LDS form for both networks: the wider hidden layer of the two and the padded state tile
    const int kp = ((int)K + KC - 1) / KC * KC, maxw = maxw_t > maxw_p ? maxw_t : maxw_p;
    if (maxw <= 256 && kp <= 256)
        hipLaunchKernelGGL(rnd_reward_kernel<256>, grid, block, 0, st, N, obs, obs_cols, priv, priv_cols, nets, dones, reward_stats, weight, target_out, intrinsic, rewards);
    else
        hipLaunchKernelGGL(rnd_reward_kernel<512>, grid, block, 0, st, N, obs, obs_cols, priv, priv_cols, nets, dones, reward_stats, weight, target_out, intrinsic, rewards);
    HIP_OK(hipGetLastError());
    return 0;
}

// The distillation entry points: DA_PLAIN = bg_distill_act (sobs = obs, sstride = stride), DA_HIST = bg_distill_act_hist (the student's own buffer),
// DA_MIX = bg_distill_act_mix (DA_HIST's rows and rules, the teacher acting with probability beta).
enum { DA_PLAIN = 0, DA_HIST = 1, DA_MIX = 2 };
static int distill_act(int kind, float beta, int32_t teacher_noise, int32_t N, const float* obs, int32_t stride, const float* sobs, int32_t sstride, int32_t n_student, const bg_mlp_layer_desc* student,
                       int32_t n_teacher, const bg_mlp_layer_desc* teacher, int32_t scan_points, const float* student_logstd, uint64_t seed, uint64_t counter,
                       float* student_mu, float* actions, float* teacher_mu, void* stream) {
    const bool hist = kind != DA_PLAIN;
    const std::string who(kind == DA_MIX ? "bg_distill_act_mix" : hist ? "bg_distill_act_hist" : "bg_distill_act");
    if (kind == DA_MIX && !(beta >= 0.f && beta <= 1.f))  // (a NaN fails both comparisons)
        return bg_set_error(-1, (who + ": bad argument (beta: the teacher's probability of acting, a finite number in [0, 1])").c_str());
    if (N <= 0 || !obs || !sobs || !student || !teacher || !student_logstd || !actions || !teacher_mu) return bg_set_error(-1, (who + ": bad argument").c_str());
    if (scan_points < 0 || scan_points > BG_MAX_HEIGHT_SCAN_POINTS) return bg_set_error(-1, (who + ": bad argument (scan_points)").c_str());
    DistillNets nets;
    int maxw_t = 0, maxw_s = 0;
    if (const int rc = fill_net((who + " (teacher)").c_str(), n_teacher, teacher, scan_points, nets.n[0], maxw_t)) return rc;
    if (const int rc = fill_net((who + " (student)").c_str(), n_student, student, 0, nets.n[1], maxw_s)) return rc;
    if (!hist) {
        if (stride != teacher[0].in)
            return bg_set_error(-4, "bg_distill_act: obs_stride must equal the teacher's first-layer input (47 H + scan_points columns per row)");
        if (student[0].in != teacher[0].in - scan_points)
            return bg_set_error(-4, "bg_distill_act: the student's first layer takes the 47 H observation columns in front of the teacher's scan_points");
    } else {
        if (stride != teacher[0].in)
            return bg_set_error(-4, (who + ": teacher_stride must equal the teacher's first-layer input (47 H + scan_points columns per row)").c_str());
        // (the student on the teacher's own rows, same buffer and same stride: bg_distill_act's case, its prefix rule)
        if (sobs == obs && sstride == stride ? student[0].in != teacher[0].in - scan_points : sstride != student[0].in)
            return bg_set_error(-4, (who + ": student_stride must equal the student's first-layer input (47 Hs columns per row; or, on the teacher's "
                                          "buffer at the teacher's stride, the student's first layer takes the teacher's 47 H columns)").c_str());
        if (student[0].in < teacher[0].in - scan_points)
            return bg_set_error(-4, (who + ": the student's first layer (47 Hs) must take at least the teacher's 47 H observation columns").c_str());
    }
    const int nb = (N + MR - 1) / MR;
    const dim3 grid(2 * nb), block(256);
    hipStream_t st = (hipStream_t)stream;
    // one LDS form for both halves: the wider input tile of the two (the student's with a longer history) and the wider hidden layer of the two
    const int kin = teacher[0].in > student[0].in ? teacher[0].in : student[0].in;
    const int kp = (kin + KC - 1) / KC * KC, maxw = maxw_t > maxw_s ? maxw_t : maxw_s;
    if (kind == DA_MIX) {
        if (maxw <= 256 && kp <= 256)
            hipLaunchKernelGGL(distill_act_mix_kernel<256>, grid, block, 0, st, N, nb, obs, stride, sobs, sstride, nets, student_logstd, seed, (uint32_t)counter, beta,
                               teacher_noise, student_mu, actions, teacher_mu);
        else
            hipLaunchKernelGGL(distill_act_mix_kernel<512>, grid, block, 0, st, N, nb, obs, stride, sobs, sstride, nets, student_logstd, seed, (uint32_t)counter, beta,
                               teacher_noise, student_mu, actions, teacher_mu);
    } else if (maxw <= 256 && kp <= 256)
        hipLaunchKernelGGL(distill_act_kernel<256>, grid, block, 0, st, N, nb, obs, stride, sobs, sstride, nets, student_logstd, seed, (uint32_t)counter, student_mu, actions, teacher_mu);
    else
        hipLaunchKernelGGL(distill_act_kernel<512>, grid, block, 0, st, N, nb, obs, stride, sobs, sstride, nets, student_logstd, seed, (uint32_t)counter, student_mu, actions, teacher_mu);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_distill_act(int32_t N, const float* obs, int32_t obs_stride, int32_t n_student, const bg_mlp_layer_desc* student, int32_t n_teacher,
                              const bg_mlp_layer_desc* teacher, int32_t scan_points, const float* student_logstd, uint64_t seed, uint64_t counter,
                              float* student_mu, float* actions, float* teacher_mu, void* stream) {
    return distill_act(DA_PLAIN, 0.f, 0, N, obs, obs_stride, obs, obs_stride, n_student, student, n_teacher, teacher, scan_points, student_logstd, seed, counter, student_mu,
                       actions, teacher_mu, stream);
}

extern "C" int bg_distill_act_hist(int32_t N, const float* teacher_obs, int32_t teacher_stride, const float* student_obs, int32_t student_stride, int32_t n_student,
                                   const bg_mlp_layer_desc* student, int32_t n_teacher, const bg_mlp_layer_desc* teacher, int32_t scan_points,
                                   const float* student_logstd, uint64_t seed, uint64_t counter, float* student_mu, float* actions, float* teacher_mu,
                                   void* stream) {
    return distill_act(DA_HIST, 0.f, 0, N, teacher_obs, teacher_stride, student_obs, student_stride, n_student, student, n_teacher, teacher, scan_points, student_logstd, seed,
                       counter, student_mu, actions, teacher_mu, stream);
}

extern "C" int bg_distill_act_mix(int32_t N, const float* teacher_obs, int32_t teacher_stride, const float* student_obs, int32_t student_stride, int32_t n_student,
                                  const bg_mlp_layer_desc* student, int32_t n_teacher, const bg_mlp_layer_desc* teacher, int32_t scan_points,
                                  const float* student_logstd, uint64_t seed, uint64_t counter, float beta, int32_t teacher_noise, float* student_mu,
                                  float* actions, float* teacher_mu, void* stream) {
    return distill_act(DA_MIX, beta, teacher_noise, N, teacher_obs, teacher_stride, student_obs, student_stride, n_student, student, n_teacher, teacher, scan_points,
                       student_logstd, seed, counter, student_mu, actions, teacher_mu, stream);
}

// ---- the recurrent student's entry points
static int fill_cell(const std::string& who, const bg_gru_desc* gru, GruCell& cell) {
    if (!gru || !gru->W_ih || !gru->W_hh || !gru->b_ih || !gru->b_hh) return bg_set_error(-1, (who + ": bad argument (gru)").c_str());
    if (gru->in != BG_NUM_OBS) return bg_set_error(-4, (who + ": the cell takes one observation (gru.in = 47)").c_str());
    if (gru->hidden != 128 && gru->hidden != 256) return bg_set_error(-4, (who + ": unsupported gru.hidden (128 or 256)").c_str());
    if ((uintptr_t)gru->W_hh & 15) return bg_set_error(-1, (who + ": gru.W_hh must be 16-byte aligned").c_str());
    cell = GruCell{gru->W_ih, gru->W_hh, gru->b_ih, gru->b_hh};
    return 0;
}

// the kernel template K at the cell's width and the LDS form `wide` (MAXW = 512) names
#define BG_GRU_LAUNCH(K, TAIL, ...)                                                                                  \
    do {                                                                                                             \
        if (H == 128 && !wide) hipLaunchKernelGGL((K<128, 256 TAIL>), grid, block, 0, st, __VA_ARGS__);             \
        else if (H == 128) hipLaunchKernelGGL((K<128, 512 TAIL>), grid, block, 0, st, __VA_ARGS__);                 \
        else if (!wide) hipLaunchKernelGGL((K<256, 256 TAIL>), grid, block, 0, st, __VA_ARGS__);                    \
        else hipLaunchKernelGGL((K<256, 512 TAIL>), grid, block, 0, st, __VA_ARGS__);                               \
    } while (0)
#define BG_COMMA ,

extern "C" int bg_actor_sample_gru(int32_t N, const float* obs, int32_t obs_stride, const bg_gru_desc* gru, int32_t n_layers, const bg_mlp_layer_desc* layers,
                                   const float* logstd, uint64_t seed, uint64_t counter, const uint8_t* reset, const float* h_in, float* h_out, float* mu,
                                   float* actions, void* stream) {
    const std::string who("bg_actor_sample_gru");
    if (N <= 0 || !obs || !layers || !logstd || !h_in || !h_out || !actions) return bg_set_error(-1, (who + ": bad argument").c_str());
    if (obs_stride < BG_NUM_OBS) return bg_set_error(-1, (who + ": bad argument (obs_stride: at least the 47 columns the cell reads)").c_str());
    GruCell cell;
    if (const int rc = fill_cell(who, gru, cell)) return rc;
    ActorNet net;
    int maxw = 0;
    if (const int rc = fill_net((who + " (trunk)").c_str(), n_layers, layers, 0, net, maxw, gru->hidden)) return rc;
    const int H = gru->hidden;
    const bool wide = maxw > 256;
    const dim3 grid((N + MR - 1) / MR), block(256);
    hipStream_t st = (hipStream_t)stream;
    BG_GRU_LAUNCH(actor_gru_sample_kernel, , N, obs, obs_stride, cell, net, logstd, seed, (uint32_t)counter, reset, h_in, h_out, mu, actions);
    HIP_OK(hipGetLastError());
    return 0;
}

// who: the entry point's name; student_obs / student_stride: the rows of the cell's 47 inputs (bg_distill_act_gru: the teacher's)
static int distill_act_gru(const std::string& who, int32_t N, const float* teacher_obs, int32_t teacher_stride, const float* student_obs, int32_t student_stride,
                           int32_t n_teacher, const bg_mlp_layer_desc* teacher, int32_t scan_points, const bg_gru_desc* gru, int32_t n_student,
                           const bg_mlp_layer_desc* student, const float* student_logstd, uint64_t seed, uint64_t counter, float beta, int32_t teacher_noise,
                           const uint8_t* reset, const float* h_in, float* h_out, float* student_mu, float* actions, float* teacher_mu, void* stream) {
    if (!(beta >= 0.f && beta <= 1.f))  // (a NaN fails both comparisons)
        return bg_set_error(-1, (who + ": bad argument (beta: the teacher's probability of acting, a finite number in [0, 1])").c_str());
    if (N <= 0 || !teacher_obs || !student_obs || !student || !teacher || !student_logstd || !h_in || !h_out || !actions || !teacher_mu)
        return bg_set_error(-1, (who + ": bad argument").c_str());
    if (scan_points < 0 || scan_points > BG_MAX_HEIGHT_SCAN_POINTS) return bg_set_error(-1, (who + ": bad argument (scan_points)").c_str());
    GruCell cell;
    if (const int rc = fill_cell(who, gru, cell)) return rc;
    DistillNets nets;
    int maxw_t = 0, maxw_s = 0;
    if (const int rc = fill_net((who + " (teacher)").c_str(), n_teacher, teacher, scan_points, nets.n[0], maxw_t)) return rc;
    if (const int rc = fill_net((who + " (student)").c_str(), n_student, student, 0, nets.n[1], maxw_s, gru->hidden)) return rc;
    if (teacher_stride != teacher[0].in)
        return bg_set_error(-4, (who + ": teacher_stride must equal the teacher's first-layer input (47 H + scan_points columns per row)").c_str());
    if (student_stride < BG_NUM_OBS) return bg_set_error(-1, (who + ": bad argument (student_stride: at least the 47 columns the cell reads)").c_str());
    const int H = gru->hidden, nb = (N + MR - 1) / MR;
    const int kp = (teacher[0].in + KC - 1) / KC * KC, maxw = maxw_t > maxw_s ? maxw_t : maxw_s;
    const bool wide = maxw > 256 || kp > 256;
    const dim3 grid(2 * nb), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (beta > 0.f)
        BG_GRU_LAUNCH(distill_act_gru_kernel, BG_COMMA true, N, nb, teacher_obs, teacher_stride, student_obs, student_stride, nets, cell, student_logstd, seed, (uint32_t)counter, beta, teacher_noise,
                      reset, h_in, h_out, student_mu, actions, teacher_mu);
    else
        BG_GRU_LAUNCH(distill_act_gru_kernel, BG_COMMA false, N, nb, teacher_obs, teacher_stride, student_obs, student_stride, nets, cell, student_logstd, seed, (uint32_t)counter, beta, teacher_noise,
                      reset, h_in, h_out, student_mu, actions, teacher_mu);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_distill_act_gru(int32_t N, const float* teacher_obs, int32_t teacher_stride, int32_t n_teacher, const bg_mlp_layer_desc* teacher,
                                  int32_t scan_points, const bg_gru_desc* gru, int32_t n_student, const bg_mlp_layer_desc* student, const float* student_logstd,
                                  uint64_t seed, uint64_t counter, float beta, int32_t teacher_noise, const uint8_t* reset, const float* h_in, float* h_out,
                                  float* student_mu, float* actions, float* teacher_mu, void* stream) {
    return distill_act_gru("bg_distill_act_gru", N, teacher_obs, teacher_stride, teacher_obs, teacher_stride, n_teacher, teacher, scan_points, gru, n_student, student,
                           student_logstd, seed, counter, beta, teacher_noise, reset, h_in, h_out, student_mu, actions, teacher_mu, stream);
}

extern "C" int bg_distill_act_gru_own(int32_t N, const float* teacher_obs, int32_t teacher_stride, const float* student_obs, int32_t student_stride,
                                      int32_t n_teacher, const bg_mlp_layer_desc* teacher, int32_t scan_points, const bg_gru_desc* gru, int32_t n_student,
                                      const bg_mlp_layer_desc* student, const float* student_logstd, uint64_t seed, uint64_t counter, float beta,
                                      int32_t teacher_noise, const uint8_t* reset, const float* h_in, float* h_out, float* student_mu, float* actions,
                                      float* teacher_mu, void* stream) {
    return distill_act_gru("bg_distill_act_gru_own", N, teacher_obs, teacher_stride, student_obs, student_stride, n_teacher, teacher, scan_points, gru, n_student, student,
                           student_logstd, seed, counter, beta, teacher_noise, reset, h_in, h_out, student_mu, actions, teacher_mu, stream);
}

// HIP kernels + C ABI for the PPO half of the hot path (gfx950 only):
//   bg_gae            reference utils/utils.py:33-44 (discount_values) + utils/runner.py:135,144 fused into one backward scan
//   bg_ppo_loss       reference utils/runner.py:145-174 + utils/utils.py:47-52: forward AND analytic backward in one pass
//   bg_gaussian_logp  reference utils/runner.py:123-125
//   bg_actor_sample   reference utils/model.py:29-32 + dist.sample() (runner.py:109-111) as one launch
//   bg_adam_step      reference utils/runner.py:162-165 (clip_grad_norm_ + torch.optim.Adam.step) on a flat buffer
//   bg_adapt_lr       reference utils/runner.py:174-180 without the host sync
// All of these are HBM/latency-bound elementwise or scan work; none is reshaped into a GEMM.
#include <hip/hip_runtime.h>
#include <string>

#include "bg_optim.h"
#include "bg_ppo_math.h"
#include "bg_reduce.h"
#include "bg_rng.h"
#include "bg_stamps.h"

// ------------------------------------------------------------------ block reduction helper (wave64; wave_sum_d: bg_reduce.h)
template <int NV>
__device__ __forceinline__ void block_atomic_add(double (&v)[NV], double* dst, double* smem /*[NV * waves]*/) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = (blockDim.x + 63) >> 6;
    for (int k = 0; k < NV; k++) {
        double s = wave_sum_d(v[k]);
        if (lane == 0) smem[k * waves + wave] = s;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        double s = 0;
        for (int w = 0; w < waves; w++) s += smem[threadIdx.x * waves + w];
        atomicAdd(&dst[threadIdx.x], s);
    }
}

// ------------------------------------------------------------------ GAE: one lane per env, backward scan over T
// The scan is a chain of T dependent steps per env, and it sits on the critical path of every mini-epoch (the actor's loss waits for the
// advantages).  All 4 T loads of a lane are independent of the chain, so they are issued up front into registers (TMAX-way unrolled) and the
// chain then runs on registers: one memory latency per launch instead of T of them (25 -> ~5 us at T = 24, N = 4096).
template <int TMAX>
__global__ __launch_bounds__(64) void gae_kernel(int T, int N, float* __restrict__ rewards, const uint8_t* __restrict__ dones,
                                                 const uint8_t* __restrict__ touts, const float* __restrict__ values,
                                                 const float* __restrict__ last_values, float gamma, float lam, float* __restrict__ adv,
                                                 float* __restrict__ ret, double* __restrict__ sums) {
    __shared__ double sm[3 * 4];
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    double acc[3] = {0.0, 0.0, 0.0};
    if (e < N) {
        float v[TMAX], r[TMAX];
        uint8_t dn[TMAX], to[TMAX];
#pragma unroll
        for (int t = 0; t < TMAX; t++)
            if (t < T) {
                const size_t k = (size_t)t * N + e;
                v[t] = values[k]; r[t] = rewards[k]; dn[t] = dones[k]; to[t] = touts[k];
            }
        float next_v = last_values[e], last_adv = 0.f;
#pragma unroll
        for (int t = TMAX - 1; t >= 0; t--)
            if (t < T) {
                const size_t k = (size_t)t * N + e;
                float rr = r[t];
                if (to[t]) { rr = v[t]; rewards[k] = v[t]; }  // runner.py:135 (in place, repeated every mini-epoch with the current critic)
                const float nn = (dn[t] != 0 || to[t] != 0) ? 0.f : 1.f;
                const float delta = rr + gamma * nn * next_v - v[t];
                last_adv = delta + gamma * lam * nn * last_adv;
                adv[k] = last_adv;
                ret[k] = v[t] + last_adv;
                acc[0] += (double)last_adv; acc[1] += (double)last_adv * (double)last_adv; acc[2] += 1.0;
                next_v = v[t];
            }
    }
    block_atomic_add<3>(acc, sums, sm);
}
// any horizon: the plain loop (loads inside the chain)
__global__ __launch_bounds__(256) void gae_kernel_loop(int T, int N, float* __restrict__ rewards, const uint8_t* __restrict__ dones,
                                                       const uint8_t* __restrict__ touts, const float* __restrict__ values,
                                                       const float* __restrict__ last_values, float gamma, float lam, float* __restrict__ adv,
                                                       float* __restrict__ ret, double* __restrict__ sums) {
    __shared__ double sm[3 * 4];
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    double acc[3] = {0.0, 0.0, 0.0};
    if (e < N) {
        float next_v = last_values[e], last_adv = 0.f;
        for (int t = T - 1; t >= 0; t--) {
            const size_t k = (size_t)t * N + e;
            const float v = values[k];
            const bool to = touts[k] != 0;
            float r = rewards[k];
            if (to) { r = v; rewards[k] = v; }
            const float nn = (dones[k] != 0 || to) ? 0.f : 1.f;
            const float delta = r + gamma * nn * next_v - v;
            last_adv = delta + gamma * lam * nn * last_adv;
            adv[k] = last_adv;
            ret[k] = v + last_adv;
            acc[0] += (double)last_adv; acc[1] += (double)last_adv * (double)last_adv; acc[2] += 1.0;
            next_v = v;
        }
    }
    block_atomic_add<3>(acc, sums, sm);
}

// ------------------------------------------------------------------ PPO loss forward + backward, one lane per sample
using bg::kHalfLog2Pi;

template <int A>
__global__ __launch_bounds__(256) void ppo_loss_kernel(int B, const float* __restrict__ mu, const float* __restrict__ logstd,
                                                       const float* __restrict__ actions, const float* __restrict__ old_mu,
                                                       const float* __restrict__ old_logstd, const float* __restrict__ old_logp,
                                                       const float* __restrict__ adv, const double* __restrict__ adv_stats,
                                                       const float* __restrict__ values, const float* __restrict__ returns, float e_clip,
                                                       float bound_coef, float entropy_coef, float* __restrict__ grad_mu,
                                                       float* __restrict__ grad_values, double* __restrict__ grad_logstd,
                                                       double* __restrict__ stats) {
    __shared__ double sm[(A + 5) * 4];
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    bg::ActorLossConsts<A> c;
    bg::actor_loss_consts<A>(c, B, logstd, old_logstd, adv_stats, e_clip, bound_coef);
    double acc[A + 5];
    for (int k = 0; k < A + 5; k++) acc[k] = 0.0;
    if (b < B) {
        float m[A], act[A], om[A], gmu[A];
        for (int a = 0; a < A; a++) { m[a] = mu[(size_t)b * A + a]; act[a] = actions[(size_t)b * A + a]; om[a] = old_mu[(size_t)b * A + a]; }
        bg::actor_loss_row<A>(c, m, act, om, old_logp[b], adv[b], gmu, acc);
        for (int a = 0; a < A; a++) grad_mu[(size_t)b * A + a] = gmu[a];
        const float verr = values[b] - returns[b];
        grad_values[b] = 2.0f * verr * c.invB;
        acc[A + 0] = (double)(verr * verr);
    }
    // reduce: grad_logstd[A] and stats[5]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = (blockDim.x + 63) >> 6;
    for (int k = 0; k < A + 5; k++) {
        double s = wave_sum_d(acc[k]);
        if (lane == 0) sm[k * waves + wave] = s;
    }
    __syncthreads();
    if (threadIdx.x < A + 5) {
        double s = 0;
        for (int w = 0; w < waves; w++) s += sm[threadIdx.x * waves + w];
        if (threadIdx.x < A) atomicAdd(&grad_logstd[threadIdx.x], s);
        else atomicAdd(&stats[threadIdx.x - A], s);
    }
    if (blockIdx.x == 0 && threadIdx.x < A) atomicAdd(&grad_logstd[threadIdx.x], (double)entropy_coef);  // d(entropy.mean())/dlogstd = 1
}

template <int A>
__global__ void gaussian_logp_kernel(int B, const float* __restrict__ mu, const float* __restrict__ logstd, const float* __restrict__ actions,
                                     float* __restrict__ logp) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float s = 0.f;
    for (int a = 0; a < A; a++) {
        const float d = actions[(size_t)b * A + a] - mu[(size_t)b * A + a];
        const float sg = expf(logstd[a]);
        s += -0.5f * d * d / (sg * sg) - logstd[a] - kHalfLog2Pi;
    }
    logp[b] = s;
}

// ------------------------------------------------------------------ fused actor MLP + Gaussian sample (rollout inference), fp32 MFMA
// One workgroup (4 waves) = 16 observation rows; activations ping-pong between two LDS tiles; every wave owns output-neuron
// tiles of 16 and accumulates them with v_mfma_f32_16x16x4_f32 (exact fp32, D = A*B + C):
//     A[i = lane & 15][k = lane >> 4] = X[row i][k]          (from LDS, one ds_read_b128 feeds 4 MFMAs)
//     B[k = lane >> 4][j = lane & 15] = W[neuron j][k]       (from the packed copy below, one 16-byte load feeds 4 MFMAs)
//     C/D: neuron j = lane & 15, row i = (lane >> 4) * 4 + reg
// The k index inside a group of 16 is permuted identically for A and B (k = 16 t + 4 (lane >> 4) + step), which a sum over k allows.
// 992 MFMAs per workgroup.
//
// The weights come from a PACKED copy (bg_actor_pack, once per rollout; BG_ACTOR_PACKED_FLOATS floats), laid out in the order the lanes consume them, so
// that every weight load of a wave is one 16-byte load per lane at consecutive addresses (1 kB per instruction).  As torch keeps them ([out][in]) the same
// operands are 16-byte pieces 64 to 1,024 bytes apart, and the 47-column first layer 48 single dwords per lane: 16 cache lines touched per load instruction,
// by every workgroup of every launch.  Layout, `wave` and tile slot j as in the kernel (tile = wave + 4 j), neuron n = 16 tile + (lane & 15):
//     layer 0   float4 [4 waves][4 j][3 q][64 lanes]: component c = W0[n][4 (4 q + c) + (lane >> 4)], column 47 (q = 2, c = 3, lanes 48 .. 63) zero
//     layer L   float4 [waves][NT j][K / 16 t][64 lanes]: component c = WL[n][16 t + 4 (lane >> 4) + c]; zero where n is no neuron (the 12-neuron output
//               layer: lanes with lane & 15 >= 12); the output layer keeps wave 0 only, the only wave with a tile of it
//     biases    float [waves][NT j][64 lanes] = b[n] behind every layer's weights; logstd [12] (+ 4 zeros) at the end
constexpr int AROWS = 16;
constexpr int ALD = 260;  // LDS row stride (floats)
__device__ __forceinline__ float elu(float x) { return x > 0.f ? x : expm1f(x); }

// A layer = its weight fetch (from the packed copy in L2 into registers, nothing of it depends on the activations) and its MFMAs.  The two are separate
// calls so that the kernel can issue layer L + 1's fetch BEFORE it computes layer L: with fetch and MFMAs back to back per tile (the first form of this
// kernel) a workgroup spent ~1 us of exposed L2 latency per tile, 9 tiles per wave.  K % 16 == 0; tiles of 16 neurons, tile = wave + 4 j.
template <int K, int OUT, int WAVES = 4>
struct LayerW {
    static constexpr int TILES = (OUT + 15) / 16, NT = (TILES + 3) / 4, G = K / 16;
    static constexpr int W_FLOATS = WAVES * NT * G * 256, FLOATS = W_FLOATS + WAVES * NT * 64;  // packed: weights, then biases
    float4 b[NT][G];
    float bias[NT];
    __device__ __forceinline__ void fetch(const float* __restrict__ pk, int wave, int lane) {
#pragma unroll
        for (int j = 0; j < NT; j++) {
#pragma unroll
            for (int t = 0; t < G; t++) b[j][t] = reinterpret_cast<const float4*>(pk)[((wave * NT + j) * G + t) * 64 + lane];
            bias[j] = pk[W_FLOATS + (wave * NT + j) * 64 + lane];
        }
    }
    // packed element e of this layer, from the torch layout
    static __device__ __forceinline__ float packed(int e, const float* __restrict__ W, const float* __restrict__ bv) {
        const bool is_w = e < W_FLOATS;
        if (!is_w) e -= W_FLOATS;
        const int c = e & 3, lane = is_w ? (e >> 2) & 63 : e & 63, rest = is_w ? e >> 8 : e >> 6;
        const int t = is_w ? rest % G : 0, wj = is_w ? rest / G : rest, j = wj % NT, wave = wj / NT;
        const int tile = wave + 4 * j, n = tile * 16 + (lane & 15);
        if (tile >= TILES || n >= OUT) return 0.f;
        return is_w ? W[(size_t)n * K + 16 * t + 4 * (lane >> 4) + c] : bv[n];
    }
    // tile j of the wave: its MFMAs (bias + the sum over k in the order t, then x y z w of the float4) ...
    __device__ __forceinline__ f32x4 mfma(const float* in /*LDS [16][ALD]*/, int j, int lane) const {
        const int r = lane & 15, kg = lane >> 4;
        f32x4 acc = {bias[j], bias[j], bias[j], bias[j]};
#pragma unroll
        for (int t = 0; t < G; t++) {
            const float4 a = *reinterpret_cast<const float4*>(in + r * ALD + 16 * t + 4 * kg);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[j][t].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[j][t].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[j][t].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[j][t].w, acc, 0, 0, 0);
        }
        return acc;
    }
    // ... and its epilogue: the activation and the transposing store into the next layer's input tile
    template <bool ACT>
    __device__ __forceinline__ void store(float* out /*LDS [16][ALD]*/, int tile, int lane, f32x4 acc) const {
        const int r = lane & 15, kg = lane >> 4;
#pragma unroll
        for (int q = 0; q < 4; q++) out[(kg * 4 + q) * ALD + tile * 16 + r] = ACT ? elu(acc[q]) : acc[q];
    }
};

// first layer: K = 47, padded to 48 with a zero column in the packed copy; MFMA step s2 takes column 4 s2 + (lane >> 4)
template <int K, int OUT>
struct FirstLayerW {
    static constexpr int TILES = OUT / 16, NT = TILES / 4, STEPS = (K + 3) / 4, Q = STEPS / 4;
    static constexpr int W_FLOATS = 4 * NT * Q * 256, FLOATS = W_FLOATS + 4 * NT * 64;
    static_assert(STEPS % 4 == 0, "the packed first layer holds whole float4s of MFMA steps");
    float b[NT][STEPS];
    float bias[NT];
    __device__ __forceinline__ void fetch(const float* __restrict__ pk, int wave, int lane) {
#pragma unroll
        for (int j = 0; j < NT; j++) {
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const float4 v = reinterpret_cast<const float4*>(pk)[((wave * NT + j) * Q + q) * 64 + lane];
                b[j][4 * q] = v.x; b[j][4 * q + 1] = v.y; b[j][4 * q + 2] = v.z; b[j][4 * q + 3] = v.w;
            }
            bias[j] = pk[W_FLOATS + (wave * NT + j) * 64 + lane];
        }
    }
    static __device__ __forceinline__ float packed(int e, const float* __restrict__ W, const float* __restrict__ bv) {
        const bool is_w = e < W_FLOATS;
        if (!is_w) e -= W_FLOATS;
        const int c = e & 3, lane = is_w ? (e >> 2) & 63 : e & 63, rest = is_w ? e >> 8 : e >> 6;
        const int q = is_w ? rest % Q : 0, wj = is_w ? rest / Q : rest, j = wj % NT, wave = wj / NT;
        const int n = (wave + 4 * j) * 16 + (lane & 15), k = 4 * (4 * q + c) + (lane >> 4);
        return is_w ? (k < K ? W[(size_t)n * K + k] : 0.f) : bv[n];
    }
    __device__ __forceinline__ f32x4 mfma(const float* in, int j, int lane) const {
        const int r = lane & 15, kg = lane >> 4;
        f32x4 acc = {bias[j], bias[j], bias[j], bias[j]};
#pragma unroll
        for (int s2 = 0; s2 < STEPS; s2++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(in[r * ALD + 4 * s2 + kg], b[j][s2], acc, 0, 0, 0);
        return acc;
    }
    template <bool ACT>
    __device__ __forceinline__ void store(float* out, int tile, int lane, f32x4 acc) const {
        const int r = lane & 15, kg = lane >> 4;
#pragma unroll
        for (int q = 0; q < 4; q++) out[(kg * 4 + q) * ALD + tile * 16 + r] = ACT ? elu(acc[q]) : acc[q];
    }
};

using ActorL0 = FirstLayerW<BG_NUM_OBS, 256>;
using ActorL1 = LayerW<256, 128>;
using ActorL2 = LayerW<128, 128>;
using ActorL3 = LayerW<128, BG_NUM_DOFS, 1>;  // one tile: wave 0's
constexpr int PK_L0 = 0, PK_L1 = PK_L0 + ActorL0::FLOATS, PK_L2 = PK_L1 + ActorL1::FLOATS, PK_L3 = PK_L2 + ActorL2::FLOATS, PK_LOGSTD = PK_L3 + ActorL3::FLOATS;
static_assert(PK_LOGSTD + 16 == BG_ACTOR_PACKED_FLOATS, "BG_ACTOR_PACKED_FLOATS (booster_gym_amd.h) is the packed layout's size");

__global__ __launch_bounds__(256) void actor_pack_kernel(const float* __restrict__ w0, const float* __restrict__ b0, const float* __restrict__ w1,
                                                         const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                         const float* __restrict__ w3, const float* __restrict__ b3, const float* __restrict__ logstd,
                                                         float* __restrict__ packed) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= BG_ACTOR_PACKED_FLOATS) return;
    float v;
    if (e < PK_L1) v = ActorL0::packed(e - PK_L0, w0, b0);
    else if (e < PK_L2) v = ActorL1::packed(e - PK_L1, w1, b1);
    else if (e < PK_L3) v = ActorL2::packed(e - PK_L2, w2, b2);
    else if (e < PK_LOGSTD) v = ActorL3::packed(e - PK_L3, w3, b3);
    else v = e - PK_LOGSTD < BG_NUM_DOFS ? logstd[e - PK_LOGSTD] : 0.f;
    packed[e] = v;
}

// clock stamps of actor_sample_kernel, [workgroup][wave][stamp]: tools/actor_sample_stamps.py names the slots
BG_STAMP_BUFFER(bg_actor_stamp_buf, bg_probe_read_actor_stamps, 256, 32)
// one layer: the wave's tiles wave, wave + 4, ...; stamp S + 2 j behind tile j's MFMAs, S + 2 j + 1 behind its epilogue
#define ACTOR_LAYER(L, ACT, IN, OUT, S)                                  \
    _Pragma("unroll") for (int j = 0; j < L.NT; j++) {                   \
        if (wave + 4 * j >= L.TILES) break;                              \
        const f32x4 acc = L.mfma(IN, j, lane);                           \
        BG_STAMP_FENCED((S) + 2 * j);                                    \
        L.template store<ACT>(OUT, wave + 4 * j, lane, acc);             \
        BG_STAMP_FENCED((S) + 2 * j + 1);                                \
    }

__global__ __launch_bounds__(256) void actor_sample_kernel(int N, const float* __restrict__ obs, const float* __restrict__ packed, uint64_t seed,
                                                           uint32_t counter, float* __restrict__ mu_out, float* __restrict__ act_out) {
    __shared__ __attribute__((aligned(16))) float bufA[AROWS * ALD];
    __shared__ __attribute__((aligned(16))) float bufB[AROWS * ALD];
    const int r0 = blockIdx.x * AROWS, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    BG_STAMP_LOCALS(32);
    BG_STAMP_WALL(30);
    BG_STAMP_FENCED(0);
    // every global load that does not depend on the network goes out first, in the order it is needed (the waits count loads oldest first): the sampling
    // threads' log-stds (one thread per (row, group of 4 actions)), the observation tile (k padded 47 -> 48 with zeros; rows from N on are never read),
    // then the weights of the first two layers
    const int sr = threadIdx.x / 3, sg = threadIdx.x % 3, srow = r0 + sr;
    const bool sampler = threadIdx.x < AROWS * 3 && srow < N;
    const float4 ls = reinterpret_cast<const float4*>(packed + PK_LOGSTD)[sg];  // (every thread: sg < 3, no branch in front of the loads below)
    constexpr int OBS_PER_THREAD = AROWS * 48 / 256;
    float ov[OBS_PER_THREAD];
#pragma unroll
    for (int i = 0; i < OBS_PER_THREAD; i++) {
        const int k = threadIdx.x + 256 * i, r = k / 48, c = k % 48;
        ov[i] = (r0 + r < N && c < BG_NUM_OBS) ? obs[(size_t)(r0 + r) * BG_NUM_OBS + c] : 0.f;
    }
    ActorL0 l0;
    l0.fetch(packed + PK_L0, wave, lane);
    ActorL1 l1;
    l1.fetch(packed + PK_L1, wave, lane);
    __builtin_amdgcn_sched_barrier(0);  // (the scheduler would otherwise put the exponentials, and with them a wait for the log-stds, in front of the loads)
    BG_STAMP_FENCED(1);
    // the sample's noise and standard deviations, under the latency of those loads, held until the tail
    bg::Rand4 rn = {};
    float sigma[4] = {};
    if (sampler) {
        rn = bg::rand4(seed, (uint32_t)srow, counter, bg::RS_ACTOR + sg);
        sigma[0] = expf(ls.x); sigma[1] = expf(ls.y); sigma[2] = expf(ls.z); sigma[3] = expf(ls.w);
    }
#pragma unroll
    for (int i = 0; i < OBS_PER_THREAD; i++) {
        const int k = threadIdx.x + 256 * i;
        bufA[(k / 48) * ALD + k % 48] = ov[i];
    }
    BG_STAMP_FENCED(2);
    __syncthreads();
    BG_STAMP_FENCED(3);
    // same arithmetic and order as one fetch + MFMA pass per layer; only WHEN the weights are fetched differs: a layer ahead
    ACTOR_LAYER(l0, true, bufA, bufB, 4)
    ActorL2 l2;
    l2.fetch(packed + PK_L2, wave, lane);
    BG_STAMP_FENCED(12);
    __syncthreads();
    BG_STAMP_FENCED(13);
    ACTOR_LAYER(l1, true, bufB, bufA, 14)
    ActorL3 l3;
    if (wave == 0) l3.fetch(packed + PK_L3, 0, lane);
    BG_STAMP_FENCED(18);
    __syncthreads();
    BG_STAMP_FENCED(19);
    ACTOR_LAYER(l2, true, bufA, bufB, 20)
    BG_STAMP_FENCED(24);
    __syncthreads();
    BG_STAMP_FENCED(25);
    ACTOR_LAYER(l3, false, bufB, bufA, 26)
    __syncthreads();
    BG_STAMP_FENCED(28);
    // sample: the mean from the output tile, one add and the stores
    if (sampler) {
        for (int k = 0; k < 4; k++) {
            const int a = sg * 4 + k;
            const float m = bufA[sr * ALD + a];
            if (mu_out) mu_out[(size_t)srow * BG_NUM_DOFS + a] = m;
            act_out[(size_t)srow * BG_NUM_DOFS + a] = m + sigma[k] * rn.n[k];
        }
    }
    BG_STAMP_FENCED(29);
    BG_STAMP_WALL(31);
    BG_STAMP_FLUSH(bg_actor_stamp_buf, 32, blockIdx.x < 256, blockIdx.x);
}
#undef ACTOR_LAYER

// ------------------------------------------------------------------ clip_grad_norm_ + Adam on a flat buffer
__global__ __launch_bounds__(256) void sqnorm_kernel(int n, const float* __restrict__ g, double* __restrict__ out) {
    __shared__ double sm[4];
    double acc[1] = {0.0};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) acc[0] += (double)g[i] * (double)g[i];
    block_atomic_add<1>(acc, out, sm);
}
__global__ __launch_bounds__(256) void adam_kernel(int n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, const float* __restrict__ lr_dev, float bc1, float bc2_sqrt, float beta1,
                                                   float beta2, float eps, float max_norm, const double* __restrict__ sqnorm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    adam_element(p, g, m, v, i, clip_coef(*sqnorm, max_norm), *lr_dev / bc1, beta1, beta2, bc2_sqrt, eps);
}
__global__ void adapt_lr_kernel(const double* __restrict__ kl_sum, float count, float desired, float lr_min, float lr_max, float* __restrict__ lr) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float kl = (float)(kl_sum[0] / (double)count);
    *lr = kl_rule(*lr, kl, desired, lr_min, lr_max);
}

// The whole tail of a mini-epoch in ONE launch (reference utils/runner.py:162-180: clip_grad_norm_, Adam step, KL-adaptive learning rate, plus
// this build's bookkeeping of the loss statistics).  As separate launches (memset, sqnorm, adam, adapt_lr, a stats add, two fills) these seven tiny
// dependent kernels were a serial stretch of ~60 us per mini-epoch in which the GPU was otherwise idle: 1.2 ms of a 27 ms iteration.
//   phase 1  every workgroup computes the FULL squared gradient norm itself (the 712 kB bucket is L2-resident; OPT_GRID x 712 kB of L2 reads),
//            in the same order, so all workgroups hold the bit-identical norm and the result is deterministic (no atomics, no grid barrier);
//   phase 2  Adam on the workgroup's slice with the clip coefficient;
//   tail     the last workgroup to finish (ticket counter; every workgroup has read the learning rate before it takes its ticket) applies the KL rule
//            to the learning rate, publishes / accumulates the loss statistics and zeroes the accumulators for the next mini-epoch.
// grad_logstd (optional): the log-std gradient as the head kernels leave it (float64 [ls_n]); it stands for grads[ls_off .. ls_off + ls_n).
//   mirrors  every updated parameter inside one of the caller's [rows][cols] weight matrices is also written to that matrix's mirror: a transposed
//            copy (the operand layout of the backward layer kernel) or a copy with a wider row stride (the zero-padded first layer).  Six strided torch
//            copies per mini-epoch (5-20 us each, inside the two chains) otherwise.
// The norm pass is this kernel's own; the rest of the step: bg_optim.h.  (Loose __restrict__ parameters, packed into OptArgs here: with OptArgs as the
// kernel's parameter, as tail_adam_kernel has it, the slice loop's instructions come out in another order than this kernel's always had.)
constexpr int OPT_GRID = 64;
__global__ __launch_bounds__(OPT_THREADS) void optimizer_step_kernel(int n, float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                                     float* __restrict__ v, float* __restrict__ lr_dev, float bc1, float bc2_sqrt,
                                                                     float beta1, float beta2, float eps, float max_norm,
                                                                     double* __restrict__ grad_logstd, int ls_off, int ls_n,
                                                                     double* __restrict__ stats, double* __restrict__ stats_acc,
                                                                     double* __restrict__ stats_last, int n_stats, int kl_index, float kl_count,
                                                                     float desired_kl, float lr_min, float lr_max, unsigned* __restrict__ ticket,
                                                                     ParamMirrors mir) {
    const OptArgs o = {n, p, g, m, v, lr_dev, bc1, bc2_sqrt, beta1, beta2, eps, max_norm, grad_logstd, ls_off, ls_n,
                       stats, stats_acc, stats_last, n_stats, kl_index, kl_count, desired_kl, lr_min, lr_max};
    const int t = threadIdx.x;
    const float lr = *lr_dev;  // read by every thread before this workgroup takes its ticket
    // the log-std gradient arrives in float64 from the heads: put it into the flat buffer (every workgroup writes the same values)
    if (grad_logstd && t < ls_n) g[ls_off + t] = (float)grad_logstd[t];
    __syncthreads();
    double acc = 0.0;
    const int n4 = n >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(g);
#pragma unroll 8  // 8 loads in flight (the adds stay in order): 44 dependent L2 round trips per thread otherwise
    for (int i = t; i < n4; i += OPT_THREADS) {
        const float4 x = g4[i];
        acc += (double)x.x * (double)x.x + (double)x.y * (double)x.y + (double)x.z * (double)x.z + (double)x.w * (double)x.w;
    }
    for (int i = (n4 << 2) + t; i < n; i += OPT_THREADS) acc += (double)g[i] * (double)g[i];
    opt_slice(o, mir, OPT_GRID, lr, clip_coef(opt_block_total(acc), max_norm));
    opt_last_ticket(o, lr, ticket);
}


// ------------------------------------------------------------------ MLP backward helper: g <- g * elu'(a) in place and db = column sums of g
// (replaces torch's elu_backward + the separate bias-gradient reduction: the gradient tile is read once).  elu'(z) expressed through the
// OUTPUT a = elu(z): 1 if a > 0 else a + 1.  Deterministic two-stage column sum (no float atomics).
constexpr int CS_ROWS = 128;
// generic (any C): one thread per column, used for the narrow output layers (C = 12, 1)
__global__ __launch_bounds__(256) void elu_bwd_colsum_kernel(int B, int C, float* __restrict__ g, const float* __restrict__ act,
                                                             float* __restrict__ partial /*[gridDim.x][C]*/) {
    const int r0 = blockIdx.x * CS_ROWS, r1 = min(B, r0 + CS_ROWS);
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float acc = 0.f;
        for (int r = r0; r < r1; r++) {
            const size_t k = (size_t)r * C + c;
            float v = g[k];
            if (act) { const float a = act[k]; v *= a > 0.f ? 1.0f : a + 1.0f; g[k] = v; }
            acc += v;
        }
        partial[(size_t)blockIdx.x * C + c] = acc;
    }
}
// C % 4 == 0 and C <= 256: 16-byte accesses, 1 KiB per wave instruction, 4 independent rows in flight per thread.
// thread = (row lane, column group of 4); a 256-thread block covers CS_ROWS rows.
__global__ __launch_bounds__(256) void elu_bwd_colsum_vec4_kernel(int B, int C, float* __restrict__ g, const float* __restrict__ act,
                                                                  float* __restrict__ partial) {
    __shared__ float4 sm[256];
    const int groups = C >> 2;                 // column groups per row (<= 64)
    const int lanes = 256 / groups;            // rows processed concurrently by the block
    const int cg = threadIdx.x % groups, rl = threadIdx.x / groups;
    const int r0 = blockIdx.x * CS_ROWS, r1 = min(B, r0 + CS_ROWS);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rl < lanes) {
        int r = r0 + rl;
        for (; r + 3 * lanes < r1; r += 4 * lanes) {
            float4 gv[4], av[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const size_t k = ((size_t)(r + u * lanes) * C) / 4 + cg;
                gv[u] = reinterpret_cast<const float4*>(g)[k];
                av[u] = reinterpret_cast<const float4*>(act)[k];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const size_t k = ((size_t)(r + u * lanes) * C) / 4 + cg;
                gv[u].x *= av[u].x > 0.f ? 1.0f : av[u].x + 1.0f; gv[u].y *= av[u].y > 0.f ? 1.0f : av[u].y + 1.0f;
                gv[u].z *= av[u].z > 0.f ? 1.0f : av[u].z + 1.0f; gv[u].w *= av[u].w > 0.f ? 1.0f : av[u].w + 1.0f;
                reinterpret_cast<float4*>(g)[k] = gv[u];
                acc.x += gv[u].x; acc.y += gv[u].y; acc.z += gv[u].z; acc.w += gv[u].w;
            }
        }
        for (; r < r1; r += lanes) {
            const size_t k = ((size_t)r * C) / 4 + cg;
            float4 gv = reinterpret_cast<const float4*>(g)[k];
            const float4 av = reinterpret_cast<const float4*>(act)[k];
            gv.x *= av.x > 0.f ? 1.0f : av.x + 1.0f; gv.y *= av.y > 0.f ? 1.0f : av.y + 1.0f;
            gv.z *= av.z > 0.f ? 1.0f : av.z + 1.0f; gv.w *= av.w > 0.f ? 1.0f : av.w + 1.0f;
            reinterpret_cast<float4*>(g)[k] = gv;
            acc.x += gv.x; acc.y += gv.y; acc.z += gv.z; acc.w += gv.w;
        }
    }
    sm[threadIdx.x] = acc;
    __syncthreads();
    if (rl == 0) {
        for (int l = 1; l < lanes; l++) {
            const float4 o = sm[l * groups + cg];
            acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w;
        }
        reinterpret_cast<float4*>(partial + (size_t)blockIdx.x * C)[cg] = acc;
    }
}
__global__ __launch_bounds__(256) void colsum_finish_kernel(int nb, int C, const float* __restrict__ partial, float* __restrict__ out) {
    __shared__ float sm[256];
    const int c = blockIdx.x;
    float acc = 0.f;
    for (int b = threadIdx.x; b < nb; b += blockDim.x) acc += partial[(size_t)b * C + c];
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) out[c] = sm[0];
}

// ------------------------------------------------------------------ ABI
extern "C" int bg_gae(int32_t T, int32_t N, float* rewards, const uint8_t* dones, const uint8_t* time_outs, const float* values,
                      const float* last_values, float gamma, float lam, float* advantages, float* returns, double* sums, void* stream) {
    if (T <= 0 || N <= 0 || !rewards || !dones || !time_outs || !values || !last_values || !advantages || !returns || !sums)
        return bg_set_error(-1, "bg_gae: bad argument");
    if (T <= 32)
        hipLaunchKernelGGL(gae_kernel<32>, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, T, N, rewards, dones, time_outs, values, last_values,
                           gamma, lam, advantages, returns, sums);
    else
        hipLaunchKernelGGL(gae_kernel_loop, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, T, N, rewards, dones, time_outs, values, last_values,
                           gamma, lam, advantages, returns, sums);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_ppo_loss(int32_t B, int32_t A, const float* mu, const float* logstd, const float* actions, const float* old_mu,
                           const float* old_logstd, const float* old_logp, const float* adv, const double* adv_stats, const float* values,
                           const float* returns, float e_clip, float bound_coef, float entropy_coef, float* grad_mu, float* grad_values,
                           double* grad_logstd, double* stats, void* stream) {
    if (B <= 0 || !mu || !logstd || !actions || !old_mu || !old_logstd || !old_logp || !adv || !adv_stats || !values || !returns || !grad_mu ||
        !grad_values || !grad_logstd || !stats)
        return bg_set_error(-1, "bg_ppo_loss: bad argument");
    if (A != BG_NUM_DOFS) return bg_set_error(-1, "bg_ppo_loss: this build is compiled for 12 actions");
    hipLaunchKernelGGL(ppo_loss_kernel<BG_NUM_DOFS>, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, mu, logstd, actions, old_mu,
                       old_logstd, old_logp, adv, adv_stats, values, returns, e_clip, bound_coef, entropy_coef, grad_mu, grad_values, grad_logstd,
                       stats);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_gaussian_logp(int32_t B, int32_t A, const float* mu, const float* logstd, const float* actions, float* logp, void* stream) {
    if (B <= 0 || !mu || !logstd || !actions || !logp) return bg_set_error(-1, "bg_gaussian_logp: bad argument");
    if (A != BG_NUM_DOFS) return bg_set_error(-1, "bg_gaussian_logp: this build is compiled for 12 actions");
    hipLaunchKernelGGL(gaussian_logp_kernel<BG_NUM_DOFS>, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, mu, logstd, actions, logp);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_actor_pack(const float* w0, const float* b0, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                             const float* b3, const float* logstd, float* packed, void* stream) {
    if (!w0 || !b0 || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !logstd || !packed) return bg_set_error(-1, "bg_actor_pack: bad argument");
    if ((uintptr_t)packed & 15) return bg_set_error(-1, "bg_actor_pack: the packed buffer must be 16-byte aligned");
    hipLaunchKernelGGL(actor_pack_kernel, dim3((BG_ACTOR_PACKED_FLOATS + 255) / 256), dim3(256), 0, (hipStream_t)stream, w0, b0, w1, b1, w2, b2, w3, b3,
                       logstd, packed);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_actor_sample(int32_t N, const float* obs, const float* packed, uint64_t seed, uint64_t counter, float* mu, float* actions,
                               void* stream) {
    if (N <= 0 || !obs || !packed || !actions) return bg_set_error(-1, "bg_actor_sample: bad argument");
    if ((uintptr_t)packed & 15) return bg_set_error(-1, "bg_actor_sample: the packed weights must be 16-byte aligned");
    hipLaunchKernelGGL(actor_sample_kernel, dim3((N + AROWS - 1) / AROWS), dim3(256), 0, (hipStream_t)stream, N, obs, packed, seed, (uint32_t)counter, mu,
                       actions);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_adam_step(int32_t n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const float* lr_device, int32_t step,
                            float beta1, float beta2, float eps, float max_grad_norm, double* gnorm_scratch, void* stream) {
    if (n <= 0 || !params || !grads || !exp_avg || !exp_avg_sq || !lr_device || !gnorm_scratch || step < 1)
        return bg_set_error(-1, "bg_adam_step: bad argument");
    HIP_OK(hipMemsetAsync(gnorm_scratch, 0, sizeof(double), (hipStream_t)stream));
    int blocks = (n + 255) / 256;
    hipLaunchKernelGGL(sqnorm_kernel, dim3(blocks < 256 ? blocks : 256), dim3(256), 0, (hipStream_t)stream, n, grads, gnorm_scratch);
    float bc1, bc2s;
    adam_bias_corrections(beta1, beta2, step, bc1, bc2s);
    hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, params, grads, exp_avg, exp_avg_sq, lr_device, bc1, bc2s,
                       beta1, beta2, eps, max_grad_norm, gnorm_scratch);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_adapt_lr(const double* kl_sum, float count, float desired_kl, float lr_min, float lr_max, float* lr_device, void* stream) {
    if (!kl_sum || !lr_device || !(count > 0.f)) return bg_set_error(-1, "bg_adapt_lr: bad argument");
    hipLaunchKernelGGL(adapt_lr_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, kl_sum, count, desired_kl, lr_min, lr_max, lr_device);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_optimizer_step(int32_t n, float* params, float* grads, float* exp_avg, float* exp_avg_sq, float* lr_device, int32_t step, float beta1,
                                 float beta2, float eps, float max_grad_norm, double* grad_logstd, int32_t ls_off, int32_t ls_n, double* stats,
                                 double* stats_acc, double* stats_last, int32_t n_stats, int32_t kl_index, float kl_count, float desired_kl,
                                 float lr_min, float lr_max, uint32_t* ticket, const bg_param_mirror* mirrors, int32_t n_mirrors, void* stream) {
    OptArgs o;
    ParamMirrors mir;
    if (const int rc = opt_args_fill("bg_optimizer_step", n, params, grads, exp_avg, exp_avg_sq, lr_device, step, beta1, beta2, eps, max_grad_norm, grad_logstd,
                                     ls_off, ls_n, stats, stats_acc, stats_last, n_stats, kl_index, kl_count, desired_kl, lr_min, lr_max, ticket, mirrors,
                                     n_mirrors, o, mir))
        return rc;
    if (!aligned16(grads)) return bg_set_error(-1, "bg_optimizer_step: grads must be 16-byte aligned");  // (the norm pass reads float4)
    hipLaunchKernelGGL(optimizer_step_kernel, dim3(OPT_GRID), dim3(OPT_THREADS), 0, (hipStream_t)stream, o.n, o.p, o.g, o.m, o.v, o.lr_dev, o.bc1, o.bc2_sqrt,
                       o.beta1, o.beta2, o.eps, o.max_norm, o.grad_logstd, o.ls_off, o.ls_n, o.stats, o.stats_acc, o.stats_last, o.n_stats, o.kl_index,
                       o.kl_count, o.desired_kl, o.lr_min, o.lr_max, ticket, mir);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_elu_backward_colsum(int32_t B, int32_t C, float* grad, const float* act, float* colsum, float* scratch, void* stream) {
    if (B <= 0 || C <= 0 || !grad || !colsum || !scratch) return bg_set_error(-1, "bg_elu_backward_colsum: bad argument");
    const int nb = (B + CS_ROWS - 1) / CS_ROWS;
    // (the 16-byte form only on 16-byte aligned buffers: the header promises no alignment, and the generic form needs none)
    if (act && C % 4 == 0 && C <= 256 && 256 % (C / 4) == 0 && aligned16(grad) && aligned16(act) && aligned16(scratch))
        hipLaunchKernelGGL(elu_bwd_colsum_vec4_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, B, C, grad, act, scratch);
    else
        hipLaunchKernelGGL(elu_bwd_colsum_kernel, dim3(nb), dim3(C >= 256 ? 256 : (C >= 128 ? 128 : 64)), 0, (hipStream_t)stream, B, C, grad, act, scratch);
    hipLaunchKernelGGL(colsum_finish_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, nb, C, scratch, colsum);
    HIP_OK(hipGetLastError());
    return 0;
}

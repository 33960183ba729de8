// Output ("head") layers of the two MLPs fused with the loss (gfx950 only).
//
// The 128 -> 12 (actor) and 128 -> 1 (critic) output layers of reference utils/model.py:9-26 are skinny: as library GEMMs + elementwise
// kernels they cost 7 launches per network and mini-epoch, each re-reading the [B][128] hidden activations (50 MB at B = 98,304), for work
// that is HBM-bound.  Here one launch per network reads the hidden activations once:
//   bg_actor_head           mu = h W^T + b -> PPO actor loss forward + analytic backward (runner.py:145-174, bg_ppo_math.h) ->
//                           dL/dz of the last hidden layer (g W * elu'(h)), weight / bias gradients of the output layer, bias gradient of the
//                           hidden layer, log-std gradient and the loss statistics
//   bg_critic_head_forward  values = h w + b for every row (the GAE scan between forward and backward needs all of them first)
//   bg_critic_head_backward value loss (runner.py:148) backward through the output layer into the last hidden layer
//   bg_distill_head         mu = h W^T + b -> behaviour-cloning loss mean((mu - target)^2) and its backward (teacher-student distillation,
//                           utils/distill.py): bg_actor_head's forward and backward mappings around bg_critic_head_backward's form of loss
//   bg_actor_head_sym       bg_actor_head on a batch of 2B rows (the rollout's, then their mirror images) plus the mirror-symmetry loss
//                           (algorithm.symmetry_loss); bg_mirror_rows writes the mirrored network inputs.  With the identity action map and
//                           bg_partner_rows' rows in the second half: the action-smoothness loss (algorithm.smoothness_loss)
//   bg_distill_head_sym     bg_distill_head on the original rows of such a batch of 2B rows plus the mirror-symmetry loss on the student's mean
//                           (distillation.symmetric_coef)
// Arithmetic is plain fp32 FMA on the vector ALU: 4.6 kflop per row against 1 KB of traffic is under the HBM ridge, so nothing here is
// reshaped into an MFMA GEMM.  Reductions over rows are deterministic: every workgroup writes its partial sums, a second kernel adds them
// in a fixed order (the loss statistics and the log-std gradient keep the float64 atomics of bg_ppo_loss).
#include <hip/hip_runtime.h>

#include "bg_ppo_math.h"
#include "bg_reduce.h"
#include "bg_rng.h"

namespace {

constexpr int HK = 128;    // hidden width (both networks end in a 128-wide ELU layer)
constexpr int HT = 64;     // rows per tile
constexpr int HTS = HT / 2;  // pairs per tile of the heads with a mirror-symmetry term: HTS rows and their HTS mirror images
constexpr int HLD = 132;   // LDS row stride of the activation tile: 16-byte aligned, rows 4 banks apart
constexpr int HA = BG_NUM_DOFS;
constexpr int HEAD_MAX_GRID = 768;

__device__ __forceinline__ float elu_grad_from_output(float a) { return a > 0.f ? 1.0f : a + 1.0f; }
// dL/dz of an ELU layer from dL/d(its output hv)
__device__ __forceinline__ float elu_back(float g, float hv) { return g * elu_grad_from_output(hv); }

// coalesced load of a [HT][HK] activation tile into LDS (rows past B read as zero), in two halves so that a persistent workgroup can have the
// NEXT tile's 8 float4 per thread in flight while it computes on the current one (tile_fetch before the compute, tile_put after it)
constexpr int HTV = HT * HK / 4 / 256;
__device__ __forceinline__ void tile_fetch(const float* __restrict__ h, int row0, int B, float4 (&v)[HTV]) {
#pragma unroll
    for (int i = 0; i < HTV; i++) {
        const int idx = threadIdx.x + 256 * i, r = idx >> 5, c4 = idx & 31;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + r < B) v[i] = *reinterpret_cast<const float4*>(h + (size_t)(row0 + r) * HK + c4 * 4);
    }
}
__device__ __forceinline__ void tile_put(const float4 (&v)[HTV], float* s_h) {
#pragma unroll
    for (int i = 0; i < HTV; i++) {
        const int idx = threadIdx.x + 256 * i, r = idx >> 5, c4 = idx & 31;
        *reinterpret_cast<float4*>(s_h + r * HLD + c4 * 4) = v[i];
    }
}
__device__ __forceinline__ void load_tile(const float* __restrict__ h, int row0, int B, float* s_h) {
    float4 v[HTV];
    tile_fetch(h, row0, B, v);
    tile_put(v, s_h);
}
// the pair tile of the heads with a mirror-symmetry term: LDS rows [0, HTS) from rows row0 .. of h, LDS rows [HTS, 2 HTS) from rows B + row0 ..
__device__ __forceinline__ void pair_fetch(const float* __restrict__ h, int row0, int B, float4 (&v)[HTV]) {
#pragma unroll
    for (int i = 0; i < HTV; i++) {
        const int idx = threadIdx.x + 256 * i, r = idx >> 5, c4 = idx & 31, o = row0 + (r & (HTS - 1));
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (o < B) v[i] = *reinterpret_cast<const float4*>(h + (size_t)(r < HTS ? o : B + o) * HK + c4 * 4);
    }
}
__device__ __forceinline__ void load_pair_tile(const float* __restrict__ h, int row0, int B, float* s_h) {
    float4 v[HTV];
    pair_fetch(h, row0, B, v);
    tile_put(v, s_h);
}

// Per-workgroup partial sums, added in a fixed order by reduce_group_kernel.  scratch = [HEAD_MAX_GRID records of head_record<NO>() floats:
// [NO][HK] output-layer weight gradient, [HK] hidden bias gradient, [NO] output bias gradient] followed by the float64 loss statistics,
// statistic-major [HEAD_NSTAT][groups].  (Float64 atomics from every workgroup on the 17 shared addresses cost 45-60 us per launch.)
constexpr int HEAD_NSTAT = HA + 5;
template <int NO> constexpr int head_record() { return NO * HK + HK + 16; }
template <int NO> constexpr size_t head_stat_base() { return (size_t)HEAD_MAX_GRID * head_record<NO>(); }  // even: float64 aligned

__device__ __forceinline__ float quad_sum(float v) {  // sum over the 4 lanes of a quad (DPP quad_perm)
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));  // [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));  // [2,3,0,1]
    return v;
}
// sum over the 16 lanes of a wave that share (lane & 3); valid in lanes 0..3
__device__ __forceinline__ double quadcol_sum(double v) {
    for (int o = 32; o >= 4; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float quadcol_sum(float v) {
    for (int o = 32; o >= 4; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- The four loss heads on the 12-wide actor output (actor_head_kernel, distill_head_kernel and their _sym forms) are one kernel around different
// loss lines; what they share stands here once, as functions on the kernels' own registers and LDS arrays.
// Thread mappings: forward + loss: thread = (row fr = t >> 2 of the tile, actions 3 fq .. 3 fq + 2, fq = t & 3), the four threads of a row exchange their
// partial sums with two DPP moves; backward: thread = (hidden column kc = t & 127, row half = t >> 7) with its column of W (wcol) and its accumulators (dW,
// cs) in registers for the whole launch.
// Two pieces stand twice.  The PPO row loss with its constants, in actor_head_kernel<1> and actor_head_sym_kernel: as a function, or on a struct of the
// thread's state, it compiled to other sums (the build's -fassociative-math groups the loop-invariant terms of the log-prob and KL sums by where their
// operands are defined), and the update promises the bits it had (profiles/one_head_arithmetic_identity.txt).  And the behaviour-cloning row, in bc_row
// and in distill_head_kernel, for speed (there).

// W into LDS, the thread's biases, its column of W (BACK: a forward-only launch has no use for it) and its zeroed weight-gradient accumulators.
// s_w keeps the rows of W 132 floats apart: the four (t & 3) groups of a wave read rows 3 apart at the same k, which with a 128-float stride were the
// same banks (a 4-way conflict on three of the four LDS reads of the forward loop)
template <bool BACK>
__device__ __forceinline__ void head_stage(const float* __restrict__ W, const float* __restrict__ bias, float* s_w, float (&fb)[3], float (&wcol)[HA],
                                           float (&dW)[HA]) {
    const int t = threadIdx.x;
    for (int i = t; i < HA * HK; i += 256) s_w[(i >> 7) * HLD + (i & (HK - 1))] = W[i];
    for (int i = 0; i < 3; i++) fb[i] = bias[3 * (t & 3) + i];
    for (int j = 0; j < HA; j++) { wcol[j] = BACK ? W[j * HK + (t & (HK - 1))] : 0.f; dW[j] = 0.f; }
}
// mu = h W^T + b of row fr of the tile for the thread's three actions
__device__ __forceinline__ void head_mu(const float* s_h, const float* s_w, int fr, int fq, const float (&fb)[3], float (&m)[3]) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    const float4* hr = reinterpret_cast<const float4*>(s_h + fr * HLD);
    const float4* w0 = reinterpret_cast<const float4*>(s_w + (3 * fq) * HLD);
    const float4* w1 = reinterpret_cast<const float4*>(s_w + (3 * fq + 1) * HLD);
    const float4* w2 = reinterpret_cast<const float4*>(s_w + (3 * fq + 2) * HLD);
#pragma unroll 2
    for (int k4 = 0; k4 < HK / 4; k4++) {
        const float4 x = hr[k4], u = w0[k4], v = w1[k4], w = w2[k4];
        a0 = fmaf(x.x, u.x, a0); a0 = fmaf(x.y, u.y, a0); a0 = fmaf(x.z, u.z, a0); a0 = fmaf(x.w, u.w, a0);
        a1 = fmaf(x.x, v.x, a1); a1 = fmaf(x.y, v.y, a1); a1 = fmaf(x.z, v.z, a1); a1 = fmaf(x.w, v.w, a1);
        a2 = fmaf(x.x, w.x, a2); a2 = fmaf(x.y, w.y, a2); a2 = fmaf(x.z, w.z, a2); a2 = fmaf(x.w, w.w, a2);
    }
    m[0] = a0 + fb[0]; m[1] = a1 + fb[1]; m[2] = a2 + fb[2];
}
// dL/dmu of the thread's three actions, for the backward mapping (s_g) and the output bias gradient
__device__ __forceinline__ void head_put_grad(float* s_g, int fr, int fq, const float (&gm)[3], float (&dbias)[3]) {
    for (int i = 0; i < 3; i++) { s_g[fr * HA + 3 * fq + i] = gm[i]; dbias[i] += gm[i]; }
}
// row r of the tile at hidden column kc: returns dL/dz = (dL/dmu W) * elu'(h); dW += dL/dmu^T h
__device__ __forceinline__ float head_back_row(const float* s_h, const float* s_g, int r, int kc, const float (&wcol)[HA], float (&dW)[HA]) {
    constexpr int A = HA;
    const float hv = s_h[r * HLD + kc];
    const float4* gp = reinterpret_cast<const float4*>(s_g + r * A);
    const float4 g0 = gp[0], g1 = gp[1], g2 = gp[2];
    const float g[A] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w, g2.x, g2.y, g2.z, g2.w};
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int j = 0; j < A; j += 2) {
        sa = fmaf(g[j], wcol[j], sa); sb = fmaf(g[j + 1], wcol[j + 1], sb);
        dW[j] = fmaf(g[j], hv, dW[j]); dW[j + 1] = fmaf(g[j + 1], hv, dW[j + 1]);
    }
    return elu_back(sa + sb, hv);
}
// the tile's rows of the thread's half: g_hidden, dW and cs (the hidden bias gradient: column sums of dL/dz).  PAIR: LDS rows [0, HTS) are rows row0 ..
// of the batch, LDS rows [HTS, 2 HTS) their mirror images at B + row0 ..
template <bool PAIR>
__device__ __forceinline__ void head_back_rows(const float* s_h, const float* s_g, int row0, int B, int kc, int half, const float (&wcol)[HA],
                                               float (&dW)[HA], float& cs, float* __restrict__ g_hidden) {
    for (int rr = 0; rr < HT / 2; rr++) {
        const int r = half * (HT / 2) + rr, o = row0 + (PAIR ? rr : r);
        const float gz = head_back_row(s_h, s_g, r, kc, wcol, dW);
        cs += gz;
        if (o < B) g_hidden[(size_t)(PAIR && half ? B + o : o) * HK + kc] = gz;
    }
}
// The float part of the workgroup's record: the two row halves of the column-mapped sums meet in LDS; the per-action sums of the output bias gradient go
// over the lanes sharing (lane & 3) within a wave into redf = s_h [4 waves][16], slot 3 fq + i.  The kernel's float64 statistics follow from s_h + 64
// on, then a barrier, then head_record_bias().
__device__ __forceinline__ float* head_record_sums(const float (&dW)[HA], float cs, const float (&dbias)[3], float* s_h, float* __restrict__ partial) {
    constexpr int A = HA;
    const int t = threadIdx.x, kc = t & (HK - 1), half = t >> 7, wave = t >> 6, lane = t & 63;
    float* red = s_h;  // [2][A + 1][HK]
    for (int j = 0; j < A; j++) red[(half * (A + 1) + j) * HK + kc] = dW[j];
    red[(half * (A + 1) + A) * HK + kc] = cs;
    __syncthreads();
    float* rec = partial + (size_t)blockIdx.x * head_record<A>();
    for (int i = t; i < (A + 1) * HK; i += 256) rec[i] = red[i] + red[(A + 1) * HK + i];
    __syncthreads();
    for (int i = 0; i < 3; i++) {
        const float v = quadcol_sum(dbias[i]);
        if (lane < 4) s_h[wave * 16 + 3 * lane + i] = v;
    }
    return rec;
}
__device__ __forceinline__ void head_record_bias(float* rec, const float* redf) {  // the four waves' sums
    const int t = threadIdx.x;
    if (t < HA) rec[(HA + 1) * HK + t] = redf[t] + redf[16 + t] + redf[32 + t] + redf[48 + t];
}

// N float64 statistics, each the sum of one value per thread: waves, then the four waves through LDS; statistic-major in the scratch
template <int N>
__device__ __forceinline__ void head_wave_stats(const double (&v)[N], float* s_h, float* __restrict__ partial) {
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    double* redd = reinterpret_cast<double*>(s_h + 64);  // [N][4 waves]
    for (int k = 0; k < N; k++) {
        const double w = wave_sum_d(v[k]);
        if (lane == 0) redd[4 * k + wave] = w;
    }
    __syncthreads();
    if (t < N) {
        double* srec = reinterpret_cast<double*>(partial + head_stat_base<HA>());
        srec[(size_t)t * gridDim.x + blockIdx.x] = redd[4 * t] + redd[4 * t + 1] + redd[4 * t + 2] + redd[4 * t + 3];
    }
}

// The PPO heads' float64 statistics behind head_record_sums(): lanes sharing (lane & 3) within a wave, then the four waves through LDS.  Slot 3 fq + i
// = dL/dlogstd (acc_ls), slots 12..15 = the loss terms (acc_st), slot 16 (N_STAT = 17) = the sum of `extra` over the threads.
// Statistic index: [0, A) dL/dlogstd, A unused (the value error is the critic head's), A+1.. = surrogate, bound, entropy, kl, (symmetry)
template <int N_STAT>
__device__ __forceinline__ void ppo_store_stats(const double (&acc_ls)[3], const double (&acc_st)[4], float* s_h, float* __restrict__ partial, double extra = 0.0) {
    static_assert(N_STAT == 16 || N_STAT == 17, "");
    constexpr int A = HA, SL = N_STAT == 16 ? 16 : 20;  // slots per wave
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    double* redd = reinterpret_cast<double*>(s_h + 64);  // [4 waves][SL]
    for (int i = 0; i < 3; i++) {
        const double w = quadcol_sum(acc_ls[i]);
        if (lane < 4) redd[wave * SL + 3 * lane + i] = w;
    }
    for (int i = 0; i < 4; i++) {
        const double w = quadcol_sum(acc_st[i]);  // only fq == 0 lanes carry values
        if (lane == 0) redd[wave * SL + 12 + i] = w;
    }
    if (N_STAT == 17) {
        const double w = wave_sum_d(extra);
        if (lane == 0) redd[wave * SL + 16] = w;
    }
    __syncthreads();
    if (t < N_STAT) {
        double* srec = reinterpret_cast<double*>(partial + head_stat_base<A>());
        const double w = redd[t] + redd[SL + t] + redd[2 * SL + t] + redd[3 * SL + t];
        const int k = t < A ? t : t + 1;
        srec[(size_t)k * gridDim.x + blockIdx.x] = w;
    }
}

// behaviour-cloning loss of one live row on a thread's three actions, on top of what gm holds: L = 1 / (A B) sum_r |mu_r - target_r|^2, gscale = 2 / (A B)
__device__ __forceinline__ void bc_row(bool live, float gscale, const float (&m)[3], const float* __restrict__ target, float (&gm)[3], double& sse) {
    for (int i = 0; i < 3; i++) {
        const float e = m[i] - target[i];
        if (live) { gm[i] += gscale * e; sse += (double)(e * e); }
    }
}

// Mirror-symmetry loss: the batch is 2B rows, rows [B, 2B) the mirror images of rows [0, B).  A tile holds HTS original rows in LDS rows [0, HTS) and
// their mirror images in LDS rows [HTS, 2 HTS), so that the pair's means meet in LDS (s_mu).  Per pair, with d = mu(M_o x) - M_a mu(x) and
// c = sym_scale = 2 coef / (B A):  dL/dmu of the mirrored row = c d,  of the original row = -c M_a d  (M_a a symmetric involution:
// (M_a d)[a] = sign[a] d[src[a]]); acc_sym = sum d^2.  A wave holds 16 rows, all of them original or all mirrored: `mirror` is uniform per wave,
// so what runs under it may use the DPP moves, which run in whole waves.
constexpr int HEAD_NSTAT_SYM = HEAD_NSTAT + 1;
// the scratch the header promises holds the largest launch: HEAD_MAX_GRID records of the widest head and, behind them, the float64 statistics
// (2 floats each) of the head with the most of them, one per workgroup
static_assert(head_stat_base<HA>() + 2 * (size_t)HEAD_MAX_GRID * HEAD_NSTAT_SYM <= (size_t)BG_HEAD_SCRATCH_FLOATS,
              "BG_HEAD_SCRATCH_FLOATS is too small for the heads' records and statistics");
static_assert(HEAD_NSTAT_SYM >= HEAD_NSTAT && head_record<HA>() >= head_record<1>(), "the sym head is the largest user of the scratch");
struct ActionMirror { int src[HA]; float sign[HA]; };
struct SymThread {
    static constexpr int A = HA;
    int pr, src[3];
    bool mirror;
    float sgn[3];
    double acc_sym;

    // before the kernel's first barrier / behind it
    __device__ __forceinline__ void stage(const ActionMirror& am, int* s_src, float* s_sign) {
        const int t = threadIdx.x;
        if (t < A) { s_src[t] = am.src[t]; s_sign[t] = am.sign[t]; }
        pr = (t >> 2) & (HTS - 1); mirror = (t >> 2) >= HTS;
        acc_sym = 0.0;
    }
    __device__ __forceinline__ void load(const int* s_src, const float* s_sign) {
        const int fq = threadIdx.x & 3;
        for (int i = 0; i < 3; i++) { src[i] = s_src[3 * fq + i]; sgn[i] = s_sign[3 * fq + i]; }
    }
    // the means of row b = row0 + pr of the pair tile into s_mu and, for a live row, into mu_out
    __device__ __forceinline__ void put_mu(const float (&m)[3], int b, int B, float* s_mu, float* __restrict__ mu_out) const {
        const int fr = threadIdx.x >> 2, fq = threadIdx.x & 3;
        for (int i = 0; i < 3; i++) s_mu[fr * A + 3 * fq + i] = m[i];
        if (mu_out && b < B) for (int i = 0; i < 3; i++) mu_out[(size_t)(mirror ? B + b : b) * A + 3 * fq + i] = m[i];
    }
    // gm = the symmetry term of the pair (pr, HTS + pr) for this thread's row and actions
    __device__ __forceinline__ void pair(bool live, float sym_scale, const float* s_mu, float (&gm)[3]) {
        const int fq = threadIdx.x & 3;
        const float* mo = s_mu + pr * A;
        const float* mm = s_mu + (HTS + pr) * A;
        for (int i = 0; i < 3; i++) {
            const int a = 3 * fq + i;
            gm[i] = 0.f;
            if (mirror) {
                const float d = mm[a] - sgn[i] * mo[src[i]];
                if (live) { gm[i] = sym_scale * d; acc_sym += (double)(d * d); }
            } else {
                const float d = mm[src[i]] - sgn[i] * mo[a];  // d[src[a]] (sign[src[a]] = sign[a])
                if (live) gm[i] = -sym_scale * sgn[i] * d;
            }
        }
    }
};

// MODE 0: forward only (mu_out), MODE 1: forward + PPO loss + backward.
template <int MODE>
__global__ __launch_bounds__(256) void actor_head_kernel(int B, int tiles, const float* __restrict__ h, const float* __restrict__ W,
                                                         const float* __restrict__ bias, const float* __restrict__ logstd,
                                                         const float* __restrict__ actions, const float* __restrict__ old_mu,
                                                         const float* __restrict__ old_logstd, const float* __restrict__ old_logp,
                                                         const float* __restrict__ adv, const double* __restrict__ adv_stats, float e_clip,
                                                         float bound_coef, float* __restrict__ mu_out, float* __restrict__ g_hidden,
                                                         float* __restrict__ partial) {
    constexpr int A = HA;
    __shared__ __attribute__((aligned(16))) float s_h[HT * HLD];
    __shared__ __attribute__((aligned(16))) float s_w[A * HLD];
    __shared__ __attribute__((aligned(16))) float s_g[HT * A];  // dL/dmu of the tile's rows
    const int t = threadIdx.x;
    const int fr = t >> 2, fq = t & 3;
    float fb[3];
    const int kc = t & (HK - 1), half = t >> 7;
    float wcol[A], dW[A], cs = 0.f;
    head_stage<MODE == 1>(W, bias, s_w, fb, wcol, dW);
    // loss constants of this thread's three actions (bg_ppo_math.h states the same formulas for a whole row)
    float ls[3], ols[3], isig2[3], osig2[3], dbias[3] = {0.f, 0.f, 0.f};
    float ent = 0.f, mean = 0.f, inv_std = 0.f, invB = 0.f, bscale = 0.f;
    double acc_ls[3] = {0.0, 0.0, 0.0}, acc_st[4] = {0.0, 0.0, 0.0, 0.0};
    if (MODE == 1) {
        bg::ActorLossConsts<A> c;
        bg::actor_loss_consts<A>(c, B, logstd, old_logstd, adv_stats, e_clip, bound_coef);
        for (int i = 0; i < 3; i++) { ls[i] = logstd[3 * fq + i]; ols[i] = old_logstd[3 * fq + i]; }
        for (int i = 0; i < 3; i++) { const float sg = expf(ls[i]), os = expf(ols[i]); isig2[i] = 1.0f / (sg * sg); osig2[i] = os * os; }
        ent = c.ent; mean = c.mean; inv_std = c.inv_std; invB = c.invB; bscale = c.bscale;
    }
    __syncthreads();
    // (no register prefetch of the next tile here, unlike critic_head_backward_kernel: the 32 extra registers cost this kernel a resident
    // workgroup per CU, 55.9 -> 62.9 us measured)
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int row0 = tile * HT;
        load_tile(h, row0, B, s_h);
        __syncthreads();
        {
            float m[3];
            head_mu(s_h, s_w, fr, fq, fb, m);
            const int b = row0 + fr;
            const bool live = b < B;
            const size_t o = (size_t)(live ? b : B - 1) * A + 3 * fq;
            if (mu_out && live) for (int i = 0; i < 3; i++) mu_out[o + i] = m[i];
            if (MODE == 1) {  // PPO actor loss of the row (the same lines stand in actor_head_sym_kernel: see the shared pieces' header)
                float d[3], hl[3], lp = 0.f, kl = 0.f, bound = 0.f;
                for (int i = 0; i < 3; i++) {
                    d[i] = actions[o + i] - m[i];
                    lp += -0.5f * d[i] * d[i] * isig2[i] - ls[i] - bg::kHalfLog2Pi;
                    const float dm = m[i] - old_mu[o + i];
                    kl += ls[i] - ols[i] + 0.5f * (osig2[i] + dm * dm) * isig2[i] - 0.5f;
                    const float hi = fmaxf(m[i] - 1.0f, 0.f), lo = fminf(m[i] + 1.0f, 0.f);
                    bound += hi * hi + lo * lo;
                    hl[i] = hi + lo;
                }
                lp = quad_sum(lp); kl = quad_sum(kl); bound = quad_sum(bound);
                const float An = (adv[live ? b : B - 1] - mean) * inv_std;
                const float ratio = expf(lp - old_logp[live ? b : B - 1]);
                const float rc = fminf(fmaxf(ratio, 1.0f - e_clip), 1.0f + e_clip);
                const float s1 = -An * ratio, s2 = -An * rc;
                // d max(s1,s2)/d logp: through s1 when it wins or ties, through the clamp only inside the clip range
                const bool inside = ratio >= 1.0f - e_clip && ratio <= 1.0f + e_clip;
                const float dlogp = (live && (inside || s1 > s2)) ? -An * ratio * invB : 0.f;
                for (int i = 0; i < 3; i++) {
                    const float gm = live ? dlogp * d[i] * isig2[i] + bscale * hl[i] : 0.f;
                    s_g[fr * A + 3 * fq + i] = gm;
                    dbias[i] += gm;
                    acc_ls[i] += (double)(dlogp * (d[i] * d[i] * isig2[i] - 1.0f));
                }
                if (live && fq == 0) {
                    acc_st[0] += (double)fmaxf(s1, s2); acc_st[1] += (double)bound; acc_st[2] += (double)ent; acc_st[3] += (double)kl;
                }
            }
        }
        __syncthreads();
        if (MODE == 1) {
            // g_hidden = (dL/dmu W) * elu'(h), dW += dL/dmu^T h, hidden bias gradient = column sums of g_hidden
            for (int rr = 0; rr < HT / 2; rr++) {
                const int r = half * (HT / 2) + rr;
                const float gz = head_back_row(s_h, s_g, r, kc, wcol, dW);
                cs += gz;
                if (row0 + r < B) g_hidden[(size_t)(row0 + r) * HK + kc] = gz;
            }
            __syncthreads();
        }
    }
    if (MODE == 0) return;
    float* rec = head_record_sums(dW, cs, dbias, s_h, partial);
    ppo_store_stats<16>(acc_ls, acc_st, s_h, partial);
    head_record_bias(rec, s_h);
}

__global__ __launch_bounds__(256) void critic_head_backward_kernel(int B, int tiles, const float* __restrict__ h, const float* __restrict__ w,
                                                                   const float* __restrict__ values, const float* __restrict__ returns,
                                                                   float* __restrict__ g_hidden, float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float s_h[HT * HLD];
    __shared__ float s_g[HT];
    const int t = threadIdx.x, kc = t & (HK - 1), half = t >> 7;
    const float wk = w[kc], invB = 1.0f / (float)B;
    float dW = 0.f, cs = 0.f, db = 0.f;
    double verr2 = 0.0;
    float4 nxt[HTV];
    tile_fetch(h, blockIdx.x * HT, B, nxt);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int row0 = tile * HT;
        tile_put(nxt, s_h);
        if (tile + (int)gridDim.x < tiles) tile_fetch(h, (tile + gridDim.x) * HT, B, nxt);  // in flight under this tile's compute
        if (t < HT) {
            const int b = row0 + t;
            float g = 0.f;
            if (b < B) {
                const float verr = values[b] - returns[b];
                g = 2.0f * verr * invB;  // d mean((v - ret)^2) / dv, runner.py:148
                verr2 += (double)(verr * verr);
                db += g;
            }
            s_g[t] = g;
        }
        __syncthreads();
        for (int rr = 0; rr < HT / 2; rr++) {
            const int r = half * (HT / 2) + rr;
            const float hv = s_h[r * HLD + kc], g = s_g[r];
            dW = fmaf(g, hv, dW);
            const float gz = elu_back(g * wk, hv);
            cs += gz;
            if (row0 + r < B) g_hidden[(size_t)(row0 + r) * HK + kc] = gz;
        }
        __syncthreads();
    }
    float* red = s_h;  // [2][2][HK]
    red[(half * 2) * HK + kc] = dW;
    red[(half * 2 + 1) * HK + kc] = cs;
    __syncthreads();
    float* rec = partial + (size_t)blockIdx.x * head_record<1>();
    for (int i = t; i < 2 * HK; i += 256) rec[i] = red[i] + red[2 * HK + i];
    if (t < 64) {
        float v = db;
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        const double s = wave_sum_d(verr2);
        if (t == 0) { rec[2 * HK] = v; reinterpret_cast<double*>(partial + head_stat_base<1>())[blockIdx.x] = s; }
    }
}

// ---- the fixed-order sums over the workgroups' records (bg_reduce.h: reduce_block), for up to 8 descriptors in one launch: the deferred reductions of
// bg_reduce_group, and the finish of a head's immediate form on the one descriptor of that head (head_finish)
__global__ __launch_bounds__(256) void reduce_group_kernel(ReduceGroup grp) {
    __shared__ float sm[16][17];
    __shared__ double sd[4];
    (void)reduce_block(grp, blockIdx.x, sm, sd);  // (the squares of what it wrote are the tail's business: tail_sums_kernel, bg_tail.hip)
}

// values = h w + b: half a wave per row (32 lanes x 16 bytes = one 512-byte row), 4 rows in flight per half-wave
__global__ __launch_bounds__(256) void critic_head_forward_kernel(int rows, const float* __restrict__ h, const float* __restrict__ w,
                                                                  const float* __restrict__ b, float* __restrict__ values) {
    const int lane = threadIdx.x & 31;
    const int hw = (blockIdx.x * blockDim.x + threadIdx.x) >> 5, nhw = (gridDim.x * blockDim.x) >> 5;
    const float4 wv = *reinterpret_cast<const float4*>(w + lane * 4);
    const float bias = b[0];
    for (int r0 = hw * 4; r0 < rows; r0 += nhw * 4) {
        float4 x[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int r = r0 + u < rows ? r0 + u : rows - 1;
            x[u] = *reinterpret_cast<const float4*>(h + (size_t)r * HK + lane * 4);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            float s = x[u].x * wv.x;
            s = fmaf(x[u].y, wv.y, s); s = fmaf(x[u].z, wv.z, s); s = fmaf(x[u].w, wv.w, s);
            for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if (lane == 0 && r0 + u < rows) values[r0 + u] = s + bias;
        }
    }
}

// values = h w + b for all T + 1 time rows of 16 envs, then the GAE scan of those envs, in ONE launch (what bg_critic_head_forward, a fill and bg_gae do
// as three dependent launches in front of the actor's loss: ~45 us of small kernels and gaps per mini-epoch).  One workgroup = 16 envs: the value
// phase is critic_head_forward_kernel's (half a wave per row, same sums: bit-identical values), the values go to LDS and to values_all, threads
// 0..15 then run gae_kernel's scan on registers (its loads were issued at the top of the kernel).  Moments of the advantages: one float64 triple per
// workgroup in `partial`; the last workgroup to finish (ticket) adds them up in a fixed order and WRITES sums (no zero fill, no float atomics).
// Envs per workgroup: 16 where the launch also evaluates the output layer (25 x 16 rows of activations per workgroup); 64 for the scan alone, which is what
// the training loop runs (values from the chained forward kernel's value head): a quarter of the workgroups, tickets and fences beside the actor's
// forward chain -- update 21.12 against 21.26 ms on one box, three of three alternating pairs (tools/ab_env.sh)
#ifndef BG_GAE_SCAN_ENVS
#define BG_GAE_SCAN_ENVS 64
#endif
constexpr int VG_ENVS_VALUES = 16, VG_ENVS_SCAN = BG_GAE_SCAN_ENVS;
// NORM (bg_critic_values_gae_norm, algorithm.normalize_value): the critic's output is u, its value v = fmaf(sigma, u, m) with (m, sigma, 1 / sigma) =
// value_stats.  The values are de-standardised where they enter LDS, so the scan, the bootstrap store into rewards and the advantages run on v with the
// arithmetic of the other form; values_all keeps u; ret receives (R - m) * (1 / sigma), R = v + adv, each step rounded (bg_obs_normalize's rule: this
// file compiles with contraction and reassociation on, so those three expressions are pinned); three more float64 sums per workgroup and in `sums`:
// sum R, sum R^2 and the count of the un-normalised returns, which bg_value_norm_update merges into the statistics once per iteration.
template <int TMAX, int VG_ENVS, bool NORM>
__global__ __launch_bounds__(256) void critic_values_gae_kernel(int T, int N, const float* __restrict__ h, const float* __restrict__ w,
                                                                const float* __restrict__ b, float* __restrict__ rewards,
                                                                const uint8_t* __restrict__ dones, const uint8_t* __restrict__ touts, float gamma,
                                                                float lam, float* __restrict__ values_all, float* __restrict__ adv,
                                                                float* __restrict__ ret, double* __restrict__ partial, unsigned* __restrict__ ticket,
                                                                double* __restrict__ sums, const float* __restrict__ value_stats) {
    constexpr int NS = NORM ? 6 : 3;  // float64 sums per workgroup
    __shared__ float sv[(TMAX + 1) * VG_ENVS];
    __shared__ double sd[NS * 4];
    __shared__ unsigned s_last;
    float vm = 0.f, vsig = 1.f, vinv = 1.f;
    if constexpr (NORM) { vm = value_stats[0]; vsig = value_stats[1]; vinv = value_stats[2]; }
    const int e0 = blockIdx.x * VG_ENVS, ne = N - e0 < VG_ENVS ? N - e0 : VG_ENVS;
    // the scan's operands (threads 0..15: one env each), in flight during the value phase
    float r[TMAX];
    uint8_t dn[TMAX], to[TMAX];
    const bool scan = (int)threadIdx.x < ne;
    if (scan) {
#pragma unroll
        for (int t = 0; t < TMAX; t++)
            if (t < T) {
                const size_t k = (size_t)t * N + e0 + threadIdx.x;
                r[t] = rewards[k]; dn[t] = dones[k]; to[t] = touts[k];
            }
    }
    const int lane = threadIdx.x & 31, hw = threadIdx.x >> 5, R = (T + 1) * VG_ENVS;
    if (!h) {  // the values are an input (the chained forward kernel's value head wrote them)
        for (int q = threadIdx.x; q < R; q += 256) {
            const int t = q / VG_ENVS, e = q % VG_ENVS;
            const float u = values_all[(size_t)t * N + e0 + (e < ne ? e : ne - 1)];
            if constexpr (NORM) sv[q] = __builtin_fmaf(vsig, u, vm);
            else sv[q] = u;
        }
    }
    const float4 wv = h ? *reinterpret_cast<const float4*>(w + lane * 4) : float4{0.f, 0.f, 0.f, 0.f};
    const float bias = h ? b[0] : 0.f;
    for (int r0 = hw * 4; h && r0 < R; r0 += 32) {
        float4 x[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int q = r0 + u < R ? r0 + u : R - 1, t = q / VG_ENVS, e = q % VG_ENVS;
            x[u] = *reinterpret_cast<const float4*>(h + ((size_t)t * N + e0 + (e < ne ? e : ne - 1)) * HK + lane * 4);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            float s = x[u].x * wv.x;
            s = fmaf(x[u].y, wv.y, s); s = fmaf(x[u].z, wv.z, s); s = fmaf(x[u].w, wv.w, s);
            for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o);
            const int q = r0 + u, t = q / VG_ENVS, e = q % VG_ENVS;
            if (lane == 0 && q < R) {
                if constexpr (NORM) sv[q] = __builtin_fmaf(vsig, s + bias, vm);
                else sv[q] = s + bias;
                if (e < ne) values_all[(size_t)t * N + e0 + e] = s + bias;
            }
        }
    }
    __syncthreads();
    double acc[NS] = {};
    if (scan) {
        float next_v = sv[T * VG_ENVS + threadIdx.x], last_adv = 0.f;
#pragma unroll
        for (int t = TMAX - 1; t >= 0; t--)
            if (t < T) {
                const size_t k = (size_t)t * N + e0 + threadIdx.x;
                const float v = sv[t * VG_ENVS + threadIdx.x];
                float rr = r[t];
                if (to[t]) { rr = v; rewards[k] = v; }  // runner.py:135 (in place, repeated every mini-epoch with the current critic)
                const float nn = (dn[t] != 0 || to[t] != 0) ? 0.f : 1.f;
                const float delta = rr + gamma * nn * next_v - v;
                last_adv = delta + gamma * lam * nn * last_adv;
                adv[k] = last_adv;
                if constexpr (NORM) {
                    float R, Rn;
                    {
#pragma clang fp contract(off) reassociate(off)
                        R = v + last_adv;
                        const float c = R - vm;
                        Rn = c * vinv;
                    }
                    ret[k] = Rn;
                    acc[3] += (double)R; acc[4] += (double)R * (double)R; acc[5] += 1.0;
                } else {
                    ret[k] = v + last_adv;
                }
                acc[0] += (double)last_adv; acc[1] += (double)last_adv * (double)last_adv; acc[2] += 1.0;
                next_v = v;
            }
    }
#pragma unroll
    for (int k = 0; k < NS; k++) {  // (the scanning threads are the first VG_ENVS of the workgroup; the others carry zeros)
        const double s = wave_sum_d(acc[k]);
        if ((threadIdx.x & 63) == 0) sd[k * 4 + (threadIdx.x >> 6)] = s;
    }
    __syncthreads();
    // The triple is PUBLISHED, not fenced: an agent-scope store goes through the XCD's L2 to memory, and once the wave's vmcnt is back at zero it
    // has arrived; the ticket is taken after that.  (A release fence -- __threadfence -- writes back the whole L2 of the XCD instead, every dirty
    // line of the forward chain that runs beside this launch included, once per workgroup: this launch sits between the critic's forward pass and
    // the actor's loss.)  The reader takes agent-scope loads, which do not hit a stale line of its own L2.
    // That argument rests on two properties of gfx942 / gfx950 that the HIP memory model does not promise (the return of an sc1 store into vmcnt =
    // visible at agent scope; one vmcnt counter for loads and stores), so it is compiled for those targets only: anything else gets the portable
    // release (fence + relaxed ticket), slower but correct by the model.  DESIGN.md section 5 records the assumption.
#if defined(__gfx942__) || defined(__gfx950__)
    if (threadIdx.x < NS) {
        __hip_atomic_store(&partial[(size_t)blockIdx.x * NS + threadIdx.x], sd[threadIdx.x * 4] + sd[threadIdx.x * 4 + 1] + sd[threadIdx.x * 4 + 2] + sd[threadIdx.x * 4 + 3],
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // threads 0..NS-1 and the ticket's thread 0 are one wave
    }
    __syncthreads();
    if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
#else
    if (threadIdx.x < NS)
        __hip_atomic_store(&partial[(size_t)blockIdx.x * NS + threadIdx.x], sd[threadIdx.x * 4] + sd[threadIdx.x * 4 + 1] + sd[threadIdx.x * 4 + 2] + sd[threadIdx.x * 4 + 3],
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        s_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
    }
#endif
    __syncthreads();
    if (s_last) {  // every workgroup's triple has arrived: fixed-order total
        for (int k = 0; k < NS; k++) {
            double s = 0.0;
            for (int g = threadIdx.x; g < (int)gridDim.x; g += 256) s += __hip_atomic_load(&partial[(size_t)g * NS + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s = wave_sum_d(s);
            if ((threadIdx.x & 63) == 0) sd[k * 4 + (threadIdx.x >> 6)] = s;
        }
        __syncthreads();
        if (threadIdx.x < NS) sums[threadIdx.x] = sd[threadIdx.x * 4] + sd[threadIdx.x * 4 + 1] + sd[threadIdx.x * 4 + 2] + sd[threadIdx.x * 4 + 3];
        if (threadIdx.x == 0) *ticket = 0u;
    }
}

// Behaviour-cloning head (bg_distill_head): actor_head_kernel with the behaviour-cloning row for the PPO loss, dL/dmu = 2 (mu - target) / (A B); one
// float64 statistic per workgroup: the squared errors.
__global__ __launch_bounds__(256) void distill_head_kernel(int B, int tiles, const float* __restrict__ h, const float* __restrict__ W,
                                                           const float* __restrict__ bias, const float* __restrict__ target, float* __restrict__ mu_out,
                                                           float* __restrict__ g_hidden, float* __restrict__ partial) {
    constexpr int A = HA;
    __shared__ __attribute__((aligned(16))) float s_h[HT * HLD];
    __shared__ __attribute__((aligned(16))) float s_w[A * HLD];
    __shared__ __attribute__((aligned(16))) float s_g[HT * A];
    const int t = threadIdx.x, fr = t >> 2, fq = t & 3;
    const int kc = t & (HK - 1), half = t >> 7;
    float fb[3], wcol[A], dW[A], cs = 0.f, dbias[3] = {0.f, 0.f, 0.f};
    head_stage<true>(W, bias, s_w, fb, wcol, dW);
    const float gscale = 2.0f / ((float)A * (float)B);
    double sse[1] = {0.0};
    __syncthreads();
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int row0 = tile * HT;
        load_tile(h, row0, B, s_h);
        __syncthreads();
        {
            float m[3];
            head_mu(s_h, s_w, fr, fq, fb, m);
            const int b = row0 + fr;
            const bool live = b < B;
            const size_t o = (size_t)(live ? b : B - 1) * A + 3 * fq;
            if (mu_out && live) for (int i = 0; i < 3; i++) mu_out[o + i] = m[i];
            // (bc_row's lines with a select for its branch: through bc_row the target's load moved under the branch, and the launch was 1.2 % slower)
            for (int i = 0; i < 3; i++) {
                const float e = m[i] - target[o + i];
                const float gm = live ? e * gscale : 0.f;
                s_g[fr * A + 3 * fq + i] = gm;
                dbias[i] += gm;
                if (live) sse[0] += (double)(e * e);
            }
        }
        __syncthreads();
        head_back_rows<false>(s_h, s_g, row0, B, kc, half, wcol, dW, cs, g_hidden);
        __syncthreads();
    }
    float* rec = head_record_sums(dW, cs, dbias, s_h, partial);
    head_wave_stats(sse, s_h, partial);
    head_record_bias(rec, s_h);
}

// bg_actor_head_sym: the PPO, bound and entropy terms of the original rows plus the symmetry term of both rows of a pair; statistic A + 5 = sum d^2.
__global__ __launch_bounds__(256) void actor_head_sym_kernel(int B, int tiles, const float* __restrict__ h, const float* __restrict__ W,
                                                             const float* __restrict__ bias, const float* __restrict__ logstd,
                                                             const float* __restrict__ actions, const float* __restrict__ old_mu,
                                                             const float* __restrict__ old_logstd, const float* __restrict__ old_logp,
                                                             const float* __restrict__ adv, const double* __restrict__ adv_stats, float e_clip,
                                                             float bound_coef, float sym_scale, ActionMirror am, float* __restrict__ mu_out,
                                                             float* __restrict__ g_hidden, float* __restrict__ partial) {
    constexpr int A = HA;
    __shared__ __attribute__((aligned(16))) float s_h[HT * HLD];
    __shared__ __attribute__((aligned(16))) float s_w[A * HLD];
    __shared__ __attribute__((aligned(16))) float s_g[HT * A];
    __shared__ float s_mu[HT * A];
    __shared__ int s_src[A];
    __shared__ float s_sign[A];
    const int t = threadIdx.x, fr = t >> 2, fq = t & 3;
    const int kc = t & (HK - 1), half = t >> 7;
    float fb[3], wcol[A], dW[A], cs = 0.f;
    head_stage<true>(W, bias, s_w, fb, wcol, dW);
    SymThread sym;
    sym.stage(am, s_src, s_sign);
    // loss constants of this thread's three actions (actor_head_kernel's lines)
    float ls[3], ols[3], isig2[3], osig2[3], dbias[3] = {0.f, 0.f, 0.f};
    double acc_ls[3] = {0.0, 0.0, 0.0}, acc_st[4] = {0.0, 0.0, 0.0, 0.0};
    bg::ActorLossConsts<A> c;
    bg::actor_loss_consts<A>(c, B, logstd, old_logstd, adv_stats, e_clip, bound_coef);
    for (int i = 0; i < 3; i++) { ls[i] = logstd[3 * fq + i]; ols[i] = old_logstd[3 * fq + i]; }
    for (int i = 0; i < 3; i++) { const float sg = expf(ls[i]), os = expf(ols[i]); isig2[i] = 1.0f / (sg * sg); osig2[i] = os * os; }
    const float ent = c.ent, mean = c.mean, inv_std = c.inv_std, invB = c.invB, bscale = c.bscale;
    __syncthreads();
    sym.load(s_src, s_sign);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int row0 = tile * HTS, b = row0 + sym.pr;
        load_pair_tile(h, row0, B, s_h);
        __syncthreads();
        float m[3], gm[3];
        head_mu(s_h, s_w, fr, fq, fb, m);
        sym.put_mu(m, b, B, s_mu, mu_out);
        __syncthreads();
        const bool live = b < B;
        sym.pair(live, sym_scale, s_mu, gm);
        if (!sym.mirror) {  // PPO actor loss of the original row (actor_head_kernel's lines)
            const size_t o = (size_t)(live ? b : B - 1) * A + 3 * fq;
            float d[3], hl[3], lp = 0.f, kl = 0.f, bound = 0.f;
            for (int i = 0; i < 3; i++) {
                d[i] = actions[o + i] - m[i];
                lp += -0.5f * d[i] * d[i] * isig2[i] - ls[i] - bg::kHalfLog2Pi;
                const float dm = m[i] - old_mu[o + i];
                kl += ls[i] - ols[i] + 0.5f * (osig2[i] + dm * dm) * isig2[i] - 0.5f;
                const float hi = fmaxf(m[i] - 1.0f, 0.f), lo = fminf(m[i] + 1.0f, 0.f);
                bound += hi * hi + lo * lo;
                hl[i] = hi + lo;
            }
            lp = quad_sum(lp); kl = quad_sum(kl); bound = quad_sum(bound);
            const float An = (adv[live ? b : B - 1] - mean) * inv_std;
            const float ratio = expf(lp - old_logp[live ? b : B - 1]);
            const float rc = fminf(fmaxf(ratio, 1.0f - e_clip), 1.0f + e_clip);
            const float s1 = -An * ratio, s2 = -An * rc;
            const bool inside = ratio >= 1.0f - e_clip && ratio <= 1.0f + e_clip;
            const float dlogp = (live && (inside || s1 > s2)) ? -An * ratio * invB : 0.f;
            for (int i = 0; i < 3; i++) {
                if (live) gm[i] += dlogp * d[i] * isig2[i] + bscale * hl[i];
                acc_ls[i] += (double)(dlogp * (d[i] * d[i] * isig2[i] - 1.0f));
            }
            if (live && fq == 0) {
                acc_st[0] += (double)fmaxf(s1, s2); acc_st[1] += (double)bound; acc_st[2] += (double)ent; acc_st[3] += (double)kl;
            }
        }
        head_put_grad(s_g, fr, fq, gm, dbias);
        __syncthreads();
        head_back_rows<true>(s_h, s_g, row0, B, kc, half, wcol, dW, cs, g_hidden);
        __syncthreads();
    }
    float* rec = head_record_sums(dW, cs, dbias, s_h, partial);
    ppo_store_stats<17>(acc_ls, acc_st, s_h, partial, sym.acc_sym);
    head_record_bias(rec, s_h);
}

// bg_distill_head_sym: bc_row on the original rows plus the symmetry term of both rows of a pair.  L = 1 / (A B) sum_r |mu_r - target_r|^2 +
// coef / (A B) sum_r |d_r|^2; two float64 statistics per workgroup: the squared errors and sum d^2.  The NEXT tile's 8 float4 per thread are in flight
// under this tile's compute (critic_head_backward_kernel's scheme: LDS, not registers, bounds this kernel's three workgroups per CU).
__global__ __launch_bounds__(256) void distill_head_sym_kernel(int B, int tiles, const float* __restrict__ h, const float* __restrict__ W,
                                                               const float* __restrict__ bias, const float* __restrict__ target, float sym_scale,
                                                               ActionMirror am, float* __restrict__ mu_out, float* __restrict__ g_hidden,
                                                               float* __restrict__ partial) {
    constexpr int A = HA;
    __shared__ __attribute__((aligned(16))) float s_h[HT * HLD];
    __shared__ __attribute__((aligned(16))) float s_w[A * HLD];
    __shared__ __attribute__((aligned(16))) float s_g[HT * A];
    __shared__ float s_mu[HT * A];
    __shared__ int s_src[A];
    __shared__ float s_sign[A];
    const int t = threadIdx.x, fr = t >> 2, fq = t & 3;
    const int kc = t & (HK - 1), half = t >> 7;
    float fb[3], wcol[A], dW[A], cs = 0.f, dbias[3] = {0.f, 0.f, 0.f};
    head_stage<true>(W, bias, s_w, fb, wcol, dW);
    SymThread sym;
    sym.stage(am, s_src, s_sign);
    const float gscale = 2.0f / ((float)A * (float)B);
    double sse = 0.0;
    __syncthreads();
    sym.load(s_src, s_sign);
    float4 nxt[HTV];
    pair_fetch(h, blockIdx.x * HTS, B, nxt);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int row0 = tile * HTS, b = row0 + sym.pr;
        tile_put(nxt, s_h);
        if (tile + (int)gridDim.x < tiles) pair_fetch(h, (tile + gridDim.x) * HTS, B, nxt);
        __syncthreads();
        const bool live = b < B;
        float m[3], gm[3];
        head_mu(s_h, s_w, fr, fq, fb, m);
        sym.put_mu(m, b, B, s_mu, mu_out);
        __syncthreads();
        sym.pair(live, sym_scale, s_mu, gm);
        if (!sym.mirror) bc_row(live, gscale, m, target + (size_t)(live ? b : B - 1) * A + 3 * fq, gm, sse);
        head_put_grad(s_g, fr, fq, gm, dbias);
        __syncthreads();
        head_back_rows<true>(s_h, s_g, row0, B, kc, half, wcol, dW, cs, g_hidden);
        __syncthreads();
    }
    float* rec = head_record_sums(dW, cs, dbias, s_h, partial);
    const double st[2] = {sse, sym.acc_sym};
    head_wave_stats(st, s_h, partial);
    head_record_bias(rec, s_h);
}

// y[r][c] = sign[c] x[r][src[c]] (src[c] < 0: 0) for rows x cols elements: exact, only signs change.  Up to MIRROR_MAX_COLS columns (the widest
// network input: a frame stack's 47 H observations padded to 512); the map travels as a kernel argument, one 16-bit code per column: -1 for a zero
// column, else src with MIRROR_NEG set where the sign is -1.
constexpr int MIRROR_MAX_COLS = 512;
constexpr int MIRROR_NEG = 0x4000;
struct ColumnMirror { int16_t code[MIRROR_MAX_COLS]; };
__global__ __launch_bounds__(256) void mirror_rows_kernel(int rows, int cols, ColumnMirror cm, const float* __restrict__ x, float* __restrict__ y) {
    __shared__ int16_t s_code[MIRROR_MAX_COLS];
    for (int c = threadIdx.x; c < cols; c += 256) s_code[c] = cm.code[c];
    __syncthreads();
    const size_t n = (size_t)rows * cols;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t r = i / cols;
        const int col = (int)(i - r * cols), code = s_code[col];
        const float v = code < 0 ? 0.f : x[r * cols + (code & (MIRROR_NEG - 1))];
        y[i] = (code & MIRROR_NEG) ? -v : v;
    }
}

// The partner rows of the action-smoothness loss (algorithm.smoothness_loss): y[r] = x[r] + u_r (x+[r] - x[r]) for the rows r = t N + e of x [T][N][cols],
// x+[r] = the same env's row one step later (row r + N; for t = T - 1 the row e of x_last).  Where dones[r] or time_outs[r] is set (the steps at which
// GAE cuts the trajectory) y[r] is a copy of x[r]; mode 0 (next): u = 1 as a plain copy of x+[r], no arithmetic; mode 1 (interpolate): u in [0, 1) =
// the upper 24 bits of philox entry 0 on the key (seed) and the counter (r, update, RS_PARTNER, mini-epoch), one fma per element.
// Memory-bound (mode 1: two rows read, one written; mode 0: one read, one written), shaped as bg_gather_rows: 16 bytes per lane, consecutive lanes on consecutive 16-byte pieces of one row
// (cols / 4 lanes per row, a wave on 64 / (cols / 4) whole rows or on 1 KiB of one row), so every load and store of a wave covers whole consecutive
// lines; the two flag bytes are read once per row (the lanes of a row read the same byte: one request per wave and row) and the draw, which is
// arithmetic alone, is the same in every lane of a row.  Every lane writes its own 16 bytes: no atomics, nothing past row T N.
constexpr int PARTNER_MAX_COLS = 512;
__global__ __launch_bounds__(256) void partner_rows_kernel(uint32_t rows, uint32_t N, uint32_t per_row, int mode, uint64_t seed, uint32_t update, uint32_t epoch,
                                                           const float* __restrict__ x, const float* __restrict__ x_last, const uint8_t* __restrict__ dones,
                                                           const uint8_t* __restrict__ time_outs, float* __restrict__ y) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t row = t / per_row, piece = t - row * per_row;
    if (row >= rows) return;
    const size_t cols = 4 * (size_t)per_row, at = 4 * (size_t)piece;
    const float* own = x + (size_t)row * cols + at;
    float4 v;
    if (dones[row] | time_outs[row]) {
        v = *reinterpret_cast<const float4*>(own);
    } else {
        const float* nx = row + N < rows ? x + (size_t)(row + N) * cols : x_last + (size_t)(row + N - rows) * cols;
        const float4 b = *reinterpret_cast<const float4*>(nx + at);
        v = b;
        if (mode) {  // (mode "next" reads one row per row, the successor or the row itself)
            const float4 a = *reinterpret_cast<const float4*>(own);
            uint32_t o[4];
            bg::philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), row, update, (uint32_t)bg::RS_PARTNER, epoch, o);
            const float u = (float)(o[0] >> 8) * (1.0f / 16777216.0f);
            v = make_float4(__builtin_fmaf(u, b.x - a.x, a.x), __builtin_fmaf(u, b.y - a.y, a.y), __builtin_fmaf(u, b.z - a.z, a.z),
                            __builtin_fmaf(u, b.w - a.w, a.w));
        }
    }
    *reinterpret_cast<float4*>(y + (size_t)row * cols + at) = v;
}

int head_grid(int tiles) { return tiles < HEAD_MAX_GRID ? tiles : HEAD_MAX_GRID; }

}  // namespace

// the deferred reductions of up to 8 descriptors in one launch
extern "C" int bg_reduce_group(const bg_reduce_problem* problems, int32_t count, void* stream) {
    ReduceGroup grp;
    int blocks = 0;
    if (const int rc = reduce_group_fill(problems, count, 1, grp, blocks, "bg_reduce_group")) return rc;
    hipLaunchKernelGGL(reduce_group_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, grp);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_critic_head_forward(int32_t rows, const float* h, const float* w, const float* b, float* values, void* stream) {
    if (rows <= 0 || !h || !w || !b || !values) return bg_set_error(-1, "bg_critic_head_forward: bad argument");
    if (!aligned16(h) || !aligned16(w)) return bg_set_error(-1, "bg_critic_head_forward: h and w must be 16-byte aligned");
    int blocks = (rows + 31) / 32;  // 8 half-waves x 4 rows per 256-thread workgroup and pass
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(critic_head_forward_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rows, h, w, b, values);
    HIP_OK(hipGetLastError());
    return 0;
}

// bg_critic_values_gae (value_stats == NULL: 3 float64 per workgroup in the scratch) and bg_critic_values_gae_norm (6) are one function
template <bool NORM>
static int critic_values_gae(const char* who, int32_t T, int32_t N, const float* h, const float* w, const float* b, float* rewards, const uint8_t* dones,
                             const uint8_t* time_outs, float gamma, float lam, float* values_all, float* advantages, float* returns, const float* value_stats,
                             double* sums, double* scratch, void* stream) {
    if (T <= 0 || N <= 0 || (h && (!w || !b)) || !rewards || !dones || !time_outs || !values_all || !advantages || !returns || !sums || !scratch ||
        (NORM && !value_stats))
        return bg_fail(who, -1, "bad argument");
    if (h && (!aligned16(h) || !aligned16(w))) return bg_fail(who, -1, "h and w must be 16-byte aligned");
    if (T > 32) return bg_fail(who, -4, "horizon above 32 (use bg_critic_head_forward + bg_gae)");
    unsigned* ticket = reinterpret_cast<unsigned*>(scratch + (size_t)((N + 15) / 16) * (NORM ? 6 : 3));  // the scratch's last element, whichever form runs
    if (h) hipLaunchKernelGGL((critic_values_gae_kernel<32, VG_ENVS_VALUES, NORM>), dim3((N + VG_ENVS_VALUES - 1) / VG_ENVS_VALUES), dim3(256), 0, (hipStream_t)stream, T, N, h, w,
                              b, rewards, dones, time_outs, gamma, lam, values_all, advantages, returns, scratch, ticket, sums, value_stats);
    else hipLaunchKernelGGL((critic_values_gae_kernel<32, VG_ENVS_SCAN, NORM>), dim3((N + VG_ENVS_SCAN - 1) / VG_ENVS_SCAN), dim3(256), 0, (hipStream_t)stream, T, N, h, w, b,
                            rewards, dones, time_outs, gamma, lam, values_all, advantages, returns, scratch, ticket, sums, value_stats);
    HIP_OK(hipGetLastError());
    return 0;
}
extern "C" int bg_critic_values_gae(int32_t T, int32_t N, const float* h, const float* w, const float* b, float* rewards, const uint8_t* dones,
                                    const uint8_t* time_outs, float gamma, float lam, float* values_all, float* advantages, float* returns, double* sums,
                                    double* scratch, void* stream) {
    return critic_values_gae<false>("bg_critic_values_gae", T, N, h, w, b, rewards, dones, time_outs, gamma, lam, values_all, advantages, returns, nullptr, sums,
                                    scratch, stream);
}

// ---- the heads with a loss.  Each is ONE function for its immediate and its deferred entry point: the main kernel, then the sums over its workgroups'
// records -- handed to the caller as a descriptor (`finish`: bg_reduce_group or bg_update_tail runs it later), or, without one, run now as a launch of
// reduce_group_kernel on that descriptor.  `who` prefixes the error messages.
static int head_finish(bg_reduce_problem* finish, const float* scratch, int grid, int record, float* grad_w, int n_w, float* grad_b_hidden, float* grad_b, int n_b,
                       size_t stat_base, int n_stat, int n_ls, unsigned skip, double entropy_coef, double* grad_logstd, double* stats, hipStream_t st) {
    HIP_OK(hipGetLastError());  // the main kernel's launch: a descriptor is filled only behind a launch that was taken
    bg_reduce_problem now;
    bg_reduce_problem* f = finish ? finish : &now;
    f->partial = scratch; f->groups = grid; f->record = record; f->n_out = n_w + HK + n_b;
    f->out[0] = grad_w; f->n[0] = n_w; f->out[1] = grad_b_hidden; f->n[1] = HK; f->out[2] = grad_b; f->n[2] = n_b;
    f->stat_base = stat_base; f->n_stat = n_stat; f->n_ls = n_ls; f->stat_skip = skip; f->entropy_coef = entropy_coef; f->grad_logstd = grad_logstd; f->stats = stats;
    if (finish) return 0;
    ReduceGroup grp;  // (n_out + 15) / 16 + n_stat workgroups
    int blocks = 0;
    if (const int rc = reduce_group_fill(f, 1, 1, grp, blocks, "head finish")) return rc;
    hipLaunchKernelGGL(reduce_group_kernel, dim3(blocks), dim3(256), 0, st, grp);
    HIP_OK(hipGetLastError());
    return 0;
}

static int actor_head_loss(const char* who, int32_t B, const float* h, const float* W, const float* bias, const float* logstd, const float* actions,
                           const float* old_mu, const float* old_logstd, const float* old_logp, const float* adv, const double* adv_stats, float e_clip,
                           float bound_coef, float entropy_coef, float* mu_out, float* g_hidden, float* grad_W, float* grad_b, float* grad_b_hidden,
                           double* grad_logstd, double* stats, float* scratch, bg_reduce_problem* finish, hipStream_t st) {
    if (B <= 0 || !h || !W || !bias || !logstd || !actions || !old_mu || !old_logstd || !old_logp || !adv || !adv_stats || !g_hidden || !grad_W || !grad_b ||
        !grad_b_hidden || !grad_logstd || !stats || !scratch)
        return bg_fail(who, -1, "bad argument");
    if (!aligned16(h)) return bg_fail(who, -1, "h must be 16-byte aligned");
    const int tiles = (B + HT - 1) / HT, grid = head_grid(tiles);
    hipLaunchKernelGGL(actor_head_kernel<1>, dim3(grid), dim3(256), 0, st, B, tiles, h, W, bias, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats,
                       e_clip, bound_coef, mu_out, g_hidden, scratch);
    return head_finish(finish, scratch, grid, head_record<HA>(), grad_W, HA * HK, grad_b_hidden, grad_b, HA, head_stat_base<HA>(), HEAD_NSTAT, HA, 1u << HA,
                       (double)entropy_coef, grad_logstd, stats, st);
}
extern "C" int bg_actor_head(int32_t B, int32_t mode, const float* h, const float* W, const float* bias, const float* logstd, const float* actions,
                             const float* old_mu, const float* old_logstd, const float* old_logp, const float* adv, const double* adv_stats,
                             float e_clip, float bound_coef, float entropy_coef, float* mu_out, float* g_hidden, float* grad_W, float* grad_b,
                             float* grad_b_hidden, double* grad_logstd, double* stats, float* scratch, void* stream) {
    if (mode == 1)
        return actor_head_loss("bg_actor_head", B, h, W, bias, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats, e_clip, bound_coef, entropy_coef, mu_out,
                               g_hidden, grad_W, grad_b, grad_b_hidden, grad_logstd, stats, scratch, nullptr, (hipStream_t)stream);
    if (B <= 0 || !h || !W || !bias) return bg_set_error(-1, "bg_actor_head: bad argument");
    if (!aligned16(h)) return bg_set_error(-1, "bg_actor_head: h must be 16-byte aligned");
    if (mode != 0) return bg_set_error(-1, "bg_actor_head: mode must be 0 (forward) or 1 (forward + loss + backward)");
    if (!mu_out) return bg_set_error(-1, "bg_actor_head: mode 0 needs mu_out");
    const int tiles = (B + HT - 1) / HT;
    hipLaunchKernelGGL(actor_head_kernel<0>, dim3(head_grid(tiles)), dim3(256), 0, (hipStream_t)stream, B, tiles, h, W, bias, nullptr, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr, 0.f, 0.f, mu_out, nullptr, nullptr);
    HIP_OK(hipGetLastError());
    return 0;
}
extern "C" int bg_actor_head_partial(int32_t B, const float* h, const float* W, const float* bias, const float* logstd, const float* actions,
                                     const float* old_mu, const float* old_logstd, const float* old_logp, const float* adv, const double* adv_stats,
                                     float e_clip, float bound_coef, float entropy_coef, float* mu_out, float* g_hidden, float* grad_W, float* grad_b,
                                     float* grad_b_hidden, double* grad_logstd, double* stats, float* scratch, bg_reduce_problem* finish, void* stream) {
    if (!finish) return bg_set_error(-1, "bg_actor_head_partial: bad argument");
    return actor_head_loss("bg_actor_head_partial", B, h, W, bias, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats, e_clip, bound_coef, entropy_coef,
                           mu_out, g_hidden, grad_W, grad_b, grad_b_hidden, grad_logstd, stats, scratch, finish, (hipStream_t)stream);
}

static int critic_head_backward(const char* who, int32_t B, const float* h, const float* w, const float* values, const float* returns, float* g_hidden,
                                float* grad_w, float* grad_b, float* grad_b_hidden, double* stats, float* scratch, bg_reduce_problem* finish, hipStream_t st) {
    if (B <= 0 || !h || !w || !values || !returns || !g_hidden || !grad_w || !grad_b || !grad_b_hidden || !stats || !scratch) return bg_fail(who, -1, "bad argument");
    if (!aligned16(h)) return bg_fail(who, -1, "h must be 16-byte aligned");
    const int tiles = (B + HT - 1) / HT, grid = head_grid(tiles);
    hipLaunchKernelGGL(critic_head_backward_kernel, dim3(grid), dim3(256), 0, st, B, tiles, h, w, values, returns, g_hidden, scratch);
    return head_finish(finish, scratch, grid, head_record<1>(), grad_w, HK, grad_b_hidden, grad_b, 1, head_stat_base<1>(), 1, 0, 0u, 0.0, nullptr, stats, st);
}
extern "C" int bg_critic_head_backward(int32_t B, const float* h, const float* w, const float* values, const float* returns, float* g_hidden,
                                       float* grad_w, float* grad_b, float* grad_b_hidden, double* stats, float* scratch, void* stream) {
    return critic_head_backward("bg_critic_head_backward", B, h, w, values, returns, g_hidden, grad_w, grad_b, grad_b_hidden, stats, scratch, nullptr,
                                (hipStream_t)stream);
}
extern "C" int bg_critic_head_backward_partial(int32_t B, const float* h, const float* w, const float* values, const float* returns, float* g_hidden,
                                               float* grad_w, float* grad_b, float* grad_b_hidden, double* stats, float* scratch, bg_reduce_problem* finish,
                                               void* stream) {
    if (!finish) return bg_set_error(-1, "bg_critic_head_backward_partial: bad argument");
    return critic_head_backward("bg_critic_head_backward_partial", B, h, w, values, returns, g_hidden, grad_w, grad_b, grad_b_hidden, stats, scratch, finish,
                                (hipStream_t)stream);
}

// ---- behaviour-cloning head (teacher-student distillation)
static int distill_head(const char* who, int32_t B, const float* h, const float* W, const float* bias, const float* target, float* mu_out, float* g_hidden,
                        float* grad_W, float* grad_b, float* grad_b_hidden, double* stats, float* scratch, bg_reduce_problem* finish, hipStream_t st) {
    if (B <= 0 || !h || !W || !bias || !target || !g_hidden || !grad_W || !grad_b || !grad_b_hidden || !stats || !scratch) return bg_fail(who, -1, "bad argument");
    if (!aligned16(h)) return bg_fail(who, -1, "h must be 16-byte aligned");
    const int tiles = (B + HT - 1) / HT, grid = head_grid(tiles);
    hipLaunchKernelGGL(distill_head_kernel, dim3(grid), dim3(256), 0, st, B, tiles, h, W, bias, target, mu_out, g_hidden, scratch);
    return head_finish(finish, scratch, grid, head_record<HA>(), grad_W, HA * HK, grad_b_hidden, grad_b, HA, head_stat_base<HA>(), 1, 0, 0u, 0.0, nullptr, stats, st);
}
extern "C" int bg_distill_head(int32_t B, const float* h, const float* W, const float* bias, const float* target, float* mu_out, float* g_hidden, float* grad_W,
                               float* grad_b, float* grad_b_hidden, double* stats, float* scratch, void* stream) {
    return distill_head("bg_distill_head", B, h, W, bias, target, mu_out, g_hidden, grad_W, grad_b, grad_b_hidden, stats, scratch, nullptr, (hipStream_t)stream);
}
extern "C" int bg_distill_head_partial(int32_t B, const float* h, const float* W, const float* bias, const float* target, float* mu_out, float* g_hidden,
                                       float* grad_W, float* grad_b, float* grad_b_hidden, double* stats, float* scratch, bg_reduce_problem* finish, void* stream) {
    if (!finish) return bg_set_error(-1, "bg_distill_head_partial: bad argument");
    return distill_head("bg_distill_head_partial", B, h, W, bias, target, mu_out, g_hidden, grad_W, grad_b, grad_b_hidden, stats, scratch, finish,
                        (hipStream_t)stream);
}

// ---- mirror-symmetry loss
static int action_mirror(ActionMirror* am, const int32_t* act_src, const float* act_sign) {
    if (!act_src || !act_sign) return -1;
    for (int a = 0; a < HA; a++) {
        const int s = act_src[a];
        // a symmetric signed-permutation involution: src[src[a]] = a, sign[src[a]] = sign[a], sign +-1
        if (s < 0 || s >= HA || act_src[s] != a || !(act_sign[a] == 1.f || act_sign[a] == -1.f) || act_sign[s] != act_sign[a]) return -1;
        am->src[a] = s; am->sign[a] = act_sign[a];
    }
    return 0;
}
static int actor_head_sym(const char* who, int32_t B, const float* h, const float* W, const float* bias, const float* logstd, const float* actions,
                          const float* old_mu, const float* old_logstd, const float* old_logp, const float* adv, const double* adv_stats, float e_clip,
                          float bound_coef, float entropy_coef, float sym_coef, const int32_t* act_src, const float* act_sign, float* mu_out, float* g_hidden,
                          float* grad_W, float* grad_b, float* grad_b_hidden, double* grad_logstd, double* stats, float* scratch, bg_reduce_problem* finish,
                          hipStream_t st) {
    if (B <= 0 || !h || !W || !bias || !logstd || !actions || !old_mu || !old_logstd || !old_logp || !adv || !adv_stats || !g_hidden || !grad_W || !grad_b ||
        !grad_b_hidden || !grad_logstd || !stats || !scratch)
        return bg_fail(who, -1, "bad argument");
    ActionMirror am;
    if (action_mirror(&am, act_src, act_sign))
        return bg_fail(who, -1, "act_src / act_sign must be a symmetric signed permutation of the 12 actions that is its own inverse");
    if (!aligned16(h)) return bg_fail(who, -1, "h must be 16-byte aligned");
    const int tiles = (B + HTS - 1) / HTS, grid = head_grid(tiles);
    const float sym_scale = (float)(2.0 * (double)sym_coef / ((double)B * HA));
    hipLaunchKernelGGL(actor_head_sym_kernel, dim3(grid), dim3(256), 0, st, B, tiles, h, W, bias, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats,
                       e_clip, bound_coef, sym_scale, am, mu_out, g_hidden, scratch);
    return head_finish(finish, scratch, grid, head_record<HA>(), grad_W, HA * HK, grad_b_hidden, grad_b, HA, head_stat_base<HA>(), HEAD_NSTAT_SYM, HA, 1u << HA,
                       (double)entropy_coef, grad_logstd, stats, st);
}
extern "C" int bg_actor_head_sym(int32_t B, const float* h, const float* W, const float* bias, const float* logstd, const float* actions, const float* old_mu,
                                 const float* old_logstd, const float* old_logp, const float* adv, const double* adv_stats, float e_clip, float bound_coef,
                                 float entropy_coef, float sym_coef, const int32_t* act_src, const float* act_sign, float* mu_out, float* g_hidden, float* grad_W,
                                 float* grad_b, float* grad_b_hidden, double* grad_logstd, double* stats, float* scratch, void* stream) {
    return actor_head_sym("bg_actor_head_sym", B, h, W, bias, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats, e_clip, bound_coef, entropy_coef, sym_coef,
                          act_src, act_sign, mu_out, g_hidden, grad_W, grad_b, grad_b_hidden, grad_logstd, stats, scratch, nullptr, (hipStream_t)stream);
}
extern "C" int bg_actor_head_sym_partial(int32_t B, const float* h, const float* W, const float* bias, const float* logstd, const float* actions,
                                         const float* old_mu, const float* old_logstd, const float* old_logp, const float* adv, const double* adv_stats,
                                         float e_clip, float bound_coef, float entropy_coef, float sym_coef, const int32_t* act_src, const float* act_sign,
                                         float* mu_out, float* g_hidden, float* grad_W, float* grad_b, float* grad_b_hidden, double* grad_logstd, double* stats,
                                         float* scratch, bg_reduce_problem* finish, void* stream) {
    if (!finish) return bg_set_error(-1, "bg_actor_head_sym_partial: bad argument");
    return actor_head_sym("bg_actor_head_sym_partial", B, h, W, bias, logstd, actions, old_mu, old_logstd, old_logp, adv, adv_stats, e_clip, bound_coef, entropy_coef,
                          sym_coef, act_src, act_sign, mu_out, g_hidden, grad_W, grad_b, grad_b_hidden, grad_logstd, stats, scratch, finish, (hipStream_t)stream);
}

// ---- mirror-symmetry loss on the distillation's student
static int distill_head_sym(const char* who, int32_t B, const float* h, const float* W, const float* bias, const float* target, float sym_coef,
                            const int32_t* act_src, const float* act_sign, float* mu_out, float* g_hidden, float* grad_W, float* grad_b, float* grad_b_hidden,
                            double* stats, float* scratch, bg_reduce_problem* finish, hipStream_t st) {
    if (B <= 0 || !h || !W || !bias || !target || !g_hidden || !grad_W || !grad_b || !grad_b_hidden || !stats || !scratch) return bg_fail(who, -1, "bad argument");
    if (!(sym_coef >= 0.f) || sym_coef > 3.0e38f) return bg_fail(who, -1, "sym_coef must be a finite number >= 0");
    ActionMirror am;
    if (action_mirror(&am, act_src, act_sign))
        return bg_fail(who, -1, "act_src / act_sign must be a symmetric signed permutation of the 12 actions that is its own inverse");
    if (!aligned16(h)) return bg_fail(who, -1, "h must be 16-byte aligned");
    const int tiles = (B + HTS - 1) / HTS, grid = head_grid(tiles);
    const float sym_scale = (float)(2.0 * (double)sym_coef / ((double)B * HA));
    hipLaunchKernelGGL(distill_head_sym_kernel, dim3(grid), dim3(256), 0, st, B, tiles, h, W, bias, target, sym_scale, am, mu_out, g_hidden, scratch);
    return head_finish(finish, scratch, grid, head_record<HA>(), grad_W, HA * HK, grad_b_hidden, grad_b, HA, head_stat_base<HA>(), 2, 0, 0u, 0.0, nullptr, stats, st);
}
extern "C" int bg_distill_head_sym(int32_t B, const float* h, const float* W, const float* bias, const float* target, float sym_coef, const int32_t* act_src,
                                   const float* act_sign, float* mu_out, float* g_hidden, float* grad_W, float* grad_b, float* grad_b_hidden, double* stats,
                                   float* scratch, void* stream) {
    return distill_head_sym("bg_distill_head_sym", B, h, W, bias, target, sym_coef, act_src, act_sign, mu_out, g_hidden, grad_W, grad_b, grad_b_hidden, stats, scratch,
                            nullptr, (hipStream_t)stream);
}
extern "C" int bg_distill_head_sym_partial(int32_t B, const float* h, const float* W, const float* bias, const float* target, float sym_coef, const int32_t* act_src,
                                           const float* act_sign, float* mu_out, float* g_hidden, float* grad_W, float* grad_b, float* grad_b_hidden, double* stats,
                                           float* scratch, bg_reduce_problem* finish, void* stream) {
    if (!finish) return bg_set_error(-1, "bg_distill_head_sym_partial: bad argument");
    return distill_head_sym("bg_distill_head_sym_partial", B, h, W, bias, target, sym_coef, act_src, act_sign, mu_out, g_hidden, grad_W, grad_b, grad_b_hidden, stats,
                            scratch, finish, (hipStream_t)stream);
}

extern "C" int bg_mirror_rows(int32_t rows, int32_t cols, const int32_t* src, const float* sign, const float* x, float* y, void* stream) {
    if (rows <= 0 || cols <= 0 || cols > MIRROR_MAX_COLS || !src || !sign || !x || !y) return bg_set_error(-1, "bg_mirror_rows: bad argument (1 to 512 columns)");
    ColumnMirror cm;
    for (int c = 0; c < MIRROR_MAX_COLS; c++) cm.code[c] = -1;
    for (int c = 0; c < cols; c++) {
        if (src[c] < -1 || src[c] >= cols || !(sign[c] == 1.f || sign[c] == -1.f)) return bg_set_error(-1, "bg_mirror_rows: src in [-1, cols), sign +-1");
        cm.code[c] = (int16_t)(src[c] < 0 ? -1 : (src[c] | (sign[c] < 0.f ? MIRROR_NEG : 0)));
    }
    const float *xe = x + (size_t)rows * cols, *ye = y + (size_t)rows * cols;
    if (x < ye && y < xe) return bg_set_error(-1, "bg_mirror_rows: x and y overlap");
    size_t blocks = ((size_t)rows * cols + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(mirror_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rows, cols, cm, x, y);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_partner_rows(int32_t T, int32_t N, int32_t cols, const float* x, const float* x_last, const uint8_t* dones, const uint8_t* time_outs, int32_t mode,
                               uint64_t seed, uint32_t update, uint32_t epoch, float* y, void* stream) {
    if (T <= 0 || N <= 0 || !x || !x_last || !dones || !time_outs || !y) return bg_set_error(-1, "bg_partner_rows: bad argument");
    if (cols < 4 || cols > PARTNER_MAX_COLS || cols % 4) return bg_set_error(-1, "bg_partner_rows: bad argument (cols a multiple of 4, 4 to 512)");
    if (mode != BG_PARTNER_NEXT && mode != BG_PARTNER_INTERPOLATE) return bg_set_error(-1, "bg_partner_rows: bad argument (mode 0 = next or 1 = interpolate)");
    if (!aligned16(x) || !aligned16(x_last) || !aligned16(y)) return bg_set_error(-1, "bg_partner_rows: x, x_last and y must be 16-byte aligned");
    const uint64_t rows = (uint64_t)T * (uint64_t)N, per_row = (uint64_t)cols / 4;
    if (rows >= (1ull << 31) || rows * per_row + 256 >= (1ull << 32)) return bg_set_error(-1, "bg_partner_rows: bad argument (the launch would exceed 2^32 threads)");
    const float *xe = x + rows * cols, *le = x_last + (size_t)N * cols, *ye = y + rows * cols;
    if ((x < ye && y < xe) || (x_last < ye && y < le)) return bg_set_error(-1, "bg_partner_rows: y overlaps x or x_last");
    const uint64_t blocks = (rows * per_row + 255) / 256;
    hipLaunchKernelGGL(partner_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (uint32_t)rows, (uint32_t)N, (uint32_t)per_row, (int)mode, seed,
                       update, epoch, x, x_last, dones, time_outs, y);
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- value normalisation (algorithm.normalize_value).  Its device code and entry points stand at the end of the file, so that every kernel above keeps
// its place in the code object.  (The two small kernels are templates for that reason alone: a template's code is emitted behind the plain kernels'.)
namespace {

// values[i] = fmaf(sigma, values[i], m): the critic's standardised output u of algorithm.normalize_value in reward units, the one rounding that
// critic_values_gae_kernel<NORM> gives it on the way into LDS
template <int = 0>
__global__ __launch_bounds__(256) void value_denormalize_kernel(int rows, float* __restrict__ values, const float* __restrict__ value_stats) {
    const float m = value_stats[0], sigma = value_stats[1];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < rows; i += gridDim.x * 256) values[i] = __builtin_fmaf(sigma, values[i], m);
}

// Chan et al.'s merge of the running (mean, population variance, count) in state with the batch whose (sum R, sum R^2, count) stand in sums[3..5]
// (utils/obs_norm.py: moments_from_sums, merge_moments, restated in float64 on the device), then the fp32 triple (m, sigma, 1 / sigma) the kernels
// read, sigma = sqrt(var) + eps.  A batch of no rows changes nothing.  One wave, one lane at work: 30 flops once per iteration.
template <int = 0>
__global__ __launch_bounds__(64) void value_norm_update_kernel(const double* __restrict__ sums, double* __restrict__ state, float* __restrict__ value_stats,
                                                               double eps) {
#pragma clang fp contract(off) reassociate(off)
    const double n = sums[5];
    if (threadIdx.x != 0 || !(n > 0.0)) return;
    const double mean = state[0], var = state[1], count = state[2];
    const double m_b = sums[3] / n;
    double v_b = sums[4] / n - m_b * m_b;
    v_b = v_b > 0.0 ? v_b : 0.0;
    const double total = count + n, r = n / total, d = m_b - mean;
    const double new_mean = mean + r * d;
    double new_var = var + r * (v_b - var + d * (m_b - new_mean));
    new_var = new_var > 0.0 ? new_var : 0.0;
    state[0] = new_mean; state[1] = new_var; state[2] = total;
    const double sigma = sqrt(new_var) + eps;
    value_stats[0] = (float)new_mean; value_stats[1] = (float)sigma; value_stats[2] = (float)(1.0 / sigma);
}

}  // namespace

extern "C" int bg_critic_values_gae_norm(int32_t T, int32_t N, const float* h, const float* w, const float* b, float* rewards, const uint8_t* dones,
                                         const uint8_t* time_outs, float gamma, float lam, float* values_all, float* advantages, float* returns,
                                         const float* value_stats, double* sums, double* scratch, void* stream) {
    return critic_values_gae<true>("bg_critic_values_gae_norm", T, N, h, w, b, rewards, dones, time_outs, gamma, lam, values_all, advantages, returns, value_stats,
                                   sums, scratch, stream);
}

extern "C" int bg_value_denormalize(int32_t rows, float* values, const float* value_stats, void* stream) {
    if (rows <= 0 || !values || !value_stats) return bg_set_error(-1, "bg_value_denormalize: bad argument");
    int blocks = (rows + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(value_denormalize_kernel<>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rows, values, value_stats);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_value_norm_update(const double* sums, double* state, float* value_stats, double eps, void* stream) {
    if (!sums || !state || !value_stats || !(eps > 0.0)) return bg_set_error(-1, "bg_value_norm_update: bad argument (eps > 0)");
    hipLaunchKernelGGL(value_norm_update_kernel<>, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, state, value_stats, eps);
    HIP_OK(hipGetLastError());
    return 0;
}

// Shuffled mini-batches of the PPO update (runner.num_mini_batches > 1; utils/runner.py): the two launches the feature adds per mini-epoch.  Neither
// runs when the key is absent or 1.
//
//   bg_perm_fill     pi[i] = perm_index(key, n, i) (bg_perm.h: a keyed Feistel bijection with cycle walking), one thread per index.
//   bg_gather_rows   dst_s[i][:] = src_s[pi[i]][:] for up to BG_GATHER_MAX_STREAMS row-major fp32 streams of their own widths in ONE launch: the
//                    rows every optimiser step of the mini-epoch reads, laid out mini-batch after mini-batch.
//
// The gather is memory-bound and does no arithmetic.  A stream whose width is a multiple of 4 floats (and whose buffers are 16-byte aligned) moves
// 16 bytes per thread, consecutive threads on consecutive 16-byte pieces of one row: a wave reads 64 / (width / 4) whole rows -- every row a run of
// whole 64- or 128-byte pieces of lines (a 64-float row is 256 bytes = two 128-byte lines) -- and writes 1 KiB of consecutive destination bytes.  The
// other streams (the per-row scalars) move 4 bytes per thread: random 4-byte reads, consecutive 4-byte writes; they are 3 of 155 floats per row at
// the default shape.  pi is read once per thread (the threads of a row read the same word: one request per wave and row).
//
// Env-wise mini-batches of sequences for a recurrent actor (runner.num_env_mini_batches > 1) add one launch per mini-epoch, beside a bg_perm_fill
// over the N envs:
//
//   bg_gather_sequences   dst_s[(k T + t) n + j][:] = src_s[t N + sigma[k n + j]][:], n = N / K: the whole T-step sequences of the envs of mini-batch k,
//                         step-major, mini-batch after mini-batch, from the env permutation sigma alone (no B-long row permutation exists); a
//                         per-env stream (the state h0) dst_s[i][:] = src_s[sigma[i]][:]; elements of 4 bytes or of 1 byte (the reset flags).
//
// It is the same copy with another index rule: one kernel body (gather_kernel) serves both, the rule is its template parameter.

#include "bg_common.h"
#include "bg_perm.h"

constexpr int MB_BLOCK = 256;

__global__ __launch_bounds__(MB_BLOCK) void perm_fill_kernel(bg::PermKey key, uint32_t n, int32_t* __restrict__ perm) {
    const uint32_t i = blockIdx.x * MB_BLOCK + threadIdx.x;
    if (i < n) perm[i] = (int32_t)bg::perm_index(key, n, i);
}

extern "C" int bg_perm_fill(int32_t n, uint64_t seed, uint32_t update, uint32_t epoch, int32_t* perm, void* stream) {
    if (n <= 0 || !perm) return bg_set_error(-1, "bg_perm_fill: bad argument");
    if (epoch >= (1u << 24)) return bg_set_error(-1, "bg_perm_fill: bad argument (epoch must stay below 2^24)");
    const bg::PermKey key{seed, update, epoch};
    hipLaunchKernelGGL(perm_fill_kernel, dim3(((unsigned)n + MB_BLOCK - 1) / MB_BLOCK), dim3(MB_BLOCK), 0, (hipStream_t)stream, key, (uint32_t)n, perm);
    HIP_OK(hipGetLastError());
    return 0;
}

// The copy both gathers share.  A launch serves up to MAX streams; the blocks [first_block[s], first_block[s + 1]) serve stream s, unit[s] bytes per thread
// (16, 4 or 1), per_row[s] = row bytes / unit threads per row.  Which destination rows a stream has and which source row each of them copies is the
// launch's index rule (the template parameter of gather_kernel):
//   rows(per_env)                the destination rows of a stream;
//   source(per_env, row, from)   from = the source row of destination row `row`; false: the permutation names no row of the source, the destination
//                                row is left as it is (never an out-of-bounds read).
template <int MAX>
struct GatherStreams {
    const char* src[MAX];
    char* dst[MAX];
    uint32_t row_bytes[MAX];
    uint32_t per_row[MAX];   // threads per row
    uint32_t unit[MAX];      // bytes per thread: 16 (whole 16-byte pieces of aligned rows), else the element size
    uint32_t per_env[MAX];   // bg_gather_sequences: one row per env, not per (step, env)
    uint32_t first_block[MAX + 1];
    int32_t n;
};

struct PermutedRows {  // bg_gather_rows: destination row i <- source row perm[i]
    const int32_t* perm;
    uint32_t n_rows, src_rows;
    __device__ uint32_t rows(uint32_t) const { return n_rows; }
    __device__ bool source(uint32_t, uint32_t row, size_t& from) const {
        const uint32_t f = (uint32_t)perm[row];
        from = f;
        return f < src_rows;
    }
};

struct PermutedSequences {  // bg_gather_sequences: [K][T][n] <- [T][N] by the env permutation sigma, n = N / K; a per-env stream [K][n] <- [N]
    const int32_t* sigma;
    uint32_t T, N, n;
    __device__ uint32_t rows(uint32_t per_env) const { return per_env ? N : T * N; }
    __device__ bool source(uint32_t per_env, uint32_t row, size_t& from) const {
        uint32_t t = 0, i = row;  // i: the position in sigma, k n + j
        if (!per_env) {
            const uint32_t k = row / (T * n), r = row - k * (T * n);
            t = r / n;
            i = k * n + (r - t * n);
        }
        const uint32_t env = (uint32_t)sigma[i];
        from = (size_t)t * N + env;
        return env < N;
    }
};

template <int MAX, class Rule>
__global__ __launch_bounds__(MB_BLOCK) void gather_kernel(GatherStreams<MAX> q, Rule rule) {
    int s = 0;
    while (s + 1 < q.n && blockIdx.x >= q.first_block[s + 1]) s++;
    const uint32_t t = (blockIdx.x - q.first_block[s]) * MB_BLOCK + threadIdx.x;
    const uint32_t per_row = q.per_row[s];
    const uint32_t row = t / per_row, piece = t - row * per_row;
    if (row >= rule.rows(q.per_env[s])) return;
    size_t from;
    if (!rule.source(q.per_env[s], row, from)) return;
    const size_t w = q.row_bytes[s];
    const uint32_t unit = q.unit[s];
    const char* src = q.src[s] + from * w + (size_t)unit * piece;
    char* dst = q.dst[s] + (size_t)row * w + (size_t)unit * piece;
    if (unit == 16) {
        *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
    } else if (unit == 4) {
        *reinterpret_cast<uint32_t*>(dst) = *reinterpret_cast<const uint32_t*>(src);
    } else {
        *dst = *src;
    }
}

// One stream's place in the launch: its unit and threads per row, its blocks behind those of the streams before it.  False: over 2^32 threads.
template <int MAX>
static bool place_stream(GatherStreams<MAX>& q, int s, const void* src, void* dst, uint32_t row_bytes, uint32_t elem, uint32_t per_env, uint64_t rows,
                         uint64_t& blocks) {
    const bool vec = row_bytes % 16 == 0 && ((uintptr_t)src | (uintptr_t)dst) % 16 == 0;
    q.src[s] = (const char*)src; q.dst[s] = (char*)dst; q.row_bytes[s] = row_bytes; q.unit[s] = vec ? 16 : elem; q.per_env[s] = per_env;
    q.per_row[s] = row_bytes / q.unit[s];
    q.first_block[s] = (uint32_t)blocks;
    blocks += (rows * q.per_row[s] + MB_BLOCK - 1) / MB_BLOCK;
    return blocks * MB_BLOCK < (1ull << 32);
}

extern "C" int bg_gather_rows(int32_t rows, int32_t src_rows, const int32_t* perm, const bg_gather_stream* streams, int32_t n_streams, void* stream) {
    if (rows <= 0 || src_rows <= 0 || !perm || !streams) return bg_set_error(-1, "bg_gather_rows: bad argument");
    if (n_streams < 1 || n_streams > BG_GATHER_MAX_STREAMS) return bg_set_error(-1, "bg_gather_rows: bad argument (1 to BG_GATHER_MAX_STREAMS streams)");
    GatherStreams<BG_GATHER_MAX_STREAMS> q{};
    q.n = n_streams;
    uint64_t blocks = 0;
    for (int s = 0; s < n_streams; s++) {
        const bg_gather_stream& g = streams[s];
        if (!g.src || !g.dst || g.width < 1 || g.width > 4096) return bg_set_error(-1, "bg_gather_rows: bad stream (NULL buffer, or a width outside 1 to 4096 floats)");
        const float *se = g.src + (size_t)src_rows * g.width, *de = g.dst + (size_t)rows * g.width;
        if (g.src < de && g.dst < se) return bg_set_error(-1, "bg_gather_rows: bad stream (source and destination overlap)");
        if (!place_stream(q, s, g.src, g.dst, 4u * (uint32_t)g.width, 4, 0, (uint64_t)rows, blocks))
            return bg_set_error(-1, "bg_gather_rows: bad argument (the launch would exceed 2^32 threads)");
    }
    q.first_block[n_streams] = (uint32_t)blocks;
    const PermutedRows rule{perm, (uint32_t)rows, (uint32_t)src_rows};
    hipLaunchKernelGGL((gather_kernel<BG_GATHER_MAX_STREAMS, PermutedRows>), dim3((unsigned)blocks), dim3(MB_BLOCK), 0, (hipStream_t)stream, q, rule);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bg_gather_sequences(int32_t T, int32_t N, int32_t K, const int32_t* sigma, const bg_sequence_stream* streams, int32_t n_streams, void* stream) {
    if (T <= 0 || N <= 0 || K <= 0 || !sigma || !streams) return bg_set_error(-1, "bg_gather_sequences: bad argument");
    if (N % K) return bg_set_error(-1, "bg_gather_sequences: bad argument (K must divide N: every mini-batch holds the sequences of N / K envs)");
    if ((uint64_t)T * (uint64_t)N >= (1ull << 31)) return bg_set_error(-1, "bg_gather_sequences: bad argument (T x N must stay below 2^31 rows)");
    if (n_streams < 1 || n_streams > BG_SEQUENCE_MAX_STREAMS)
        return bg_set_error(-1, "bg_gather_sequences: bad argument (1 to BG_SEQUENCE_MAX_STREAMS streams)");
    GatherStreams<BG_SEQUENCE_MAX_STREAMS> q{};
    q.n = n_streams;
    uint64_t blocks = 0;
    for (int s = 0; s < n_streams; s++) {
        const bg_sequence_stream& g = streams[s];
        if (!g.src || !g.dst || g.width < 1 || g.width > 4096)
            return bg_set_error(-1, "bg_gather_sequences: bad stream (NULL buffer, or a width outside 1 to 4096 elements)");
        if (g.elem_size != 4 && g.elem_size != 1) return bg_set_error(-1, "bg_gather_sequences: bad stream (the element size must be 4 bytes or 1 byte)");
        if (((uintptr_t)g.src | (uintptr_t)g.dst) % (uintptr_t)g.elem_size)
            return bg_set_error(-1, "bg_gather_sequences: bad stream (a buffer of 4-byte elements must be 4-byte aligned)");
        const uint64_t rows = g.per_env ? (uint64_t)N : (uint64_t)T * (uint64_t)N;
        const uint32_t row_bytes = (uint32_t)g.width * (uint32_t)g.elem_size;
        const char *sb = (const char*)g.src, *db = (const char*)g.dst;
        if (sb < db + rows * row_bytes && db < sb + rows * row_bytes) return bg_set_error(-1, "bg_gather_sequences: bad stream (source and destination overlap)");
        if (!place_stream(q, s, g.src, g.dst, row_bytes, (uint32_t)g.elem_size, g.per_env ? 1u : 0u, rows, blocks))
            return bg_set_error(-1, "bg_gather_sequences: bad argument (the launch would exceed 2^32 threads)");
    }
    q.first_block[n_streams] = (uint32_t)blocks;
    const PermutedSequences rule{sigma, (uint32_t)T, (uint32_t)N, (uint32_t)(N / K)};
    hipLaunchKernelGGL((gather_kernel<BG_SEQUENCE_MAX_STREAMS, PermutedSequences>), dim3((unsigned)blocks), dim3(MB_BLOCK), 0, (hipStream_t)stream, q, rule);
    HIP_OK(hipGetLastError());
    return 0;
}

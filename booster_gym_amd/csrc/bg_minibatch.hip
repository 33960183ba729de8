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

struct GatherArgs {
    const float* src[BG_GATHER_MAX_STREAMS];
    float* dst[BG_GATHER_MAX_STREAMS];
    uint32_t width[BG_GATHER_MAX_STREAMS];  // floats per row
    uint32_t per_row[BG_GATHER_MAX_STREAMS];  // threads per row: width / 4 (16-byte pieces) or width (single floats)
    uint32_t vec[BG_GATHER_MAX_STREAMS];
    uint32_t first_block[BG_GATHER_MAX_STREAMS + 1];  // the blocks [first_block[s], first_block[s + 1]) serve stream s
    int32_t n, rows, src_rows;
};

__global__ __launch_bounds__(MB_BLOCK) void gather_rows_kernel(GatherArgs q, const int32_t* __restrict__ perm) {
    int s = 0;
    while (s + 1 < q.n && blockIdx.x >= q.first_block[s + 1]) s++;
    const uint32_t t = (blockIdx.x - q.first_block[s]) * MB_BLOCK + threadIdx.x;
    const uint32_t per_row = q.per_row[s];
    const uint32_t row = t / per_row, piece = t - row * per_row;
    if (row >= (uint32_t)q.rows) return;
    const uint32_t from = (uint32_t)perm[row];
    if (from >= (uint32_t)q.src_rows) return;  // (an index outside the source: the destination row is left as it is; never an out-of-bounds read)
    const size_t w = q.width[s];
    if (q.vec[s]) {
        const float4 v = *reinterpret_cast<const float4*>(q.src[s] + (size_t)from * w + 4 * piece);
        *reinterpret_cast<float4*>(q.dst[s] + (size_t)row * w + 4 * piece) = v;
    } else {
        q.dst[s][(size_t)row * w + piece] = q.src[s][(size_t)from * w + piece];
    }
}

extern "C" int bg_gather_rows(int32_t rows, int32_t src_rows, const int32_t* perm, const bg_gather_stream* streams, int32_t n_streams, void* stream) {
    if (rows <= 0 || src_rows <= 0 || !perm || !streams) return bg_set_error(-1, "bg_gather_rows: bad argument");
    if (n_streams < 1 || n_streams > BG_GATHER_MAX_STREAMS) return bg_set_error(-1, "bg_gather_rows: bad argument (1 to BG_GATHER_MAX_STREAMS streams)");
    GatherArgs q{};
    q.n = n_streams; q.rows = rows; q.src_rows = src_rows;
    uint64_t blocks = 0;
    for (int s = 0; s < n_streams; s++) {
        const bg_gather_stream& g = streams[s];
        if (!g.src || !g.dst || g.width < 1 || g.width > 4096) return bg_set_error(-1, "bg_gather_rows: bad stream (NULL buffer, or a width outside 1 to 4096 floats)");
        const float *se = g.src + (size_t)src_rows * g.width, *de = g.dst + (size_t)rows * g.width;
        if (g.src < de && g.dst < se) return bg_set_error(-1, "bg_gather_rows: bad stream (source and destination overlap)");
        const bool vec = g.width % 4 == 0 && ((uintptr_t)g.src | (uintptr_t)g.dst) % 16 == 0;
        q.src[s] = g.src; q.dst[s] = g.dst; q.width[s] = (uint32_t)g.width; q.vec[s] = vec;
        q.per_row[s] = (uint32_t)(vec ? g.width / 4 : g.width);
        q.first_block[s] = (uint32_t)blocks;
        blocks += ((uint64_t)rows * q.per_row[s] + MB_BLOCK - 1) / MB_BLOCK;
        if (blocks * MB_BLOCK >= (1ull << 32)) return bg_set_error(-1, "bg_gather_rows: bad argument (the launch would exceed 2^32 threads)");
    }
    q.first_block[n_streams] = (uint32_t)blocks;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)blocks), dim3(MB_BLOCK), 0, (hipStream_t)stream, q, perm);
    HIP_OK(hipGetLastError());
    return 0;
}

// Clock stamps of the chained kernels (bg_mlp_chain.hip, bg_mlp_chain_split.hip, bg_mlp_chain_split_bwd.hip), of the rollout actor (bg_ppo.hip) and of the split
// weight gradients (bg_wgrad_split.hip, decoder tools/wgrad_split_stamps.py): every wave notes the shader clock at
// numbered points of its run in an array of its own and writes the array to a device buffer when the kernel ends; tools/mlp_chain_stamps.py,
// tools/chain_split_stamps.py and tools/chain_split_bwd_stamps.py read the buffers (tools/build_stamps.sh builds the library they need).  The ONLY
// probe in the kernel sources, and this file the only place that tests its macro: the product build never defines BG_CHAIN_PROBE_STAMPS, and every
// macro below is then empty.
//   BG_STAMP_BUFFER(BUF, READER, RECORDS, SLOTS)  file scope: the buffer [RECORDS][4 waves][SLOTS] and the exported function that copies it to the host
//   BG_STAMP_LOCALS(SLOTS)                        the wave's array (zeros: a slot nobody stamps reads 0)
//   BG_STAMP(K) / BG_STAMP_WALL(K)                slot K = the shader clock / the 100 MHz wall clock
//   BG_STAMP_FENCED(K)                            BG_STAMP(K) that the instruction scheduler moves nothing across (bg_ppo.hip: actor_sample_kernel)
//   BG_STAMP_OPEN(K) / BG_STAMP_CLOSE(K)          slot K accumulates the shader-clock cycles between the two (fenced), over every pass: a loop's parts in a
//                                                 few slots (bg_wgrad_split.hip, tools/wgrad_split_stamps.py); BG_STAMP_TURN(K, L) closes K and opens L with ONE
//                                                 clock read; BG_STAMP_WALL_OPEN / _CLOSE(K): the same with the 100 MHz wall clock
//   BG_STAMP_FLUSH(BUF, SLOTS, OK, RECORD)        kernel end: lane 0 of every wave writes its array to record RECORD if OK
#pragma once
#ifdef BG_CHAIN_PROBE_STAMPS
#define BG_STAMP_BUFFER(BUF, READER, RECORDS, SLOTS)    \
    __device__ long long BUF[(RECORDS) * 4 * (SLOTS)]; \
    extern "C" int READER(void* dst, size_t bytes) { return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(BUF), bytes); }
#define BG_STAMP_LOCALS(SLOTS) long long stamps[SLOTS] = {}
#define BG_STAMP(K) stamps[K] = clock64()
#define BG_STAMP_WALL(K) stamps[K] = wall_clock64()
#define BG_STAMP_FENCED(K) do { __builtin_amdgcn_sched_barrier(0); stamps[K] = clock64(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define BG_STAMP_OPEN(K) do { __builtin_amdgcn_sched_barrier(0); stamps[K] -= clock64(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define BG_STAMP_CLOSE(K) do { __builtin_amdgcn_sched_barrier(0); stamps[K] += clock64(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define BG_STAMP_TURN(K, L) do { __builtin_amdgcn_sched_barrier(0); const long long t_ = clock64(); stamps[K] += t_; stamps[L] -= t_; __builtin_amdgcn_sched_barrier(0); } while (0)
#define BG_STAMP_WALL_OPEN(K) stamps[K] -= wall_clock64()
#define BG_STAMP_WALL_CLOSE(K) stamps[K] += wall_clock64()
#define BG_STAMP_FLUSH(BUF, SLOTS, OK, RECORD)                                                                                   \
    do {                                                                                                                         \
        if ((threadIdx.x & 63) == 0 && (OK))                                                                                   \
            for (int k_ = 0; k_ < (SLOTS); k_++) BUF[((size_t)(RECORD) * 4 + (threadIdx.x >> 6)) * (SLOTS) + k_] = stamps[k_];  \
    } while (0)
#else
#define BG_STAMP_BUFFER(BUF, READER, RECORDS, SLOTS)
#define BG_STAMP_LOCALS(SLOTS) do { } while (0)
#define BG_STAMP(K) do { } while (0)
#define BG_STAMP_WALL(K) do { } while (0)
#define BG_STAMP_FENCED(K) do { } while (0)
#define BG_STAMP_OPEN(K) do { } while (0)
#define BG_STAMP_CLOSE(K) do { } while (0)
#define BG_STAMP_TURN(K, L) do { } while (0)
#define BG_STAMP_WALL_OPEN(K) do { } while (0)
#define BG_STAMP_WALL_CLOSE(K) do { } while (0)
#define BG_STAMP_FLUSH(BUF, SLOTS, OK, RECORD) do { } while (0)
#endif

// The preamble of the library's translation units, written once: the error plumbing of the entry points, the helpers that one .hip file defines for
// another, the native vector types of the MFMA operands and the small device helpers the layer and chain kernels share.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <type_traits>
#include <utility>

#include "../../include/booster_gym_amd.h"

int bg_set_error(int code, const char* msg);  // bg_model.cpp (host-only code): keeps the message of bg_last_error, returns `code`
// (bg_sim.hip has a HIP_OK of its own: its message also names the failing call)
#define HIP_OK(expr)                                                          \
    do {                                                                      \
        hipError_t _e = (expr);                                               \
        if (_e != hipSuccess) return bg_set_error(-2, hipGetErrorString(_e)); \
    } while (0)
// the message of a check that several entry points share: "<who>: <what>"
inline int bg_fail(const char* who, int code, const char* what) { return bg_set_error(code, (std::string(who) + ": " + what).c_str()); }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- defined in one translation unit, called from others
struct WgradGroup;  // bg_wgrad.h
// bg_wgrad.hip: validation + descriptor build of a grouped weight-gradient launch (`who` prefixes the error messages); the launch of its fixed-order finish
int bg_wgrad_group_fill(const bg_wgrad_problem* problems, int32_t count, WgradGroup& grp, int& wg, int& fin, const char* who);
int bg_wgrad_group_finish_launch(const WgradGroup& grp, int fin, hipStream_t st);
// bg_mlp.hip: the launch of the backward layer's fixed-order column-sum finish
int bg_colsum_finish_launch(int nb, int C, const float* partial, float* out, hipStream_t st);

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));  // native vector: stays in registers (HIP's float4 struct blocked SROA in the layer kernels)
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// one split-bf16 product into its accumulator, and the scheduling barrier that pins the instruction order around it
#define BG_MFMA(ACC, A, B) ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A), __builtin_bit_cast(bf16x8, B), ACC, 0, 0, 0)
#define BG_PIN() __builtin_amdgcn_sched_barrier(0)

// exp(x) - 1 through v_exp_f32: absolute error ~1e-7 on (-1, 0], far below fp32 activation noise; expm1f costs ~20 VALU per element
__device__ __forceinline__ float elu_f(float x) { return x > 0.f ? x : __expf(x) - 1.0f; }

// f(integral_constant<int, 0>{}) ... f(integral_constant<int, N - 1>{}): a loop whose index is a compile-time constant in its body
template <int... I, class F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(std::make_integer_sequence<int, N>{}, f); }

// s_waitcnt vmcnt(n) only (gfx9 encoding: vmcnt = bits 3:0 and 15:14, expcnt 6:4, lgkmcnt 11:8)
template <int N>
__device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0, "");
    constexpr int n = N > 63 ? 63 : N;
    __builtin_amdgcn_s_waitcnt((n & 15) | ((n >> 4) << 14) | 0x0F70);
}

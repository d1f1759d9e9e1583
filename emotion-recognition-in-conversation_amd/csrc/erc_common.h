// Shared helpers of libercgraft (host-side error plumbing + device utilities).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/ercgraft.h"

#define ERC_WAVE 64

extern "C" void erc_set_error(const char* fmt, ...);

#define ERC_REQUIRE(cond, ...)              \
    do {                                    \
        if (!(cond)) {                      \
            erc_set_error(__VA_ARGS__);     \
            return ERC_E_ARG;               \
        }                                   \
    } while (0)

#define ERC_LAUNCH_CHECK(name)                                                   \
    do {                                                                         \
        hipError_t e__ = hipGetLastError();                                      \
        if (e__ != hipSuccess) {                                                 \
            erc_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
            return ERC_E_LAUNCH;                                                 \
        }                                                                        \
    } while (0)

static inline int erc_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

#ifdef __HIPCC__
// register vectors: MFMA operands / accumulators and 8- / 16-byte memory accesses.  f4 and f2 are the short names of the
// attention and scan kernels.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// workgroup barrier that orders LDS traffic only: __syncthreads() also waits for every global load, store and LDS-DMA request
// in flight (vmcnt), which serialises whatever a kernel prefetches across the barrier behind it
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// fp32 <-> bf16 bits
__device__ __forceinline__ unsigned short f2bf(float f) {
    const __bf16 h = (__bf16)f;  // plain cast: v_cvt_pk_bf16_f32, RNE, NaN stays NaN
    return __builtin_bit_cast(unsigned short, h);
}
__device__ __forceinline__ float bf2f(unsigned short h) { return __builtin_bit_cast(float, (unsigned)h << 16); }
// {bf16(lo), bf16(hi)} as one dword, lo in the low half: v_cvt_pk_bf16_f32; and the two halves back as fp32
__device__ __forceinline__ unsigned bf_pack(float lo, float hi) {
    const __bf16 a = (__bf16)lo, b = (__bf16)hi;
    return (unsigned)__builtin_bit_cast(unsigned short, a) | ((unsigned)__builtin_bit_cast(unsigned short, b) << 16);
}
__device__ __forceinline__ float bf_lo(unsigned d) { return __builtin_bit_cast(float, d << 16); }
__device__ __forceinline__ float bf_hi(unsigned d) { return __builtin_bit_cast(float, d & 0xffff0000u); }

// Cross-workgroup hand-offs WITHOUT fences (an agent-scope release/acquire fence pair costs ~3.5 us per workgroup on
// MI355X: L2 write-back + invalidate): the data is written with write-through (sc1) stores, drained with s_waitcnt vmcnt(0)
// before the workgroup's arrival ticket; the last arriver reads it with sc1 loads.
__device__ __forceinline__ float ld_sc1(const float* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1(float* p, float v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_sc1d(const double* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1d(double* p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// DPP lane exchanges inside a row of 16 lanes (VALU, no LDS traffic)
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
constexpr int DPP_X1 = 0xB1, DPP_X2 = 0x4E, DPP_HMIR = 0x141, DPP_MIR = 0x140;  // quad_perm xor 1 / xor 2, row_half_mirror, row_mirror
// value of lane Q of the caller's quad (lanes 4u .. 4u+3), in every lane of the quad: one DPP move, no LDS
template <int Q>
__device__ __forceinline__ float quad_bcast(float v) { return dpp_mov<Q * 0x55>(v); }
// sum over the quad, the same bits in its four lanes (xor 1, then xor 2: both orders add the same two pairs)
__device__ __forceinline__ float quad_sum(float v) {
    v += dpp_mov<DPP_X1>(v);
    return v + dpp_mov<DPP_X2>(v);
}
// sum over the 16 lanes of a DPP row, in every lane, in a fixed order: quad xor 1 / xor 2, half mirror, mirror.  By value, one
// sum a call: a form that takes the scans' four backward sums as an array reference keeps the array in memory until after
// inlining, and the compiler then schedules the whole step differently
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_mov<DPP_X1>(v);
    v += dpp_mov<DPP_X2>(v);
    v += dpp_mov<DPP_HMIR>(v);
    return v + dpp_mov<DPP_MIR>(v);
}

// full-wave (64 lane) sum, result in every lane
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// Sum 16 per-lane values over the wavefront in 17 shuffles (instead of 16 x 6): halve the set of values and the lane
// distance together.  Lane l ends up with the total of entry ((l>>5)&1)*8 + ((l>>4)&1)*4 + ((l>>3)&1)*2 + ((l>>2)&1).
// (The steps are a macro expanded in the two forms below, not a function one form calls: built on butterfly16_sum, wave_sums_ch
//  made hipcc schedule cogmen_fused.hip's forward kernels differently.)
#define ERC_BUTTERFLY16(a, e)                                                                                              \
    float b[8], c[4], d[2];                                                                                                \
    const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8, h2 = lane & 4;                                               \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) b[j] = (h5 ? a[8 + j] : a[j]) + __shfl_xor(h5 ? a[j] : a[8 + j], 32, 64); \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) c[j] = (h4 ? b[4 + j] : b[j]) + __shfl_xor(h4 ? b[j] : b[4 + j], 16, 64); \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) d[j] = (h3 ? c[2 + j] : c[j]) + __shfl_xor(h3 ? c[j] : c[2 + j], 8, 64);  \
    float e = (h2 ? d[1] : d[0]) + __shfl_xor(h2 ? d[0] : d[1], 4, 64);                                                    \
    e += __shfl_xor(e, 2, 64);                                                                                             \
    e += __shfl_xor(e, 1, 64)
__device__ __forceinline__ float butterfly16_sum(const float (&a)[16], int lane) {
    ERC_BUTTERFLY16(a, e);
    return e;
}
// CH (<= 16) per-lane partial dot products -> every lane gets all CH wave totals: one butterfly and CH lane reads instead of
// CH full wave reductions (6 shuffles each).
template <int CH>
__device__ __forceinline__ void wave_sums_ch(const float (&part)[16], float (&tot)[CH], int lane) {
    static_assert(CH <= 16, "one butterfly");
    ERC_BUTTERFLY16(part, e);
#pragma unroll
    for (int u = 0; u < CH; ++u) tot[u] = __shfl(e, ((u >> 3) & 1) * 32 + ((u >> 2) & 1) * 16 + ((u >> 1) & 1) * 8 + (u & 1) * 4, 64);
}
#undef ERC_BUTTERFLY16

// Window graph (track_mm/cogmen_utils.py:109-172): sum_{q<p} deg(q) with deg(q) = min(L-1, q+fwd) - max(0, q-back) + 1 --
// the closed form behind every CSR offset of a dialogue of L utterances.
__device__ __forceinline__ int erc_window_prefix(int p, int L, int back, int fwd) {
    const int a = min(p, max(0, L - fwd));  // #q<p whose upper end is not clipped
    const int c = max(0, p - back);         // #q<p whose lower end is not clipped
    return a * (a - 1) / 2 + a * fwd + (p - a) * (L - 1) - c * (c - 1) / 2 + p;
}

// Counter-based RNG (splitmix64 finaliser over (seed, offset, index)): one
// uniform in [0,1) per element, reproducible between forward and backward.
__device__ __forceinline__ float erc_uniform(uint64_t seed, uint64_t offset, uint64_t idx) {
    uint64_t z = seed ^ (offset * 0x9E3779B97F4A7C15ull) ^ (idx + 0xD1B54A32D192ED03ull) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (float)(z >> 40) * (1.0f / 16777216.0f);
}
#endif

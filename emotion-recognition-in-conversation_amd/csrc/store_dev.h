// 16-byte OUTPUT stores of the step's kernels, plain or write-through (DESIGN.md finding 65).
//
// A plain store leaves its line dirty in the XCD's L2; what is still dirty when the kernel ends is written back at the kernel
// boundary, in front of the next launch.  A write-through (sc1) store sends the bytes on while the kernel still runs and leaves
// nothing behind -- and drops the line from that L2, so it is for outputs that NO workgroup of the same launch reads again.
// Only the 16-byte form costs what a plain store does (narrower write-through stores are one fabric write each: 2.7 x per
// byte at 8 bytes, ~6 x at 4, ~12.5 x at 2), so there are no narrow forms here: a store under 16 bytes stays plain, always.
//
// The mode is per process (erc_set_store_mode, ERC_STEP_STORES) and reaches a kernel as a uniform field of its parameter
// struct, fixed when the launch is enqueued: a captured step keeps the mode it was captured with.
#pragma once
#include "erc_common.h"

// host side: the process-wide mode (1 = write-through, the default; 0 = plain), defined in launch_chain.hip
int erc_store_mode(void);

#ifdef __HIPCC__
template <bool WT>
__device__ __forceinline__ void st_out16(void* p, const f32x4 v) {
    if constexpr (WT) {
        // (s_nop: a store of more than 64 bits needs wait states before its data registers may be overwritten, and the compiler's
        //  hazard recognizer does not look inside an asm statement -- without them a v_cndmask scheduled right behind the store
        //  replaced the last dword of lanes 12-15 of every 16: finding 44)
        asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
    } else {
        *(__attribute__((address_space(1))) f32x4*)p = v;
    }
}
// `wt` must be uniform over the wavefront (a field of the kernel's parameter struct): ONE scalar branch per store site
__device__ __forceinline__ void st_out16(void* p, const f32x4 v, const int wt) {
    if (wt) st_out16<true>(p, v);
    else st_out16<false>(p, v);
}
#endif

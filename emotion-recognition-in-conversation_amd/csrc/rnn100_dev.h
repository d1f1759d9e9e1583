// Device helpers shared by the hidden-100 weight-stationary scans (lstm.hip, gru100.hip): the row maps and step counts of a
// (dialogue, direction) workgroup, the chunked LDS layout of the vectors every thread reads, the fast activations and the
// dropout uniform of an element.  The DPP moves and reductions of the quad / 16-lane-row thread layout are erc_common.h's.
// A scan file supplies its parameter struct (the fields named below), its cell math, its chunk load / store lambdas and its
// entry points.
#pragma once
#include "erc_common.h"

#ifdef __HIPCC__
namespace rnn100 {

constexpr int H = 100;
constexpr int NTH = 512;
// Global memory is touched once per SC steps, not per step: the wavefront's memory counter (vmcnt) retires loads and
// stores in issue order, so a step that stores its results and then needs a prefetched operand waits for its own stores --
// one L2 round trip (~0.9 us) per step whatever the prefetch distance.  A chunk's operands are requested one chunk ahead
// and its results are kept in registers until the chunk ends; inside a chunk a step is LDS + ALU only.
constexpr int SC = 8;
// Vectors that every thread reads (h_{t-1}: 100 values, the gate gradients: 400 / 300) sit in LDS as chunks of 25 values
// padded to 28 (16-byte rows, chunks 28 banks apart: the distinct addresses of one wavefront read never share a bank).
constexpr int CHK = 25, CHP = 28;
constexpr int HP = 4 * CHP;        // hidden state
__device__ __forceinline__ int chunk_pos(int k) { return (k / CHK) * CHP + k % CHK; }

// rows of a dialogue: row(t) = base + t * step
struct RowMap {
    int64_t base, step;
    __device__ __forceinline__ int64_t operator()(int t) const { return base + (int64_t)t * step; }
};
// P: node_off (null: row(b,t) = b*sb + t*st; else compact rows node_off[b] + t), sb, st
template <class P>
__device__ __forceinline__ RowMap rows_of(const P& p, int b) {
    return p.node_off ? RowMap{(int64_t)p.node_off[b], 1} : RowMap{(int64_t)b * p.sb, p.st};
}
// P: lengths ([B] or null), node_off, T.  lengths is a device input no host check sees: on padded rows a dialogue owns T
// rows, and a longer length would make the scan read and write the rows of the next dialogue.  It may still be negative:
// every loop over the padded positions of a dialogue starts at max(L, 0).
template <class P>
__device__ __forceinline__ int length_of(const P& p, int b) {
    if (p.node_off) return p.lengths ? (int)p.lengths[b] : p.node_off[b + 1] - p.node_off[b];
    return p.lengths ? min((int)p.lengths[b], p.T) : p.T;      // padded rows: never past the T rows of the dialogue
}
// T capacity (TDEV): the launch is sized for T = T_cap, the batch's own longest dialogue is read from the device.  Everything
// in a scan depends on the step count through L alone, so a (dialogue, direction) computes exactly what a launch with
// T = *t_dev computes, in the same order, and the rows t >= *t_dev fall to the padded-position tails (zero outputs / gate
// gradients).
template <bool TDEV, class P>
__device__ __forceinline__ int steps_of(const P& p, int b) {
    return TDEV ? min(max(*p.t_dev, 0), p.T) : length_of(p, b);
}

// sigmoid / tanh on the hardware exponential and reciprocal (v_exp_f32, v_rcp_f32: 1 ulp each; absolute error < 3e-7):
// 4 and 6 instructions -- the library expf + IEEE division + tanhf were 90 of the 230 instructions of a step, and the
// step is bound by instruction issue (two wavefronts per SIMD, finding 26)
__device__ __forceinline__ float fast_sigm(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504f * x));
}
__device__ __forceinline__ float fast_tanh(float x) { return 2.0f * fast_sigm(2.0f * x) - 1.0f; }

// Inverted dropout of the layer's output rows [., 2H]: the uniform of element (row, d * H + u), the same forward and backward.
// An element is kept, and scaled by 1 / (1 - p), when it is >= p; that select stays in the kernels (inside a helper the
// compiler forms it before inlining and the instruction streams of all four scans change).
__device__ __forceinline__ float drop_uniform(uint64_t seed, uint64_t off, int64_t row, int d, int u) {
    return erc_uniform(seed, off, (uint64_t)row * 2 * H + d * H + u);
}

}  // namespace rnn100
#endif

// Device pieces shared by DialogueGCN's tail in training (dgcn_tail.hip) and in eval mode (dgcn_tail_eval.hip): the geometry
// of a workgroup's row tile and its LDS pitches, and the v_mfma_f32_16x16x4_f32 tile product with its operand loads.
#pragma once
#include "erc_common.h"

#ifdef __HIPCC__
constexpr int TG = 200, TH = 100, TX = 300;     // features, hidden width, classifier input
constexpr int TR = 16;                          // rows of a workgroup
constexpr int THL = 10;                         // window the kernels are built for (wp, wf <= 10: erc_dgcn_tail_max_window())
constexpr int TW = TR + 2 * THL;                // 36 window rows
constexpr int PX = 308;                         // LDS pitch of the [features | graph_out] tile (K = 304 used)
constexpr int PH = 116;                         // LDS pitch of the 100-wide tiles (K = 112 used)
constexpr int TMAXC = 8;
constexpr int TNT = 7;                          // 16-column tiles over 100
constexpr int TNW = 8;                          // wavefronts of a workgroup
constexpr int TNTH = 64 * TNW;

__device__ __forceinline__ f32x4 mfma4(const float4& a, const float4& b, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    return acc;
}

// B operand of one group for a weight stored [n][k] (nn.Linear layout, the product x W^T): 16 bytes of row n
__device__ __forceinline__ float4 wrow4(const float* __restrict__ W, int ldw, int n, bool nv, int k0, int K) {
    // (rows are 16-byte aligned: ldw % 4 == 0; K % 4 == 0, so a quad is inside the row or outside)
    const bool v = nv && k0 < K;
    const float4 w = *reinterpret_cast<const float4*>(W + (int64_t)n * ldw + (v ? k0 : 0));
    const float m = v ? 1.f : 0.f;
    return make_float4(w.x * m, w.y * m, w.z * m, w.w * m);
}

// one 16 x 16 output tile over NG groups of 16 k: A rows from LDS (pitch pa, K padded with zeros), B fragments from registers
template <int NG>
__device__ __forceinline__ f32x4 tile_product(const float* sA, int pa, int l15, int kq, const float4 (&b)[NG], f32x4 acc) {
#pragma unroll
    for (int S = 0; S < NG; ++S) {
        const float4 a = *reinterpret_cast<const float4*>(sA + l15 * pa + 16 * S + 4 * kq);
        acc = mfma4(a, b[S], acc);
    }
    return acc;
}
#endif

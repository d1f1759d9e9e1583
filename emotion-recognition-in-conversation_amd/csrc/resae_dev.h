// Device and host pieces shared by csrc/resae.hip (training: erc_resae_fwd / _bwd) and csrc/resae_eval.hip (inference:
// erc_resae_latents): the sizes, the job table, the forward layer, the forward kernel in its two modes and the job check.
// Each translation unit instantiates ONE mode of resae_fwd_kernel: with both in one module the compiler schedules the training
// form differently; apart, its instruction stream is the one it had before the inference mode existed.
#pragma once
#include "erc_common.h"

namespace {

constexpr int D = 384, L1 = 256, L2 = 128, L3 = 64;
constexpr int R = 16, NTH = 512, NW = NTH / 64, MAX_JOBS = 2, MAX_BLOCKS = 5;
constexpr int PX = D + 4, P1 = L1 + 4, P2 = L2 + 4, P3 = L3 + 4;
constexpr int BLK = D + L1 + L2 + L3 + L2 + L1;      // 1216 floats per row and block, in both scratch layouts
// act: inputs of the block's layers.  dY: gradients wrt the pre-activation outputs of the block's layers.
constexpr int A_XIN = 0, A_H1 = D, A_H2 = A_H1 + L1, A_LAT = A_H2 + L2, A_G1 = A_LAT + L3, A_G2 = A_G1 + L2;
constexpr int Y_E0 = 0, Y_E1 = L1, Y_E2 = Y_E1 + L2, Y_D0 = Y_E2 + L3, Y_D1 = Y_D0 + L2, Y_D2 = Y_D1 + L1;
constexpr float SLOPE = 0.01f;      // nn.LeakyReLU()'s default negative slope
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_LEAKY = 2 };

struct Jobs {
    ErcResaeJob j[MAX_JOBS];
};

__device__ __forceinline__ f32x4 mma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// dst[m][n] (= or +=) act(sum_k src[m][k] W[n][k] + bias[n]) for the group's 16 rows; `save` [B, N] and `out` [B, ldo] receive
// the value that dst receives (either may be null, and dst may be null).  The caller puts a barrier behind the call.
template <int N, int K, int ACT, bool ACCUM>
__device__ __forceinline__ void fwd_layer(const float* __restrict__ W, const float* __restrict__ bias, const float* src, const int ps,
                                          float* dst, const int pd, float* __restrict__ save, float* __restrict__ out, const int ldo,
                                          const int row0, const int B) {
    constexpr int NT = N / 16, TPW = (NT + NW - 1) / NW;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    if (wave >= NT) return;      // uniform per wavefront (N = 64: four tiles)
    // eight accumulation chains per tile (chunk parity x element of the 16-byte reads), added in a tree at the end: a single
    // chain over K = 384 is 96 dependent instructions, and its rounding error grows like the square root of its length
    f32x4 acc[TPW][2][4];
    const float* wp[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[t][s][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        wp[t] = W + (int64_t)((wave + t * NW) * 16 + c) * K + 4 * g;      // NT is a multiple of NW wherever TPW > 1
    }
    const float* ap = src + c * ps + 4 * g;
    static_assert(K % 32 == 0, "two chunks of 16 per trip");
#pragma unroll 2
    for (int k = 0; k < K; k += 32) {
        f4 a[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) a[s] = *(const f4*)(ap + k + 16 * s);
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const f4 w = *(const f4*)(wp[t] + k + 16 * s);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[t][s][j] = mma(a[s][j], w[j], acc[t][s][j]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int n = (wave + t * NW) * 16 + c;
        const float bn = bias[n];
        const f32x4 sum = ((acc[t][0][0] + acc[t][0][1]) + (acc[t][0][2] + acc[t][0][3])) +
                          ((acc[t][1][0] + acc[t][1][1]) + (acc[t][1][2] + acc[t][1][3]));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 4 * g + r;
            float v = sum[r] + bn;
            if (ACT == ACT_RELU) v = v > 0.f ? v : 0.f;
            if (ACT == ACT_LEAKY) v = v > 0.f ? v : SLOPE * v;
            if (dst) {
                if (ACCUM) v += dst[m * pd + n];
                dst[m * pd + n] = v;
            }
            const int64_t row = row0 + m;
            if (row < B) {
                if (save) save[row * N + n] = v;
                if (out) out[row * ldo + n] = v;
            }
        }
    }
}

// LATENTS (erc_resae_latents): the inference form.  The same layers in the same order on the same LDS rows, so every latent
// carries the bits of the training form's; nothing is saved (no act row is written), the last block's decoder and the transition
// are not run, and recon / act are never dereferenced.
template <bool LATENTS>
__global__ __launch_bounds__(NTH) void resae_fwd_kernel(const Jobs P, const int nb) {
    const ErcResaeJob& p = P.j[blockIdx.y];
    const int B = p.B, row0 = blockIdx.x * R, tid = threadIdx.x;
    if (row0 >= B) return;      // uniform: the grid is sized for the larger job
    __shared__ __attribute__((aligned(16))) float sX[R * PX];
    __shared__ __attribute__((aligned(16))) float sU[R * (P1 + P2)];      // s1 | s2, or one [16][388] buffer (the transition)
    __shared__ __attribute__((aligned(16))) float s3[R * P3];
    float* const s1 = sU;
    float* const s2 = sU + R * P1;
    static_assert(R * PX <= R * (P1 + P2), "the transition's hidden rows fit s1 | s2");
    float* const A = p.act;
    const int64_t Bl = B;
    for (int e = tid; e < R * D; e += NTH) {
        const int m = e / D, k = e % D;
        const int64_t row = row0 + m;
        float v = 0.f;
        if (row < B) {
            v = p.x[row * p.ldx + k];
            if (!LATENTS) A[Bl * A_XIN + row * D + k] = v;      // x_in of block 0 (x_out = 0)
        }
        sX[m * PX + k] = v;
    }
    __syncthreads();
    for (int i = 0; i < nb; ++i) {
        float* const Ab = A + Bl * BLK * i;
        const float* const* Wl = p.W + 6 * i;
        const float* const* bl = p.b + 6 * i;
        fwd_layer<L1, D, ACT_LEAKY, false>(Wl[0], bl[0], sX, PX, s1, P1, LATENTS ? nullptr : Ab + Bl * A_H1, nullptr, 0, row0, B);
        __syncthreads();
        fwd_layer<L2, L1, ACT_LEAKY, false>(Wl[1], bl[1], s1, P1, s2, P2, LATENTS ? nullptr : Ab + Bl * A_H2, nullptr, 0, row0, B);
        __syncthreads();
        fwd_layer<L3, L2, ACT_NONE, false>(Wl[2], bl[2], s2, P2, s3, P3, LATENTS ? nullptr : Ab + Bl * A_LAT, p.latents + L3 * i, p.ldl,
                                           row0, B);
        if (LATENTS && i == nb - 1) return;      // the last latent is out: nothing reads this block's decoder (uniform)
        __syncthreads();
        fwd_layer<L2, L3, ACT_RELU, false>(Wl[3], bl[3], s3, P3, s2, P2, LATENTS ? nullptr : Ab + Bl * A_G1, nullptr, 0, row0, B);
        __syncthreads();
        fwd_layer<L1, L2, ACT_RELU, false>(Wl[4], bl[4], s2, P2, s1, P1, LATENTS ? nullptr : Ab + Bl * A_G2, nullptr, 0, row0, B);
        __syncthreads();
        // x_in of the next block (of the transition behind the last one) = x_in + x_out; Ab + BLK rows on is that slot in both cases
        fwd_layer<D, L1, ACT_NONE, true>(Wl[5], bl[5], s1, P1, sX, PX, LATENTS ? nullptr : Ab + Bl * BLK + Bl * A_XIN, nullptr, 0, row0, B);
        __syncthreads();
    }
    if (LATENTS) return;      // (reached with nb < 1 only, which the host refuses)
    float* const At = A + Bl * BLK * nb;      // t_in [B, 384] | t1 [B, 384]
    fwd_layer<D, D, ACT_RELU, false>(p.W[6 * nb], p.b[6 * nb], sX, PX, sU, PX, At + Bl * D, nullptr, 0, row0, B);
    __syncthreads();
    fwd_layer<D, D, ACT_NONE, false>(p.W[6 * nb + 1], p.b[6 * nb + 1], sU, PX, nullptr, 0, nullptr, p.recon, p.ldr, row0, B);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

enum FillMode { FILL_FWD = 0, FILL_BWD = 1, FILL_LATENTS = 2 };

int fill(const char* name, Jobs& P, const ErcResaeJob* jobs, int n_jobs, int nb, FillMode mode, int& max_b) {
    const bool bwd = mode == FILL_BWD;
    ERC_REQUIRE(jobs && n_jobs >= 1 && n_jobs <= MAX_JOBS, "%s: n_jobs=%d outside [1, %d] (or null jobs_host)", name, n_jobs, MAX_JOBS);
    ERC_REQUIRE(nb >= 1 && nb <= MAX_BLOCKS, "%s: n_blocks=%d outside [1, %d]", name, nb, MAX_BLOCKS);
    max_b = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const ErcResaeJob& j = jobs[i];
        ERC_REQUIRE(j.B > 0 && (int64_t)j.B * BLK * (nb + 1) < ((int64_t)1 << 40), "%s: job %d: B=%d", name, i, j.B);
        for (int l = 0; l < 6 * nb + 2; ++l) {
            ERC_REQUIRE(j.W[l] && aligned16(j.W[l]), "%s: job %d: weight %d is null or not 16-byte aligned", name, i, l);
            ERC_REQUIRE(bwd || j.b[l], "%s: job %d: bias %d is null", name, i, l);
        }
        if (mode == FILL_LATENTS) {      // recon, act, dx, dY are never read: any value, NULL included
            ERC_REQUIRE(j.x && j.latents, "%s: job %d: null pointer (x, latents)", name, i);
            ERC_REQUIRE(j.ldx >= D, "%s: job %d: ldx=%d < %d", name, i, j.ldx, D);
            ERC_REQUIRE(j.ldl >= L3 * nb, "%s: job %d: ldl=%d < %d", name, i, j.ldl, L3 * nb);
            P.j[i] = j;
            max_b = j.B > max_b ? j.B : max_b;
            continue;
        }
        ERC_REQUIRE(j.act && aligned16(j.act), "%s: job %d: act is null or not 16-byte aligned", name, i);
        if (bwd) {
            ERC_REQUIRE(j.d_recon && j.dx && j.dY && aligned16(j.dY), "%s: job %d: null pointer (d_recon, dx, dY; dY 16-byte aligned)", name, i);
            ERC_REQUIRE(j.lddr >= D && j.lddx >= D, "%s: job %d: lddr=%d / lddx=%d < %d", name, i, j.lddr, j.lddx, D);
            ERC_REQUIRE(!j.d_latents || j.lddl >= L3 * nb, "%s: job %d: lddl=%d < %d", name, i, j.lddl, L3 * nb);
        } else {
            ERC_REQUIRE(j.x && j.recon && j.latents, "%s: job %d: null pointer (x, recon, latents)", name, i);
            ERC_REQUIRE(j.ldx >= D && j.ldr >= D, "%s: job %d: ldx=%d / ldr=%d < %d", name, i, j.ldx, j.ldr, D);
            ERC_REQUIRE(j.ldl >= L3 * nb, "%s: job %d: ldl=%d < %d", name, i, j.ldl, L3 * nb);
        }
        P.j[i] = j;
        max_b = j.B > max_b ? j.B : max_b;
    }
    for (int i = n_jobs; i < MAX_JOBS; ++i) P.j[i] = ErcResaeJob{};
    return ERC_OK;
}

}  // namespace

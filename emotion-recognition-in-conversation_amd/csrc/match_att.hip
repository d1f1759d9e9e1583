// Matching attention 'general2' (MatchingAttention, dgcnv2_models.py:109-148) per dialogue over its valid rows, for a row
// width F given as an argument and built for 200 (= 2 D_e: bc-LSTM / bc-GRU, DialogueRNN, :473-480) and 300 (the nodal
// attention of the conv-emotion DialogueGCN over E = [x | conv2_out], :693-751).  E [N, F] in node order (row
// node_off[b] + t), with Q = E W^T + b computed by the caller:
//     th_tj = tanh(q_t . e_j),   p_tj = exp(th_tj) / sum_{k < L} exp(th_tk),   a_t = sum_j p_tj e_j
// (|th| <= 1: no max subtraction; the padded exp(0) terms of the reference's softmax cancel in its renormalisation).
// Forward: one workgroup per (dialogue, 16-query tile), keys streamed through LDS in chunks of 16 rows; p and th are
// saved as [B, T, T].  Backward in two launches:
//   query side, per (dialogue, 16-query tile):  dp = dA E^T,  dz = p (dp - rowsum(p dp)) (1 - th^2)  (saved),  dQ = dz E
//   key side, per (dialogue, 16-key tile):      dE_j = sum_t p_tj dA_t + dz_tj Q_t
// Every output element is written by one thread that sums in a fixed order: a step is bit-reproducible.
#include "erc_common.h"

namespace {

constexpr int MAXT = 110;          // longest dialogue: two score columns per lane of a wavefront
constexpr int TILE = 16;           // query / key rows per workgroup, and rows per streamed chunk
constexpr int TPAD = 112;          // score row pitch in LDS (T <= 110)
constexpr int MT = 256;

template <int F>
struct Att {
    static constexpr int F4 = F / 4;
    static constexpr int PER = (TILE * F4 + MT - 1) / MT;

    static __device__ __forceinline__ float dot(const float* a, const float* b) {
        const f4* a4 = reinterpret_cast<const f4*>(a);
        const f4* b4 = reinterpret_cast<const f4*>(b);
        f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 5
        for (int k = 0; k < F4; ++k) acc += a4[k] * b4[k];
        return (acc.x + acc.y) + (acc.z + acc.w);
    }

    static __device__ __forceinline__ void load_tile(float* dst, const float* src, int ld, int base, int r0, int L) {
        for (int e = threadIdx.x; e < TILE * F4; e += MT) {
            const int r = e / F4, k4 = e % F4;
            f4 v = {0.f, 0.f, 0.f, 0.f};
            if (r0 + r < L) v = reinterpret_cast<const f4*>(src + (int64_t)(base + r0 + r) * ld)[k4];
            reinterpret_cast<f4*>(dst + r * F)[k4] = v;
        }
    }

    static __device__ __forceinline__ void tile_times_rows(f4 (&acc)[PER], const float* sW, const float* X, int ldx, int base, int L,
                                                           float* sChunk) {
        for (int c0 = 0; c0 < L; c0 += TILE) {
            __syncthreads();
            load_tile(sChunk, X, ldx, base, c0, L);
            __syncthreads();
            const int nc = min(TILE, L - c0);
#pragma unroll
            for (int r = 0; r < PER; ++r) {
                const int e = threadIdx.x + r * MT;
                if (e >= TILE * F4) break;
                const int qi = e / F4, k4 = e % F4;
                for (int kj = 0; kj < nc; ++kj)
                    acc[r] += sW[qi * TPAD + c0 + kj] * reinterpret_cast<const f4*>(sChunk + kj * F)[k4];
            }
        }
    }

    static __device__ __forceinline__ void tile_dots(float* sS, const float* sA, const float* X, int ldx, int base, int L, int q0,
                                                     float* sChunk, bool do_tanh) {
        for (int c0 = 0; c0 < L; c0 += TILE) {
            __syncthreads();
            load_tile(sChunk, X, ldx, base, c0, L);
            __syncthreads();
            const int qi = threadIdx.x / TILE, kj = threadIdx.x % TILE;
            if (q0 + qi < L && c0 + kj < L) {
                const float s = dot(sA + qi * F, sChunk + kj * F);
                sS[qi * TPAD + c0 + kj] = do_tanh ? tanhf(s) : s;
            }
        }
        __syncthreads();
    }

    static __device__ __forceinline__ void store_tile(const f4 (&acc)[PER], float* out, int ld, int base, int r0, int L) {
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int e = threadIdx.x + r * MT;
            if (e >= TILE * F4) break;
            const int qi = e / F4, k4 = e % F4;
            if (r0 + qi < L) reinterpret_cast<f4*>(out + (int64_t)(base + r0 + qi) * ld)[k4] = acc[r];
        }
    }
};

template <int F>
__global__ __launch_bounds__(MT) void match_fwd_kernel(const float* __restrict__ E, int lde, const float* __restrict__ Q, int ldq,
                                                       const int32_t* __restrict__ node_off, int T, float* __restrict__ A, int lda,
                                                       float* __restrict__ Pg, float* __restrict__ THg) {
    using M = Att<F>;
    __shared__ __attribute__((aligned(16))) float sQ[TILE * F];
    __shared__ __attribute__((aligned(16))) float sC[TILE * F];
    __shared__ float sS[TILE * TPAD];
    const int b = blockIdx.y, q0 = blockIdx.x * TILE;
    const int base = node_off[b], L = min(node_off[b + 1] - base, T);
    if (q0 >= L) return;
    M::load_tile(sQ, Q, ldq, base, q0, L);
    M::tile_dots(sS, sQ, E, lde, base, L, q0, sC, true);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int qi = wave; qi < TILE && q0 + qi < L; qi += MT / 64) {
        float* row = sS + qi * TPAD;
        const int64_t g = ((int64_t)b * T + q0 + qi) * T;
        const float th0 = lane < L ? row[lane] : 0.f, th1 = lane + 64 < L ? row[lane + 64] : 0.f;
        const float x0 = lane < L ? expf(th0) : 0.f, x1 = lane + 64 < L ? expf(th1) : 0.f;
        const float inv = 1.f / wave_sum(x0 + x1);
        if (lane < L) row[lane] = x0 * inv, Pg[g + lane] = x0 * inv, THg[g + lane] = th0;
        if (lane + 64 < L) row[lane + 64] = x1 * inv, Pg[g + lane + 64] = x1 * inv, THg[g + lane + 64] = th1;
    }
    f4 acc[M::PER];
#pragma unroll
    for (int r = 0; r < M::PER; ++r) acc[r] = f4{0.f, 0.f, 0.f, 0.f};
    M::tile_times_rows(acc, sS, E, lde, base, L, sC);
    M::store_tile(acc, A, lda, base, q0, L);
}

// capacity rows [n, n_cap) of a gradient the attention backward owns: written 0 by the whole grid, a row per workgroup and
// round (no row has a dialogue, so no tile writes there; the caller's weight-gradient products run over all n_cap rows)
template <int F>
__device__ __forceinline__ void zero_tail_rows(float* __restrict__ out, int ld, int n, int n_cap) {
    const int nwg = gridDim.x * gridDim.y, wg = blockIdx.y * gridDim.x + blockIdx.x;
    static_assert(F <= MT, "one column per thread: a wider row needs a column loop");
    for (int row = max(n, 0) + wg; row < n_cap; row += nwg)
        if (threadIdx.x < F) out[(int64_t)row * ld + threadIdx.x] = 0.f;
}

template <int F, bool CAP>
__global__ __launch_bounds__(MT) void match_bwd_q_kernel(const float* __restrict__ E, int lde, const float* __restrict__ dA, int ldda,
                                                         const int32_t* __restrict__ node_off, int T, const float* __restrict__ Pg,
                                                         const float* __restrict__ THg, float* __restrict__ DZg,
                                                         float* __restrict__ dQ, int lddq, int B, int n_cap) {
    using M = Att<F>;
    __shared__ __attribute__((aligned(16))) float sG[TILE * F];
    __shared__ __attribute__((aligned(16))) float sC[TILE * F];
    __shared__ float sS[TILE * TPAD];
    const int b = blockIdx.y, q0 = blockIdx.x * TILE;
    const int base = node_off[b], L = min(node_off[b + 1] - base, T);
    if constexpr (CAP) zero_tail_rows<F>(dQ, lddq, node_off[B], n_cap);
    if (q0 >= L) return;
    M::load_tile(sG, dA, ldda, base, q0, L);
    M::tile_dots(sS, sG, E, lde, base, L, q0, sC, false);          // dp
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int qi = wave; qi < TILE && q0 + qi < L; qi += MT / 64) {
        float* row = sS + qi * TPAD;
        const int64_t g = ((int64_t)b * T + q0 + qi) * T;
        const float p0 = lane < L ? Pg[g + lane] : 0.f, p1 = lane + 64 < L ? Pg[g + lane + 64] : 0.f;
        const float d0 = lane < L ? row[lane] : 0.f, d1 = lane + 64 < L ? row[lane + 64] : 0.f;
        const float rs = wave_sum(p0 * d0 + p1 * d1);
        if (lane < L) {
            const float th = THg[g + lane], z = p0 * (d0 - rs) * (1.f - th * th);
            row[lane] = z, DZg[g + lane] = z;
        }
        if (lane + 64 < L) {
            const float th = THg[g + lane + 64], z = p1 * (d1 - rs) * (1.f - th * th);
            row[lane + 64] = z, DZg[g + lane + 64] = z;
        }
    }
    f4 acc[M::PER];
#pragma unroll
    for (int r = 0; r < M::PER; ++r) acc[r] = f4{0.f, 0.f, 0.f, 0.f};
    M::tile_times_rows(acc, sS, E, lde, base, L, sC);
    M::store_tile(acc, dQ, lddq, base, q0, L);
}

template <int F, bool CAP>
__global__ __launch_bounds__(MT) void match_bwd_k_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ dA, int ldda,
                                                         const int32_t* __restrict__ node_off, int T, const float* __restrict__ Pg,
                                                         const float* __restrict__ DZg, float* __restrict__ dE, int ldde, int B,
                                                         int n_cap) {
    using M = Att<F>;
    __shared__ __attribute__((aligned(16))) float sG[TILE * F];
    __shared__ __attribute__((aligned(16))) float sQ[TILE * F];
    __shared__ float sP[TILE * TILE];
    __shared__ float sZ[TILE * TILE];
    const int b = blockIdx.y, k0 = blockIdx.x * TILE;
    const int base = node_off[b], L = min(node_off[b + 1] - base, T);
    if constexpr (CAP) zero_tail_rows<F>(dE, ldde, node_off[B], n_cap);
    if (k0 >= L) return;
    f4 acc[M::PER];
#pragma unroll
    for (int r = 0; r < M::PER; ++r) acc[r] = f4{0.f, 0.f, 0.f, 0.f};
    for (int i0 = 0; i0 < L; i0 += TILE) {
        __syncthreads();
        M::load_tile(sG, dA, ldda, base, i0, L);
        M::load_tile(sQ, Q, ldq, base, i0, L);
        {
            const int ii = threadIdx.x / TILE, kj = threadIdx.x % TILE;
            const bool ok = i0 + ii < L && k0 + kj < L;
            const int64_t g = ((int64_t)b * T + i0 + ii) * T + k0 + kj;
            sP[ii * TILE + kj] = ok ? Pg[g] : 0.f;
            sZ[ii * TILE + kj] = ok ? DZg[g] : 0.f;
        }
        __syncthreads();
        const int ni = min(TILE, L - i0);
#pragma unroll
        for (int r = 0; r < M::PER; ++r) {
            const int e = threadIdx.x + r * MT;
            if (e >= TILE * M::F4) break;
            const int kj = e / M::F4, k4 = e % M::F4;
            for (int ii = 0; ii < ni; ++ii)
                acc[r] += sP[ii * TILE + kj] * reinterpret_cast<const f4*>(sG + ii * F)[k4] +
                          sZ[ii * TILE + kj] * reinterpret_cast<const f4*>(sQ + ii * F)[k4];
        }
    }
    M::store_tile(acc, dE, ldde, base, k0, L);
}

bool aligned16(const void* p, int ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; }

template <int F>
void launch_fwd(dim3 grid, hipStream_t stream, const float* E, int lde, const float* Q, int ldq, const int32_t* node_off, int T,
                float* A, int lda, float* P, float* TH) {
    hipLaunchKernelGGL(match_fwd_kernel<F>, grid, dim3(MT), 0, stream, E, lde, Q, ldq, node_off, T, A, lda, P, TH);
}

template <int F, bool CAP>
int launch_bwd(dim3 grid, hipStream_t stream, const float* E, int lde, const float* Q, int ldq, const float* dA, int ldda,
               const int32_t* node_off, int B, int T, const float* P, const float* TH, float* DZ, float* dQ, int lddq, float* dE,
               int ldde, int n_cap) {
    hipLaunchKernelGGL((match_bwd_q_kernel<F, CAP>), grid, dim3(MT), 0, stream, E, lde, dA, ldda, node_off, T, P, TH, DZ, dQ, lddq, B,
                       n_cap);
    ERC_LAUNCH_CHECK("match_att_bwd_q");
    hipLaunchKernelGGL((match_bwd_k_kernel<F, CAP>), grid, dim3(MT), 0, stream, Q, ldq, dA, ldda, node_off, T, P, DZ, dE, ldde, B,
                       n_cap);
    ERC_LAUNCH_CHECK("match_att_bwd_k");
    return ERC_OK;
}

}  // namespace

extern "C" int erc_match_att_fwd(const float* E, int lde, const float* Q, int ldq, const int32_t* node_off, int B, int T, int F,
                                 float* A, int lda, float* P, float* TH, void* stream) {
    ERC_REQUIRE(E && Q && node_off && A && P && TH, "match_att_fwd: null pointer");
    ERC_REQUIRE(F == 200 || F == 300, "match_att_fwd: built for row widths 200 and 300, got %d", F);
    ERC_REQUIRE(B > 0 && T > 0 && T <= MAXT, "match_att_fwd: bad sizes B=%d T=%d (T <= %d)", B, T, MAXT);
    ERC_REQUIRE(aligned16(E, lde) && aligned16(Q, ldq) && aligned16(A, lda), "match_att_fwd: rows must be 16-byte aligned");
    ERC_REQUIRE(lde >= F && ldq >= F && lda >= F, "match_att_fwd: row pitches below %d", F);
    const dim3 grid(erc_cdiv(T, TILE), B);
    (F == 200 ? launch_fwd<200> : launch_fwd<300>)(grid, (hipStream_t)stream, E, lde, Q, ldq, node_off, T, A, lda, P, TH);
    ERC_LAUNCH_CHECK("match_att_fwd");
    return ERC_OK;
}

extern "C" int erc_match_att_bwd_cap(const float* E, int lde, const float* Q, int ldq, const float* dA, int ldda,
                                     const int32_t* node_off, int B, int T, int F, const float* P, const float* TH, float* DZ,
                                     float* dQ, int lddq, float* dE, int ldde, int n_cap, void* stream) {
    ERC_REQUIRE(E && Q && dA && node_off && P && TH && DZ && dQ && dE, "match_att_bwd: null pointer");
    ERC_REQUIRE(F == 200 || F == 300, "match_att_bwd: built for row widths 200 and 300, got %d", F);
    ERC_REQUIRE(n_cap <= 0 || F == 200, "match_att_bwd: capacity mode (n_cap=%d) is built for row width 200 alone, got %d", n_cap, F);
    ERC_REQUIRE(B > 0 && T > 0 && T <= MAXT, "match_att_bwd: bad sizes B=%d T=%d (T <= %d)", B, T, MAXT);
    ERC_REQUIRE(aligned16(E, lde) && aligned16(Q, ldq) && aligned16(dA, ldda) && aligned16(dQ, lddq) && aligned16(dE, ldde),
                "match_att_bwd: rows must be 16-byte aligned");
    ERC_REQUIRE(lde >= F && ldq >= F && ldda >= F && lddq >= F && ldde >= F, "match_att_bwd: row pitches below %d", F);
    // dQ == Q included: the key-side launch reads Q after the query-side launch has written dQ
    ERC_REQUIRE(dE != E && dE != Q && dE != dA && dQ != E && dQ != Q && dQ != dA && dQ != dE,
                "match_att_bwd: outputs must not alias inputs or each other");
    const auto launch = n_cap > 0 ? launch_bwd<200, true> : F == 200 ? launch_bwd<200, false> : launch_bwd<300, false>;
    return launch(dim3(erc_cdiv(T, TILE), B), (hipStream_t)stream, E, lde, Q, ldq, dA, ldda, node_off, B, T, P, TH, DZ, dQ, lddq, dE,
                  ldde, n_cap);
}

extern "C" int erc_match_att_bwd(const float* E, int lde, const float* Q, int ldq, const float* dA, int ldda, const int32_t* node_off,
                                 int B, int T, int F, const float* P, const float* TH, float* DZ, float* dQ, int lddq, float* dE,
                                 int ldde, void* stream) {
    return erc_match_att_bwd_cap(E, lde, Q, ldq, dA, ldda, node_off, B, T, F, P, TH, DZ, dQ, lddq, dE, ldde, 0, stream);
}

// The two attentions of the conv-emotion DialogueGCN (track_mm/dgcnv2.py, track_mm/dgcnv2_models.py) and its batch tables.
//
// Positional edge attention ('attn1', dgcnv2_models.py:533-566).  S = M Wscalar^T is computed by the caller over the B*T
// padded, time-major rows of the sequence encoder's output (row t*B + b, 110 columns).  Row j of Wscalar scores every
// position of the dialogue for source j; after the softmax over time, the mask (1 inside j's window, 1e-10 outside it,
// padded positions included) and the renormalisation, the weight of edge j -> i is
//     norm = u_i / (sum_{t in win(j)} u_t + 1e-10 sum_{t < T, t not in win(j)} u_t),   u_t = exp(S[t, j] - max_t S[t, j])
// (the softmax's own denominator cancels).  One wave per (dialogue, source position), lane t holding positions t and
// t + 64 (T <= 110).  The backward writes dS [B*T, 110]: column p of dialogue b's rows belongs to source p alone, so every
// element has one writer and no atomics are needed; columns p >= L_b are written as zeros.
//
// Nodal attention (MatchingAttention 'general2', dgcnv2_models.py:109-148,693-751) per dialogue over E = [x | conv2_out]
// [N, 300] in node order (row node_off[b] + t), with Q = E W^T + b computed by the caller:
//     th_tj = tanh(q_t . e_j),   p_tj = exp(th_tj) / sum_{k < L} exp(th_tk),   a_t = sum_j p_tj e_j
// (|th| <= 1: no max subtraction; the padded exp(0) terms of the reference's softmax cancel in its renormalisation).
// Forward: one workgroup per (dialogue, 16-query tile), keys streamed through LDS in chunks of 16 rows; p and th are
// saved as [B, T, T].  Backward in two launches:
//   query side, per (dialogue, 16-query tile):  dp = dA E^T,  dz = p (dp - rowsum(p dp)) (1 - th^2)  (saved),  dQ = dz E
//   key side, per (dialogue, 16-key tile):      dE_j = sum_t p_tj dA_t + dz_tj Q_t
// Every output element is written by one thread that sums in a fixed order: a step is bit-reproducible.
#include "erc_common.h"

namespace {

constexpr int F = 300;             // E / Q / A row width
constexpr int F4 = F / 4;
constexpr int NSCAL = 110;         // rows of Wscalar: the reference's max_seq_len
constexpr int TILE = 16;           // query / key rows per workgroup, and rows per streamed chunk
constexpr int TPAD = 112;          // score row pitch in LDS (T <= 110)
constexpr int NT = 256;
constexpr int PER = (TILE * F4 + NT - 1) / NT;     // f4 outputs per thread of a [16, 300] tile

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float dot300(const float* a, const float* b) {
    const f4* a4 = reinterpret_cast<const f4*>(a);
    const f4* b4 = reinterpret_cast<const f4*>(b);
    f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 5
    for (int k = 0; k < F4; ++k) acc += a4[k] * b4[k];
    return (acc.x + acc.y) + (acc.z + acc.w);
}

// [16, 300] rows r0 .. r0 + 15 of a compact matrix into LDS; rows >= L are zero
__device__ __forceinline__ void load_tile(float* dst, const float* src, int ld, int base, int r0, int L) {
    for (int e = threadIdx.x; e < TILE * F4; e += NT) {
        const int r = e / F4, k4 = e % F4;
        f4 v = {0.f, 0.f, 0.f, 0.f};
        if (r0 + r < L) v = reinterpret_cast<const f4*>(src + (int64_t)(base + r0 + r) * ld)[k4];
        reinterpret_cast<f4*>(dst + r * F)[k4] = v;
    }
}

// ------------------------------------------------------------------ batch tables
__global__ void meta_kernel(const float* onehot, int S, const int64_t* lengths, int B, int T, int n_cap, int64_t* spk,
                            int32_t* node_row) {
    __shared__ int s_off[1025];
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int b = 0; b < B; ++b) {
            s_off[b] = acc;
            acc += (int)min(max(lengths[b], (int64_t)0), (int64_t)T);
        }
        s_off[B] = acc;
    }
    __syncthreads();
    // speaker = the first index whose one-hot entry equals 1 (dgcnv2_models.py:671-672); padded rows: 0
    for (int r = threadIdx.x; r < T * B; r += blockDim.x) {
        const float* row = onehot + (int64_t)r * S;
        int s = 0;
        for (int k = S - 1; k >= 0; --k)
            if (row[k] == 1.f) s = k;
        spk[r] = s;
    }
    for (int b = 0; b < B; ++b) {
        const int o = s_off[b], L = s_off[b + 1] - o;
        for (int t = threadIdx.x; t < L; t += blockDim.x)
            if (o + t < n_cap) node_row[o + t] = t * B + b;
    }
}

// ------------------------------------------------------------------ positional edge attention
struct WinSoftmax {
    float u0, u1, den;    // u at positions lane, lane + 64; the masked denominator
    int lo, hi;           // window [lo, hi)
};

__device__ __forceinline__ WinSoftmax win_softmax(const float* Sc, int ldS, int B, int T, int b, int p, int L, int wp, int wf,
                                                  int lane) {
    WinSoftmax w;
    const int t0 = lane, t1 = lane + 64;
    const float s0 = t0 < T ? Sc[((int64_t)t0 * B + b) * ldS + p] : -INFINITY;
    const float s1 = t1 < T ? Sc[((int64_t)t1 * B + b) * ldS + p] : -INFINITY;
    const float mx = wave_max(fmaxf(s0, s1));
    w.u0 = t0 < T ? expf(s0 - mx) : 0.f;
    w.u1 = t1 < T ? expf(s1 - mx) : 0.f;
    w.lo = wp < 0 ? 0 : max(0, p - wp);
    w.hi = wf < 0 ? L : min(L, p + wf + 1);
    const bool in0 = t0 >= w.lo && t0 < w.hi, in1 = t1 >= w.lo && t1 < w.hi;
    const float win = wave_sum((in0 ? w.u0 : 0.f) + (in1 ? w.u1 : 0.f));
    const float out = wave_sum((in0 ? 0.f : w.u0) + (in1 ? 0.f : w.u1));
    w.den = win + 1e-10f * out;
    return w;
}

__global__ __launch_bounds__(NT) void edge_att_fwd_kernel(const float* __restrict__ Sc, int ldS, const int32_t* __restrict__ node_off,
                                                          int B, int T, int wp, int wf, const int32_t* __restrict__ out_ptr,
                                                          const int32_t* __restrict__ out_dst,
                                                          const int32_t* __restrict__ out_eid, float* __restrict__ norm) {
    const int lane = threadIdx.x & 63, p = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), b = blockIdx.y;
    const int base = node_off[b], L = node_off[b + 1] - base;
    if (p >= L) return;
    const WinSoftmax w = win_softmax(Sc, ldS, B, T, b, p, L, wp, wf, lane);
    const int j = base + p;
    // lane l writes out-edge l of the pass; u of its target comes from the lane that holds that position
    const int e0 = out_ptr[j], e1 = out_ptr[j + 1];
    for (int eb = e0; eb < e1; eb += 64) {
        const int e = eb + lane;
        const int i = e < e1 ? out_dst[e] - base : 0;
        const float ua = __shfl(w.u0, i & 63, 64), ub = __shfl(w.u1, i & 63, 64);
        if (e < e1) norm[out_eid[e]] = (i < 64 ? ua : ub) / w.den;
    }
}

__global__ __launch_bounds__(NT) void edge_att_bwd_kernel(const float* __restrict__ Sc, int ldS, const int32_t* __restrict__ node_off,
                                                          int B, int T, int wp, int wf, const int32_t* __restrict__ out_ptr,
                                                          const int32_t* __restrict__ out_dst,
                                                          const int32_t* __restrict__ out_eid, const float* __restrict__ dnorm,
                                                          int dn_parts, int64_t dn_stride, float* __restrict__ dS) {
    const int lane = threadIdx.x & 63, p = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), b = blockIdx.y;
    if (p >= NSCAL) return;
    const int base = node_off[b], L = node_off[b + 1] - base;
    const int t0 = lane, t1 = lane + 64;
    if (p >= L) {       // no source at this position: its column of Wscalar receives nothing from dialogue b
        if (t0 < T) dS[((int64_t)t0 * B + b) * ldS + p] = 0.f;
        if (t1 < T) dS[((int64_t)t1 * B + b) * ldS + p] = 0.f;
        return;
    }
    const WinSoftmax w = win_softmax(Sc, ldS, B, T, b, p, L, wp, wf, lane);
    const int j = base + p;
    const int e0 = out_ptr[j], e1 = out_ptr[j + 1];
    // dn at positions t0 / t1 (0 outside the window); sum_i dn_i norm_i
    float dn0 = 0.f, dn1 = 0.f;
    for (int e = e0; e < e1; ++e) {
        const int i = out_dst[e] - base, id = out_eid[e];
        float g = 0.f;
        for (int q = 0; q < dn_parts; ++q) g += dnorm[q * dn_stride + id];
        if (i == t0) dn0 = g;
        if (i == t1) dn1 = g;
    }
    const float n0 = w.u0 / w.den, n1 = w.u1 / w.den;
    const bool in0 = t0 >= w.lo && t0 < w.hi, in1 = t1 >= w.lo && t1 < w.hi;
    const float dot = wave_sum((in0 ? dn0 * n0 : 0.f) + (in1 ? dn1 * n1 : 0.f));
    if (t0 < T) dS[((int64_t)t0 * B + b) * ldS + p] = in0 ? n0 * (dn0 - dot) : -1e-10f * n0 * dot;
    if (t1 < T) dS[((int64_t)t1 * B + b) * ldS + p] = in1 ? n1 * (dn1 - dot) : -1e-10f * n1 * dot;
}

// ------------------------------------------------------------------ nodal attention
// out[16, 300] tile (rows r0..) += W[16, L] (LDS, pitch TPAD) times the dialogue's rows of X, streamed in chunks of 16
__device__ __forceinline__ void tile_times_rows(f4 (&acc)[PER], const float* sW, const float* X, int ldx, int base, int L,
                                                float* sChunk) {
    for (int c0 = 0; c0 < L; c0 += TILE) {
        __syncthreads();
        load_tile(sChunk, X, ldx, base, c0, L);
        __syncthreads();
        const int nc = min(TILE, L - c0);
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int e = threadIdx.x + r * NT;
            if (e >= TILE * F4) break;
            const int qi = e / F4, k4 = e % F4;
            for (int kj = 0; kj < nc; ++kj)
                acc[r] += sW[qi * TPAD + c0 + kj] * reinterpret_cast<const f4*>(sChunk + kj * F)[k4];
        }
    }
}

// sS[16, L] = rows of sA (16 x 300) dotted with the dialogue's rows of X
__device__ __forceinline__ void tile_dots(float* sS, const float* sA, const float* X, int ldx, int base, int L, int q0,
                                          float* sChunk, bool do_tanh) {
    for (int c0 = 0; c0 < L; c0 += TILE) {
        __syncthreads();
        load_tile(sChunk, X, ldx, base, c0, L);
        __syncthreads();
        const int qi = threadIdx.x / TILE, kj = threadIdx.x % TILE;
        if (q0 + qi < L && c0 + kj < L) {
            const float s = dot300(sA + qi * F, sChunk + kj * F);
            sS[qi * TPAD + c0 + kj] = do_tanh ? tanhf(s) : s;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(NT) void nodal_fwd_kernel(const float* __restrict__ E, int lde, const float* __restrict__ Q, int ldq,
                                                       const int32_t* __restrict__ node_off, int T, float* __restrict__ A, int lda,
                                                       float* __restrict__ Pg, float* __restrict__ THg) {
    __shared__ __attribute__((aligned(16))) float sQ[TILE * F];
    __shared__ __attribute__((aligned(16))) float sC[TILE * F];
    __shared__ float sS[TILE * TPAD];
    const int b = blockIdx.y, q0 = blockIdx.x * TILE;
    const int base = node_off[b], L = node_off[b + 1] - base;
    if (q0 >= L) return;
    load_tile(sQ, Q, ldq, base, q0, L);
    tile_dots(sS, sQ, E, lde, base, L, q0, sC, true);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int qi = wave; qi < TILE && q0 + qi < L; qi += NT / 64) {
        float* row = sS + qi * TPAD;
        const int64_t g = ((int64_t)b * T + q0 + qi) * T;
        const float th0 = lane < L ? row[lane] : 0.f, th1 = lane + 64 < L ? row[lane + 64] : 0.f;
        const float x0 = lane < L ? expf(th0) : 0.f, x1 = lane + 64 < L ? expf(th1) : 0.f;
        const float inv = 1.f / wave_sum(x0 + x1);
        if (lane < L) row[lane] = x0 * inv, Pg[g + lane] = x0 * inv, THg[g + lane] = th0;
        if (lane + 64 < L) row[lane + 64] = x1 * inv, Pg[g + lane + 64] = x1 * inv, THg[g + lane + 64] = th1;
    }
    f4 acc[PER];
#pragma unroll
    for (int r = 0; r < PER; ++r) acc[r] = f4{0.f, 0.f, 0.f, 0.f};
    tile_times_rows(acc, sS, E, lde, base, L, sC);
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int e = threadIdx.x + r * NT;
        if (e >= TILE * F4) break;
        const int qi = e / F4, k4 = e % F4;
        if (q0 + qi < L) reinterpret_cast<f4*>(A + (int64_t)(base + q0 + qi) * lda)[k4] = acc[r];
    }
}

__global__ __launch_bounds__(NT) void nodal_bwd_q_kernel(const float* __restrict__ E, int lde, const float* __restrict__ dA, int ldda,
                                                         const int32_t* __restrict__ node_off, int T, const float* __restrict__ Pg,
                                                         const float* __restrict__ THg, float* __restrict__ DZg,
                                                         float* __restrict__ dQ, int lddq) {
    __shared__ __attribute__((aligned(16))) float sG[TILE * F];
    __shared__ __attribute__((aligned(16))) float sC[TILE * F];
    __shared__ float sS[TILE * TPAD];
    const int b = blockIdx.y, q0 = blockIdx.x * TILE;
    const int base = node_off[b], L = node_off[b + 1] - base;
    if (q0 >= L) return;
    load_tile(sG, dA, ldda, base, q0, L);
    tile_dots(sS, sG, E, lde, base, L, q0, sC, false);          // dp
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int qi = wave; qi < TILE && q0 + qi < L; qi += NT / 64) {
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
    f4 acc[PER];
#pragma unroll
    for (int r = 0; r < PER; ++r) acc[r] = f4{0.f, 0.f, 0.f, 0.f};
    tile_times_rows(acc, sS, E, lde, base, L, sC);
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int e = threadIdx.x + r * NT;
        if (e >= TILE * F4) break;
        const int qi = e / F4, k4 = e % F4;
        if (q0 + qi < L) reinterpret_cast<f4*>(dQ + (int64_t)(base + q0 + qi) * lddq)[k4] = acc[r];
    }
}

__global__ __launch_bounds__(NT) void nodal_bwd_k_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ dA, int ldda,
                                                         const int32_t* __restrict__ node_off, int T, const float* __restrict__ Pg,
                                                         const float* __restrict__ DZg, float* __restrict__ dE, int ldde) {
    __shared__ __attribute__((aligned(16))) float sG[TILE * F];
    __shared__ __attribute__((aligned(16))) float sQ[TILE * F];
    __shared__ float sP[TILE * TILE];
    __shared__ float sZ[TILE * TILE];
    const int b = blockIdx.y, k0 = blockIdx.x * TILE;
    const int base = node_off[b], L = node_off[b + 1] - base;
    if (k0 >= L) return;
    f4 acc[PER];
#pragma unroll
    for (int r = 0; r < PER; ++r) acc[r] = f4{0.f, 0.f, 0.f, 0.f};
    for (int i0 = 0; i0 < L; i0 += TILE) {
        __syncthreads();
        load_tile(sG, dA, ldda, base, i0, L);
        load_tile(sQ, Q, ldq, base, i0, L);
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
        for (int r = 0; r < PER; ++r) {
            const int e = threadIdx.x + r * NT;
            if (e >= TILE * F4) break;
            const int kj = e / F4, k4 = e % F4;
            for (int ii = 0; ii < ni; ++ii)
                acc[r] += sP[ii * TILE + kj] * reinterpret_cast<const f4*>(sG + ii * F)[k4] +
                          sZ[ii * TILE + kj] * reinterpret_cast<const f4*>(sQ + ii * F)[k4];
        }
    }
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int e = threadIdx.x + r * NT;
        if (e >= TILE * F4) break;
        const int kj = e / F4, k4 = e % F4;
        if (k0 + kj < L) reinterpret_cast<f4*>(dE + (int64_t)(base + k0 + kj) * ldde)[k4] = acc[r];
    }
}

bool aligned16(const void* p, int ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; }

}  // namespace

extern "C" int erc_dgcnv2_max_t(void) { return NSCAL; }

extern "C" int erc_dgcnv2_meta(const float* onehot, int S, const int64_t* lengths, int B, int T, int n_cap, int64_t* spk,
                               int32_t* node_row, void* stream) {
    ERC_REQUIRE(onehot && lengths && spk && node_row, "dgcnv2_meta: null pointer");
    ERC_REQUIRE(B > 0 && B <= 1024 && T > 0 && S > 0 && n_cap > 0, "dgcnv2_meta: bad sizes B=%d T=%d S=%d n_cap=%d", B, T, S,
                n_cap);
    hipLaunchKernelGGL(meta_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, onehot, S, lengths, B, T, n_cap, spk, node_row);
    ERC_LAUNCH_CHECK("dgcnv2_meta");
    return ERC_OK;
}

extern "C" int erc_dgcnv2_edge_att_fwd(const float* S, int ldS, const int32_t* node_off, int B, int T, int wp, int wf,
                                       const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid, float* norm,
                                       void* stream) {
    ERC_REQUIRE(S && node_off && out_ptr && out_dst && out_eid && norm, "dgcnv2_edge_att_fwd: null pointer");
    ERC_REQUIRE(B > 0 && T > 0 && ldS >= NSCAL, "dgcnv2_edge_att_fwd: bad sizes B=%d T=%d ldS=%d", B, T, ldS);
    ERC_REQUIRE(T <= NSCAL, "dgcnv2_edge_att_fwd: Wscalar has %d rows, dialogues of up to %d utterances (batch T=%d)", NSCAL, NSCAL,
                T);
    hipLaunchKernelGGL(edge_att_fwd_kernel, dim3(erc_cdiv(T, NT / 64), B), dim3(NT), 0, (hipStream_t)stream, S, ldS, node_off, B, T,
                       wp, wf, out_ptr, out_dst, out_eid, norm);
    ERC_LAUNCH_CHECK("dgcnv2_edge_att_fwd");
    return ERC_OK;
}

extern "C" int erc_dgcnv2_edge_att_bwd(const float* S, int ldS, const int32_t* node_off, int B, int T, int wp, int wf,
                                       const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid, const float* dnorm,
                                       int dn_parts, int64_t dn_stride, float* dS, void* stream) {
    ERC_REQUIRE(S && node_off && out_ptr && out_dst && out_eid && dnorm && dS, "dgcnv2_edge_att_bwd: null pointer");
    ERC_REQUIRE(B > 0 && T > 0 && ldS >= NSCAL, "dgcnv2_edge_att_bwd: bad sizes B=%d T=%d ldS=%d", B, T, ldS);
    ERC_REQUIRE(T <= NSCAL, "dgcnv2_edge_att_bwd: dialogues of up to %d utterances (batch T=%d)", NSCAL, T);
    ERC_REQUIRE(dn_parts >= 1 && (dn_parts == 1 || dn_stride > 0), "dgcnv2_edge_att_bwd: dn_parts=%d", dn_parts);
    ERC_REQUIRE(S != dS, "dgcnv2_edge_att_bwd: dS must not alias S");
    hipLaunchKernelGGL(edge_att_bwd_kernel, dim3(erc_cdiv(NSCAL, NT / 64), B), dim3(NT), 0, (hipStream_t)stream, S, ldS, node_off, B,
                       T, wp, wf, out_ptr, out_dst, out_eid, dnorm, dn_parts, dn_stride, dS);
    ERC_LAUNCH_CHECK("dgcnv2_edge_att_bwd");
    return ERC_OK;
}

extern "C" int erc_dgcnv2_nodal_fwd(const float* E, int lde, const float* Q, int ldq, const int32_t* node_off, int B, int T,
                                    float* A, int lda, float* P, float* TH, void* stream) {
    ERC_REQUIRE(E && Q && node_off && A && P && TH, "dgcnv2_nodal_fwd: null pointer");
    ERC_REQUIRE(B > 0 && T > 0 && T <= NSCAL, "dgcnv2_nodal_fwd: bad sizes B=%d T=%d (T <= %d)", B, T, NSCAL);
    ERC_REQUIRE(aligned16(E, lde) && aligned16(Q, ldq) && aligned16(A, lda), "dgcnv2_nodal_fwd: rows must be 16-byte aligned");
    ERC_REQUIRE(lde >= F && ldq >= F && lda >= F, "dgcnv2_nodal_fwd: row pitches below %d", F);
    hipLaunchKernelGGL(nodal_fwd_kernel, dim3(erc_cdiv(T, TILE), B), dim3(NT), 0, (hipStream_t)stream, E, lde, Q, ldq, node_off, T, A,
                       lda, P, TH);
    ERC_LAUNCH_CHECK("dgcnv2_nodal_fwd");
    return ERC_OK;
}

extern "C" int erc_dgcnv2_nodal_bwd(const float* E, int lde, const float* Q, int ldq, const float* dA, int ldda,
                                    const int32_t* node_off, int B, int T, const float* P, const float* TH, float* DZ, float* dQ,
                                    int lddq, float* dE, int ldde, void* stream) {
    ERC_REQUIRE(E && Q && dA && node_off && P && TH && DZ && dQ && dE, "dgcnv2_nodal_bwd: null pointer");
    ERC_REQUIRE(B > 0 && T > 0 && T <= NSCAL, "dgcnv2_nodal_bwd: bad sizes B=%d T=%d (T <= %d)", B, T, NSCAL);
    ERC_REQUIRE(aligned16(E, lde) && aligned16(Q, ldq) && aligned16(dA, ldda) && aligned16(dQ, lddq) && aligned16(dE, ldde),
                "dgcnv2_nodal_bwd: rows must be 16-byte aligned");
    ERC_REQUIRE(lde >= F && ldq >= F && ldda >= F && lddq >= F && ldde >= F, "dgcnv2_nodal_bwd: row pitches below %d", F);
    ERC_REQUIRE(dE != E && dE != Q && dE != dA && dQ != E && dQ != dA, "dgcnv2_nodal_bwd: outputs must not alias inputs");
    const dim3 grid(erc_cdiv(T, TILE), B);
    hipLaunchKernelGGL(nodal_bwd_q_kernel, grid, dim3(NT), 0, (hipStream_t)stream, E, lde, dA, ldda, node_off, T, P, TH, DZ, dQ, lddq);
    ERC_LAUNCH_CHECK("dgcnv2_nodal_bwd_q");
    hipLaunchKernelGGL(nodal_bwd_k_kernel, grid, dim3(NT), 0, (hipStream_t)stream, Q, ldq, dA, ldda, node_off, T, P, DZ, dE, ldde);
    ERC_LAUNCH_CHECK("dgcnv2_nodal_bwd_k");
    return ERC_OK;
}

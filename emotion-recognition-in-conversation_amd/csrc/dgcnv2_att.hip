// The positional edge attention of the conv-emotion DialogueGCN (track_mm/dgcnv2.py, track_mm/dgcnv2_models.py) and its batch
// tables.  Its nodal attention is the matching attention of match_att.hip at row width 300.
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
// Capacity form (erc_dgcnv2_edge_att_*_cap, CAP = true): the launch is sized for (B_cap, T_cap) and the batch's own longest
// dialogue arrives on the device; T_eff = clamp(*t_dev, 0, T_cap) takes T's place in the softmax, in the leak term and in the
// rows that are read, so a wave does exactly the arithmetic of the exact launch with T = *t_dev.  The backward writes rows
// t >= T_eff of dS as zeros (they belong to no position of this batch), still one writer per element.
#include "erc_common.h"

namespace {

constexpr int NSCAL = 110;         // rows of Wscalar: the reference's max_seq_len
constexpr int NT = 256;

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

// T of a capacity launch: the batch's longest dialogue, read from the device
__device__ __forceinline__ int t_eff(const int32_t* __restrict__ t_dev, int T_cap) { return min(max(*t_dev, 0), T_cap); }

template <bool CAP>
__global__ __launch_bounds__(NT) void edge_att_fwd_kernel(const float* __restrict__ Sc, int ldS, const int32_t* __restrict__ node_off,
                                                          int B, int T, int wp, int wf, const int32_t* __restrict__ out_ptr,
                                                          const int32_t* __restrict__ out_dst,
                                                          const int32_t* __restrict__ out_eid, float* __restrict__ norm,
                                                          const int32_t* __restrict__ t_dev) {
    const int lane = threadIdx.x & 63, p = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), b = blockIdx.y;
    const int base = node_off[b], L = node_off[b + 1] - base;
    if (p >= L) return;
    if constexpr (CAP) T = t_eff(t_dev, T);
    const WinSoftmax w = win_softmax(Sc, ldS, B, T, b, p, L, wp, wf, lane);
    const int j = base + p;
    // lane l writes out-edge l of the pass; u of its target comes from the lane that holds that position
    const int e0 = out_ptr[j], e1 = out_ptr[j + 1];
    for (int eb = e0; eb < e1; eb += 64) {
        const int e = eb + lane;
        const int i = e < e1 ? out_dst[e] - base : 0;
        const float ua = __shfl(w.u0, i & 63, 64), ub = __shfl(w.u1, i & 63, 64);
        // (CAP, T_eff == 0: no position was read, den is 0 -- the edge of a batch that claims no step gets weight 0, not 0 / 0)
        if (e < e1) norm[out_eid[e]] = CAP && T == 0 ? 0.f : (i < 64 ? ua : ub) / w.den;
    }
}

template <bool CAP>
__global__ __launch_bounds__(NT) void edge_att_bwd_kernel(const float* __restrict__ Sc, int ldS, const int32_t* __restrict__ node_off,
                                                          int B, int T, int wp, int wf, const int32_t* __restrict__ out_ptr,
                                                          const int32_t* __restrict__ out_dst,
                                                          const int32_t* __restrict__ out_eid, const float* __restrict__ dnorm,
                                                          int dn_parts, int64_t dn_stride, float* __restrict__ dS,
                                                          const int32_t* __restrict__ t_dev) {
    const int lane = threadIdx.x & 63, p = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), b = blockIdx.y;
    if (p >= NSCAL) return;
    const int base = node_off[b], L = node_off[b + 1] - base;
    const int t0 = lane, t1 = lane + 64;
    const int T_cap = T;      // rows [T, T_cap) of a capacity launch: written 0
    if constexpr (CAP) T = t_eff(t_dev, T);
    // no source at this position: its column of Wscalar receives nothing from dialogue b (CAP, T == 0: nor from anything)
    if (p >= L || (CAP && T == 0)) {
        if (t0 < T_cap) dS[((int64_t)t0 * B + b) * ldS + p] = 0.f;
        if (t1 < T_cap) dS[((int64_t)t1 * B + b) * ldS + p] = 0.f;
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
    if constexpr (CAP) {
        if (t0 >= T && t0 < T_cap) dS[((int64_t)t0 * B + b) * ldS + p] = 0.f;
        if (t1 >= T && t1 < T_cap) dS[((int64_t)t1 * B + b) * ldS + p] = 0.f;
    }
}

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

// The two entry points of each pass share their checks and their launch; t_dev == NULL is the exact form.
static int edge_att_fwd(const char* name, const float* S, int ldS, const int32_t* node_off, int B, int T, int wp, int wf,
                        const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid, float* norm, const int32_t* t_dev,
                        void* stream) {
    ERC_REQUIRE(S && node_off && out_ptr && out_dst && out_eid && norm, "%s: null pointer", name);
    ERC_REQUIRE(B > 0 && T > 0 && ldS >= NSCAL, "%s: bad sizes B=%d T=%d ldS=%d", name, B, T, ldS);
    ERC_REQUIRE(T <= NSCAL, "%s: Wscalar has %d rows, dialogues of up to %d utterances (batch T=%d)", name, NSCAL, NSCAL, T);
    const dim3 grid(erc_cdiv(T, NT / 64), B);
    if (t_dev)
        hipLaunchKernelGGL(edge_att_fwd_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, S, ldS, node_off, B, T, wp, wf, out_ptr,
                           out_dst, out_eid, norm, t_dev);
    else
        hipLaunchKernelGGL(edge_att_fwd_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, S, ldS, node_off, B, T, wp, wf,
                           out_ptr, out_dst, out_eid, norm, t_dev);
    ERC_LAUNCH_CHECK(name);
    return ERC_OK;
}

static int edge_att_bwd(const char* name, const float* S, int ldS, const int32_t* node_off, int B, int T, int wp, int wf,
                        const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid, const float* dnorm, int dn_parts,
                        int64_t dn_stride, float* dS, const int32_t* t_dev, void* stream) {
    ERC_REQUIRE(S && node_off && out_ptr && out_dst && out_eid && dnorm && dS, "%s: null pointer", name);
    ERC_REQUIRE(B > 0 && T > 0 && ldS >= NSCAL, "%s: bad sizes B=%d T=%d ldS=%d", name, B, T, ldS);
    ERC_REQUIRE(T <= NSCAL, "%s: dialogues of up to %d utterances (batch T=%d)", name, NSCAL, T);
    ERC_REQUIRE(dn_parts >= 1 && (dn_parts == 1 || dn_stride > 0), "%s: dn_parts=%d", name, dn_parts);
    ERC_REQUIRE(S != dS, "%s: dS must not alias S", name);
    const dim3 grid(erc_cdiv(NSCAL, NT / 64), B);
    if (t_dev)
        hipLaunchKernelGGL(edge_att_bwd_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, S, ldS, node_off, B, T, wp, wf, out_ptr,
                           out_dst, out_eid, dnorm, dn_parts, dn_stride, dS, t_dev);
    else
        hipLaunchKernelGGL(edge_att_bwd_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, S, ldS, node_off, B, T, wp, wf,
                           out_ptr, out_dst, out_eid, dnorm, dn_parts, dn_stride, dS, t_dev);
    ERC_LAUNCH_CHECK(name);
    return ERC_OK;
}

extern "C" int erc_dgcnv2_edge_att_fwd(const float* S, int ldS, const int32_t* node_off, int B, int T, int wp, int wf,
                                       const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid, float* norm,
                                       void* stream) {
    return edge_att_fwd("dgcnv2_edge_att_fwd", S, ldS, node_off, B, T, wp, wf, out_ptr, out_dst, out_eid, norm, nullptr, stream);
}

extern "C" int erc_dgcnv2_edge_att_fwd_cap(const float* S, int ldS, const int32_t* node_off, int B, int T, int wp, int wf,
                                           const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid, float* norm,
                                           const int32_t* t_dev, void* stream) {
    return edge_att_fwd("dgcnv2_edge_att_fwd_cap", S, ldS, node_off, B, T, wp, wf, out_ptr, out_dst, out_eid, norm, t_dev, stream);
}

extern "C" int erc_dgcnv2_edge_att_bwd(const float* S, int ldS, const int32_t* node_off, int B, int T, int wp, int wf,
                                       const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid, const float* dnorm,
                                       int dn_parts, int64_t dn_stride, float* dS, void* stream) {
    return edge_att_bwd("dgcnv2_edge_att_bwd", S, ldS, node_off, B, T, wp, wf, out_ptr, out_dst, out_eid, dnorm, dn_parts, dn_stride,
                        dS, nullptr, stream);
}

extern "C" int erc_dgcnv2_edge_att_bwd_cap(const float* S, int ldS, const int32_t* node_off, int B, int T, int wp, int wf,
                                           const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_eid,
                                           const float* dnorm, int dn_parts, int64_t dn_stride, float* dS, const int32_t* t_dev,
                                           void* stream) {
    return edge_att_bwd("dgcnv2_edge_att_bwd_cap", S, ldS, node_off, B, T, wp, wf, out_ptr, out_dst, out_eid, dnorm, dn_parts,
                        dn_stride, dS, t_dev, stream);
}

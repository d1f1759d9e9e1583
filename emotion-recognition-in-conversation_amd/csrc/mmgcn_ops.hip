// MMGCN graph operators (track_mm/mmgcn_models.py:8-39,344-394,493-646).
//
// The reference builds a dense (modalities*N)^2 adjacency on the host (python loops, a CPU-allocated scratch
// block per dialogue) and multiplies it densely in each of the 64 GCNII layers although only the per-dialogue,
// per-modality L x L blocks and the same-utterance cross-modal entries are non-zero.  Here the adjacency is kept
// as exactly that structure:
//     blocks  ADJ [B*M][P][P]   (P = padded max length, multiple of 4), cross CR [B][M*M][P]
// Node rows are ordered modality-major: node (m, b, t) = m*N + node_off[b] + t, like torch.cat([a, v, l]).
// The block products are grouped MFMA GEMMs (gemm.hip); this file holds the remaining small operators.
#include "erc_common.h"

namespace {

constexpr int FD = 200;     // node feature width (n_dim = nhidden = 200)
constexpr int MAXP = 128;   // padded dialogue length supported by the per-dialogue kernels
constexpr float PI_F = 3.14159265358979323846f;
constexpr float SHRINK = 0.99999f;

struct L4 {
    float v[4];
};
__device__ __forceinline__ L4 ld4(const float* row, int lane) {
    L4 r;
#pragma unroll
    for (int u = 0; u < 4; ++u) r.v[u] = lane + 64 * u < FD ? row[lane + 64 * u] : 0.f;
    return r;
}
__device__ __forceinline__ float dt4(const L4& a, const L4& b) {
    return a.v[0] * b.v[0] + a.v[1] * b.v[1] + a.v[2] * b.v[2] + a.v[3] * b.v[3];
}

// node tables of the time-major MMGCN batch: node i = node_off[b] + t  ->  row t*B + b of the [T,B,.] blocks,
// its dialogue and its speaker id (argmax of the one-hot qmask, mmgcn_models.py:540-541)
__global__ __launch_bounds__(256) void mm_meta_kernel(const int64_t* __restrict__ lengths, const float* __restrict__ qmask,
                                                      int64_t q_st, int64_t q_sb, int S, int B, int32_t* __restrict__ node_off,
                                                      int32_t* __restrict__ node_row, int32_t* __restrict__ node_dlg,
                                                      int32_t* __restrict__ node_spk) {
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ int red[256];
    int acc = 0;
    for (int i = tid; i < b; i += 256) acc += (int)lengths[i];
    red[tid] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const int off = red[0], L = (int)lengths[b];
    if (tid == 0) {
        node_off[b] = off;
        if (b == B - 1) node_off[B] = off + L;
    }
    for (int t = tid; t < L; t += 256) {
        node_row[off + t] = t * B + b;
        node_dlg[off + t] = b;
        const float* row = qmask + (int64_t)t * q_st + (int64_t)b * q_sb;
        int s = 0;
        float best = row[0];
        for (int c = 1; c < S; ++c)
            if (row[c] > best) best = row[c], s = c;
        node_spk[off + t] = s;
    }
}

// CAPACITY mode (mmgcn.py, MMGCNModule.dynamic_n): the launches are sized for B dialogue slots (missing ones: length 0), T = T_cap
// and n_cap nodes per modality while the batch's own node count lives on the device.  Modality m's rows start at m * n_cap; its
// rows [m * n_cap + n, (m + 1) * n_cap) are TAIL rows.  The <CAP> instances below read n = *n_dev and give the tail a fixed
// content: zero in every output (so a gradient-side tail is exactly zero), and no part in any sum.
__device__ __forceinline__ int n_live(const int32_t* __restrict__ n_dev, int n_cap) { return min(max(*n_dev, 0), n_cap); }

// The node tables of a capacity step, from lengths [B] + the padded time-major qmask (bucket form) or from desc [2 B] (int32:
// lengths | first store rows) + the store's speaker ids (RESIDENT form).  One workgroup; B <= 1024.
__global__ __launch_bounds__(1024) void mm_meta_cap_kernel(
    const int64_t* __restrict__ lengths, const float* __restrict__ qmask, int64_t q_st, int64_t q_sb, int S,
    const int32_t* __restrict__ desc, const int64_t* __restrict__ store_spk, const int64_t* __restrict__ store_label,
    int zero_store_row, int B, int T, int n_cap, int32_t* __restrict__ node_off, int32_t* __restrict__ node_row,
    int32_t* __restrict__ node_pad, int32_t* __restrict__ node_dlg, int32_t* __restrict__ node_spk, int32_t* __restrict__ pad_node,
    int32_t* __restrict__ x_row, int64_t* __restrict__ label_out, int32_t* __restrict__ counts) {
    __shared__ int s_off[1025];
    if (threadIdx.x == 0) {
        int acc = 0, tmax = 0;
        for (int b = 0; b < B; ++b) {
            s_off[b] = acc;
            const int L = (int)min(max(desc ? (int64_t)desc[b] : lengths[b], (int64_t)0), (int64_t)T);
            const int Lc = min(L, n_cap - acc);       // never past the capacity (the host sizes n_cap >= sum(lengths))
            acc += Lc;
            tmax = max(tmax, Lc);
        }
        s_off[B] = acc;
        counts[0] = acc;       // n_dev
        counts[1] = tmax;      // t_dev
    }
    __syncthreads();
    const int N = s_off[B];
    for (int b = threadIdx.x; b <= B; b += blockDim.x) node_off[b] = s_off[b];
    for (int i = threadIdx.x; i < B * T; i += blockDim.x) {
        const int t = i / B, b = i % B;
        const int o = s_off[b], L = s_off[b + 1] - o;
        pad_node[i] = t < L ? o + t : n_cap;        // (n_cap: the zero row the caller keeps behind its node gradient)
        if (x_row) x_row[i] = t < L ? desc[B + b] + t : zero_store_row;
        if (t >= L) continue;
        const int j = o + t;
        node_pad[j] = i;
        node_dlg[j] = b;
        int s = 0;
        if (desc) {
            const int r = desc[B + b] + t;
            node_row[j] = r;
            s = (int)min(max(store_spk[r], (int64_t)0), (int64_t)(S - 1));
            if (label_out) label_out[j] = store_label[r];
        } else {
            node_row[j] = i;
            const float* row = qmask + (int64_t)t * q_st + (int64_t)b * q_sb;
            float best = row[0];
            for (int c = 1; c < S; ++c)
                if (row[c] > best) best = row[c], s = c;
        }
        node_spk[j] = s;
    }
    // tail entries: a row that is valid to read (padded row 0; resident: the store's zero row), dialogue 0, speaker 0, label 0
    for (int j = N + threadIdx.x; j < n_cap; j += blockDim.x) {
        node_row[j] = desc ? zero_store_row : 0;
        node_pad[j] = 0;
        node_dlg[j] = 0;
        node_spk[j] = 0;
        if (desc && label_out) label_out[j] = 0;
    }
}

// dst[(m_off + i), :] = src[row_map[i], :] (+ emb[spk[i], :])  : simple_batch_graphify (mmgcn_utils.py:5-21) plus
// the speaker-embedding add of mmgcn_models.py:540-545
template <bool CAP>
__global__ __launch_bounds__(256) void flatten_kernel(const float* __restrict__ src, int lds, const int32_t* __restrict__ row_map,
                                                      const float* __restrict__ emb, const int32_t* __restrict__ spk,
                                                      int N, float* __restrict__ dst, int ldd, const int32_t* __restrict__ n_dev) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;
    if (CAP && i >= n_live(n_dev, N)) {
        for (int c = lane; c < FD; c += 64) dst[(int64_t)i * ldd + c] = 0.f;
        return;
    }
    const float* s = src + (int64_t)row_map[i] * lds;
    const float* e = emb ? emb + (int64_t)spk[i] * FD : nullptr;
    for (int c = lane; c < FD; c += 64) dst[(int64_t)i * ldd + c] = s[c] + (e ? e[c] : 0.f);
}

// demb[s, :] = sum_{i: spk[i]==s} dl[i, :], fixed order, two stages: EG_CH row chunks per speaker into ws, then their sum.
// Rows are read 8 at a time unconditionally and masked by multiplication.  (One workgroup per speaker walked all N rows
// on 2 of the 256 CUs: 69 us at N = 920; a guarded load per row before that: 152 us.)
constexpr int EG_CH = 32;
template <bool CAP>
__global__ __launch_bounds__(256) void emb_grad_part_kernel(const float* __restrict__ dl, int ld, const int32_t* __restrict__ spk,
                                                             int N, float* __restrict__ part, const int32_t* __restrict__ n_dev) {
    const int s = blockIdx.x, ch = blockIdx.y, c = threadIdx.x;
    if (CAP) N = n_live(n_dev, N);       // the sum runs over the batch's own rows (N == 0: no row is read)
    const int cc = min(c, FD - 1);
    const int per = (N + EG_CH - 1) / EG_CH, lo = ch * per, hi = min(N, lo + per);
    float acc = 0.f;
    for (int i0 = lo; i0 < hi; i0 += 8) {
        float v[8], m[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = min(i0 + u, N - 1);
            v[u] = dl[(int64_t)i * ld + cc];
            m[u] = (i0 + u < hi && spk[i] == s) ? 1.f : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u] * m[u];
    }
    if (c < FD) part[((int64_t)s * EG_CH + ch) * FD + c] = acc;
}
__global__ __launch_bounds__(256) void emb_grad_sum_kernel(const float* __restrict__ part, float* __restrict__ demb) {
    const int s = blockIdx.x, c = threadIdx.x;
    if (c >= FD) return;
    float v[EG_CH];
#pragma unroll
    for (int ch = 0; ch < EG_CH; ++ch) v[ch] = part[((int64_t)s * EG_CH + ch) * FD + c];
    float acc = 0.f;
#pragma unroll
    for (int ch = 0; ch < EG_CH; ++ch) acc += v[ch];
    demb[s * FD + c] = acc;
}

// xhat = x / |x| ; inv = 1/|x|
template <bool CAP>
__global__ __launch_bounds__(256) void row_normalize_kernel(const float* __restrict__ x, int R, float* __restrict__ xhat,
                                                            float* __restrict__ inv, int n_cap, const int32_t* __restrict__ n_dev) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= R) return;
    if (CAP && i % n_cap >= n_live(n_dev, n_cap)) {       // a tail row: xhat = 0, inv = 0, whatever x holds (no 1 / |x|)
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (lane + 64 * u < FD) xhat[(int64_t)i * FD + lane + 64 * u] = 0.f;
        if (lane == 0) inv[i] = 0.f;
        return;
    }
    const L4 v = ld4(x + (int64_t)i * FD, lane);
    const float rn = 1.0f / sqrtf(wave_sum(dt4(v, v)));
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (lane + 64 * u < FD) xhat[(int64_t)i * FD + lane + 64 * u] = v.v[u] * rn;
    if (lane == 0) inv[i] = rn;
}

// dx += inv * (dxhat - xhat (xhat . dxhat))
template <bool CAP>
__global__ __launch_bounds__(256) void row_normalize_bwd_kernel(const float* __restrict__ xhat, const float* __restrict__ inv,
                                                                const float* __restrict__ dxhat, int R,
                                                                float* __restrict__ dx, int n_cap, const int32_t* __restrict__ n_dev) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= R) return;
    if (CAP && i % n_cap >= n_live(n_dev, n_cap)) {       // a tail row of the gradient: written 0, not accumulated into
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (lane + 64 * u < FD) dx[(int64_t)i * FD + lane + 64 * u] = 0.f;
        return;
    }
    const L4 h = ld4(xhat + (int64_t)i * FD, lane), d = ld4(dxhat + (int64_t)i * FD, lane);
    const float dot = wave_sum(dt4(h, d)), rn = inv[i];
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (lane + 64 * u < FD) dx[(int64_t)i * FD + lane + 64 * u] += rn * (d.v[u] - h.v[u] * dot);
}

__device__ __forceinline__ float sim_of(float c) { return 1.0f - acosf(SHRINK * c) / PI_F; }
// Cosine (p, q) of a COS block [P][P], renormalised by the block's own diagonal: the grouped GEMM's |xhat_p|^2 is 1 only to a few
// roundings, and at cos -> 1 (the diagonal itself, duplicate rows) such a rounding is the whole of 1 - cos, which acos and
// dsim_dc amplify by 1e2 .. 5e4.  The diagonal comes out as exactly 1, and so do rows that coincide (same products, same order).
__device__ __forceinline__ float cos_n(const float* __restrict__ blk, int P, int p, int q) {
    return blk[(int64_t)p * P + q] / sqrtf(blk[(int64_t)p * P + p] * blk[(int64_t)q * P + q]);
}
// d sim / d c = SHRINK / (pi sqrt(1 - t^2)), t = SHRINK c.  Where |c| -> 1 (every diagonal entry, duplicate or opposite rows) 1 - t^2
// is ~2e-5 and `1.0f - t * t` loses three digits to the roundings of t and of t * t; instead 1 - t^2 = (1 - t)(1 + t) with
// 1 -+ t = (1 - SHRINK) + SHRINK (1 -+ c), whose differences are exact near the ends.
__device__ __forceinline__ float dsim_dc(float c) {
    constexpr float OMS = 1e-5f;     // 1 - 0.99999, not 1.0f - SHRINK (SHRINK itself is rounded by 1.4e-8)
    const float omt = OMS + SHRINK * (1.0f - c), opt = OMS + SHRINK * (1.0f + c);
    return SHRINK / (PI_F * sqrtf(fmaxf(omt * opt, 1e-12f)));
}

// COS blocks (raw cosines from the grouped GEMM) -> normalised adjacency blocks ADJ, normalised cross entries
// CR[b][m*M+n][p] (m != n), degrees DEG[node], raw cross cosines CCOS.  One wavefront per adjacency row (m, p) of a
// dialogue, two launches: similarities + degrees, then the D^-1/2 . D^-1/2 scaling that needs every degree of the block.
// (One workgroup per dialogue ran the three phases behind barriers on 32 of the 256 CUs: 91 us; and its backward 84 us.)
__global__ __launch_bounds__(256) void adj_rows_kernel(const float* __restrict__ COS, const float* __restrict__ xhat,
                                                       const int32_t* __restrict__ node_off, int M, int N, int P,
                                                       float* __restrict__ ADJ, float* __restrict__ CCOS,
                                                       float* __restrict__ DEG) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, it = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int off = node_off[b], L = node_off[b + 1] - off;
    if (it >= M * L) return;
    const int m = it / L, p = it % L;
    // cross-modal same-utterance similarities of this node
    float cross = 0.f;
    const L4 mine = ld4(xhat + ((int64_t)m * N + off + p) * FD, lane);
    const float nm = wave_sum(dt4(mine, mine));
    for (int n = 0; n < M; ++n) {
        if (n == m) continue;
        // renormalised: |xhat|^2 is 1 only to a rounding, and where the two rows coincide that rounding would be the whole of
        // 1 - c (dsim_dc); dot and norms are summed in the same order, so coinciding rows give exactly 1
        const L4 other = ld4(xhat + ((int64_t)n * N + off + p) * FD, lane);
        const float c = wave_sum(dt4(mine, other)) / sqrtf(nm * wave_sum(dt4(other, other)));
        if (lane == 0) CCOS[((int64_t)b * M * M + m * M + n) * P + p] = c;
        cross += sim_of(c);
    }
    const float* blk = COS + ((int64_t)b * M + m) * P * P;
    float* ar = ADJ + (((int64_t)b * M + m) * P + p) * P;
    float rs = 0.f;
    for (int q = lane; q < L; q += 64) {
        const float s = sim_of(cos_n(blk, P, p, q));
        ar[q] = s;
        rs += s;
    }
    rs = wave_sum(rs) + cross;
    if (lane == 0) DEG[(int64_t)m * N + off + p] = rs;
}

__global__ __launch_bounds__(256) void adj_scale_kernel(const float* __restrict__ CCOS, const float* __restrict__ DEG,
                                                        const int32_t* __restrict__ node_off, int M, int N, int P,
                                                        float* __restrict__ ADJ, float* __restrict__ CR) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, it = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int off = node_off[b], L = node_off[b + 1] - off;
    if (it >= M * L) return;
    const int m = it / L, p = it % L;
    const float up = 1.0f / sqrtf(DEG[(int64_t)m * N + off + p]);
    float* ar = ADJ + (((int64_t)b * M + m) * P + p) * P;
    for (int q = lane; q < L; q += 64) ar[q] *= up * (1.0f / sqrtf(DEG[(int64_t)m * N + off + q]));
    if (lane < M && lane != m) {
        const int64_t i_mn = ((int64_t)b * M * M + m * M + lane) * P + p;
        CR[i_mn] = sim_of(CCOS[i_mn]) * up * (1.0f / sqrtf(DEG[(int64_t)lane * N + off + p]));
    }
}

// Backward of adj_finish: from dADJ (blocks) and dCR (directional cross gradients) to
//   G = dCOS + dCOS^T (blocks, so that dXhat_block = G Xhat is one grouped GEMM) and GC (cross, symmetric per
//   unordered pair, applied with cross_apply on Xhat).  Same split: per-row degree gradients DD, then the entries.
__global__ __launch_bounds__(256) void adj_bwd_rows_kernel(const float* __restrict__ COS, const float* __restrict__ CCOS,
                                                           const float* __restrict__ DEG, const float* __restrict__ dADJ,
                                                           const float* __restrict__ dCR,
                                                           const int32_t* __restrict__ node_off, int M, int N, int P,
                                                           float* __restrict__ DD) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, it = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int off = node_off[b], L = node_off[b + 1] - off;
    if (it >= M * L) return;
    const int m = it / L, p = it % L;
    // du_p = sum_q (dA_pq + dA_qp) S_pq u_q  + cross terms;  dd_p = -1/2 du_p d_p^-3/2
    const int64_t base = ((int64_t)b * M + m) * P;
    float acc = 0.f;
    for (int q = lane; q < L; q += 64) {
        const float s = sim_of(cos_n(COS + base * P, P, p, q));
        acc += (dADJ[(base + p) * P + q] + dADJ[(base + q) * P + p]) * s * (1.0f / sqrtf(DEG[(int64_t)m * N + off + q]));
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        for (int n = 0; n < M; ++n)
            if (n != m) {
                const float s = sim_of(CCOS[((int64_t)b * M * M + m * M + n) * P + p]);
                // entry ((m,p),(n,p)) and entry ((n,p),(m,p)) both carry u^m_p
                acc += (dCR[((int64_t)b * M * M + m * M + n) * P + p] + dCR[((int64_t)b * M * M + n * M + m) * P + p]) *
                       s * (1.0f / sqrtf(DEG[(int64_t)n * N + off + p]));
            }
        const float u = 1.0f / sqrtf(DEG[(int64_t)m * N + off + p]);
        DD[(int64_t)m * N + off + p] = -0.5f * acc * u * u * u;
    }
}

__global__ __launch_bounds__(256) void adj_bwd_entries_kernel(const float* __restrict__ COS, const float* __restrict__ CCOS,
                                                              const float* __restrict__ DEG, const float* __restrict__ DD,
                                                              const float* __restrict__ dADJ, const float* __restrict__ dCR,
                                                              const int32_t* __restrict__ node_off, int M, int N, int P,
                                                              float* __restrict__ G, float* __restrict__ GC) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, it = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int off = node_off[b], L = node_off[b + 1] - off;
    if (it >= M * L) return;
    const int m = it / L, p = it % L;
    const int64_t base = ((int64_t)b * M + m) * P;
    const float up = 1.0f / sqrtf(DEG[(int64_t)m * N + off + p]), ddp = DD[(int64_t)m * N + off + p];
    // dS_pq = dA_pq u_p u_q + dd_p ; dcos = dS * dsim/dc ; G_pq = dcos_pq + dcos_qp
    for (int q = lane; q < L; q += 64) {
        const float c = cos_n(COS + base * P, P, p, q);  // symmetric up to rounding; use the (p,q) entry for both halves
        const float uu = up * (1.0f / sqrtf(DEG[(int64_t)m * N + off + q]));
        const float dpq = dADJ[(base + p) * P + q] * uu + ddp;
        const float dqp = dADJ[(base + q) * P + p] * uu + DD[(int64_t)m * N + off + q];
        G[(base + p) * P + q] = (dpq + dqp) * dsim_dc(c);
    }
    if (lane < M && lane != m) {
        const int n = lane;
        const int64_t i_mn = ((int64_t)b * M * M + m * M + n) * P + p, i_nm = ((int64_t)b * M * M + n * M + m) * P + p;
        const float uu = up * (1.0f / sqrtf(DEG[(int64_t)n * N + off + p]));
        // directional entries (m,n) and (n,m) share one cosine: total gradient of that cosine, stored for both
        const float ds = (dCR[i_mn] * uu + ddp) + (dCR[i_nm] * uu + DD[(int64_t)n * N + off + p]);
        GC[i_mn] = ds * dsim_dc(CCOS[i_mn]);
    }
}

// out[(m,p), :] += sum_{n != m} CR[b][m*M+n][p] * h[(n,p), :]   (cross-modal part of A*h, and of its transpose)
template <bool CAP>
__global__ __launch_bounds__(256) void cross_apply_kernel(const float* __restrict__ CR, const float* __restrict__ h, int ldh,
                                                          const int32_t* __restrict__ node_dlg,
                                                          const int32_t* __restrict__ node_off, int M, int N, int P,
                                                          float* __restrict__ out, int ldo, const int32_t* __restrict__ n_dev) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M * N) return;
    if (CAP && r % N >= n_live(n_dev, N)) return;        // a tail row has no adjacency entry: its row of out is not touched
    const int m = r / N, i = r % N, b = node_dlg[i], p = i - node_off[b];
    L4 acc = {{0.f, 0.f, 0.f, 0.f}};
    for (int n = 0; n < M; ++n) {
        if (n == m) continue;
        const float c = CR[((int64_t)b * M * M + m * M + n) * P + p];
        const L4 v = ld4(h + ((int64_t)n * N + i) * ldh, lane);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc.v[u] += c * v.v[u];
    }
    float* o = out + (int64_t)r * ldo;
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (lane + 64 * u < FD) o[lane + 64 * u] += acc.v[u];
}

// dCR[b][m*M+n][p] += sum over planes of dhi_pl[(m,p), :] . h_pl[(n,p), :]   (directional); planes = the layers whose
// contributions only meet in this sum (one launch for all of them)
template <bool CAP>
__global__ __launch_bounds__(256) void cross_grad_kernel(const float* __restrict__ dhi, int ldd, const float* __restrict__ h,
                                                         int ldh, const int32_t* __restrict__ node_dlg,
                                                         const int32_t* __restrict__ node_off, int M, int N, int P,
                                                         float* __restrict__ dCR, int planes, int64_t d_plane, int64_t h_plane,
                                                         const int32_t* __restrict__ n_dev) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M * N) return;
    // a tail row owns no entry of dCR: with its sentinel dialogue it would add (a zero) to an entry another wavefront owns
    if (CAP && r % N >= n_live(n_dev, N)) return;
    const int m = r / N, i = r % N, b = node_dlg[i], p = i - node_off[b];
    for (int n = 0; n < M; ++n) {
        if (n == m) continue;
        float acc = 0.f;
        for (int pl0 = 0; pl0 < planes; pl0 += 4) {      // 4 planes (8 row loads) in flight
            L4 g[4], hh[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int pl = min(pl0 + u, planes - 1);
                g[u] = ld4(dhi + (int64_t)pl * d_plane + (int64_t)r * ldd, lane);
                hh[u] = ld4(h + (int64_t)pl * h_plane + ((int64_t)n * N + i) * ldh, lane);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc += (pl0 + u < planes) ? dt4(g[u], hh[u]) : 0.f;
        }
        const float d = wave_sum(acc);
        if (lane == 0) dCR[((int64_t)b * M * M + m * M + n) * P + p] += d;
    }
}

// GCNII layer tail (mmgcn_models.py:27-39,385-388): out = theta*G + (1-theta)((1-alpha) hi + alpha h0);
// hd = dropout(relu(out))
__global__ __launch_bounds__(256) void gcnii_combine_fwd_kernel(const float* __restrict__ Gm, const float* __restrict__ hi,
                                                                const float* __restrict__ h0, int64_t n, float theta,
                                                                float alpha, float drop_p, const uint64_t* rng,
                                                                uint64_t stream_id, float* __restrict__ hd) {
    uint64_t roff = 0, rseed = 0;
    if (drop_p > 0.f) roff = rng[0], rseed = rng[1] ^ stream_id;
    const float ks = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float v = Gm[i];
        if (hi) v = theta * v + (1.f - theta) * ((1.f - alpha) * hi[i] + alpha * h0[i]);
        v = fmaxf(v, 0.f);
        if (drop_p > 0.f) v = erc_uniform(rseed, roff, (uint64_t)i) >= drop_p ? v * ks : 0.f;
        hd[i] = v;
    }
}

// backward of the tail: dout = d_hd * [hd > 0] * keep_scale; dG = theta dout; dhi = (1-theta)(1-alpha) dout;
// dh0 += (1-theta) alpha dout.   With hi == nullptr (input layer): dG = dout only.
template <bool CAP>
__global__ __launch_bounds__(256) void gcnii_combine_bwd_kernel(const float* __restrict__ d_hd, const float* __restrict__ hd,
                                                                int64_t n, float theta, float alpha, float keep_scale,
                                                                int plain, float* __restrict__ dG, float* __restrict__ dhi,
                                                                float* __restrict__ dh0, int F, int ld_d, int n_cap,
                                                                const int32_t* __restrict__ n_dev) {
    const int nl = CAP ? n_live(n_dev, n_cap) : 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (CAP && (int)((i / F) % n_cap) >= nl) {       // a tail row: dG (and dhi) written 0, nothing added to dh0
            dG[i] = 0.f;
            if (!plain) dhi[(i / F) * ld_d + i % F] = 0.f;
            continue;
        }
        const float g = hd[i] > 0.f ? d_hd[i] * keep_scale : 0.f;
        if (plain) {
            dG[i] = g;
        } else {
            const int64_t row = i / F, j = row * ld_d + (i - row * F);   // dhi / dh0 rows have pitch ld_d
            dG[i] = theta * g;
            dhi[j] = (1.f - theta) * (1.f - alpha) * g;
            dh0[j] += (1.f - theta) * alpha * g;
        }
    }
}

// y = dropout(x) elementwise (input dropout of GCNII, mmgcn_models.py:382) and its backward (in place)
template <bool CAP>
__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ x, int64_t n, float drop_p,
                                                      const uint64_t* rng, uint64_t stream_id, float* __restrict__ y, int row_w,
                                                      int n_cap, const int32_t* __restrict__ n_dev) {
    const uint64_t roff = rng[0], rseed = rng[1] ^ stream_id;
    const float ks = 1.0f / (1.0f - drop_p);
    const int nl = CAP ? n_live(n_dev, n_cap) : 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (CAP && (int)((i / row_w) % n_cap) >= nl) {
            y[i] = 0.f;
            continue;
        }
        y[i] = erc_uniform(rseed, roff, (uint64_t)i) >= drop_p ? x[i] * ks : 0.f;
    }
}

// FE[p, m*400 + c] = relu(dropout(cat[xd, h][(m,p), c]))  (regroup of mmgcn_models.py:570-576 + dropout_/ReLU of
// mmgcn.py:119-120);  backward scatters dFE back to d_xd / d_h.
template <bool CAP>
__global__ __launch_bounds__(256) void regroup_fwd_kernel(const float* __restrict__ xd, const float* __restrict__ hl, int M,
                                                          int N, float drop_p, const uint64_t* rng, uint64_t stream_id,
                                                          float* __restrict__ FE, const int32_t* __restrict__ n_dev) {
    const int nl = CAP ? n_live(n_dev, N) : 0;
    uint64_t roff = 0, rseed = 0;
    if (drop_p > 0.f) roff = rng[0], rseed = rng[1] ^ stream_id;
    const float ks = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
    const int64_t total = (int64_t)N * M * 2 * FD;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % (2 * FD)), m = (int)((i / (2 * FD)) % M);
        const int64_t p = i / ((int64_t)2 * FD * M);
        if (CAP && p >= nl) {
            FE[i] = 0.f;
            continue;
        }
        const int64_t row = (int64_t)m * N + p;
        float v = c < FD ? xd[row * FD + c] : hl[row * FD + c - FD];
        if (drop_p > 0.f) v = erc_uniform(rseed, roff, (uint64_t)i) >= drop_p ? v * ks : 0.f;
        FE[i] = fmaxf(v, 0.f);
    }
}
template <bool CAP>
__global__ __launch_bounds__(256) void regroup_bwd_kernel(const float* __restrict__ dFE, const float* __restrict__ FE, int M,
                                                          int N, float keep_scale, float* __restrict__ d_xd,
                                                          float* __restrict__ d_h, const int32_t* __restrict__ n_dev) {
    const int nl = CAP ? n_live(n_dev, N) : 0;
    const int64_t total = (int64_t)N * M * 2 * FD;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % (2 * FD)), m = (int)((i / (2 * FD)) % M);
        const int64_t p = i / ((int64_t)2 * FD * M);
        const int64_t row = (int64_t)m * N + p;
        const float g = (CAP && p >= nl) ? 0.f : FE[i] > 0.f ? dFE[i] * keep_scale : 0.f;
        if (c < FD)
            d_xd[row * FD + c] = g;
        else
            d_h[row * FD + c - FD] = g;
    }
}

// y[i] (+)= a*x[i] masked by (mask[i] != 0) * scale  -- small axpy used to merge gradient streams
template <bool CAP>
__global__ __launch_bounds__(256) void axpy_mask_kernel(const float* __restrict__ x, const float* __restrict__ mask, int64_t n,
                                                        float scale, int accumulate, float* __restrict__ y, int row_w, int n_cap,
                                                        const int32_t* __restrict__ n_dev) {
    const int nl = CAP ? n_live(n_dev, n_cap) : 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (CAP && (int)((i / row_w) % n_cap) >= nl) {       // a tail row of the gradient: written 0, accumulating or not
            y[i] = 0.f;
            continue;
        }
        const float v = (mask ? (mask[i] != 0.f ? x[i] * scale : 0.f) : x[i] * scale);
        y[i] = accumulate ? y[i] + v : v;
    }
}

// buf[(m * n_cap + i), 0 .. width) = 0 for n <= i < n_cap: the tail rows of a buffer whose valid rows a node_off-walking kernel
// (the GCNII chain, the grouped products) writes and whose tail therefore still holds an earlier, larger batch
__global__ __launch_bounds__(256) void zero_tail_kernel(float* __restrict__ buf, int64_t ld, int width, int n_mod, int n_cap,
                                                        const int32_t* __restrict__ n_dev) {
    const int n = n_live(n_dev, n_cap), tail = n_cap - n;
    const int64_t total = (int64_t)n_mod * tail * width;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / width;
        const int c = (int)(i - r * width), m = (int)(r / tail), k = (int)(r - (int64_t)m * tail);
        buf[((int64_t)m * n_cap + n + k) * ld + c] = 0.f;
    }
}

int ew_grid(int64_t n) {
    int64_t g = (n + 255) / 256;
    return (int)(g > 2048 ? 2048 : g);
}

}  // namespace

#define NODEG(R) dim3(erc_cdiv(R, 4)), dim3(256), 0, (hipStream_t)stream
// one launch site per operator: the exact-shape instance (n_dev == nullptr) or the capacity one
#define LAUNCH_CAP(kernel, cap, ...)                               \
    do {                                                           \
        if (cap) hipLaunchKernelGGL(kernel<true>, __VA_ARGS__);    \
        else hipLaunchKernelGGL(kernel<false>, __VA_ARGS__);       \
    } while (0)

extern "C" int erc_mm_meta(const int64_t* lengths, const float* qmask, int64_t q_st, int64_t q_sb, int n_speakers, int B,
                           int32_t* node_off, int32_t* node_row, int32_t* node_dlg, int32_t* node_spk, void* stream) {
    ERC_REQUIRE(lengths && qmask && node_off && node_row && node_dlg && node_spk && B > 0 && n_speakers > 0,
                "mm_meta: bad arguments");
    hipLaunchKernelGGL(mm_meta_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, lengths, qmask, q_st, q_sb, n_speakers,
                       B, node_off, node_row, node_dlg, node_spk);
    ERC_LAUNCH_CHECK("mm_meta");
    return ERC_OK;
}
extern "C" int erc_mm_meta_cap(const int64_t* lengths, const float* qmask, int64_t q_st, int64_t q_sb, int n_speakers,
                               const int32_t* desc, const int64_t* store_spk, const int64_t* store_label, int zero_store_row, int B,
                               int T, int n_cap, int32_t* node_off, int32_t* node_row, int32_t* node_pad, int32_t* node_dlg,
                               int32_t* node_spk, int32_t* pad_node, int32_t* x_row, int64_t* label_out, int32_t* counts,
                               void* stream) {
    ERC_REQUIRE(node_off && node_row && node_pad && node_dlg && node_spk && pad_node && counts, "mm_meta_cap: null pointer");
    ERC_REQUIRE(desc ? (store_spk && x_row && !lengths && !qmask && zero_store_row >= 0) : (lengths && qmask && !store_spk && !x_row),
                "mm_meta_cap: lengths + qmask (bucket form) or desc + store_spk + x_row (resident form)");
    ERC_REQUIRE(!store_label == !label_out && (!store_label || desc), "mm_meta_cap: store_label and label_out come with desc");
    ERC_REQUIRE(B > 0 && B <= 1024 && T > 0 && n_cap > 0 && n_speakers > 0, "mm_meta_cap: bad sizes B=%d T=%d n_cap=%d", B, T, n_cap);
    hipLaunchKernelGGL(mm_meta_cap_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, lengths, qmask, q_st, q_sb, n_speakers, desc,
                       store_spk, store_label, zero_store_row, B, T, n_cap, node_off, node_row, node_pad, node_dlg, node_spk, pad_node,
                       x_row, label_out, counts);
    ERC_LAUNCH_CHECK("mm_meta_cap");
    return ERC_OK;
}

static int mm_flatten(const float* src, int lds, const int32_t* row_map, const float* emb, const int32_t* spk, int N, float* dst,
                      int ldd, const int32_t* n_dev, void* stream) {
    ERC_REQUIRE(src && row_map && dst && N > 0 && (!emb || spk), "mm_flatten: bad arguments");
    LAUNCH_CAP(flatten_kernel, n_dev, NODEG(N), src, lds, row_map, emb, spk, N, dst, ldd, n_dev);
    ERC_LAUNCH_CHECK("mm_flatten");
    return ERC_OK;
}
extern "C" int erc_mm_flatten(const float* src, int lds, const int32_t* row_map, const float* emb, const int32_t* spk, int N,
                              float* dst, int ldd, void* stream) {
    return mm_flatten(src, lds, row_map, emb, spk, N, dst, ldd, nullptr, stream);
}
extern "C" int erc_mm_flatten_cap(const float* src, int lds, const int32_t* row_map, const float* emb, const int32_t* spk, int n_cap,
                                  const int32_t* n_dev, float* dst, int ldd, void* stream) {
    ERC_REQUIRE(n_dev, "mm_flatten_cap: n_dev is NULL");
    return mm_flatten(src, lds, row_map, emb, spk, n_cap, dst, ldd, n_dev, stream);
}
extern "C" int64_t erc_mm_emb_grad_ws_floats(int n_speakers) { return (int64_t)n_speakers * EG_CH * FD; }
static int mm_emb_grad(const float* dl, int ld, const int32_t* spk, int N, int n_speakers, float* demb, float* ws,
                       const int32_t* n_dev, void* stream) {
    ERC_REQUIRE(dl && spk && demb && ws && N > 0 && n_speakers > 0, "mm_emb_grad: bad arguments");
    LAUNCH_CAP(emb_grad_part_kernel, n_dev, dim3(n_speakers, EG_CH), dim3(256), 0, (hipStream_t)stream, dl, ld, spk, N, ws, n_dev);
    hipLaunchKernelGGL(emb_grad_sum_kernel, dim3(n_speakers), dim3(256), 0, (hipStream_t)stream, ws, demb);
    ERC_LAUNCH_CHECK("mm_emb_grad");
    return ERC_OK;
}
extern "C" int erc_mm_emb_grad(const float* dl, int ld, const int32_t* spk, int N, int n_speakers, float* demb, float* ws,
                               void* stream) {
    return mm_emb_grad(dl, ld, spk, N, n_speakers, demb, ws, nullptr, stream);
}
extern "C" int erc_mm_emb_grad_cap(const float* dl, int ld, const int32_t* spk, int n_cap, const int32_t* n_dev, int n_speakers,
                                   float* demb, float* ws, void* stream) {
    ERC_REQUIRE(n_dev, "mm_emb_grad_cap: n_dev is NULL");
    return mm_emb_grad(dl, ld, spk, n_cap, n_speakers, demb, ws, n_dev, stream);
}
static int mm_row_normalize(const float* x, int R, float* xhat, float* inv, int n_cap, const int32_t* n_dev, void* stream) {
    ERC_REQUIRE(x && xhat && inv && R > 0, "mm_row_normalize: bad arguments");
    LAUNCH_CAP(row_normalize_kernel, n_dev, NODEG(R), x, R, xhat, inv, n_cap, n_dev);
    ERC_LAUNCH_CHECK("mm_row_normalize");
    return ERC_OK;
}
extern "C" int erc_mm_row_normalize(const float* x, int R, float* xhat, float* inv, void* stream) {
    return mm_row_normalize(x, R, xhat, inv, 1, nullptr, stream);
}
extern "C" int erc_mm_row_normalize_cap(const float* x, int n_mod, int n_cap, const int32_t* n_dev, float* xhat, float* inv,
                                        void* stream) {
    ERC_REQUIRE(n_dev && n_mod > 0 && n_cap > 0, "mm_row_normalize_cap: bad arguments");
    return mm_row_normalize(x, n_mod * n_cap, xhat, inv, n_cap, n_dev, stream);
}
static int mm_row_normalize_bwd(const float* xhat, const float* inv, const float* dxhat, int R, float* dx, int n_cap,
                                const int32_t* n_dev, void* stream) {
    ERC_REQUIRE(xhat && inv && dxhat && dx && R > 0, "mm_row_normalize_bwd: bad arguments");
    LAUNCH_CAP(row_normalize_bwd_kernel, n_dev, NODEG(R), xhat, inv, dxhat, R, dx, n_cap, n_dev);
    ERC_LAUNCH_CHECK("mm_row_normalize_bwd");
    return ERC_OK;
}
extern "C" int erc_mm_row_normalize_bwd(const float* xhat, const float* inv, const float* dxhat, int R, float* dx,
                                        void* stream) {
    return mm_row_normalize_bwd(xhat, inv, dxhat, R, dx, 1, nullptr, stream);
}
extern "C" int erc_mm_row_normalize_bwd_cap(const float* xhat, const float* inv, const float* dxhat, int n_mod, int n_cap,
                                            const int32_t* n_dev, float* dx, void* stream) {
    ERC_REQUIRE(n_dev && n_mod > 0 && n_cap > 0, "mm_row_normalize_bwd_cap: bad arguments");
    return mm_row_normalize_bwd(xhat, inv, dxhat, n_mod * n_cap, dx, n_cap, n_dev, stream);
}
extern "C" int erc_mm_adj_finish(const float* COS, const float* xhat, const int32_t* node_off, int B, int M, int N, int P,
                                 float* ADJ, float* CR, float* CCOS, float* DEG, void* stream) {
    ERC_REQUIRE(COS && xhat && node_off && ADJ && CR && CCOS && DEG, "mm_adj_finish: null pointer");
    ERC_REQUIRE(B > 0 && M >= 2 && M <= 3 && N > 0 && P > 0 && P <= MAXP, "mm_adj_finish: M=%d P=%d unsupported", M, P);
    const dim3 grid(erc_cdiv(M * P, 4), B);
    hipLaunchKernelGGL(adj_rows_kernel, grid, dim3(256), 0, (hipStream_t)stream, COS, xhat, node_off, M, N, P, ADJ, CCOS, DEG);
    ERC_LAUNCH_CHECK("mm_adj_rows");
    hipLaunchKernelGGL(adj_scale_kernel, grid, dim3(256), 0, (hipStream_t)stream, CCOS, DEG, node_off, M, N, P, ADJ, CR);
    ERC_LAUNCH_CHECK("mm_adj_scale");
    return ERC_OK;
}
extern "C" int erc_mm_adj_finish_bwd(const float* COS, const float* CCOS, const float* DEG, const float* dADJ,
                                     const float* dCR, const int32_t* node_off, int B, int M, int N, int P, float* G,
                                     float* GC, float* DD, void* stream) {
    ERC_REQUIRE(COS && CCOS && DEG && dADJ && dCR && node_off && G && GC && DD, "mm_adj_finish_bwd: null pointer");
    ERC_REQUIRE(B > 0 && M >= 2 && M <= 3 && N > 0 && P > 0 && P <= MAXP, "mm_adj_finish_bwd: bad sizes");
    const dim3 grid(erc_cdiv(M * P, 4), B);
    hipLaunchKernelGGL(adj_bwd_rows_kernel, grid, dim3(256), 0, (hipStream_t)stream, COS, CCOS, DEG, dADJ, dCR, node_off, M,
                       N, P, DD);
    ERC_LAUNCH_CHECK("mm_adj_bwd_rows");
    hipLaunchKernelGGL(adj_bwd_entries_kernel, grid, dim3(256), 0, (hipStream_t)stream, COS, CCOS, DEG, DD, dADJ, dCR,
                       node_off, M, N, P, G, GC);
    ERC_LAUNCH_CHECK("mm_adj_bwd_entries");
    return ERC_OK;
}
static int mm_cross_apply(const float* CR, const float* h, int ldh, const int32_t* node_dlg, const int32_t* node_off, int M, int N,
                          int P, float* out, int ldo, const int32_t* n_dev, void* stream) {
    ERC_REQUIRE(CR && h && node_dlg && node_off && out && M >= 2 && N > 0, "mm_cross_apply: bad arguments");
    LAUNCH_CAP(cross_apply_kernel, n_dev, NODEG(M * N), CR, h, ldh, node_dlg, node_off, M, N, P, out, ldo, n_dev);
    ERC_LAUNCH_CHECK("mm_cross_apply");
    return ERC_OK;
}
extern "C" int erc_mm_cross_apply(const float* CR, const float* h, int ldh, const int32_t* node_dlg, const int32_t* node_off,
                                  int M, int N, int P, float* out, int ldo, void* stream) {
    return mm_cross_apply(CR, h, ldh, node_dlg, node_off, M, N, P, out, ldo, nullptr, stream);
}
extern "C" int erc_mm_cross_apply_cap(const float* CR, const float* h, int ldh, const int32_t* node_dlg, const int32_t* node_off,
                                      int M, int n_cap, const int32_t* n_dev, int P, float* out, int ldo, void* stream) {
    ERC_REQUIRE(n_dev, "mm_cross_apply_cap: n_dev is NULL");
    return mm_cross_apply(CR, h, ldh, node_dlg, node_off, M, n_cap, P, out, ldo, n_dev, stream);
}
static int mm_cross_grad(const float* dhi, int ldd, const float* h, int ldh, const int32_t* node_dlg, const int32_t* node_off, int M,
                         int N, int P, float* dCR, int planes, int64_t d_plane, int64_t h_plane, const int32_t* n_dev,
                         void* stream) {
    ERC_REQUIRE(dhi && h && node_dlg && node_off && dCR && M >= 2 && N > 0 && planes >= 1, "mm_cross_grad: bad arguments");
    LAUNCH_CAP(cross_grad_kernel, n_dev, NODEG(M * N), dhi, ldd, h, ldh, node_dlg, node_off, M, N, P, dCR, planes, d_plane, h_plane,
               n_dev);
    ERC_LAUNCH_CHECK("mm_cross_grad");
    return ERC_OK;
}
extern "C" int erc_mm_cross_grad(const float* dhi, int ldd, const float* h, int ldh, const int32_t* node_dlg,
                                 const int32_t* node_off, int M, int N, int P, float* dCR, int planes, int64_t d_plane,
                                 int64_t h_plane, void* stream) {
    return mm_cross_grad(dhi, ldd, h, ldh, node_dlg, node_off, M, N, P, dCR, planes, d_plane, h_plane, nullptr, stream);
}
extern "C" int erc_mm_cross_grad_cap(const float* dhi, int ldd, const float* h, int ldh, const int32_t* node_dlg,
                                     const int32_t* node_off, int M, int n_cap, const int32_t* n_dev, int P, float* dCR, int planes,
                                     int64_t d_plane, int64_t h_plane, void* stream) {
    ERC_REQUIRE(n_dev, "mm_cross_grad_cap: n_dev is NULL");
    return mm_cross_grad(dhi, ldd, h, ldh, node_dlg, node_off, M, n_cap, P, dCR, planes, d_plane, h_plane, n_dev, stream);
}
extern "C" int erc_gcnii_combine_fwd(const float* G, const float* hi, const float* h0, int64_t n, float theta, float alpha,
                                     float drop_p, const uint64_t* rng_state, uint64_t rng_stream, float* hd,
                                     void* stream) {
    ERC_REQUIRE(G && hd && n > 0 && (!hi || h0) && (drop_p <= 0.f || rng_state), "gcnii_combine_fwd: bad arguments");
    hipLaunchKernelGGL(gcnii_combine_fwd_kernel, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, G, hi, h0, n, theta,
                       alpha, drop_p, rng_state, rng_stream, hd);
    ERC_LAUNCH_CHECK("gcnii_combine_fwd");
    return ERC_OK;
}
static int gcnii_combine_bwd(const float* d_hd, const float* hd, int64_t n, float theta, float alpha, float keep_scale, int plain,
                             float* dG, float* dhi, float* dh0, int F, int ld_d, int n_cap, const int32_t* n_dev, void* stream) {
    ERC_REQUIRE(d_hd && hd && dG && n > 0 && (plain || (dhi && dh0 && F > 0 && ld_d >= F)), "gcnii_combine_bwd: bad arguments");
    LAUNCH_CAP(gcnii_combine_bwd_kernel, n_dev, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, d_hd, hd, n, theta, alpha,
               keep_scale, plain, dG, dhi, dh0, F > 0 ? F : 1, ld_d, n_cap, n_dev);
    ERC_LAUNCH_CHECK("gcnii_combine_bwd");
    return ERC_OK;
}
extern "C" int erc_gcnii_combine_bwd(const float* d_hd, const float* hd, int64_t n, float theta, float alpha,
                                     float keep_scale, int plain, float* dG, float* dhi, float* dh0, int F, int ld_d,
                                     void* stream) {
    return gcnii_combine_bwd(d_hd, hd, n, theta, alpha, keep_scale, plain, dG, dhi, dh0, F, ld_d, 1, nullptr, stream);
}
extern "C" int erc_gcnii_combine_bwd_cap(const float* d_hd, const float* hd, int n_mod, int n_cap, const int32_t* n_dev, float theta,
                                         float alpha, float keep_scale, int plain, float* dG, float* dhi, float* dh0, int F,
                                         int ld_d, void* stream) {
    ERC_REQUIRE(n_dev && n_mod > 0 && n_cap > 0 && F > 0, "gcnii_combine_bwd_cap: bad arguments");
    return gcnii_combine_bwd(d_hd, hd, (int64_t)n_mod * n_cap * F, theta, alpha, keep_scale, plain, dG, dhi, dh0, F, ld_d, n_cap,
                             n_dev, stream);
}
static int dropout_fwd(const float* x, int64_t n, float drop_p, const uint64_t* rng_state, uint64_t rng_stream, float* y, int row_w,
                       int n_cap, const int32_t* n_dev, void* stream) {
    ERC_REQUIRE(x && y && rng_state && n > 0 && drop_p > 0.f && drop_p < 1.f, "dropout_fwd: bad arguments");
    LAUNCH_CAP(dropout_kernel, n_dev, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, x, n, drop_p, rng_state, rng_stream, y,
               row_w, n_cap, n_dev);
    ERC_LAUNCH_CHECK("dropout_fwd");
    return ERC_OK;
}
extern "C" int erc_dropout_fwd(const float* x, int64_t n, float drop_p, const uint64_t* rng_state, uint64_t rng_stream,
                               float* y, void* stream) {
    return dropout_fwd(x, n, drop_p, rng_state, rng_stream, y, 1, 1, nullptr, stream);
}
extern "C" int erc_dropout_fwd_cap(const float* x, int n_mod, int n_cap, const int32_t* n_dev, int row_w, float drop_p,
                                   const uint64_t* rng_state, uint64_t rng_stream, float* y, void* stream) {
    ERC_REQUIRE(n_dev && n_mod > 0 && n_cap > 0 && row_w > 0, "dropout_fwd_cap: bad arguments");
    return dropout_fwd(x, (int64_t)n_mod * n_cap * row_w, drop_p, rng_state, rng_stream, y, row_w, n_cap, n_dev, stream);
}
static int mm_regroup_fwd(const float* xd, const float* hl, int M, int N, float drop_p, const uint64_t* rng_state,
                          uint64_t rng_stream, float* FE, const int32_t* n_dev, void* stream) {
    ERC_REQUIRE(xd && hl && FE && M >= 2 && N > 0 && (drop_p <= 0.f || rng_state), "mm_regroup_fwd: bad arguments");
    LAUNCH_CAP(regroup_fwd_kernel, n_dev, dim3(ew_grid((int64_t)N * M * 2 * FD)), dim3(256), 0, (hipStream_t)stream, xd, hl, M, N,
               drop_p, rng_state, rng_stream, FE, n_dev);
    ERC_LAUNCH_CHECK("mm_regroup_fwd");
    return ERC_OK;
}
extern "C" int erc_mm_regroup_fwd(const float* xd, const float* hl, int M, int N, float drop_p, const uint64_t* rng_state,
                                  uint64_t rng_stream, float* FE, void* stream) {
    return mm_regroup_fwd(xd, hl, M, N, drop_p, rng_state, rng_stream, FE, nullptr, stream);
}
extern "C" int erc_mm_regroup_fwd_cap(const float* xd, const float* hl, int M, int n_cap, const int32_t* n_dev, float drop_p,
                                      const uint64_t* rng_state, uint64_t rng_stream, float* FE, void* stream) {
    ERC_REQUIRE(n_dev, "mm_regroup_fwd_cap: n_dev is NULL");
    return mm_regroup_fwd(xd, hl, M, n_cap, drop_p, rng_state, rng_stream, FE, n_dev, stream);
}
static int mm_regroup_bwd(const float* dFE, const float* FE, int M, int N, float keep_scale, float* d_xd, float* d_h,
                          const int32_t* n_dev, void* stream) {
    ERC_REQUIRE(dFE && FE && d_xd && d_h && M >= 2 && N > 0, "mm_regroup_bwd: bad arguments");
    LAUNCH_CAP(regroup_bwd_kernel, n_dev, dim3(ew_grid((int64_t)N * M * 2 * FD)), dim3(256), 0, (hipStream_t)stream, dFE, FE, M, N,
               keep_scale, d_xd, d_h, n_dev);
    ERC_LAUNCH_CHECK("mm_regroup_bwd");
    return ERC_OK;
}
extern "C" int erc_mm_regroup_bwd(const float* dFE, const float* FE, int M, int N, float keep_scale, float* d_xd, float* d_h,
                                  void* stream) {
    return mm_regroup_bwd(dFE, FE, M, N, keep_scale, d_xd, d_h, nullptr, stream);
}
extern "C" int erc_mm_regroup_bwd_cap(const float* dFE, const float* FE, int M, int n_cap, const int32_t* n_dev, float keep_scale,
                                      float* d_xd, float* d_h, void* stream) {
    ERC_REQUIRE(n_dev, "mm_regroup_bwd_cap: n_dev is NULL");
    return mm_regroup_bwd(dFE, FE, M, n_cap, keep_scale, d_xd, d_h, n_dev, stream);
}
static int axpy_mask(const float* x, const float* mask, int64_t n, float scale, int accumulate, float* y, int row_w, int n_cap,
                     const int32_t* n_dev, void* stream) {
    ERC_REQUIRE(x && y && n > 0, "axpy_mask: bad arguments");
    LAUNCH_CAP(axpy_mask_kernel, n_dev, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, x, mask, n, scale, accumulate, y, row_w,
               n_cap, n_dev);
    ERC_LAUNCH_CHECK("axpy_mask");
    return ERC_OK;
}
extern "C" int erc_axpy_mask(const float* x, const float* mask, int64_t n, float scale, int accumulate, float* y,
                             void* stream) {
    return axpy_mask(x, mask, n, scale, accumulate, y, 1, 1, nullptr, stream);
}
extern "C" int erc_axpy_mask_cap(const float* x, const float* mask, int n_mod, int n_cap, const int32_t* n_dev, int row_w, float scale,
                                 int accumulate, float* y, void* stream) {
    ERC_REQUIRE(n_dev && n_mod > 0 && n_cap > 0 && row_w > 0, "axpy_mask_cap: bad arguments");
    return axpy_mask(x, mask, (int64_t)n_mod * n_cap * row_w, scale, accumulate, y, row_w, n_cap, n_dev, stream);
}
extern "C" int erc_mm_zero_tail(float* buf, int64_t ld, int width, int n_mod, int n_cap, const int32_t* n_dev, void* stream) {
    ERC_REQUIRE(buf && n_dev && width > 0 && ld >= width && n_mod > 0 && n_cap > 0, "mm_zero_tail: bad arguments");
    // sized for the largest tail a step of this capacity can have; a full batch (n == n_cap) finds nothing to write
    hipLaunchKernelGGL(zero_tail_kernel, dim3(ew_grid((int64_t)n_mod * n_cap * width)), dim3(256), 0, (hipStream_t)stream, buf, ld,
                       width, n_mod, n_cap, n_dev);
    ERC_LAUNCH_CHECK("mm_zero_tail");
    return ERC_OK;
}

// Bidirectional GRU recurrence, hidden size 200 per direction -- the per-modality encoders of CIM
// (track_mm/cim.py:73-77,136-146: nn.GRU(d_m, 200, bidirectional=True) over packed sequences).  torch.nn.GRU semantics,
// gate order r|z|n:
//   r = sigm(gx_r + W_hr h + b_hr)   z = sigm(gx_z + W_hz h + b_hz)   n = tanh(gx_n + r (W_hn h + b_hn))
//   h' = (1 - z) n + z h,   h0 = 0,   the reverse direction of a dialogue starts at its own last valid step.
//
// One workgroup per (dialogue, direction, modality): all three modalities x both directions x all dialogues in ONE launch.
// The input-side pre-activations GX = x W_ih^T + b_ih are GEMMs over all rows before the scan (both directions: 1200
// columns per modality).  Rows are compact: row(b, t) = node_off[b] + t, the sum(lengths) valid positions.
//
// Layout of the recurrent matrix: W_hh of a direction is 600 x 200 fp32 = 480 KB -- as much as the register file of a whole
// CU (512 KB) and three times its LDS (160 KB), so it cannot stay resident in one workgroup the way lstm.hip keeps its 160 KB.
// It is streamed from L2 every step instead (the 6 matrices, 2.9 MB, stay L2 / MALL resident for the whole scan): the
// forward reads the TRANSPOSED copy W_hh^T [200, 600] (erc_transpose_batched, once per step of training), thread j < 600
// owns gate row j and walks k, so every load of a wavefront is 256 contiguous bytes; the backward needs W_hh^T g, for which
// the stored [600, 200] layout is already the coalesced one (thread = column k, 5 threads per column split the 600 rows).
//
// Capacity mode (B dialogue slots, `rows` a capacity): a slot of length 0 runs no step in either kernel, and both write only
// the rows node_off[b] + t, t < length -- rows at or beyond node_off[B] keep what they held.  The forward needs no other form;
// the backward's erc_gru_scan_bwd_cap also writes 0 into the tail rows of dGX / dGH, which enter weight-gradient products.
#include "erc_common.h"

namespace {

constexpr int H = 200;
constexpr int G3 = 600;
constexpr int FWD_THREADS = 640;
constexpr int BWD_THREADS = 1024;
constexpr int BWD_PARTS = 5;            // 5 x 200 threads, 120 gate rows each

struct GruP {
    const float* GX;      // [3][rows][1200]: modality stride rows*1200, direction d at columns [600d, 600d+600)
    const float* W;       // fwd: W_hh^T [6][200][600]; bwd: W_hh [6][600][200]; index 2m + d
    const float* b_hh;    // [6][600]
    const int64_t* lengths;
    const int32_t* node_off;
    int B, T;
    int64_t rows;
    float* Hout;          // [3][rows][400]   GRU output (pad_packed_sequence layout of the valid rows)
    float* Hdrop;         // [3][rows][400]   optional drop0-masked copy
    float drop_p; const uint64_t* rng; uint64_t rng_stream;
    float* gates;         // [3][rows][1200]  post-activation r|z|n per direction (saved)
    float* ghn;           // [3][rows][400]   W_hn h + b_hn                         (saved)
    float* Hprev;         // [3][rows][400]   h_{t-1} in scan order                 (saved)
    // backward
    const float* dH;      // [3][rows][400]   gradient wrt Hout (wrt Hdrop when drop_p > 0)
    float* dGX;           // [3][rows][1200]  gradient wrt the input-side pre-activations
    float* dGH;           // [3][rows][1200]  ... wrt the recurrent-side pre-activations (n block scaled by r)
    int64_t zero_to;      // erc_gru_scan_bwd_cap: rows [node_off[B], zero_to) of dGX / dGH are written 0 (0: none)
};

__device__ __forceinline__ bool kept(const GruP& p, int m, int64_t row, int d, int u, uint64_t off, uint64_t seed) {
    return erc_uniform(seed ^ (p.rng_stream + (uint64_t)m), off, (uint64_t)row * (2 * H) + d * H + u) >= p.drop_p;
}

__global__ __launch_bounds__(FWD_THREADS) void gru_fwd_kernel(GruP p) {
    const int b = blockIdx.x, d = blockIdx.y, m = blockIdx.z, tid = threadIdx.x;
    const int L = min((int)p.lengths[b], p.T);
    const int64_t base = p.node_off[b];
    __shared__ float s_h[H];
    __shared__ float s_gh[G3];
    const float* WT = p.W + (int64_t)(2 * m + d) * H * G3;
    const float bj = tid < G3 ? p.b_hh[(2 * m + d) * G3 + tid] : 0.f;
    const float* GX = p.GX + (int64_t)m * p.rows * 2 * G3 + d * G3;
    const int64_t mo = (int64_t)m * p.rows * 2 * H;
    const bool dropping = p.Hdrop && p.drop_p > 0.f;
    uint64_t roff = 0, rseed = 0;
    if (dropping) roff = p.rng[0], rseed = p.rng[1];
    const float keep_scale = dropping ? 1.0f / (1.0f - p.drop_p) : 1.0f;
    float hprev = 0.f;
    if (tid < H) s_h[tid] = 0.f;
    __syncthreads();
    for (int s = 0; s < L; ++s) {
        const int t = d == 0 ? s : L - 1 - s;
        const int64_t row = base + t;
        if (tid < G3) {
            float acc = bj;
            const float* w = WT + tid;
#pragma unroll 8
            for (int k = 0; k < H; ++k) acc = fmaf(w[(int64_t)k * G3], s_h[k], acc);
            s_gh[tid] = acc;
        }
        __syncthreads();
        if (tid < H) {
            const int u = tid;
            const float* gx = GX + row * 2 * G3;
            const float r = sigm(gx[u] + s_gh[u]);
            const float z = sigm(gx[H + u] + s_gh[H + u]);
            const float gn = s_gh[2 * H + u];
            const float n = tanhf(gx[2 * H + u] + r * gn);
            const float h = (1.f - z) * n + z * hprev;
            float* g = p.gates + (int64_t)m * p.rows * 2 * G3 + row * 2 * G3 + d * G3;
            g[u] = r, g[H + u] = z, g[2 * H + u] = n;
            const int64_t o = mo + row * 2 * H + d * H + u;
            p.ghn[o] = gn;
            p.Hprev[o] = hprev;
            p.Hout[o] = h;
            if (p.Hdrop) p.Hdrop[o] = dropping ? (kept(p, m, row, d, u, roff, rseed) ? h * keep_scale : 0.f) : h;
            hprev = h;
            s_h[u] = h;       // every reader of the old h passed the barrier above
        }
        __syncthreads();
    }
}

// ZERO_TAIL (zero_to > 0): its own instance, so that the exact-shape launch keeps the code it always had
template <bool ZERO_TAIL>
__global__ __launch_bounds__(BWD_THREADS) void gru_bwd_kernel(GruP p) {
    const int b = blockIdx.x, d = blockIdx.y, m = blockIdx.z, tid = threadIdx.x;
    const int L = min((int)p.lengths[b], p.T);
    const int64_t base = p.node_off[b];
    __shared__ float s_dg[G3];
    __shared__ float s_part[BWD_PARTS][H];
    const float* W = p.W + (int64_t)(2 * m + d) * G3 * H;
    const int64_t mo = (int64_t)m * p.rows * 2 * H, mg = (int64_t)m * p.rows * 2 * G3;
    const bool dropped = p.drop_p > 0.f;
    uint64_t roff = 0, rseed = 0;
    if (dropped) roff = p.rng[0], rseed = p.rng[1];
    const float keep_scale = dropped ? 1.0f / (1.0f - p.drop_p) : 1.0f;
    const int kcol = tid % H, part = tid / H;
    // capacity mode: the tail rows [n, zero_to) no dialogue owns, this (direction, modality)'s 600 columns of them dealt out
    // over the B workgroups -- the weight-gradient products then run over zero_to rows whatever an earlier batch left there
    if (ZERO_TAIL && tid < G3)
        for (int64_t r = max(p.node_off[p.B], 0) + b; r < p.zero_to; r += p.B) {
            p.dGX[mg + r * 2 * G3 + d * G3 + tid] = 0.f;
            p.dGH[mg + r * 2 * G3 + d * G3 + tid] = 0.f;
        }
    float dh_rec = 0.f, dh_direct = 0.f;
    for (int s = L - 1; s >= 0; --s) {
        const int t = d == 0 ? s : L - 1 - s;
        const int64_t row = base + t;
        if (tid < H) {
            const int u = tid;
            const int64_t o = mo + row * 2 * H + d * H + u;
            float g = p.dH[o];
            if (dropped) g = kept(p, m, row, d, u, roff, rseed) ? g * keep_scale : 0.f;
            const float dh = g + dh_rec;
            const float* gt = p.gates + mg + row * 2 * G3 + d * G3;
            const float r = gt[u], z = gt[H + u], n = gt[2 * H + u];
            const float hp = p.Hprev[o], gn = p.ghn[o];
            const float dnp = dh * (1.f - z) * (1.f - n * n);
            const float dzp = dh * (hp - n) * z * (1.f - z);
            const float drp = dnp * gn * r * (1.f - r);
            float* dx = p.dGX + mg + row * 2 * G3 + d * G3;
            float* dg = p.dGH + mg + row * 2 * G3 + d * G3;
            dx[u] = drp, dx[H + u] = dzp, dx[2 * H + u] = dnp;
            dg[u] = drp, dg[H + u] = dzp, dg[2 * H + u] = dnp * r;
            s_dg[u] = drp, s_dg[H + u] = dzp, s_dg[2 * H + u] = dnp * r;
            dh_direct = dh * z;
        }
        __syncthreads();
        if (part < BWD_PARTS) {
            float acc = 0.f;
            const int j0 = part * (G3 / BWD_PARTS);
            const float* w = W + (int64_t)j0 * H + kcol;
#pragma unroll 8
            for (int j = 0; j < G3 / BWD_PARTS; ++j) acc = fmaf(w[(int64_t)j * H], s_dg[j0 + j], acc);
            s_part[part][kcol] = acc;
        }
        __syncthreads();
        if (tid < H) {
            float acc = s_part[0][tid];
#pragma unroll
            for (int q = 1; q < BWD_PARTS; ++q) acc += s_part[q][tid];
            dh_rec = dh_direct + acc;
        }
        // s_dg / s_part are next written after the next step's first barrier: no third barrier needed
    }
}

GruP common(const int64_t* lengths, const int32_t* node_off, int B, int T, int64_t rows) {
    GruP p{};
    p.lengths = lengths; p.node_off = node_off; p.B = B; p.T = T; p.rows = rows;
    return p;
}

}  // namespace

extern "C" int erc_gru_scan_fwd(const float* GX, const float* W_hhT, const float* b_hh, const int64_t* lengths,
                                const int32_t* node_off, int B, int T, int64_t rows, float* Hout, float* Hdrop,
                                float drop_p, const uint64_t* rng_state, uint64_t rng_stream, float* gates, float* ghn,
                                float* Hprev, void* stream) {
    ERC_REQUIRE(GX && W_hhT && b_hh && lengths && node_off && Hout && gates && ghn && Hprev, "gru_scan_fwd: null pointer");
    ERC_REQUIRE(B > 0 && T > 0 && rows > 0, "gru_scan_fwd: bad sizes B=%d T=%d rows=%lld", B, T, (long long)rows);
    ERC_REQUIRE(!(Hdrop && drop_p > 0.f) || rng_state, "gru_scan_fwd: dropout needs rng_state");
    ERC_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "gru_scan_fwd: drop_p %f", drop_p);
    GruP p = common(lengths, node_off, B, T, rows);
    p.GX = GX; p.W = W_hhT; p.b_hh = b_hh; p.Hout = Hout; p.Hdrop = Hdrop; p.drop_p = drop_p; p.rng = rng_state;
    p.rng_stream = rng_stream; p.gates = gates; p.ghn = ghn; p.Hprev = Hprev;
    hipLaunchKernelGGL(gru_fwd_kernel, dim3(B, 2, 3), dim3(FWD_THREADS), 0, (hipStream_t)stream, p);
    ERC_LAUNCH_CHECK("gru_scan_fwd");
    return ERC_OK;
}

extern "C" int erc_gru_scan_bwd_cap(const float* W_hh, const int64_t* lengths, const int32_t* node_off, int B, int T,
                                    int64_t rows, const float* gates, const float* ghn, const float* Hprev, const float* dH,
                                    float drop_p, const uint64_t* rng_state, uint64_t rng_stream, float* dGX, float* dGH,
                                    int64_t zero_to, void* stream) {
    ERC_REQUIRE(W_hh && lengths && node_off && gates && ghn && Hprev && dH && dGX && dGH, "gru_scan_bwd: null pointer");
    ERC_REQUIRE(B > 0 && T > 0 && rows > 0, "gru_scan_bwd: bad sizes B=%d T=%d rows=%lld", B, T, (long long)rows);
    ERC_REQUIRE(zero_to >= 0 && zero_to <= rows, "gru_scan_bwd: zero_to %lld outside [0, rows=%lld]", (long long)zero_to,
                (long long)rows);
    ERC_REQUIRE(drop_p <= 0.f || rng_state, "gru_scan_bwd: dropout needs rng_state");
    ERC_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "gru_scan_bwd: drop_p %f", drop_p);
    GruP p = common(lengths, node_off, B, T, rows);
    p.W = W_hh; p.gates = const_cast<float*>(gates); p.ghn = const_cast<float*>(ghn); p.Hprev = const_cast<float*>(Hprev);
    p.dH = dH; p.drop_p = drop_p; p.rng = rng_state; p.rng_stream = rng_stream; p.dGX = dGX; p.dGH = dGH;
    p.zero_to = zero_to;
    if (zero_to > 0)
        hipLaunchKernelGGL(gru_bwd_kernel<true>, dim3(B, 2, 3), dim3(BWD_THREADS), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(gru_bwd_kernel<false>, dim3(B, 2, 3), dim3(BWD_THREADS), 0, (hipStream_t)stream, p);
    ERC_LAUNCH_CHECK("gru_scan_bwd");
    return ERC_OK;
}

extern "C" int erc_gru_scan_bwd(const float* W_hh, const int64_t* lengths, const int32_t* node_off, int B, int T,
                                int64_t rows, const float* gates, const float* ghn, const float* Hprev, const float* dH,
                                float drop_p, const uint64_t* rng_state, uint64_t rng_stream, float* dGX, float* dGH,
                                void* stream) {
    return erc_gru_scan_bwd_cap(W_hh, lengths, node_off, B, T, rows, gates, ghn, Hprev, dH, drop_p, rng_state, rng_stream, dGX,
                                dGH, 0, stream);
}

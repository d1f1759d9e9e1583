// (Bi)GRU recurrence, hidden size 100 per direction -- the sequence encoder of conv-emotion's bc-GRU baseline (GRUModel,
// track_mm/dgcnv2_models.py:350-386: nn.GRU(D_m, 100, num_layers=2, bidirectional=True), unpacked over the padded length).
// torch.nn.GRU semantics, gate order r|z|n, h0 = 0:
//   r = sigm(gx_r + W_hr h + b_hr)   z = sigm(gx_z + W_hz h + b_hz)   n = tanh(gx_n + r (W_hn h + b_hn))   h' = (1 - z) n + z h
//
// The weight-stationary sibling of lstm.hip (csrc/gru.hip is CIM's hidden-200 scan, whose 480 KB W_hh are streamed from L2):
// one workgroup per (dialogue, direction); the input-side pre-activations GX = x W_ih^T + b_ih are one hoisted GEMM over all
// rows (both directions: 600 columns); the direction's W_hh [300,100] (120 KB) lives in REGISTERS for the whole scan, h_{t-1}
// is broadcast from LDS, so a step is LDS + ALU only and global memory is touched once per SC steps: the GX rows of a chunk
// are requested one chunk ahead, the chunk's results leave at its end.  The backward scan keeps the transposed slices in
// registers the same way and leaves all weight gradients to GEMMs over the gate gradients it writes (dGX, dGH) and the saved
// h_{t-1}.  Every output element is produced by one thread in a fixed order (no atomics); no workgroup waits for another.
// What it shares with lstm.hip -- row maps, step counts, the chunked LDS layout, DPP moves, activations, the dropout
// uniform -- is csrc/rnn100_dev.h.
#include "rnn100_dev.h"

namespace {
using namespace rnn100;

constexpr int G3 = 300;
constexpr int DGP = 12 * CHP;      // recurrent gate gradients in LDS (rnn100_dev.h: chunks of 25 padded to 28)

// barrier that orders LDS traffic only: __syncthreads() fences global memory too, and so would wait for the chunk's loads
// and stores in flight at every step.  In builtins (the workgroup fence on the local address space around s_barrier), not
// erc_common.h's lds_barrier(): that asm statement's memory clobber makes the compiler schedule the forward kernel differently
__device__ __forceinline__ void lds_fence_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

struct GruP {
    const float* GX; int ldgx;           // hoisted pre-activations, direction d at columns [300d, 300d+300)
    const float* W_hh;                   // [2][300,100]  (forward, reverse)
    const float* b_hh;                   // [2][300]
    const int64_t* lengths;              // [B] or null: T for every dialogue (unpacked run), or node_off[b+1] - node_off[b] with compact rows
    const int32_t* node_off;             // null: row(b,t) = b*sb + t*st ; else compact rows node_off[b] + t
    int64_t sb, st;
    int B, T;
    float* Hout; int ldh;                // outputs, direction d at columns [100d, 100d+100); rows as above
    float* Hdrop; int ldhd;              // optional copy with inverted dropout applied (input of the next layer)
    float drop_p; const uint64_t* rng;   // rng[0] = offset, rng[1] = seed
    uint64_t rng_stream;                 // distinguishes the layers' masks
    float* gates;                        // [rows,600] post-activation r|z|n per direction   (saved)
    float* ghn;                          // [rows,200] W_hn h + b_hn                          (saved)
    float* Hprev;                        // [rows,200] h_{t-1} in scan order                  (saved)
    // backward only
    const float* dHout; int lddh;        // gradient wrt Hout (or wrt Hdrop when drop_p > 0)
    float* dGX;                          // [rows,600] gradient wrt the input-side pre-activations (0 on padded rows)
    float* dGH;                          // [rows,600] the recurrent side: the n block scaled by r  (0 on padded rows)
    const int32_t* t_dev;                // *_tcap entry points (padded rows, unpacked): every dialogue runs *t_dev <= T steps
};

// Thread layout of both scans: quad u = tid / 4 (< 100 live) owns hidden unit u.  Forward: lane q of the quad multiplies the
// unit's THREE gate rows by h[25q .. 25q+25) (75 weights in registers, 25 LDS values a step), the quad sums by DPP and every
// lane of it evaluates the cell (the same bits in the four lanes); lane q < 3 owns column q*100 + u of GX / gates.
template <bool TDEV>
__global__ __launch_bounds__(NTH) void gru100_fwd_kernel(GruP p) {
    const int b = blockIdx.x, d = blockIdx.y, tid = threadIdx.x;
    const int L = steps_of<TDEV>(p, b);
    const RowMap rmap = rows_of(p, b);
    __shared__ __attribute__((aligned(16))) float s_h[2][HP];
    const int u = tid >> 2, q = tid & 3;
    const bool live = u < H;
    const int uc = min(u, H - 1), qc = min(q, 2);
    const int gcol = d * G3 + qc * H + uc;
    f2 wrz[CHK];
    float wn[CHK];
    {
        const float* src = p.W_hh + ((int64_t)d * G3 + uc) * H + q * CHK;
#pragma unroll
        for (int i = 0; i < CHK; ++i) {
            wrz[i] = f2{src[i], src[H * H + i]};
            wn[i] = src[2 * H * H + i];
        }
    }
    const float bq = q < 2 ? p.b_hh[d * G3 + q * H + uc] : 0.f;      // b_hr | b_hz join the lane's GX value
    const float bhn = p.b_hh[d * G3 + 2 * H + uc];                   // b_hn stays inside r * (W_hn h + b_hn)
    if (tid < HP) s_h[0][tid] = 0.f, s_h[1][tid] = 0.f;
    uint64_t roff = 0, rseed = 0;
    const bool dropping = p.Hdrop && p.drop_p > 0.f;
    if (dropping) roff = p.rng[0], rseed = p.rng[1] ^ p.rng_stream;
    const float keep_scale = p.drop_p > 0.f ? 1.0f / (1.0f - p.drop_p) : 1.0f;
    float hprev = 0.f;
    __syncthreads();
    // row of scan step s = row_first + s * dstep (the reverse direction starts at L - 1)
    const int64_t dstep = d == 0 ? rmap.step : -rmap.step;
    const int64_t row_first = rmap(d == 0 ? 0 : L - 1);
    // the unit's four per-step outputs, one per lane of the quad: h_{t-1} | W_hn h + b_hn | h | dropped h
    float* const obase = q == 0 ? p.Hprev : q == 1 ? p.ghn : q == 2 ? p.Hout : p.Hdrop;
    const int64_t opitch = q < 2 ? 2 * H : q == 2 ? p.ldh : p.ldhd;
    const bool ostore = live && (q < 3 || p.Hdrop);
    const bool gstore = live && q < 3;
    float gx_cur[SC], gx_nxt[SC], o_gate[SC], o_unit[SC];
    auto load_chunk = [&](int c0) {      // rows past the end of the dialogue are clamped to its last row
#pragma unroll
        for (int r = 0; r < SC; ++r)
            gx_nxt[r] = p.GX[(row_first + (int64_t)min(c0 + r, L - 1) * dstep) * p.ldgx + gcol];
    };
    auto store_chunk = [&](int c0) {
#pragma unroll
        for (int r = 0; r < SC; ++r) {
            if (c0 + r < L) {       // uniform
                const int64_t row = row_first + (int64_t)(c0 + r) * dstep;
                if (gstore) p.gates[row * (2 * G3) + gcol] = o_gate[r];
                float val = o_unit[r];
                if (dropping && q == 3) {
                    const float uu = drop_uniform(rseed, roff, row, d, uc);
                    val = uu >= p.drop_p ? val * keep_scale : 0.f;
                }
                if (ostore) obase[row * opitch + d * H + uc] = val;
            }
        }
    };
    if (L > 0) load_chunk(0);
    for (int s0 = 0; s0 < L; s0 += SC) {
        // chunk boundary: this chunk's operands, the previous chunk's results to memory, the next chunk's operands requested
#pragma unroll
        for (int r = 0; r < SC; ++r) gx_cur[r] = gx_nxt[r] + bq;
        if (s0 > 0) store_chunk(s0 - SC);
        if (s0 + SC < L) load_chunk(s0 + SC);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < SC; ++r) {
            const int s = s0 + r;
            if (s < L) {       // uniform
                const int cur = s & 1;
                const float* hv = s_h[cur] + q * CHP;
                // two accumulator sets (even / odd k): independent chains of multiply-adds
                f2 a01 = {0.f, 0.f}, c01 = {0.f, 0.f};
                float a2 = 0.f, c2 = 0.f;
#pragma unroll
                for (int i = 0; i < CHK; ++i) {
                    const float hk = hv[i];
                    if (i & 1) {
                        c01 = __builtin_elementwise_fma(wrz[i], f2{hk, hk}, c01);
                        c2 = __builtin_fmaf(wn[i], hk, c2);
                    } else {
                        a01 = __builtin_elementwise_fma(wrz[i], f2{hk, hk}, a01);
                        a2 = __builtin_fmaf(wn[i], hk, a2);
                    }
                }
                a01 += c01, a2 += c2;
                const float sr = quad_sum(a01.x), sz = quad_sum(a01.y), sn = quad_sum(a2);
                const float xq = gx_cur[r];
                const float gr = fast_sigm(quad_bcast<0>(xq) + sr);
                const float gz = fast_sigm(quad_bcast<1>(xq) + sz);
                const float hn = sn + bhn;
                const float gn = fast_tanh(quad_bcast<2>(xq) + gr * hn);
                const float h = gn + gz * (hprev - gn);
                o_gate[r] = q == 0 ? gr : q == 1 ? gz : gn;
                o_unit[r] = q == 0 ? hprev : q == 1 ? hn : h;      // lane 3: h, dropped when it is stored
                if (live && q == 0) s_h[cur ^ 1][chunk_pos(u)] = h;
                hprev = h;
                lds_fence_barrier();
            }
        }
    }
    if (L > 0) store_chunk((L - 1) / SC * SC);
    // padded positions: zero output (pad_packed_sequence) -- only meaningful for padded row addressing
    if (!p.node_off)
        for (int t = max(L, 0); t < p.T; ++t) {
            const int64_t row = rmap(t);
            if (tid < H) {
                p.Hout[row * p.ldh + d * H + tid] = 0.f;
                if (p.Hdrop) p.Hdrop[row * p.ldhd + d * H + tid] = 0.f;
            }
        }
}

// Backward: with dh = dHout_t + dh_rec (the gradient of h_t) and the saved r, z, n, hn = W_hn h + b_hn, h_{t-1}:
//   d pre_n = dh (1 - z)(1 - n^2)    d pre_z = dh (h_{t-1} - n) z (1 - z)    d pre_r = d pre_n hn r (1 - r)
//   dGX = d pre_r | d pre_z | d pre_n      dGH = d pre_r | d pre_z | d pre_n r      dh_rec' = dh z + W_hh^T dGH
// so everything but dh is known a chunk ahead: the dependent chain of a step is one add, one multiply, the recurrent product.
// The recurrent product (W_hh^T dGH)[u]: a DPP row of 16 lanes = 4 units; lane `part` < 12 of the row multiplies entries
// [25 part, 25 part + 25) of the 300 gate gradients into each of the row's 4 units (100 weights in registers, 25 LDS values a
// step; lanes 12 .. 15 hold zeros), the row sums by DPP in a fixed order.  The elementwise part keeps the quad layout.
template <bool TDEV>
__global__ __launch_bounds__(NTH) void gru100_bwd_kernel(GruP p) {
    const int b = blockIdx.x, d = blockIdx.y, tid = threadIdx.x;
    const int L = steps_of<TDEV>(p, b);
    const RowMap rmap = rows_of(p, b);
    __shared__ __attribute__((aligned(16))) float s_dp[2][DGP];
    const int u = tid >> 2, q = tid & 3;
    const bool live = u < H;
    const int uc = min(u, H - 1), qc = min(q, 2);
    const int part = tid & 15, pc = min(part, 11), u0 = min(tid >> 4, H / 4 - 1) * 4;
    f2 wt01[CHK], wt23[CHK];
#pragma unroll
    for (int i = 0; i < CHK; ++i) {
        const float* src = p.W_hh + ((int64_t)d * G3 + pc * CHK + i) * H + u0;
        const float m = part < 12 ? 1.f : 0.f;
        wt01[i] = f2{src[0] * m, src[1] * m};
        wt23[i] = f2{src[2] * m, src[3] * m};
    }
    const int myr = (tid >> 2) & 3;
    uint64_t roff = 0, rseed = 0;
    const bool dropped = p.drop_p > 0.f;
    if (dropped) roff = p.rng[0], rseed = p.rng[1] ^ p.rng_stream;
    const float keep_scale = dropped ? 1.0f / (1.0f - p.drop_p) : 1.0f;
    const int64_t dstep = d == 0 ? rmap.step : -rmap.step;       // row of scan step s = row_first + s * dstep
    const int64_t row_first = rmap(d == 0 ? 0 : L - 1);
    const int lane_h = d * H + uc, lane_g = d * G3 + qc * H + uc;
    // operands of a step: upstream gradient, h_{t-1}, and the lane's saved value r | z | n | hn (met through the quad)
    const float* const qbase = q < 3 ? p.gates : p.ghn;
    const int64_t qpitch = q < 3 ? 2 * G3 : 2 * H;
    const int qcol = q < 3 ? lane_g : lane_h;
    const bool gstore = live && q < 3;
    struct ChunkIn { float g[SC], gq[SC], hp[SC]; };       // steps s0, s0 - 1, ..
    auto load_chunk = [&](int s0, ChunkIn& X) {
#pragma unroll
        for (int r = 0; r < SC; ++r) {
            const int64_t row = row_first + (int64_t)max(s0 - r, 0) * dstep;     // uniform, clamped to the first step
            X.g[r] = p.dHout[row * p.lddh + lane_h];
            X.gq[r] = qbase[row * qpitch + qcol];
            X.hp[r] = p.Hprev[row * (2 * H) + lane_h];
        }
    };
    float o_x[SC], o_h[SC];
    auto store_chunk = [&](int s0) {
#pragma unroll
        for (int r = 0; r < SC; ++r) {
            const int s = s0 - r;
            if (s >= 0 && gstore) {
                const int64_t at = (row_first + (int64_t)s * dstep) * (2 * G3) + lane_g;
                p.dGX[at] = o_x[r];
                p.dGH[at] = o_h[r];
            }
        }
    };
    float dh_rec = 0.f;
    auto steps = [&](int s0, const ChunkIn& X) {
        float fX[SC], fH[SC], fZ[SC], fG[SC];
#pragma unroll
        for (int r = 0; r < SC; ++r) {
            const int s = max(s0 - r, 0);
            float g = X.g[r];
            if (dropped) {     // uniform
                const float uu = drop_uniform(rseed, roff, row_first + (int64_t)s * dstep, d, uc);
                g = uu >= p.drop_p ? g * keep_scale : 0.f;
            }
            const float gq = X.gq[r];
            const float gr = quad_bcast<0>(gq), gz = quad_bcast<1>(gq), gn = quad_bcast<2>(gq), hn = quad_bcast<3>(gq);
            const float kn = (1.f - gz) * (1.f - gn * gn);
            const float kz = (X.hp[r] - gn) * gz * (1.f - gz);
            const float kr = kn * hn * gr * (1.f - gr);
            fX[r] = q == 0 ? kr : q == 1 ? kz : kn;
            fH[r] = q == 2 ? kn * gr : fX[r];
            fZ[r] = gz;
            fG[r] = g;
        }
#pragma unroll
        for (int r = 0; r < SC; ++r) {
            const int s = s0 - r;
            if (s >= 0) {      // uniform
                const int buf = s & 1;
                const float dh = fG[r] + dh_rec;
                const float dp = dh * fH[r];
                o_x[r] = dh * fX[r];
                o_h[r] = dp;
                if (gstore) s_dp[buf][chunk_pos(q * H + u)] = dp;
                lds_fence_barrier();
                const float* dv = s_dp[buf] + pc * CHP;
                f2 a01 = {0.f, 0.f}, a23 = {0.f, 0.f};
#pragma unroll
                for (int i = 0; i < CHK; ++i) {
                    const f2 dk = {dv[i], dv[i]};
                    a01 = __builtin_elementwise_fma(wt01[i], dk, a01);
                    a23 = __builtin_elementwise_fma(wt23[i], dk, a23);
                }
                float acc[4] = {a01.x, a01.y, a23.x, a23.y};
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) acc[r4] = row16_sum(acc[r4]);
                dh_rec = (myr == 0 ? acc[0] : myr == 1 ? acc[1] : myr == 2 ? acc[2] : acc[3]) + dh * fZ[r];
            }
        }
    };
    ChunkIn inA, inB;
    if (L > 0) load_chunk(L - 1, inA);
    for (int s0 = L - 1; s0 >= 0; s0 -= 2 * SC) {
        __builtin_amdgcn_sched_barrier(0);
        if (s0 < L - 1) store_chunk(s0 + SC);
        __builtin_amdgcn_sched_barrier(0);
        if (s0 - SC >= 0) load_chunk(s0 - SC, inB);      // only requests that will be consumed
        __builtin_amdgcn_sched_barrier(0);
        steps(s0, inA);
        if (s0 - SC >= 0) {
            __builtin_amdgcn_sched_barrier(0);
            store_chunk(s0);
            __builtin_amdgcn_sched_barrier(0);
            if (s0 - 2 * SC >= 0) load_chunk(s0 - 2 * SC, inA);
            __builtin_amdgcn_sched_barrier(0);
            steps(s0 - SC, inB);
        }
    }
    if (L > 0) store_chunk(L - 1 - (L - 1) / SC * SC);
    if (!p.node_off)
        for (int t = max(L, 0); t < p.T; ++t) {
            const int64_t at = rmap(t) * (2 * G3) + d * G3 + tid;
            if (tid < G3) p.dGX[at] = 0.f, p.dGH[at] = 0.f;
        }
}

// the checks and the parameter fill of the forward / backward entry points; `name` is the entry point's, `tcap` its T-capacity
// form (t_dev instead of lengths / node_off)
int check_and_fill(const char* name, GruP& p, const float* GX, int ldgx, const float* W_hh, const float* b_hh,
                   const int64_t* lengths, const int32_t* node_off, int64_t sb, int64_t st, int B, int T, bool tcap,
                   const int32_t* t_dev, float* Hout, int ldh, float* Hdrop, int ldhd, float drop_p, const uint64_t* rng_state,
                   uint64_t rng_stream, float* gates, float* ghn, float* Hprev) {
    ERC_REQUIRE(GX && W_hh && b_hh && Hout && gates && ghn && Hprev && (t_dev || !tcap), "%s: null pointer", name);
    ERC_REQUIRE(B > 0 && T > 0 && ldgx >= 2 * G3 && ldh >= 2 * H, "%s: bad sizes B=%d T=%d ldgx=%d ldh=%d", name, B, T, ldgx, ldh);
    ERC_REQUIRE(!Hdrop || ldhd >= 2 * H, "%s: ldhd=%d < 200", name, ldhd);
    ERC_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "%s: drop_p=%g outside [0, 1)", name, (double)drop_p);
    ERC_REQUIRE(!(Hdrop && drop_p > 0.f) || rng_state, "%s: dropout needs rng_state", name);
    p.GX = GX; p.ldgx = ldgx; p.W_hh = W_hh; p.b_hh = b_hh; p.lengths = lengths; p.node_off = node_off;
    p.sb = sb; p.st = st; p.B = B; p.T = T; p.t_dev = t_dev; p.Hout = Hout; p.ldh = ldh; p.Hdrop = Hdrop; p.ldhd = ldhd;
    p.drop_p = drop_p; p.rng = rng_state; p.rng_stream = rng_stream; p.gates = gates; p.ghn = ghn; p.Hprev = Hprev;
    return ERC_OK;
}

int check_and_fill(const char* name, GruP& p, const float* W_hh, const int64_t* lengths, const int32_t* node_off, int64_t sb,
                   int64_t st, int B, int T, bool tcap, const int32_t* t_dev, const float* gates, const float* ghn,
                   const float* Hprev, const float* dHout, int lddh, float drop_p, const uint64_t* rng_state, uint64_t rng_stream,
                   float* dGX, float* dGH) {
    ERC_REQUIRE(W_hh && gates && ghn && Hprev && dHout && dGX && dGH && (t_dev || !tcap), "%s: null pointer", name);
    ERC_REQUIRE(B > 0 && T > 0 && lddh >= 2 * H, "%s: bad sizes B=%d T=%d lddh=%d", name, B, T, lddh);
    ERC_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "%s: drop_p=%g outside [0, 1)", name, (double)drop_p);
    ERC_REQUIRE(drop_p <= 0.f || rng_state, "%s: dropout needs rng_state", name);
    p.W_hh = W_hh; p.lengths = lengths; p.node_off = node_off; p.sb = sb; p.st = st; p.B = B; p.T = T; p.t_dev = t_dev;
    p.gates = const_cast<float*>(gates); p.ghn = const_cast<float*>(ghn); p.Hprev = const_cast<float*>(Hprev);
    p.dHout = dHout; p.lddh = lddh; p.drop_p = drop_p; p.rng = rng_state; p.rng_stream = rng_stream; p.dGX = dGX; p.dGH = dGH;
    return ERC_OK;
}

}  // namespace

extern "C" int erc_gru100_scan_fwd(const float* GX, int ldgx, const float* W_hh, const float* b_hh, const int64_t* lengths,
                                   const int32_t* node_off, int64_t sb, int64_t st, int B, int T, float* Hout, int ldh,
                                   float* Hdrop, int ldhd, float drop_p, const uint64_t* rng_state, uint64_t rng_stream,
                                   float* gates, float* ghn, float* Hprev, void* stream) {
    GruP p{};
    if (int e = check_and_fill("gru100_scan_fwd", p, GX, ldgx, W_hh, b_hh, lengths, node_off, sb, st, B, T, false, nullptr, Hout,
                               ldh, Hdrop, ldhd, drop_p, rng_state, rng_stream, gates, ghn, Hprev))
        return e;
    hipLaunchKernelGGL(gru100_fwd_kernel<false>, dim3(B, 2), dim3(NTH), 0, (hipStream_t)stream, p);
    ERC_LAUNCH_CHECK("gru100_scan_fwd");
    return ERC_OK;
}

extern "C" int erc_gru100_scan_bwd(const float* W_hh, const int64_t* lengths, const int32_t* node_off, int64_t sb, int64_t st,
                                   int B, int T, const float* gates, const float* ghn, const float* Hprev, const float* dHout,
                                   int lddh, float drop_p, const uint64_t* rng_state, uint64_t rng_stream, float* dGX,
                                   float* dGH, void* stream) {
    GruP p{};
    if (int e = check_and_fill("gru100_scan_bwd", p, W_hh, lengths, node_off, sb, st, B, T, false, nullptr, gates, ghn, Hprev,
                               dHout, lddh, drop_p, rng_state, rng_stream, dGX, dGH))
        return e;
    hipLaunchKernelGGL(gru100_bwd_kernel<false>, dim3(B, 2), dim3(NTH), 0, (hipStream_t)stream, p);
    ERC_LAUNCH_CHECK("gru100_scan_bwd");
    return ERC_OK;
}

// T capacity: the unpacked padded-row form (lengths = NULL, node_off = NULL) with the step count read from the device
extern "C" int erc_gru100_scan_fwd_tcap(const float* GX, int ldgx, const float* W_hh, const float* b_hh, int64_t sb, int64_t st,
                                        int B, int T, const int32_t* t_dev, float* Hout, int ldh, float* Hdrop, int ldhd,
                                        float drop_p, const uint64_t* rng_state, uint64_t rng_stream, float* gates, float* ghn,
                                        float* Hprev, void* stream) {
    GruP p{};
    if (int e = check_and_fill("gru100_scan_fwd_tcap", p, GX, ldgx, W_hh, b_hh, nullptr, nullptr, sb, st, B, T, true, t_dev, Hout,
                               ldh, Hdrop, ldhd, drop_p, rng_state, rng_stream, gates, ghn, Hprev))
        return e;
    hipLaunchKernelGGL(gru100_fwd_kernel<true>, dim3(B, 2), dim3(NTH), 0, (hipStream_t)stream, p);
    ERC_LAUNCH_CHECK("gru100_scan_fwd_tcap");
    return ERC_OK;
}

extern "C" int erc_gru100_scan_bwd_tcap(const float* W_hh, int64_t sb, int64_t st, int B, int T, const int32_t* t_dev,
                                        const float* gates, const float* ghn, const float* Hprev, const float* dHout, int lddh,
                                        float drop_p, const uint64_t* rng_state, uint64_t rng_stream, float* dGX, float* dGH,
                                        void* stream) {
    GruP p{};
    if (int e = check_and_fill("gru100_scan_bwd_tcap", p, W_hh, nullptr, nullptr, sb, st, B, T, true, t_dev, gates, ghn, Hprev,
                               dHout, lddh, drop_p, rng_state, rng_stream, dGX, dGH))
        return e;
    hipLaunchKernelGGL(gru100_bwd_kernel<true>, dim3(B, 2), dim3(NTH), 0, (hipStream_t)stream, p);
    ERC_LAUNCH_CHECK("gru100_scan_bwd_tcap");
    return ERC_OK;
}

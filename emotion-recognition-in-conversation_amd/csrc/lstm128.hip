// LSTM recurrence, hidden size 128, with a max-pool over time -- the audio and visual encoders of MMIN's full-modality base
// model (LSTMEncoder(d, 128, 'maxpool'), track_mm/mmin_models.py:43-95: one-layer unidirectional nn.LSTM(batch_first=True),
// gate order i|f|g|o, then F.max_pool1d over ALL T steps of the padded batch).
//
// One workgroup per (sample, encoder).  The two encoders of a step are independent and short (B workgroups each on a chip of
// 256 CUs), so they go in ONE launch through a table of up to erc_lstm128_max_jobs() jobs passed by value: blockIdx.y picks
// the job, and the step's scan time is the longer of the two sequences instead of their sum.
//
// The input-side gate pre-activations GX = x W_ih^T + b_ih are the caller's hoisted GEMM over all B*T rows (row b*T + t,
// 512 columns).  W_hh [512,128] lives in REGISTERS for the whole scan.  Thread layout (that of lstm.hip): quad u = tid / 4
// owns hidden unit u, lane q = tid % 4 of the quad activates gate q, and the quad splits K -- lane q multiplies the unit's
// FOUR gate rows by h[32q, 32q+32): 128 weights per thread as 64 packed pairs, 32 LDS values per step.  h_{t-1} is
// double-buffered in LDS (chunks of 32 padded to 36 floats: 16-byte rows, the four addresses of a wavefront read 4 banks
// apart), so a step has one barrier.  Global memory is touched once per SC steps (rnn100_dev.h: why).  Every sample runs all
// T steps: padding is the caller's zero rows of x, and padded steps take part in the maximum, as in the reference.  The
// running maximum and the FIRST step that attains it stay in registers.
//
// The backward scan routes dpool[b,u] to step arg[b,u], keeps W_hh^T slices in registers the same way (a DPP row of 16
// lanes = 4 units; lane `part` of the row multiplies gate gradients [32 part, 32 part + 32) into the row's 4 units) and
// writes dGX on every row; all weight gradients are the caller's GEMMs over dGX, x and Hprev.
//
// Capacity forms (erc_lstm128_pool_fwd_tcap / _bwd_tcap: one captured step for every batch of a bucket): the same kernels
// instantiated with MODE = Capacity read the batch's sample count and audio length from device memory; a job's B and T then
// size the launch and pitch the rows.  Per sample the code is the exact form's.
//
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), both modes alike: forward 202 VGPRs, backward 210
// VGPRs, no AGPRs, no scratch, no spills, occupancy 2 wavefronts per SIMD (= the 512 threads of one workgroup: up to 256
// registers per lane).
#include "rnn100_dev.h"

namespace {
using rnn100::fast_sigm;
using rnn100::fast_tanh;

constexpr int H = 128, G4 = 512, NTH = 512, MAX_JOBS = 2;
constexpr int SC = 8;              // steps between two visits of global memory
constexpr int KQ = 32, KP = 36;    // LDS chunks: 32 values padded to 36
__device__ __forceinline__ int chunk_pos(int k) { return (k / KQ) * KP + k % KQ; }

struct Jobs {
    ErcLstm128Job j[MAX_JOBS];
};

// T and B capacity (erc_lstm128_pool_*_tcap): the job's B and T size the launch and pitch the rows, counts = {B, Ta} of the
// batch is read on the device.  Job i runs counts[1] steps when bit i of dyn_mask is set (audio), its own T otherwise (visual).
struct Exact {
    static constexpr bool CAP = false;
};
struct Capacity {
    static constexpr bool CAP = true;
    const int32_t* counts;
    int dyn_mask;
    __device__ __forceinline__ int B(const ErcLstm128Job& p) const { return min(max(counts[0], 0), p.B); }
    __device__ __forceinline__ int T(const ErcLstm128Job& p) const {
        return (dyn_mask >> blockIdx.y) & 1 ? min(max(counts[1], 1), p.T) : p.T;
    }
};

// MODE = Exact: every sample runs the job's T steps.  MODE = Capacity: T steps of rows pitched p.T steps apart per sample; a
// slot the batch does not have pools to zero and writes nothing else.
template <class MODE>
__global__ __launch_bounds__(NTH) void lstm128_fwd_kernel(Jobs P, MODE mode) {
    const ErcLstm128Job& p = P.j[blockIdx.y];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= p.B) return;      // uniform: the grid is sized for the larger job
    int T = p.T;
    if constexpr (MODE::CAP) {
        if (b >= mode.B(p)) {  // uniform
            if (tid < H) p.pool[(int64_t)b * p.ldp + tid] = 0.f;
            return;
        }
        T = mode.T(p);
    }
    const int TP = p.T;
    __shared__ __attribute__((aligned(16))) float s_h[2][4 * KP];
    const int u = tid >> 2, q = tid & 3;
    const int gcol = q * H + u;       // the gate this thread activates: its column of GX / gates
    f2 w01[KQ], w23[KQ];
    {
        const float* src = p.W_hh + (int64_t)u * H + q * KQ;
#pragma unroll
        for (int i = 0; i < KQ; ++i) {
            w01[i] = f2{src[i], src[H * H + i]};
            w23[i] = f2{src[2 * H * H + i], src[3 * H * H + i]};
        }
    }
    const float bhh = p.b_hh[gcol];
    if (tid < 2 * 4 * KP) (&s_h[0][0])[tid] = 0.f;
    const float am = q == 2 ? 2.f : 1.f;       // tanh(a) = 2 sigm(2a) - 1: one exponential whatever the gate
    const bool odd = q & 1, hi = q & 2;
    float c = 0.f, hprev = 0.f, best = -2.f;    // |h| < 1
    int best_t = 0;
    __syncthreads();
    const int64_t row0 = (int64_t)b * TP;
    const float* const gx0 = p.GX + row0 * G4 + gcol;
    float* const gate0 = p.gates + row0 * G4 + gcol;
    // the unit's per-step outputs: lane 0 stores c, lane 1 h_{t-1}
    float* const unit0 = (q == 0 ? p.Cst : p.Hprev) + row0 * H + u;
    float gx_cur[SC], gx_nxt[SC], o_gate[SC], o_unit[SC];
    auto load_chunk = [&](int c0) {
#pragma unroll
        for (int r = 0; r < SC; ++r) gx_nxt[r] = gx0[(int64_t)min(c0 + r, T - 1) * G4];
    };
    auto store_chunk = [&](int c0) {
#pragma unroll
        for (int r = 0; r < SC; ++r)
            if (c0 + r < T) {       // uniform
                gate0[(int64_t)(c0 + r) * G4] = o_gate[r];
                if (q < 2) unit0[(int64_t)(c0 + r) * H] = o_unit[r];
            }
    };
    load_chunk(0);
    for (int s0 = 0; s0 < T; s0 += SC) {
#pragma unroll
        for (int r = 0; r < SC; ++r) gx_cur[r] = gx_nxt[r];
        if (s0 > 0) store_chunk(s0 - SC);
        if (s0 + SC < T) load_chunk(s0 + SC);
#pragma unroll
        for (int r = 0; r < SC; ++r) {
            const int s = s0 + r;
            if (s < T) {       // uniform
                const int cur = s & 1;
                const float* hv = s_h[cur] + q * KP;
                // two accumulator sets (even / odd k): four independent chains of packed multiply-adds
                f2 p01 = {0.f, 0.f}, p23 = {0.f, 0.f}, r01 = {0.f, 0.f}, r23 = {0.f, 0.f};
#pragma unroll
                for (int i = 0; i < KQ; ++i) {
                    const f2 hk = {hv[i], hv[i]};
                    if (i & 1) {
                        r01 = __builtin_elementwise_fma(w01[i], hk, r01);
                        r23 = __builtin_elementwise_fma(w23[i], hk, r23);
                    } else {
                        p01 = __builtin_elementwise_fma(w01[i], hk, p01);
                        p23 = __builtin_elementwise_fma(w23[i], hk, p23);
                    }
                }
                p01 += r01, p23 += r23;
                // quad transpose-reduce: lane q ends with gate q's sum over the four lanes
                const float k0 = odd ? p01.y : p01.x, g0 = odd ? p01.x : p01.y;
                const float k1 = odd ? p23.y : p23.x, g1 = odd ? p23.x : p23.y;
                const float e0 = k0 + dpp_mov<DPP_X1>(g0), e1 = k1 + dpp_mov<DPP_X1>(g1);
                const float a = gx_cur[r] + bhh + ((hi ? e1 : e0) + dpp_mov<DPP_X2>(hi ? e0 : e1));
                const float sg = fast_sigm(am * a);
                const float act = q == 2 ? 2.f * sg - 1.f : sg;
                const float gi = quad_bcast<0>(act), gf = quad_bcast<1>(act), gg = quad_bcast<2>(act), go = quad_bcast<3>(act);
                c = gf * c + gi * gg;
                const float h = go * fast_tanh(c);
                o_gate[r] = act;
                o_unit[r] = q == 0 ? c : hprev;
                if (h > best) best = h, best_t = s;      // strict: the first step that attains the maximum
                if (q == 0) s_h[cur ^ 1][chunk_pos(u)] = h;
                hprev = h;
                lds_barrier();
            }
        }
    }
    store_chunk((T - 1) / SC * SC);
    if (q == 0) {
        p.pool[(int64_t)b * p.ldp + u] = best;
        p.arg[(int64_t)b * H + u] = best_t;
    }
}

// MODE = Capacity: dGX rows the scan does not reach (t >= T, and every row of a slot the batch does not have) are written
// zero, 16 bytes a store (a dGX row is 2048 bytes), before the scan starts: the weight-gradient products over all B * T rows
// then add exact zeros.
template <class MODE>
__global__ __launch_bounds__(NTH) void lstm128_bwd_kernel(Jobs P, MODE mode) {
    const ErcLstm128Job& p = P.j[blockIdx.y];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= p.B) return;      // uniform
    int T = p.T;
    if constexpr (MODE::CAP) {
        T = b >= mode.B(p) ? 0 : mode.T(p);
        f4* const tail = reinterpret_cast<f4*>(p.dGX + ((int64_t)b * p.T + T) * G4);
        const int n4 = (p.T - T) * (G4 / 4);
        for (int i = tid; i < n4; i += NTH) tail[i] = f4{0.f, 0.f, 0.f, 0.f};
        if (T == 0) return;    // uniform
    }
    const int TP = p.T;
    __shared__ __attribute__((aligned(16))) float s_dp[2][16 * KP];     // gate gradients of the step, entry q*H + u chunked
    const int u = tid >> 2, q = tid & 3;
    const int part = tid & 15, u0 = (tid >> 4) * 4, myr = (tid >> 2) & 3;
    f2 wt01[KQ], wt23[KQ];
#pragma unroll
    for (int i = 0; i < KQ; ++i) {
        const float* src = p.W_hh + (int64_t)(part * KQ + i) * H + u0;
        wt01[i] = f2{src[0], src[1]};
        wt23[i] = f2{src[2], src[3]};
    }
    const int gcol = q * H + u;
    const int64_t row0 = (int64_t)b * TP;
    const float* const gate0 = p.gates + row0 * G4 + gcol;
    const float* const c0p = p.Cst + row0 * H + u;
    float* const dgx0 = p.dGX + row0 * G4 + gcol;
    const int my_arg = p.arg[(int64_t)b * H + u];
    const float my_dp = p.dpool[(int64_t)b * p.lddp + u];
    // operands of the steps s0, s0-1, ..: the thread's own gate and the cell state (one more: c_{t-1} of the chunk's last step)
    float gq_cur[SC], c_cur[SC + 1], gq_nxt[SC], c_nxt[SC + 1], o_dp[SC];
    auto load_chunk = [&](int s0) {
#pragma unroll
        for (int r = 0; r <= SC; ++r) {
            const int64_t t = max(s0 - r, 0);     // uniform
            if (r < SC) gq_nxt[r] = gate0[t * G4];
            c_nxt[r] = c0p[t * H];
        }
    };
    auto store_chunk = [&](int s0) {
#pragma unroll
        for (int r = 0; r < SC; ++r)
            if (s0 - r >= 0) dgx0[(int64_t)(s0 - r) * G4] = o_dp[r];
    };
    float dh_rec = 0.f, dc_carry = 0.f;
    load_chunk(T - 1);
    for (int s0 = T - 1; s0 >= 0; s0 -= SC) {
#pragma unroll
        for (int r = 0; r <= SC; ++r) {
            if (r < SC) gq_cur[r] = gq_nxt[r];
            c_cur[r] = c_nxt[r];
        }
        if (s0 < T - 1) store_chunk(s0 + SC);
        if (s0 - SC >= 0) load_chunk(s0 - SC);
#pragma unroll
        for (int r = 0; r < SC; ++r) {
            const int s = s0 - r;
            if (s >= 0) {      // uniform
                const int buf = s & 1;
                const float cprev = s > 0 ? c_cur[r + 1] : 0.f;
                const float gq = gq_cur[r];
                const float gi = quad_bcast<0>(gq), gf = quad_bcast<1>(gq), gg = quad_bcast<2>(gq), go = quad_bcast<3>(gq);
                const float tc = fast_tanh(c_cur[r]);
                // d pre-activation of this lane's gate: i: dc g i(1-i) | f: dc c' f(1-f) | g: dc i (1-g^2) | o: dh tanh(c) o(1-o)
                const float der = q == 2 ? 1.f - gq * gq : gq * (1.f - gq);
                const float K = der * (q == 0 ? gg : q == 1 ? cprev : q == 2 ? gi : tc);
                const float dh = (my_arg == s ? my_dp : 0.f) + dh_rec;
                const float dc = dc_carry + dh * (go * (1.f - tc * tc));
                const float dp = (q == 3 ? dh : dc) * K;
                dc_carry = dc * gf;
                o_dp[r] = dp;
                s_dp[buf][chunk_pos(gcol)] = dp;
                lds_barrier();
                const float* dv = s_dp[buf] + part * KP;
                f2 a01 = {0.f, 0.f}, a23 = {0.f, 0.f}, b01 = {0.f, 0.f}, b23 = {0.f, 0.f};
#pragma unroll
                for (int i = 0; i < KQ; ++i) {
                    const f2 dk = {dv[i], dv[i]};
                    if (i & 1) {
                        b01 = __builtin_elementwise_fma(wt01[i], dk, b01);
                        b23 = __builtin_elementwise_fma(wt23[i], dk, b23);
                    } else {
                        a01 = __builtin_elementwise_fma(wt01[i], dk, a01);
                        a23 = __builtin_elementwise_fma(wt23[i], dk, a23);
                    }
                }
                a01 += b01, a23 += b23;
                const float s0_ = row16_sum(a01.x), s1_ = row16_sum(a01.y), s2_ = row16_sum(a23.x), s3_ = row16_sum(a23.y);
                dh_rec = myr == 0 ? s0_ : myr == 1 ? s1_ : myr == 2 ? s2_ : s3_;
            }
        }
    }
    store_chunk((T - 1) % SC);
}

// The running maximum over the saved hidden rows of ONE sample: thread u owns hidden unit u and walks rows 1 .. t_rows - 1 of
// Hprev (row t = h_{t-1}; row 0 is the initial state, not a step's output) with the forward's rule -- strict comparison from -2,
// so row t carries the bits the forward's pool has after t steps.  Loads do not depend on the running value.
__global__ __launch_bounds__(H) void lstm128_prefix_max_kernel(const float* __restrict__ hprev, const int t_rows, float* __restrict__ out) {
    const int u = threadIdx.x;
    out[u] = 0.f;
    float best = -2.f;      // |h| < 1
#pragma unroll 8
    for (int t = 1; t < t_rows; ++t) {
        const float h = hprev[(int64_t)t * H + u];
        if (h > best) best = h;
        out[(int64_t)t * H + u] = best;
    }
}

int fill(const char* name, Jobs& P, const ErcLstm128Job* jobs, int n_jobs, bool bwd, int& max_b) {
    ERC_REQUIRE(jobs && n_jobs >= 1 && n_jobs <= MAX_JOBS, "%s: n_jobs=%d outside [1, %d] (or null jobs_host)", name, n_jobs, MAX_JOBS);
    max_b = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const ErcLstm128Job& j = jobs[i];
        ERC_REQUIRE(j.B > 0 && j.T > 0 && (int64_t)j.B * j.T <= (int64_t)1 << 30, "%s: job %d: bad sizes B=%d T=%d", name, i, j.B, j.T);
        ERC_REQUIRE(j.W_hh && j.arg && j.gates && j.Cst, "%s: job %d: null pointer", name, i);
        if (bwd) {
            ERC_REQUIRE(j.dpool && j.dGX, "%s: job %d: null pointer (dpool, dGX)", name, i);
            ERC_REQUIRE(j.lddp >= H, "%s: job %d: lddp=%d < %d", name, i, j.lddp, H);
        } else {
            ERC_REQUIRE(j.GX && j.b_hh && j.pool && j.Hprev, "%s: job %d: null pointer (GX, b_hh, pool, Hprev)", name, i);
            ERC_REQUIRE(j.ldp >= H, "%s: job %d: ldp=%d < %d", name, i, j.ldp, H);
        }
        P.j[i] = j;
        max_b = j.B > max_b ? j.B : max_b;
    }
    for (int i = n_jobs; i < MAX_JOBS; ++i) P.j[i] = ErcLstm128Job{};
    return ERC_OK;
}

}  // namespace

extern "C" int erc_lstm128_hidden(void) { return H; }
extern "C" int erc_lstm128_max_jobs(void) { return MAX_JOBS; }

extern "C" int erc_lstm128_pool_fwd(const ErcLstm128Job* jobs_host, int n_jobs, void* stream) {
    Jobs P;
    int max_b = 0;
    if (int e = fill("lstm128_pool_fwd", P, jobs_host, n_jobs, false, max_b)) return e;
    hipLaunchKernelGGL(lstm128_fwd_kernel<Exact>, dim3(max_b, n_jobs), dim3(NTH), 0, (hipStream_t)stream, P, Exact{});
    ERC_LAUNCH_CHECK("lstm128_pool_fwd");
    return ERC_OK;
}

extern "C" int erc_lstm128_pool_bwd(const ErcLstm128Job* jobs_host, int n_jobs, void* stream) {
    Jobs P;
    int max_b = 0;
    if (int e = fill("lstm128_pool_bwd", P, jobs_host, n_jobs, true, max_b)) return e;
    hipLaunchKernelGGL(lstm128_bwd_kernel<Exact>, dim3(max_b, n_jobs), dim3(NTH), 0, (hipStream_t)stream, P, Exact{});
    ERC_LAUNCH_CHECK("lstm128_pool_bwd");
    return ERC_OK;
}

extern "C" int erc_lstm128_prefix_max(const float* Hprev, int t_rows, float* out, void* stream) {
    ERC_REQUIRE(Hprev && out && Hprev != out, "lstm128_prefix_max: null pointer (or out == Hprev)");
    ERC_REQUIRE(t_rows >= 2 && t_rows <= 1 << 22, "lstm128_prefix_max: t_rows=%d outside [2, 2^22]", t_rows);
    hipLaunchKernelGGL(lstm128_prefix_max_kernel, dim3(1), dim3(H), 0, (hipStream_t)stream, Hprev, t_rows, out);
    ERC_LAUNCH_CHECK("lstm128_prefix_max");
    return ERC_OK;
}

static int tcap_args(const char* name, const int32_t* counts, int dyn_mask, int n_jobs) {
    ERC_REQUIRE(counts, "%s: null counts", name);
    ERC_REQUIRE(dyn_mask >= 0 && dyn_mask < (1 << n_jobs), "%s: dyn_mask=%d names a job beyond n_jobs=%d", name, dyn_mask, n_jobs);
    return ERC_OK;
}

extern "C" int erc_lstm128_pool_fwd_tcap(const ErcLstm128Job* jobs_host, int n_jobs, const int32_t* counts, int dyn_mask,
                                         void* stream) {
    Jobs P;
    int max_b = 0;
    if (int e = fill("lstm128_pool_fwd_tcap", P, jobs_host, n_jobs, false, max_b)) return e;
    if (int e = tcap_args("lstm128_pool_fwd_tcap", counts, dyn_mask, n_jobs)) return e;
    hipLaunchKernelGGL(lstm128_fwd_kernel<Capacity>, dim3(max_b, n_jobs), dim3(NTH), 0, (hipStream_t)stream, P, Capacity{counts, dyn_mask});
    ERC_LAUNCH_CHECK("lstm128_pool_fwd_tcap");
    return ERC_OK;
}

extern "C" int erc_lstm128_pool_bwd_tcap(const ErcLstm128Job* jobs_host, int n_jobs, const int32_t* counts, int dyn_mask,
                                         void* stream) {
    Jobs P;
    int max_b = 0;
    if (int e = fill("lstm128_pool_bwd_tcap", P, jobs_host, n_jobs, true, max_b)) return e;
    if (int e = tcap_args("lstm128_pool_bwd_tcap", counts, dyn_mask, n_jobs)) return e;
    for (int i = 0; i < n_jobs; ++i)
        ERC_REQUIRE(((uintptr_t)jobs_host[i].dGX & 15) == 0, "lstm128_pool_bwd_tcap: job %d: dGX is not 16-byte aligned", i);
    hipLaunchKernelGGL(lstm128_bwd_kernel<Capacity>, dim3(max_b, n_jobs), dim3(NTH), 0, (hipStream_t)stream, P, Capacity{counts, dyn_mask});
    ERC_LAUNCH_CHECK("lstm128_pool_bwd_tcap");
    return ERC_OK;
}

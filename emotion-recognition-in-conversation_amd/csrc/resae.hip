// The residual autoencoder of MMIN's missing-modality model as ONE forward and ONE backward launch -- ResidualAE(layers =
// [256, 128, 64], n_blocks, input_dim = 384, dropout = 0, use_bn = False), track_mm/mmin_models.py:133-199, the two networks
// netAE / netAE_cycle of MMINMissModule (track_mm/mmin_miss.py:77-80, 103-104) -- and the mean-squared-error pair of its
// training step (F.mse_loss, track_mm/mmin_miss.py:207-208).
//
// A network is a strictly sequential chain of 6 n_blocks + 2 small Linears on [B, <= 384] rows; per layer launches cannot fill
// their own launch overhead (ercgraft.h).  Rows are independent, so a workgroup OWNS erc_resae_rows_per_group() = 16 rows of one
// job and runs the whole chain for them: the activations of its rows stay in LDS, the weights stream from L2 (every workgroup
// reads all of them once), and workgroups never wait for each other -- no grid barrier, no counters, no atomics, no spin loop.
// blockIdx.y picks the job (by-value table, as lstm128.hip), so both networks share a launch and a job's bits do not depend
// on its neighbour.
//
// Products are exact fp32 on the matrix cores (v_mfma_f32_16x16x4_f32; the 16 rows of the group are the 16 rows of the
// instruction):
//   forward   y[m][n] = sum_k a[m][k] W[n][k]: wavefront w of 8 owns the 16-column tiles w, w + 8, ..; lane (c = lane % 16,
//             g = lane / 16) reads 16 bytes of W row n0 + c at k + 4g and 16 bytes of LDS row c at k + 4g: four instructions
//             per 16 k (instruction j takes element j of both: the k of one instruction are k + 4g + j, g = 0..3)
//   backward  dx[m][k] = sum_n dy[m][n] W[n][k]: the reduction runs over W's ROWS, so 16 bytes of a row are four OUTPUT columns:
//             wavefront w owns the 64 columns [64w, 64w + 64) as four interleaved tiles (instruction j: columns k0 + 4c + j),
//             lane (c, g) reads W[n + g][k0 + 4c .. + 3] and LDS dy[c][n + g]; each lane ends with 4 rows x 4 consecutive columns
// The accumulation order of every element is fixed by the code: a repeated launch is bit-identical.  Row pitches of the LDS
// buffers are 4 mod 64 floats (388 / 260 / 132 / 68): the 16 rows of an operand read start 4 banks apart.
//
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950) is recorded in DESIGN.md section 8k.
//
// The sizes, the forward layer and the forward kernel live in csrc/resae_dev.h, shared with csrc/resae_eval.hip (the inference
// mode of the same kernel, erc_resae_latents); this file instantiates the training mode only (why).
#include "resae_dev.h"

namespace {

// dst[m][k] (= or +=) mask(sum_n src[m][n] W[n][k] (+ add[row][k])) for the group's 16 rows, W [NR, KC]; the mask is that of the
// activation whose saved OUTPUT is `act` [B, KC] (ReLU: out > 0; LeakyReLU: out > 0 ? 1 : 0.01); gout [B, ldg] receives what dst
// receives.  The caller puts a barrier behind the call.
template <int NR, int KC, int ACT, bool ACCUM>
__device__ __forceinline__ void bwd_layer(const float* __restrict__ W, const float* src, const int ps, float* dst, const int pd,
                                          const float* __restrict__ act, const float* __restrict__ add, const int lda,
                                          float* __restrict__ gout, const int ldg, const int row0, const int B) {
    constexpr int NU = KC / 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    if (wave >= NU) return;      // uniform per wavefront
    const int k0 = wave * 64 + 4 * c;
    // four accumulation chains per column tile (row step mod 4), added in a tree at the end (fwd_layer: why)
    f32x4 acc[4][4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[s][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wp = W + (int64_t)g * KC + k0;
    const float* ap = src + c * ps + g;
    static_assert(NR % 16 == 0, "four steps of 4 rows per trip");
#pragma unroll 2
    for (int n = 0; n < NR; n += 16) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float a = ap[n + 4 * s];
            const f4 w = *(const f4*)(wp + (int64_t)(n + 4 * s) * KC);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[s][j] = mma(a, w[j], acc[s][j]);
        }
    }
    f32x4 sum[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sum[j] = (acc[0][j] + acc[1][j]) + (acc[2][j] + acc[3][j]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = 4 * g + r;
        const int64_t row = row0 + m;
        const bool live = row < B;
        f4 v = {sum[0][r], sum[1][r], sum[2][r], sum[3][r]};
        if (add && live) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += add[row * lda + k0 + j];
        }
        if (ACT != ACT_NONE) {
            const f4 o = live ? *(const f4*)(act + row * KC + k0) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = o[j] > 0.f ? v[j] : (ACT == ACT_RELU ? 0.f : SLOPE * v[j]);
        }
        f4* d4 = (f4*)(dst + m * pd + k0);
        if (ACCUM) v += *d4;
        *d4 = v;
        if (gout && live) {
#pragma unroll
            for (int j = 0; j < 4; ++j) gout[row * ldg + k0 + j] = v[j];
        }
    }
}

__global__ __launch_bounds__(NTH) void resae_bwd_kernel(const Jobs P, const int nb) {
    const ErcResaeJob& p = P.j[blockIdx.y];
    const int B = p.B, row0 = blockIdx.x * R, tid = threadIdx.x;
    if (row0 >= B) return;      // uniform
    __shared__ __attribute__((aligned(16))) float sG[R * PX];      // gradient wrt x_in of the block at hand
    __shared__ __attribute__((aligned(16))) float sU[R * (P1 + P2)];
    __shared__ __attribute__((aligned(16))) float s3[R * P3];
    float* const s1 = sU;
    float* const s2 = sU + R * P1;
    const float* const A = p.act;
    float* const Y = p.dY;
    const int64_t Bl = B;
    float* const Yt = Y + Bl * BLK * nb;      // dY of transition.0 [B, 384] | of transition.2 [B, 384] (= d_recon)
    for (int e = tid; e < R * D; e += NTH) {
        const int m = e / D, k = e % D;
        const int64_t row = row0 + m;
        float v = 0.f;
        if (row < B) {
            v = p.d_recon[row * p.lddr + k];
            Yt[Bl * D + row * D + k] = v;
        }
        sG[m * PX + k] = v;
    }
    __syncthreads();
    const float* const At = A + Bl * BLK * nb;
    bwd_layer<D, D, ACT_RELU, false>(p.W[6 * nb + 1], sG, PX, sU, PX, At + Bl * D, nullptr, 0, Yt, D, row0, B);
    __syncthreads();
    // t_in = x_in + x_out of the last block: its gradient is that of the last x_in AND of the last decoder's output
    {
        float* const go = nb > 0 ? Y + Bl * BLK * (nb - 1) + Bl * Y_D2 : nullptr;
        bwd_layer<D, D, ACT_NONE, false>(p.W[6 * nb], sU, PX, sG, PX, nullptr, nullptr, 0, go, D, row0, B);
    }
    __syncthreads();
    for (int i = nb - 1; i >= 0; --i) {
        const float* const Ab = A + Bl * BLK * i;
        float* const Yb = Y + Bl * BLK * i;
        const float* const* Wl = p.W + 6 * i;
        bwd_layer<D, L1, ACT_RELU, false>(Wl[5], sG, PX, s1, P1, Ab + Bl * A_G2, nullptr, 0, Yb + Bl * Y_D1, L1, row0, B);
        __syncthreads();
        bwd_layer<L1, L2, ACT_RELU, false>(Wl[4], s1, P1, s2, P2, Ab + Bl * A_G1, nullptr, 0, Yb + Bl * Y_D0, L2, row0, B);
        __syncthreads();
        bwd_layer<L2, L3, ACT_NONE, false>(Wl[3], s2, P2, s3, P3, nullptr, p.d_latents ? p.d_latents + L3 * i : nullptr, p.lddl,
                                           Yb + Bl * Y_E2, L3, row0, B);
        __syncthreads();
        bwd_layer<L3, L2, ACT_LEAKY, false>(Wl[2], s3, P3, s2, P2, Ab + Bl * A_H2, nullptr, 0, Yb + Bl * Y_E1, L2, row0, B);
        __syncthreads();
        bwd_layer<L2, L1, ACT_LEAKY, false>(Wl[1], s2, P2, s1, P1, Ab + Bl * A_H1, nullptr, 0, Yb + Bl * Y_E0, L1, row0, B);
        __syncthreads();
        // x_in_i = x_in_{i-1} + x_out_{i-1}: the sum over the encoder's path and everything behind it is the gradient of both
        // (block 0: x_in = x, x_out = 0: it is dx)
        if (i > 0)
            bwd_layer<L1, D, ACT_NONE, true>(Wl[0], s1, P1, sG, PX, nullptr, nullptr, 0, Yb - Bl * BLK + Bl * Y_D2, D, row0, B);
        else
            bwd_layer<L1, D, ACT_NONE, true>(Wl[0], s1, P1, sG, PX, nullptr, nullptr, 0, p.dx, p.lddx, row0, B);
        __syncthreads();
    }
}

// loss_out[0] = mean((a - b)^2), d = weight * 2 (a - b) / (B n): one workgroup; every thread sums its elements (index order,
// stride MSE_TH) in double, the threads' sums are added in a fixed tree
constexpr int MSE_TH = 1024;
__global__ __launch_bounds__(MSE_TH) void mse_grad_kernel(const float* __restrict__ a, const int lda, const float* __restrict__ b,
                                                          const int ldb, const int B, const int n, const float scale,
                                                          float* __restrict__ d, const int ldd, float* __restrict__ loss_out) {
    __shared__ double red[MSE_TH];
    const int64_t total = (int64_t)B * n;
    double s = 0.0;
    for (int64_t e = threadIdx.x; e < total; e += MSE_TH) {
        const int64_t r = e / n;
        const int c = (int)(e % n);
        const float df = a[r * lda + c] - b[r * ldb + c];
        s += (double)df * (double)df;
        d[r * ldd + c] = scale * df;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = MSE_TH / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss_out[0] = (float)(red[0] / (double)total);
}

// dfeat = dx0 + dx1 - dcyc (left to right), the text columns through embd's ReLU mask into dtext; thread 0 of block 0 the step's
// loss slots
__global__ __launch_bounds__(256) void miss_combine_kernel(const float* __restrict__ dx0, const float* __restrict__ dx1,
                                                           const float* __restrict__ dcyc, const float* __restrict__ feat, const int ldf,
                                                           const int B, float* __restrict__ dfeat, const int lddf,
                                                           float* __restrict__ dtext, const int lddt, const float* __restrict__ ce_stats,
                                                           const float w_mse, const float w_cyc, float* __restrict__ stats) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < (int64_t)B * D) {
        const int64_t r = e / D;
        const int c = (int)(e % D);
        const float v = dx0[e] + dx1[e] - dcyc[e];
        dfeat[r * lddf + c] = v;
        if (c >= 2 * L2) dtext[r * lddt + c - 2 * L2] = feat[r * ldf + c] > 0.f ? v : 0.f;
    }
    if (e == 0) {
        const float lce = ce_stats[0];
        stats[0] = lce + w_mse * stats[2] + w_cyc * stats[3];
        stats[1] = ce_stats[1];
        stats[4] = lce;
    }
}

}  // namespace

extern "C" int erc_resae_input(void) { return D; }
extern "C" int erc_resae_latent(void) { return L3; }
extern "C" int erc_resae_max_jobs(void) { return MAX_JOBS; }
extern "C" int erc_resae_max_blocks(void) { return MAX_BLOCKS; }
extern "C" int erc_resae_rows_per_group(void) { return R; }
extern "C" int64_t erc_resae_act_floats(int B, int n_blocks) {
    return B > 0 && n_blocks >= 1 && n_blocks <= MAX_BLOCKS ? (int64_t)B * (BLK * n_blocks + 2 * D) : 0;
}

// ResidualAE.forward (mmin_models.py:187-199)
extern "C" int erc_resae_fwd(const ErcResaeJob* jobs_host, int n_jobs, int n_blocks, void* stream) {
    Jobs P;
    int max_b = 0;
    if (int e = fill("resae_fwd", P, jobs_host, n_jobs, n_blocks, FILL_FWD, max_b)) return e;
    hipLaunchKernelGGL(resae_fwd_kernel<false>, dim3(erc_cdiv(max_b, R), n_jobs), dim3(NTH), 0, (hipStream_t)stream, P, n_blocks);
    ERC_LAUNCH_CHECK("resae_fwd");
    return ERC_OK;
}

// autograd of ResidualAE.forward (mmin_models.py:187-199) down to every layer's pre-activation gradient and dx
extern "C" int erc_resae_bwd(const ErcResaeJob* jobs_host, int n_jobs, int n_blocks, void* stream) {
    Jobs P;
    int max_b = 0;
    if (int e = fill("resae_bwd", P, jobs_host, n_jobs, n_blocks, FILL_BWD, max_b)) return e;
    hipLaunchKernelGGL(resae_bwd_kernel, dim3(erc_cdiv(max_b, R), n_jobs), dim3(NTH), 0, (hipStream_t)stream, P, n_blocks);
    ERC_LAUNCH_CHECK("resae_bwd");
    return ERC_OK;
}

// F.mse_loss(a, b) and its gradient (mmin_miss.py:207-208)
extern "C" int erc_mse_grad(const float* a, int lda, const float* b, int ldb, int B, int n_cols, float weight, float* d, int ldd,
                            float* loss_out, void* stream) {
    ERC_REQUIRE(a && b && d && loss_out, "mse_grad: null pointer");
    ERC_REQUIRE(B > 0 && n_cols > 0, "mse_grad: B=%d n_cols=%d", B, n_cols);
    ERC_REQUIRE(lda >= n_cols && ldb >= n_cols && ldd >= n_cols, "mse_grad: pitch below n_cols=%d (lda=%d ldb=%d ldd=%d)", n_cols, lda,
                ldb, ldd);
    const float scale = (float)((double)weight * 2.0 / ((double)B * (double)n_cols));
    hipLaunchKernelGGL(mse_grad_kernel, dim3(1), dim3(MSE_TH), 0, (hipStream_t)stream, a, lda, b, ldb, B, n_cols, scale, d, ldd, loss_out);
    ERC_LAUNCH_CHECK("mse_grad");
    return ERC_OK;
}

// the feature gradient of MMINMissTrainer.train_step (mmin_miss.py:196-213) and the step's loss slots
extern "C" int erc_mmin_miss_combine(const float* dx0, const float* dx1, const float* dcyc, const float* feat, int ldf, int B,
                                     float* dfeat, int lddf, float* dtext, int lddt, const float* ce_stats, float w_mse, float w_cyc,
                                     float* stats, void* stream) {
    ERC_REQUIRE(dx0 && dx1 && dcyc && feat && dfeat && dtext && ce_stats && stats, "mmin_miss_combine: null pointer");
    ERC_REQUIRE(B > 0, "mmin_miss_combine: B=%d", B);
    ERC_REQUIRE(ldf >= D && lddf >= D && lddt >= L2, "mmin_miss_combine: pitch below its width (ldf=%d lddf=%d lddt=%d)", ldf, lddf, lddt);
    hipLaunchKernelGGL(miss_combine_kernel, dim3(erc_cdiv((int64_t)B * D, 256)), dim3(256), 0, (hipStream_t)stream, dx0, dx1, dcyc, feat,
                       ldf, B, dfeat, lddf, dtext, lddt, ce_stats, w_mse, w_cyc, stats);
    ERC_LAUNCH_CHECK("mmin_miss_combine");
    return ERC_OK;
}

// K5 (BatchNorm1d + LeakyReLU over the nodes of this rank) and S3 (cross entropy).
//
// BatchNorm: column statistics of an [N,F] matrix are accumulated in fp64 by
// BN_G workgroups into per-workgroup partials; every workgroup of the apply
// kernel re-reduces the (tiny) partial table, so there is no third launch, no
// atomics, and the result does not depend on scheduling.
#include "erc_common.h"

namespace {

constexpr int BN_G = 64;  // workgroups of the statistics pass

// partial[g][0..F) = sum_rows a(row,c) ; partial[g][F..2F) = sum_rows b(row,c)
// MODE 0: a = x, b = x*x.  MODE 1 (backward): a = dz, b = dz*xhat.
template <int MODE>
__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ x, int ldx, int N, int F,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ saved, float slope,
                                                       const float* __restrict__ dy, int lddy,
                                                       double* __restrict__ partial) {
    const int c = threadIdx.x & 127, half = threadIdx.x >> 7;
    __shared__ double sh[2][128];
    double a = 0.0, b = 0.0;
    if (c < F) {
        float mean = 0.f, rstd = 0.f, ga = 0.f, be = 0.f;
        if (MODE == 1) mean = saved[c], rstd = saved[F + c], ga = gamma[c], be = beta[c];
        for (int row = blockIdx.x * 2 + half; row < N; row += 2 * BN_G) {
            const float v = x[(int64_t)row * ldx + c];
            if (MODE == 0) {
                a += (double)v;
                b += (double)v * (double)v;
            } else {
                const float xh = (v - mean) * rstd;
                const float zz = xh * ga + be;
                const float dz = dy[(int64_t)row * lddy + c] * (zz > 0.f ? 1.f : slope);
                a += (double)dz;
                b += (double)dz * (double)xh;
            }
        }
    }
    if (half == 1) sh[0][c] = a, sh[1][c] = b;
    __syncthreads();
    if (half == 0 && c < F) {
        partial[(int64_t)blockIdx.x * 2 * F + c] = a + sh[0][c];
        partial[(int64_t)blockIdx.x * 2 * F + F + c] = b + sh[1][c];
    }
}

__global__ __launch_bounds__(256) void bn_apply_fwd_kernel(const float* __restrict__ x, int ldx, int N, int F,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* running_mean,
                                                           float* running_var, float momentum, float eps, float slope,
                                                           int training, float* __restrict__ saved,
                                                           float* __restrict__ y, int ldy,
                                                           const double* __restrict__ partial) {
    const int c = threadIdx.x & 127, half = threadIdx.x >> 7;
    __shared__ float s_mean[128], s_rstd[128];
    if (half == 0 && c < F) {
        float mean, rstd;
        if (training) {
            double s = 0.0, ss = 0.0;
            for (int g = 0; g < BN_G; ++g) {
                s += partial[(int64_t)g * 2 * F + c];
                ss += partial[(int64_t)g * 2 * F + F + c];
            }
            const double m = s / (double)N;
            double var = ss / (double)N - m * m;
            if (var < 0.0) var = 0.0;
            mean = (float)m;
            rstd = (float)(1.0 / sqrt(var + (double)eps));
            if (blockIdx.x == 0) {
                saved[c] = mean;
                saved[F + c] = rstd;
                const double unbiased = N > 1 ? var * (double)N / (double)(N - 1) : var;
                running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
                running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
            }
        } else {
            mean = running_mean[c];
            rstd = 1.0f / sqrtf(running_var[c] + eps);
        }
        s_mean[c] = mean;
        s_rstd[c] = rstd;
    }
    __syncthreads();
    if (c >= F) return;
    const float mean = s_mean[c], rstd = s_rstd[c], ga = gamma[c], be = beta[c];
    for (int row = blockIdx.x * 2 + half; row < N; row += 2 * gridDim.x) {
        const float z = (x[(int64_t)row * ldx + c] - mean) * rstd * ga + be;
        y[(int64_t)row * ldy + c] = z > 0.f ? z : z * slope;
    }
}

__global__ __launch_bounds__(256) void bn_apply_bwd_kernel(const float* __restrict__ x, int ldx, int N, int F,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta,
                                                           const float* __restrict__ saved, float slope,
                                                           const float* __restrict__ dy, int lddy,
                                                           float* __restrict__ dx, int lddx,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           const double* __restrict__ partial) {
    const int c = threadIdx.x & 127, half = threadIdx.x >> 7;
    __shared__ float s_a[128], s_b[128];
    if (half == 0 && c < F) {
        double s = 0.0, ss = 0.0;
        for (int g = 0; g < BN_G; ++g) {
            s += partial[(int64_t)g * 2 * F + c];
            ss += partial[(int64_t)g * 2 * F + F + c];
        }
        s_a[c] = (float)(s / (double)N);   // mean of dz
        s_b[c] = (float)(ss / (double)N);  // mean of dz*xhat
        if (blockIdx.x == 0) {
            dbeta[c] = (float)s;
            dgamma[c] = (float)ss;
        }
    }
    __syncthreads();
    if (c >= F) return;
    const float mean = saved[c], rstd = saved[F + c], ga = gamma[c], be = beta[c];
    const float ma = s_a[c], mb = s_b[c];
    for (int row = blockIdx.x * 2 + half; row < N; row += 2 * gridDim.x) {
        const float xh = (x[(int64_t)row * ldx + c] - mean) * rstd;
        const float zz = xh * ga + be;
        const float dz = dy[(int64_t)row * lddy + c] * (zz > 0.f ? 1.f : slope);
        dx[(int64_t)row * lddx + c] = ga * rstd * (dz - ma - xh * mb);
    }
}

// ------------------------------------------------------------ cross entropy
// Rows are spread over up to CE_MAXWG workgroups (the gradient needs only the normaliser, which every workgroup
// recomputes from the labels); loss / accuracy partials are combined by the LAST workgroup to finish, in
// workgroup order, so the result is independent of scheduling.  stats[] layout: [0] loss [1] #correct [2] sum of
// weights [8 + 2w], [9 + 2w] partials of workgroup w, [4] (as int) arrival counter (zero between calls).
constexpr int CE_MAXWG = 64;

// CAP (erc_cross_entropy_cap): n_rows is a capacity, the batch's sample count is *n_dev (clamped to [0, n_rows]); samples at
// or beyond it are not read, and a count of 0 gives loss 0 / stats 0 with nothing written to dlogits.
template <bool CAP>
__global__ __launch_bounds__(256) void cross_entropy_kernel(const float* __restrict__ logits, int ld, int C,
                                                            int n_rows, const int32_t* __restrict__ row_map,
                                                            const int64_t* __restrict__ labels,
                                                            const float* __restrict__ weight, float grad_scale,
                                                            float* __restrict__ dlogits, int lddl,
                                                            float* __restrict__ stats, const int32_t* __restrict__ n_dev) {
    if (CAP) n_rows = min(max(*n_dev, 0), n_rows);
    __shared__ double red[256];
    double* const s_red = red;
    __shared__ double s_wsum;
    __shared__ int s_last;
    const int tid = threadIdx.x;
    double wacc = 0.0;
    if (weight) {
        for (int i = tid; i < n_rows; i += 256) wacc += (double)weight[labels[i]];
        red[tid] = wacc;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        if (tid == 0) s_wsum = red[0];
    } else if (tid == 0) {
        s_wsum = (double)n_rows;
    }
    __syncthreads();
    const double wsum = s_wsum;
    const float inv_w = (float)(1.0 / wsum);
    double lacc = 0.0;
    int hit = 0;
    for (int i = blockIdx.x * 256 + tid; i < n_rows; i += gridDim.x * 256) {
        const int64_t row = row_map ? (int64_t)row_map[i] : (int64_t)i;
        const float* z = logits + row * ld;
        const int y = (int)labels[i];
        float mx = z[0];
        int am = 0;
        for (int c = 1; c < C; ++c) {
            const float v = z[c];
            if (v > mx) mx = v, am = c;
        }
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(z[c] - mx);
        const float w = weight ? weight[y] : 1.f;
        // (max - z[y]) + log(sum) and exp(z - max) / sum, not lse = max + log(sum) and exp(z - lse): lse rounds at the ulp of the
        // largest logit (7.6e-6 at 100), which the row's loss takes as an absolute and the softmax as a relative error --
        // 3.9e-6 on the gradient of 30 randn or 3 randn +- 100 logits where this form has 2e-7 (tests/test_gpu_cross_entropy.py)
        lacc += (double)(w * ((mx - z[y]) + logf(se)));
        hit += (am == y) ? 1 : 0;
        if (dlogits) {
            float* d = dlogits + row * lddl;
            const float coef = w * inv_w * grad_scale, inv_se = 1.f / se;
            for (int c = 0; c < C; ++c) d[c] = coef * (expf(z[c] - mx) * inv_se - (c == y ? 1.f : 0.f));
        }
    }
    __syncthreads();
    red[tid] = lacc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const double lsum = red[0];
    __syncthreads();
    red[tid] = (double)hit;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        stats[8 + 2 * blockIdx.x] = (float)lsum;
        stats[9 + 2 * blockIdx.x] = (float)red[0];
        __threadfence();
        const int prev = atomicAdd(reinterpret_cast<int*>(stats + 4), 1);
        s_last = (prev == (int)gridDim.x - 1);
    }
    __syncthreads();
    if (s_last) {  // the last workgroup combines the partials: one (parallel) load per thread, fixed-order tree
        __threadfence();
        double l = 0.0, h = 0.0;
        if (tid < (int)gridDim.x) {
            l = (double)__hip_atomic_load(stats + 8 + 2 * tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            h = (double)__hip_atomic_load(stats + 9 + 2 * tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        s_red[tid] = l;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) s_red[tid] += s_red[tid + o];
            __syncthreads();
        }
        const double lsum = s_red[0];
        __syncthreads();
        s_red[tid] = h;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) s_red[tid] += s_red[tid + o];
            __syncthreads();
        }
        if (tid == 0) {
            stats[0] = (CAP && n_rows == 0) ? 0.f : (float)(lsum / wsum);
            stats[1] = (float)s_red[0];
            stats[2] = (float)wsum;
            *reinterpret_cast<int*>(stats + 4) = 0;
        }
    }
}

// ------------------------------------------------------------ scoring of padded logits (erc_rows_score)
// Sample i < n = clamp(*n_dev, 0, n_cap) reads logits row row_map[i] (or i), predicts the first index of the maximum and
// counts cm[label * C + pred].  Integer counts: a histogram per workgroup in LDS, then one 64-bit vector atomic add per
// non-empty cell, so the result does not depend on the order.  A NaN logit never wins (fmaxf skips it, and NaN == max is
// false); a row of nothing but NaN, a label outside [0, C) and a row index outside [0, n_logit_rows) are not counted.
constexpr int RS_MAXC = 16;
constexpr int RS_MAXWG = 64;

__global__ __launch_bounds__(256) void rows_score_kernel(const float* __restrict__ logits, int ld, int n_logit_rows, int C,
                                                         int n_cap, const int32_t* __restrict__ n_dev,
                                                         const int32_t* __restrict__ row_map,
                                                         const int64_t* __restrict__ labels, unsigned long long* cm) {
    __shared__ int s_cm[RS_MAXC * RS_MAXC];
    const int tid = threadIdx.x;
    s_cm[tid] = 0;      // 256 threads = RS_MAXC * RS_MAXC cells
    __syncthreads();
    const int n = min(max(*n_dev, 0), n_cap);
    for (int i = blockIdx.x * 256 + tid; i < n; i += gridDim.x * 256) {
        const int64_t row = row_map ? (int64_t)row_map[i] : (int64_t)i;
        if (row < 0 || row >= n_logit_rows) continue;
        const float* z = logits + row * ld;
        float mx = z[0];
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, z[c]);
        int am = -1;
        for (int c = C - 1; c >= 0; --c)
            if (z[c] == mx) am = c;
        const int64_t y = labels[i];
        if (am >= 0 && y >= 0 && y < C) atomicAdd(&s_cm[(int)y * C + am], 1);
    }
    __syncthreads();
    if (tid < C * C && s_cm[tid] > 0) atomicAdd(cm + tid, (unsigned long long)s_cm[tid]);
}
static_assert(RS_MAXC * RS_MAXC == 256, "one histogram cell per thread");

// ------------------------------------------------------------ fused classifier tail
// logits = Z W^T + b (C <= 8 classes, F <= 128 features), cross entropy, and the gradient wrt Z through the
// relu/dropout mask -- cls[3] + F.cross_entropy + their backward (track_mm/cogmen.py:116-122,185) in ONE launch
// instead of GEMM + CE + GEMM.  One wavefront per row, lane l owns features l and l+64.
constexpr int HC_MAXC = 8;
constexpr int HC_MAXWG = 256;  // workgroups (one arrival atomic each)

// CAP (erc_head_ce_cap): the launch is sized for n_rows = the capacity, the batch is the first *n_dev rows.  Rows past them
// add nothing to the loss, the correct count or the weight sum, and their dlogits / dZ rows are written 0 (the weight-gradient
// products of the caller run over all n_rows rows).
template <bool CAP>
__global__ __launch_bounds__(256) void head_ce_kernel(const float* __restrict__ Z, int ldz, int F, int C, int n_rows,
                                                      const float* __restrict__ W, const float* __restrict__ bias,
                                                      const int64_t* __restrict__ labels,
                                                      const float* __restrict__ weight, float mask_scale,
                                                      float* __restrict__ logits, int ldl, float* __restrict__ dlogits,
                                                      int lddl, float* __restrict__ dZ, int lddz,
                                                      float* __restrict__ stats, int rows_per_wg,
                                                      const int32_t* __restrict__ n_dev) {
    __shared__ double s_red[256];
    __shared__ double s_wsum;
    __shared__ float s_part[4][2];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_valid = CAP ? min(max(*n_dev, 0), n_rows) : n_rows;
    if (weight) {
        double wacc = 0.0;
        for (int i = tid; i < n_valid; i += 256) wacc += (double)weight[labels[i]];
        s_red[tid] = wacc;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) s_red[tid] += s_red[tid + o];
            __syncthreads();
        }
        if (tid == 0) s_wsum = s_red[0];
    } else if (tid == 0) {
        s_wsum = (double)n_valid;
    }
    __syncthreads();
    const double wsum = s_wsum;
    // an empty capacity batch (*n_dev = 0) has no row to weigh: every gradient row is written 0 and the loss reads 0, not 0 / 0
    const float inv_w = CAP && !(wsum > 0.0) ? 0.f : (float)(1.0 / wsum);
    const bool h0 = lane < F, h1 = lane + 64 < F;
    const int c0 = min(lane, F - 1), c1 = min(lane + 64, F - 1);
    // unconditional clamped loads, masked afterwards (a guarded load costs a full round trip each)
    float w0[HC_MAXC], w1[HC_MAXC], bk[HC_MAXC];
    const float m0 = h0 ? 1.f : 0.f, m1 = h1 ? 1.f : 0.f;
#pragma unroll
    for (int k = 0; k < HC_MAXC; ++k) {
        const int kc = min(k, C - 1);
        w0[k] = W[(int64_t)kc * F + c0] * m0;
        w1[k] = W[(int64_t)kc * F + c1] * m1;
        bk[k] = bias[kc];
    }
    float lacc = 0.f, hits = 0.f;
    for (int rr = wave; rr < rows_per_wg; rr += 4) {
        const int row = blockIdx.x * rows_per_wg + rr;
        if (row >= n_rows) break;
        if (CAP && row >= n_valid) {      // wave-uniform: a capacity row
            if (lane < C) logits[(int64_t)row * ldl + lane] = 0.f, dlogits[(int64_t)row * lddl + lane] = 0.f;
            if (h0) dZ[(int64_t)row * lddz + lane] = 0.f;
            if (h1) dZ[(int64_t)row * lddz + lane + 64] = 0.f;
            continue;
        }
        const float z0 = Z[(int64_t)row * ldz + c0], z1 = Z[(int64_t)row * ldz + c1];
        const int y = (int)labels[row];
        float lg[HC_MAXC];
#pragma unroll
        for (int k = 0; k < HC_MAXC; ++k) lg[k] = wave_sum(z0 * w0[k] + z1 * w1[k]) + bk[k];
        float mx = lg[0];
        int am = 0;
#pragma unroll
        for (int k = 1; k < HC_MAXC; ++k)
            if (k < C && lg[k] > mx) mx = lg[k], am = k;
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < HC_MAXC; ++k)
            if (k < C) se += expf(lg[k] - mx);
        const float lse = mx + logf(se);
        float wy = 1.f;
        if (weight) wy = weight[y];   // wave-uniform branch
        float ly = 0.f, g0 = 0.f, g1 = 0.f;
        const float coef = wy * inv_w;
#pragma unroll
        for (int k = 0; k < HC_MAXC; ++k) {
            if (k < C) {
                const float d = coef * (expf(lg[k] - lse) - (k == y ? 1.f : 0.f));
                if (k == y) ly = lg[k];
                g0 += d * w0[k];
                g1 += d * w1[k];
                if (lane == k) {
                    logits[(int64_t)row * ldl + k] = lg[k];
                    dlogits[(int64_t)row * lddl + k] = d;
                }
            }
        }
        if (h0) dZ[(int64_t)row * lddz + lane] = z0 > 0.f ? g0 * mask_scale : 0.f;
        if (h1) dZ[(int64_t)row * lddz + lane + 64] = z1 > 0.f ? g1 * mask_scale : 0.f;
        lacc += wy * (lse - ly);
        hits += (am == y) ? 1.f : 0.f;
    }
    if (lane == 0) s_part[wave][0] = lacc, s_part[wave][1] = hits;
    __syncthreads();
    if (tid == 0) {
        stats[8 + 2 * blockIdx.x] = s_part[0][0] + s_part[1][0] + s_part[2][0] + s_part[3][0];
        stats[9 + 2 * blockIdx.x] = s_part[0][1] + s_part[1][1] + s_part[2][1] + s_part[3][1];
        __threadfence();
        const int prev = atomicAdd(reinterpret_cast<int*>(stats + 4), 1);
        s_last = (prev == (int)gridDim.x - 1);
    }
    __syncthreads();
    if (s_last) {  // the last workgroup combines the partials: one (parallel) load per thread, fixed-order tree
        __threadfence();
        double l = 0.0, h = 0.0;
        if (tid < (int)gridDim.x) {
            l = (double)__hip_atomic_load(stats + 8 + 2 * tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            h = (double)__hip_atomic_load(stats + 9 + 2 * tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        s_red[tid] = l;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) s_red[tid] += s_red[tid + o];
            __syncthreads();
        }
        const double lsum = s_red[0];
        __syncthreads();
        s_red[tid] = h;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) s_red[tid] += s_red[tid + o];
            __syncthreads();
        }
        if (tid == 0) {
            stats[0] = CAP && !(wsum > 0.0) ? 0.f : (float)(lsum / wsum);
            stats[1] = (float)s_red[0];
            stats[2] = (float)wsum;
            *reinterpret_cast<int*>(stats + 4) = 0;
        }
    }
}

// ------------------------------------------------------------ CIM multi-task loss (cross entropy + 7-way BCE)
// F.cross_entropy(logits[:, :C], label) + F.binary_cross_entropy_with_logits(logits[:, C:C+7], emo_label.float())
// (track_mm/cim.py:204-216) and their gradient in one launch.  One thread per row; per-thread sums in fp64, a fixed
// tree per workgroup, and the LAST workgroup to finish combines the per-workgroup partials in workgroup order, as
// cross_entropy_kernel does: the result does not depend on scheduling.  stats[] layout: [0] Lall = w_ce Lce +
// w_bce Lmulti, [1] #correct, [2] Lce, [3] Lmulti, [4] (as int) arrival counter (zero between calls),
// [8 + 3w .. 10 + 3w] partials of workgroup w.
constexpr int MT_MAXWG = 64;
constexpr int MT_EMO = 7;

__device__ __forceinline__ double block_sum_fixed(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

// CAP (erc_ce_bce_multitask_cap): n_rows is a capacity and the batch's sample count n = *n_dev clamped to [0, n_rows].  Both
// means run over n; rows at or beyond n are not read, and their dlogits rows are WRITTEN 0 (the head's weight-gradient
// product and the GEMM behind dmerged run over all n_rows rows).  n == 0: every term is 0, not 0 / 0.
template <bool CAP>
__global__ __launch_bounds__(256) void ce_bce_multitask_kernel(const float* __restrict__ logits, int ld, int C,
                                                               int n_rows, const int64_t* __restrict__ labels,
                                                               const int64_t* __restrict__ emo, int lde, float w_ce,
                                                               float w_bce, float grad_scale,
                                                               float* __restrict__ dlogits, int lddl,
                                                               float* __restrict__ stats, const int32_t* __restrict__ n_dev) {
    __shared__ double red[256];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    const int n_cap = n_rows;
    if (CAP) n_rows = min(max(*n_dev, 0), n_cap);
    const bool empty = CAP && n_rows == 0;
    const float coef_ce = empty ? 0.f : (float)((double)w_ce / (double)n_rows) * grad_scale;
    const float coef_bce = empty ? 0.f : (float)((double)w_bce / (7.0 * (double)n_rows)) * grad_scale;
    double ce_acc = 0.0, bce_acc = 0.0;
    int hit = 0;
    if (CAP && dlogits)
        for (int i = n_rows + blockIdx.x * 256 + tid; i < n_cap; i += gridDim.x * 256)
            for (int c = 0; c < C + MT_EMO; ++c) dlogits[(int64_t)i * lddl + c] = 0.f;
    for (int i = blockIdx.x * 256 + tid; i < n_rows; i += gridDim.x * 256) {
        const float* z = logits + (int64_t)i * ld;
        const int y = (int)labels[i];
        float mx = z[0], zy = z[0];
        int am = 0;
        for (int c = 1; c < C; ++c) {
            const float v = z[c];
            if (v > mx) mx = v, am = c;
            if (c == y) zy = v;   // no logits read through an out-of-range label
        }
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(z[c] - mx);
        const float lse = mx + logf(se);
        ce_acc += (double)(lse - zy);
        hit += (am == y) ? 1 : 0;
        const int64_t* e = emo + (int64_t)i * lde;
        float* d = dlogits ? dlogits + (int64_t)i * lddl : nullptr;
        if (d) {  // exp(z - max) / sum, not exp(z - lse): lse rounds at the ulp of the largest logit (7.6e-6 at 100)
            const float inv_se = 1.f / se;
            for (int c = 0; c < C; ++c) d[c] = coef_ce * (expf(z[c] - mx) * inv_se - (c == y ? 1.f : 0.f));
        }
#pragma unroll
        for (int k = 0; k < MT_EMO; ++k) {
            const float x = z[C + k], t = (float)e[k];
            // torch's stable form (1 - t) x + m + log(exp(-m) + exp(-x - m)), m = max(-x, 0), written as
            // (1 - t) x + m + log1p(exp(-|x|)): the same value for either sign of x, finite for any finite x
            const float m = fmaxf(-x, 0.f);
            const float ex = expf(-fabsf(x));
            bce_acc += (double)((1.f - t) * x + m + log1pf(ex));
            if (d) {
                const float sig = x >= 0.f ? 1.f / (1.f + ex) : ex / (1.f + ex);
                d[C + k] = coef_bce * (sig - t);
            }
        }
    }
    const double ce_sum = block_sum_fixed(ce_acc, red);
    const double bce_sum = block_sum_fixed(bce_acc, red);
    const double hit_sum = block_sum_fixed((double)hit, red);
    if (tid == 0) {
        stats[8 + 3 * blockIdx.x] = (float)ce_sum;
        stats[9 + 3 * blockIdx.x] = (float)hit_sum;
        stats[10 + 3 * blockIdx.x] = (float)bce_sum;
        __threadfence();
        const int prev = atomicAdd(reinterpret_cast<int*>(stats + 4), 1);
        s_last = (prev == (int)gridDim.x - 1);
    }
    __syncthreads();
    if (s_last) {  // the last workgroup combines the partials: one (parallel) load per thread, fixed-order tree
        __threadfence();
        double l = 0.0, h = 0.0, b = 0.0;
        if (tid < (int)gridDim.x) {
            l = (double)__hip_atomic_load(stats + 8 + 3 * tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            h = (double)__hip_atomic_load(stats + 9 + 3 * tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            b = (double)__hip_atomic_load(stats + 10 + 3 * tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const double lsum = block_sum_fixed(l, red);
        const double hsum = block_sum_fixed(h, red);
        const double bsum = block_sum_fixed(b, red);
        if (tid == 0) {
            const double lce = empty ? 0.0 : lsum / (double)n_rows, lmulti = empty ? 0.0 : bsum / (7.0 * (double)n_rows);
            stats[0] = (float)((double)w_ce * lce + (double)w_bce * lmulti);
            stats[1] = (float)hsum;
            stats[2] = (float)lce;
            stats[3] = (float)lmulti;
            *reinterpret_cast<int*>(stats + 4) = 0;
        }
    }
}

}  // namespace

extern "C" int64_t erc_head_ce_stats_floats(int n_rows) { return 16 + 2 * HC_MAXWG; }

extern "C" int erc_head_ce_cap(const float* Z, int ldz, int F, int C, int n_rows, const float* W, const float* bias,
                               const int64_t* labels, const float* weight, float mask_scale, float* logits, int ldl,
                               float* dlogits, int lddl, float* dZ, int lddz, float* stats, const int32_t* n_dev, void* stream) {
    ERC_REQUIRE(Z && W && bias && labels && logits && dlogits && dZ && stats, "head_ce: null pointer");
    ERC_REQUIRE(F > 0 && F <= 128 && C > 0 && C <= HC_MAXC && n_rows > 0, "head_ce: F=%d C=%d n_rows=%d unsupported", F, C, n_rows);
    int grid = erc_cdiv(n_rows, 16);
    if (grid > HC_MAXWG) grid = HC_MAXWG;
    const int rows_per_wg = erc_cdiv(n_rows, grid);
    grid = erc_cdiv(n_rows, rows_per_wg);
    if (n_dev)
        hipLaunchKernelGGL(head_ce_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, Z, ldz, F, C, n_rows, W, bias,
                           labels, weight, mask_scale, logits, ldl, dlogits, lddl, dZ, lddz, stats, rows_per_wg, n_dev);
    else
        hipLaunchKernelGGL(head_ce_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, Z, ldz, F, C, n_rows, W, bias,
                           labels, weight, mask_scale, logits, ldl, dlogits, lddl, dZ, lddz, stats, rows_per_wg, n_dev);
    ERC_LAUNCH_CHECK("head_ce");
    return ERC_OK;
}

extern "C" int erc_head_ce(const float* Z, int ldz, int F, int C, int n_rows, const float* W, const float* bias,
                           const int64_t* labels, const float* weight, float mask_scale, float* logits, int ldl,
                           float* dlogits, int lddl, float* dZ, int lddz, float* stats, void* stream) {
    return erc_head_ce_cap(Z, ldz, F, C, n_rows, W, bias, labels, weight, mask_scale, logits, ldl, dlogits, lddl, dZ, lddz, stats,
                           nullptr, stream);
}

extern "C" int64_t erc_bn_ws_floats(int F) { return (int64_t)BN_G * 2 * F * 2 + 16; }

extern "C" int erc_bn_lrelu_fwd(const float* x, int ldx, int N, int F, const float* gamma, const float* beta,
                                float* running_mean, float* running_var, float momentum, float eps, float slope,
                                int training, float* saved, float* y, int ldy, float* ws, void* stream) {
    ERC_REQUIRE(x && gamma && beta && running_mean && running_var && y && ws, "bn_lrelu_fwd: null pointer");
    ERC_REQUIRE(!training || saved, "bn_lrelu_fwd: training needs saved[2F]");
    ERC_REQUIRE(N > 0 && F > 0 && F <= 128, "bn_lrelu_fwd: N=%d F=%d unsupported", N, F);
    ERC_REQUIRE(((uintptr_t)ws & 7) == 0, "bn_lrelu_fwd: ws must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)ws;
    if (training) {
        hipLaunchKernelGGL(bn_stats_kernel<0>, dim3(BN_G), dim3(256), 0, st, x, ldx, N, F, gamma, beta, saved, slope,
                           (const float*)nullptr, 0, partial);
        ERC_LAUNCH_CHECK("bn_stats");
    }
    int grid = erc_cdiv(N, 8);
    if (grid > 512) grid = 512;
    hipLaunchKernelGGL(bn_apply_fwd_kernel, dim3(grid), dim3(256), 0, st, x, ldx, N, F, gamma, beta, running_mean,
                       running_var, momentum, eps, slope, training, saved, y, ldy, partial);
    ERC_LAUNCH_CHECK("bn_apply_fwd");
    return ERC_OK;
}

extern "C" int erc_bn_lrelu_bwd(const float* x, int ldx, int N, int F, const float* gamma, const float* beta,
                                const float* saved, float slope, const float* dy, int lddy, float* dx, int lddx,
                                float* dgamma, float* dbeta, float* ws, void* stream) {
    ERC_REQUIRE(x && gamma && beta && saved && dy && dx && dgamma && dbeta && ws, "bn_lrelu_bwd: null pointer");
    ERC_REQUIRE(N > 0 && F > 0 && F <= 128, "bn_lrelu_bwd: N=%d F=%d unsupported", N, F);
    ERC_REQUIRE(((uintptr_t)ws & 7) == 0, "bn_lrelu_bwd: ws must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)ws;
    hipLaunchKernelGGL(bn_stats_kernel<1>, dim3(BN_G), dim3(256), 0, st, x, ldx, N, F, gamma, beta, saved, slope, dy,
                       lddy, partial);
    ERC_LAUNCH_CHECK("bn_bwd_stats");
    int grid = erc_cdiv(N, 8);
    if (grid > 512) grid = 512;
    hipLaunchKernelGGL(bn_apply_bwd_kernel, dim3(grid), dim3(256), 0, st, x, ldx, N, F, gamma, beta, saved, slope, dy,
                       lddy, dx, lddx, dgamma, dbeta, partial);
    ERC_LAUNCH_CHECK("bn_apply_bwd");
    return ERC_OK;
}

extern "C" int erc_cross_entropy(const float* logits, int ld, int C, int n_rows, const int32_t* row_map,
                                 const int64_t* labels, const float* weight, float grad_scale, float* dlogits,
                                 int lddl, float* stats, void* stream) {
    ERC_REQUIRE(logits && labels && stats, "cross_entropy: null pointer");
    ERC_REQUIRE(C > 0 && n_rows > 0 && ld >= C && (!dlogits || lddl >= C), "cross_entropy: C=%d n_rows=%d ld=%d lddl=%d", C, n_rows,
                ld, lddl);
    int grid = erc_cdiv(n_rows, 256);
    if (grid > CE_MAXWG) grid = CE_MAXWG;
    hipLaunchKernelGGL(cross_entropy_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, ld, C, n_rows,
                       row_map, labels, weight, grad_scale, dlogits, lddl, stats, (const int32_t*)nullptr);
    ERC_LAUNCH_CHECK("cross_entropy");
    return ERC_OK;
}

extern "C" int erc_cross_entropy_cap(const float* logits, int ld, int C, int n_cap, const int32_t* n_dev,
                                     const int32_t* row_map, const int64_t* labels, const float* weight, float grad_scale,
                                     float* dlogits, int lddl, float* stats, void* stream) {
    ERC_REQUIRE(logits && labels && stats && n_dev, "cross_entropy_cap: null pointer");
    ERC_REQUIRE(C > 0 && n_cap > 0 && ld >= C && (!dlogits || lddl >= C), "cross_entropy_cap: C=%d n_cap=%d ld=%d lddl=%d", C,
                n_cap, ld, lddl);
    int grid = erc_cdiv(n_cap, 256);
    if (grid > CE_MAXWG) grid = CE_MAXWG;
    hipLaunchKernelGGL(cross_entropy_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, ld, C, n_cap, row_map,
                       labels, weight, grad_scale, dlogits, lddl, stats, n_dev);
    ERC_LAUNCH_CHECK("cross_entropy_cap");
    return ERC_OK;
}

extern "C" int erc_rows_score_max_classes(void) { return RS_MAXC; }

extern "C" int erc_rows_score(const float* logits, int ld, int n_logit_rows, int C, int n_cap, const int32_t* n_dev,
                              const int32_t* row_map, const int64_t* labels, int64_t* cm, void* stream) {
    ERC_REQUIRE(logits && labels && n_dev && cm, "rows_score: null pointer");
    ERC_REQUIRE(C > 0 && C <= RS_MAXC && n_cap > 0 && n_logit_rows > 0 && ld >= C, "rows_score: C=%d n_cap=%d rows=%d ld=%d (C <= %d)",
                C, n_cap, n_logit_rows, ld, RS_MAXC);
    ERC_REQUIRE(((uintptr_t)cm & 7) == 0, "rows_score: cm must be 8-byte aligned");
    int grid = erc_cdiv(n_cap, 256);
    if (grid > RS_MAXWG) grid = RS_MAXWG;
    hipLaunchKernelGGL(rows_score_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, ld, n_logit_rows, C, n_cap, n_dev,
                       row_map, labels, reinterpret_cast<unsigned long long*>(cm));
    ERC_LAUNCH_CHECK("rows_score");
    return ERC_OK;
}

extern "C" int erc_ce_bce_multitask(const float* logits, int ld, int C, int n_rows, const int64_t* labels,
                                    const int64_t* emo_label, int lde, float w_ce, float w_bce, float grad_scale,
                                    float* dlogits, int lddl, float* stats, void* stream) {
    ERC_REQUIRE(logits && labels && emo_label && stats, "ce_bce_multitask: null pointer");
    ERC_REQUIRE(C > 0 && n_rows > 0 && ld >= C + MT_EMO && lde >= MT_EMO && (!dlogits || lddl >= C + MT_EMO),
                "ce_bce_multitask: C=%d n_rows=%d ld=%d lde=%d lddl=%d", C, n_rows, ld, lde, lddl);
    int grid = erc_cdiv(n_rows, 256);
    if (grid > MT_MAXWG) grid = MT_MAXWG;
    hipLaunchKernelGGL(ce_bce_multitask_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, ld, C, n_rows,
                       labels, emo_label, lde, w_ce, w_bce, grad_scale, dlogits, lddl, stats, (const int32_t*)nullptr);
    ERC_LAUNCH_CHECK("ce_bce_multitask");
    return ERC_OK;
}

extern "C" int erc_ce_bce_multitask_cap(const float* logits, int ld, int C, int n_cap, const int32_t* n_dev, const int64_t* labels,
                                        const int64_t* emo_label, int lde, float w_ce, float w_bce, float grad_scale,
                                        float* dlogits, int lddl, float* stats, void* stream) {
    ERC_REQUIRE(logits && labels && emo_label && stats && n_dev, "ce_bce_multitask_cap: null pointer");
    ERC_REQUIRE(C > 0 && n_cap > 0 && ld >= C + MT_EMO && lde >= MT_EMO && (!dlogits || lddl >= C + MT_EMO),
                "ce_bce_multitask_cap: C=%d n_cap=%d ld=%d lde=%d lddl=%d", C, n_cap, ld, lde, lddl);
    int grid = erc_cdiv(n_cap, 256);
    if (grid > MT_MAXWG) grid = MT_MAXWG;
    hipLaunchKernelGGL(ce_bce_multitask_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, ld, C, n_cap, labels,
                       emo_label, lde, w_ce, w_bce, grad_scale, dlogits, lddl, stats, n_dev);
    ERC_LAUNCH_CHECK("ce_bce_multitask_cap");
    return ERC_OK;
}

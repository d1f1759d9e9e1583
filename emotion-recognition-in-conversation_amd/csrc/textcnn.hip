// Text CNN with ReLU and a max over time -- the text encoder of MMIN's full-modality base model (TextCNN(1024, 128),
// track_mm/mmin_models.py:8-40): for k = 3, 4, 5 a Conv2d(1, 128, (k, D)) over the token rows of a sample, ReLU, and
// F.max_pool1d over all T - k + 1 windows; the three [B, 128] results side by side in the order k = 3, 4, 5.
//
// Forward.  Window (b, t) of width k is the contiguous k * D floats that start at row b*T + t of x [B*T, D], so the convolution
// of one k over the whole batch is ONE GEMM whose A operand has row pitch D and K = k * D (overlapping rows): erc_gemm_f32
// (exact fp32 products on the matrix cores, no rounding of the operands) reads A(m, kk) = x[m * D + kk] and puts no bound between
// lda and K.  M = B*T - k + 1 rows: the last window that lies inside the buffer.  Windows that cross into the next sample
// (t > T - k) are computed and never read.  Each product is cut into SPLIT = 8 pieces of K (erc_gemm_f32's split_k): K is
// 3072 .. 5120 long, and one fp32 accumulation chain over all of it loses ~sqrt(K / 4) roundings of a partial sum of the result's
// own size, where eight chains an eighth as long, added in index order, lose a third of that; the cut also gives the launch eight
// times the workgroups (B*T / 16 x 4 tiles do not fill the chip at B = 32).  The partial products land in the caller's scratch conv
// [8][B*T, 384]; one launch then sums them in index order, adds the bias, applies the ReLU and takes the maximum over t and the
// FIRST window that attains it.  A channel whose every window is <= 0 pools to 0 with arg 0; its gradient is 0.
//
// Backward.  dW_k[ch, j, :] = sum_b g[b, ch] x[b, arg[b, ch] + j, :] with g = dpooled where pooled > 0: every (b, ch) picks its
// own rows, so this is a gather, not a GEMM.  One workgroup per (ch, k, j) output row, the samples summed in the fixed order
// b = 0, 1, .. in registers: deterministic, no atomics.  Gradients are WRITTEN (not added).
#include "erc_common.h"

namespace {
constexpr int CH = 128, NK = 3, KMIN = 3, KMAX = 5, W = NK * CH, NJ = 3 + 4 + 5, SPLIT = 8;

struct PoolP {
    const float* conv;        // [SPLIT][B*T, 384] partial products
    const float* bias[NK];    // [128] each
    float* pooled; int ldp;   // [B, 384]
    int32_t* arg;             // [B, 384]
    int B, T;
};

__global__ __launch_bounds__(W) void textcnn_pool_kernel(PoolP p) {
    const int b = blockIdx.x, col = threadIdx.x;
    const int ki = col / CH, k = KMIN + ki;
    const float bias = p.bias[ki][col - ki * CH];
    const float* src = p.conv + (int64_t)b * p.T * W + col;
    float best = 0.f;
    int best_t = 0;
    const int64_t slab = (int64_t)p.B * p.T * W;
    for (int t = 0; t + k <= p.T; ++t) {
        float v = src[(int64_t)t * W];
#pragma unroll
        for (int z = 1; z < SPLIT; ++z) v += src[z * slab + (int64_t)t * W];      // fixed order
        v += bias;
        if (v > best) best = v, best_t = t;      // ReLU: the maximum starts at 0; strict: the first window that attains it
    }
    p.pooled[(int64_t)b * p.ldp + col] = best;
    p.arg[(int64_t)b * W + col] = best_t;
}

struct BwdP {
    const float* x;              // [B*T, D]
    const float* pooled; int ldp;
    const int32_t* arg;
    const float* dpooled; int lddp;
    float* dW[NK];               // [128, k, D]
    float* db[NK];               // [128]
    int B, T, D;
};

template <bool VEC>
__global__ __launch_bounds__(256) void textcnn_bwd_kernel(BwdP p) {
    const int jj = blockIdx.x, ch = blockIdx.y, tid = threadIdx.x;
    const int ki = jj < 3 ? 0 : jj < 7 ? 1 : 2;
    const int k = KMIN + ki, j = jj - (ki == 0 ? 0 : ki == 1 ? 3 : 7);
    const int col = ki * CH + ch;
    float* const out = p.dW[ki] + ((int64_t)ch * k + j) * p.D;
    constexpr int STEP = VEC ? 1024 : 256;
    for (int d0 = 0; d0 < p.D; d0 += STEP) {
        const int d = d0 + (VEC ? 4 * tid : tid);
        f4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int b = 0; b < p.B; ++b) {       // fixed order
            const float g = p.pooled[(int64_t)b * p.ldp + col] > 0.f ? p.dpooled[(int64_t)b * p.lddp + col] : 0.f;
            if (g != 0.f && d < p.D) {
                // arg is a device input no host check sees: kept inside the sample's windows
                const int t = min(max(p.arg[(int64_t)b * W + col], 0), p.T - k) + j;
                const float* xr = p.x + ((int64_t)b * p.T + t) * p.D + d;
                if (VEC) {
                    const f4 xv = *reinterpret_cast<const f4*>(xr);
                    acc.x = fmaf(g, xv.x, acc.x), acc.y = fmaf(g, xv.y, acc.y), acc.z = fmaf(g, xv.z, acc.z), acc.w = fmaf(g, xv.w, acc.w);
                } else {
                    acc.x = fmaf(g, xr[0], acc.x);
                }
            }
        }
        if (d < p.D) {
            if (VEC)
                *reinterpret_cast<f4*>(out + d) = acc;
            else
                out[d] = acc.x;
        }
    }
    if (j == 0 && tid == 0) {
        float s = 0.f;
        for (int b = 0; b < p.B; ++b)
            s += p.pooled[(int64_t)b * p.ldp + col] > 0.f ? p.dpooled[(int64_t)b * p.lddp + col] : 0.f;
        p.db[ki][ch] = s;
    }
}

inline bool al16(const void* q) { return ((uintptr_t)q & 15) == 0; }

}  // namespace

extern "C" int erc_textcnn_min_t(void) { return KMAX; }
extern "C" int erc_textcnn_channels(void) { return CH; }
extern "C" int64_t erc_textcnn_conv_floats(int B, int T) { return B > 0 && T > 0 ? (int64_t)SPLIT * B * T * W : 0; }

extern "C" int erc_textcnn_pool_fwd(const float* x, int B, int T, int D, const float* W3, const float* W4, const float* W5,
                                    const float* b3, const float* b4, const float* b5, float* conv, float* pooled, int ldp,
                                    int32_t* arg, void* stream) {
    ERC_REQUIRE(x && W3 && W4 && W5 && b3 && b4 && b5 && conv && pooled && arg, "textcnn_pool_fwd: null pointer");
    ERC_REQUIRE(T >= KMAX, "textcnn_pool_fwd: T=%d: the widest convolution needs at least %d tokens", T, KMAX);
    ERC_REQUIRE(B > 0 && D > 0 && ldp >= W && (int64_t)B * T <= (int64_t)1 << 24 && (int64_t)KMAX * D <= (int64_t)1 << 24,
                "textcnn_pool_fwd: bad sizes B=%d T=%d D=%d ldp=%d", B, T, D, ldp);
    ERC_REQUIRE(KMIN * D >= 16 * SPLIT, "textcnn_pool_fwd: D=%d: the products are cut into %d pieces of at least 16 k", D, SPLIT);
    const float* Wk[NK] = {W3, W4, W5};
    for (int ki = 0; ki < NK; ++ki) {
        const int k = KMIN + ki;
        if (int e = erc_gemm_f32(x, D, 0, nullptr, Wk[ki], k * D, 0, nullptr, conv + ki * CH, W, B * T - k + 1, CH, k * D, SPLIT,
                                 (int64_t)B * T * W, 0, nullptr, 0, nullptr, 0, nullptr, 0, 1.0f, 0.0f, nullptr, 0, stream))
            return e;
    }
    PoolP p{};
    p.conv = conv; p.bias[0] = b3; p.bias[1] = b4; p.bias[2] = b5; p.pooled = pooled; p.ldp = ldp; p.arg = arg; p.B = B; p.T = T;
    hipLaunchKernelGGL(textcnn_pool_kernel, dim3(B), dim3(W), 0, (hipStream_t)stream, p);
    ERC_LAUNCH_CHECK("textcnn_pool_fwd");
    return ERC_OK;
}

extern "C" int erc_textcnn_pool_bwd(const float* x, int B, int T, int D, const float* pooled, int ldp, const int32_t* arg,
                                    const float* dpooled, int lddp, float* dW3, float* dW4, float* dW5, float* db3, float* db4,
                                    float* db5, void* stream) {
    ERC_REQUIRE(x && pooled && arg && dpooled && dW3 && dW4 && dW5 && db3 && db4 && db5, "textcnn_pool_bwd: null pointer");
    ERC_REQUIRE(T >= KMAX, "textcnn_pool_bwd: T=%d: the widest convolution needs at least %d tokens", T, KMAX);
    ERC_REQUIRE(B > 0 && D > 0 && ldp >= W && lddp >= W && (int64_t)B * T <= (int64_t)1 << 24,
                "textcnn_pool_bwd: bad sizes B=%d T=%d D=%d ldp=%d lddp=%d", B, T, D, ldp, lddp);
    BwdP p{};
    p.x = x; p.pooled = pooled; p.ldp = ldp; p.arg = arg; p.dpooled = dpooled; p.lddp = lddp;
    p.dW[0] = dW3; p.dW[1] = dW4; p.dW[2] = dW5; p.db[0] = db3; p.db[1] = db4; p.db[2] = db5;
    p.B = B; p.T = T; p.D = D;
    const bool vec = D % 4 == 0 && al16(x) && al16(dW3) && al16(dW4) && al16(dW5);
    if (vec)
        hipLaunchKernelGGL(textcnn_bwd_kernel<true>, dim3(NJ, CH), dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(textcnn_bwd_kernel<false>, dim3(NJ, CH), dim3(256), 0, (hipStream_t)stream, p);
    ERC_LAUNCH_CHECK("textcnn_pool_bwd");
    return ERC_OK;
}

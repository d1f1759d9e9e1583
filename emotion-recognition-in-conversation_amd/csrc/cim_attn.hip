// CIM's cross-modal attention (track_mm/cim.py:108-115,160-172) on compact rows, and the node tables of a CIM batch.
//
//   attention_op(x, y, mask):  S = x y^T + (1 - mask_key) (-10000),  P = softmax(S) over keys,  out = (P y) * x
//
// Six ordered pairs per dialogue, (x, y) = av, va, ta, tv, at, vt, written to columns 100 p .. 100 p + 100 of the [N, 900]
// merged buffer; x and y are read from the same buffer's dense block (columns 600 + 100 m, m = a, v, t).  Padded keys get
// exp(s - 10000 - max) = 0 exactly in fp32 and padded query rows are discarded by the reference's final mask, so only the
// L valid rows of each dialogue are touched.
//
// One dialogue's X, Y (L x 100) and P (L x L) sit in LDS: (200 L + L^2 + L) floats, 137 KB at L = 110; dialogues up to
// CIM_MAX_T = 118 fit the 160 KB of a CU, longer batches are refused before launch.
//
// Forward: one workgroup per (dialogue, pair); P is also saved to a [6][B][T][T] scratch for the backward.
// Backward: one workgroup per dialogue, the six pairs in a fixed order.  Every element of the dense gradient
// dmerged[row, 600 + 100 m + 4 k4 .. +4] is read-modified-written by ONE thread (index r * 25 + k4 in every phase of every
// pair), so its contributions -- the classifier's, then per pair the x-side and the y-side terms -- add up in a fixed order
// without atomics: a step is bit-reproducible.  The last phase applies drop1 / ReLU's mask (dense > 0) and the inverted
// dropout scale, leaving the gradient wrt the adapters' pre-activations in the dense block.
//
// Capacity mode launches both kernels with (B_cap, T_cap): a dialogue slot of length 0 (node_off[b + 1] == node_off[b]) leaves
// its workgroups at their first statement -- no softmax over an empty row, nothing read, nothing written.
#include "erc_common.h"
#include "cim_meta.h"

namespace {

constexpr int D = 100;
constexpr int D4 = D / 4;
constexpr int MW = 900;              // merged row pitch
constexpr int CIM_MAX_T = 118;
constexpr int FWD_THREADS = 512;
constexpr int BWD_THREADS = 1024;
__constant__ int c_px[6] = {0, 1, 2, 2, 0, 1};    // av va ta tv at vt (dense block order a=0, v=1, t=2)
__constant__ int c_py[6] = {1, 0, 0, 1, 2, 2};

inline int64_t lds_floats(int T) { return 2 * (int64_t)T * D + (int64_t)T * T + T; }

__device__ __forceinline__ float dot100(const float* a, const float* b) {
    const f4* a4 = reinterpret_cast<const f4*>(a);
    const f4* b4 = reinterpret_cast<const f4*>(b);
    f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 5
    for (int k = 0; k < D4; ++k) acc += a4[k] * b4[k];
    return (acc.x + acc.y) + (acc.z + acc.w);
}

__global__ void cim_meta_kernel(const int64_t* lengths, int B, int T, int n_cap, int32_t* node_off, int32_t* node_row) {
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
    for (int b = threadIdx.x; b <= B; b += blockDim.x) node_off[b] = s_off[b];
    for (int b = 0; b < B; ++b) {
        const int o = s_off[b], L = s_off[b + 1] - o;
        for (int t = threadIdx.x; t < L; t += blockDim.x)
            if (o + t < n_cap) node_row[o + t] = b * T + t;
    }
}

// erc_cim_meta_cap: one workgroup; the arithmetic is cim_meta.h's (a host program runs the same functions)
constexpr int META_THREADS = 1024;

__global__ __launch_bounds__(META_THREADS) void cim_meta_cap_kernel(CimMetaP p) {
    __shared__ int s_off[1025];
    if (threadIdx.x == 0) cim_meta_prefix(p, s_off);
    __syncthreads();
    for (int b = threadIdx.x; b <= p.B; b += META_THREADS) cim_meta_slot(p, s_off, b);
    for (int i = threadIdx.x; i < p.B * p.T; i += META_THREADS) cim_meta_entry(p, s_off, i);
    for (int i = s_off[p.B] + threadIdx.x; i < p.n_cap; i += META_THREADS) cim_meta_tail(p, i);
}

__global__ __launch_bounds__(FWD_THREADS) void cim_attn_fwd_kernel(float* merged, const int32_t* node_off, int T, int B,
                                                                   float* Pbuf) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x, pr = blockIdx.y, tid = threadIdx.x;
    const int base = node_off[b], L = node_off[b + 1] - base;
    if (L <= 0) return;
    float* sX = lds;
    float* sY = sX + T * D;
    float* sP = sY + T * D;
    const int cx = 600 + D * c_px[pr], cy = 600 + D * c_py[pr];
    for (int e = tid; e < L * D4; e += FWD_THREADS) {
        const int r = e / D4, k4 = e % D4;
        const float* src = merged + (int64_t)(base + r) * MW;
        reinterpret_cast<f4*>(sX + r * D)[k4] = reinterpret_cast<const f4*>(src + cx)[k4];
        reinterpret_cast<f4*>(sY + r * D)[k4] = reinterpret_cast<const f4*>(src + cy)[k4];
    }
    __syncthreads();
    for (int e = tid; e < L * L; e += FWD_THREADS) {
        const int i = e / L, j = e % L;
        sP[i * T + j] = dot100(sX + i * D, sY + j * D);
    }
    __syncthreads();
    const int wave = tid / ERC_WAVE, lane = tid % ERC_WAVE;
    float* Pg = Pbuf + ((int64_t)pr * B + b) * T * T;
    for (int i = wave; i < L; i += FWD_THREADS / ERC_WAVE) {
        float* row = sP + i * T;
        const float s0 = lane < L ? row[lane] : -INFINITY, s1 = lane + 64 < L ? row[lane + 64] : -INFINITY;
        const float mx = wave_max(fmaxf(s0, s1));
        const float e0 = lane < L ? expf(s0 - mx) : 0.f, e1 = lane + 64 < L ? expf(s1 - mx) : 0.f;
        const float sum = wave_sum(e0 + e1);
        if (lane < L) row[lane] = e0 / sum, Pg[i * T + lane] = e0 / sum;
        if (lane + 64 < L) row[lane + 64] = e1 / sum, Pg[i * T + lane + 64] = e1 / sum;
    }
    __syncthreads();
    for (int e = tid; e < L * D4; e += FWD_THREADS) {
        const int i = e / D4, k4 = e % D4;
        f4 h = {0.f, 0.f, 0.f, 0.f};
        const float* prow = sP + i * T;
        for (int j = 0; j < L; ++j) h += prow[j] * reinterpret_cast<const f4*>(sY + j * D)[k4];
        reinterpret_cast<f4*>(merged + (int64_t)(base + i) * MW + D * pr)[k4] = h * reinterpret_cast<const f4*>(sX + i * D)[k4];
    }
}

__global__ __launch_bounds__(BWD_THREADS) void cim_attn_bwd_kernel(const float* merged, float* dmerged, const int32_t* node_off,
                                                                   int T, int B, const float* Pbuf, float mask_scale) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int base = node_off[b], L = node_off[b + 1] - base;
    if (L <= 0) return;
    float* sY = lds;
    float* sD = sY + T * D;        // dh = G * x, later x itself
    float* sP = sD + T * D;        // P, then P * dP, then dS
    float* sR = sP + T * T;        // row sums of P * dP
    auto row_m = [&](int r) { return merged + (int64_t)(base + r) * MW; };
    auto row_d = [&](int r) { return dmerged + (int64_t)(base + r) * MW; };
    for (int pr = 0; pr < 6; ++pr) {
        const int cx = 600 + D * c_px[pr], cy = 600 + D * c_py[pr], cg = D * pr;
        const float* Pg = Pbuf + ((int64_t)pr * B + b) * T * T;
        for (int e = tid; e < L * D4; e += BWD_THREADS) {
            const int r = e / D4, k4 = e % D4;
            reinterpret_cast<f4*>(sY + r * D)[k4] = reinterpret_cast<const f4*>(row_m(r) + cy)[k4];
            reinterpret_cast<f4*>(sD + r * D)[k4] =
                reinterpret_cast<const f4*>(row_d(r) + cg)[k4] * reinterpret_cast<const f4*>(row_m(r) + cx)[k4];
        }
        for (int e = tid; e < L * L; e += BWD_THREADS) sP[(e / L) * T + e % L] = Pg[(e / L) * T + e % L];
        __syncthreads();
        // dx += G * (P y)      dy += P^T dh
        for (int e = tid; e < L * D4; e += BWD_THREADS) {
            const int r = e / D4, k4 = e % D4;
            f4 h = {0.f, 0.f, 0.f, 0.f}, dy = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < L; ++j) {
                h += sP[r * T + j] * reinterpret_cast<const f4*>(sY + j * D)[k4];
                dy += sP[j * T + r] * reinterpret_cast<const f4*>(sD + j * D)[k4];
            }
            f4* ox = reinterpret_cast<f4*>(row_d(r) + cx) + k4;
            f4* oy = reinterpret_cast<f4*>(row_d(r) + cy) + k4;
            *ox = *ox + reinterpret_cast<const f4*>(row_d(r) + cg)[k4] * h;
            *oy = *oy + dy;
        }
        __syncthreads();
        // Q = P * (dh y^T)
        for (int e = tid; e < L * L; e += BWD_THREADS) {
            const int i = e / L, j = e % L;
            sP[i * T + j] *= dot100(sD + i * D, sY + j * D);
        }
        __syncthreads();
        for (int i = tid; i < L; i += BWD_THREADS) {
            float acc = 0.f;
            for (int j = 0; j < L; ++j) acc += sP[i * T + j];
            sR[i] = acc;
        }
        __syncthreads();
        // dS = Q - P rowsum(Q); x into the dh slot
        for (int e = tid; e < L * L; e += BWD_THREADS) {
            const int i = e / L, j = e % L;
            sP[i * T + j] -= Pg[i * T + j] * sR[i];
        }
        for (int e = tid; e < L * D4; e += BWD_THREADS) {
            const int r = e / D4, k4 = e % D4;
            reinterpret_cast<f4*>(sD + r * D)[k4] = reinterpret_cast<const f4*>(row_m(r) + cx)[k4];
        }
        __syncthreads();
        // dx += dS y      dy += dS^T x
        for (int e = tid; e < L * D4; e += BWD_THREADS) {
            const int r = e / D4, k4 = e % D4;
            f4 gx = {0.f, 0.f, 0.f, 0.f}, gy = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < L; ++j) {
                gx += sP[r * T + j] * reinterpret_cast<const f4*>(sY + j * D)[k4];
                gy += sP[j * T + r] * reinterpret_cast<const f4*>(sD + j * D)[k4];
            }
            f4* ox = reinterpret_cast<f4*>(row_d(r) + cx) + k4;
            f4* oy = reinterpret_cast<f4*>(row_d(r) + cy) + k4;
            *ox = *ox + gx;
            *oy = *oy + gy;
        }
        __syncthreads();
    }
    // through drop1 and the ReLU: gradient wrt the adapters' pre-activations
    for (int e = tid; e < L * D4; e += BWD_THREADS) {
        const int r = e / D4, k4 = e % D4;
        for (int m = 0; m < 3; ++m) {
            f4* o = reinterpret_cast<f4*>(row_d(r) + 600 + D * m) + k4;
            const f4 v = reinterpret_cast<const f4*>(row_m(r) + 600 + D * m)[k4];
            f4 g = *o;
            g.x = v.x > 0.f ? g.x * mask_scale : 0.f;
            g.y = v.y > 0.f ? g.y * mask_scale : 0.f;
            g.z = v.z > 0.f ? g.z * mask_scale : 0.f;
            g.w = v.w > 0.f ? g.w * mask_scale : 0.f;
            *o = g;
        }
    }
}

bool set_lds(const void* kernel, int64_t bytes) {
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}

}  // namespace

extern "C" int erc_cim_max_t(void) { return CIM_MAX_T; }

extern "C" int erc_cim_meta(const int64_t* lengths, int B, int T, int n_cap, int32_t* node_off, int32_t* node_row,
                            void* stream) {
    ERC_REQUIRE(lengths && node_off && node_row, "cim_meta: null pointer");
    ERC_REQUIRE(B > 0 && B <= 1024 && T > 0 && n_cap > 0, "cim_meta: bad sizes B=%d T=%d n_cap=%d", B, T, n_cap);
    hipLaunchKernelGGL(cim_meta_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, lengths, B, T, n_cap, node_off, node_row);
    ERC_LAUNCH_CHECK("cim_meta");
    return ERC_OK;
}

extern "C" int erc_cim_meta_cap(const int64_t* lengths, const int32_t* desc, const int64_t* store_label, const int64_t* store_emo,
                                int tail_row, int B, int T, int n_cap, int32_t* node_off, int32_t* node_row,
                                int64_t* lengths_out, int64_t* label_out, int64_t* emo_out, int32_t* counts, void* stream) {
    ERC_REQUIRE(node_off && node_row && lengths_out && counts, "cim_meta_cap: null pointer");
    ERC_REQUIRE((lengths != nullptr) != (desc != nullptr),
                "cim_meta_cap: give lengths (bucket form) or desc (resident form), one of them");
    ERC_REQUIRE(desc || !(store_label || store_emo || label_out || emo_out),
                "cim_meta_cap: the bucket form (lengths) gathers no labels: store_label, store_emo, label_out, emo_out are the "
                "resident form's");
    ERC_REQUIRE((store_label != nullptr) == (label_out != nullptr) && (store_emo != nullptr) == (emo_out != nullptr),
                "cim_meta_cap: resident form: store_label with label_out, store_emo with emo_out");
    ERC_REQUIRE(B > 0 && B <= 1024 && T > 0 && n_cap > 0 && (int64_t)n_cap <= (int64_t)B * T,
                "cim_meta_cap: bad sizes B=%d T=%d n_cap=%d (B <= 1024, n_cap <= B * T)", B, T, n_cap);
    ERC_REQUIRE(T <= CIM_MAX_T, "cim_meta_cap: dialogues of up to %d utterances are supported (T_cap=%d)", CIM_MAX_T, T);
    ERC_REQUIRE(tail_row >= 0 && (desc || tail_row <= B * T),
                "cim_meta_cap: tail_row %d is neither a row of the padded block nor the one behind it (%d)", tail_row, B * T);
    CimMetaP p{lengths, desc, store_label, store_emo, tail_row, B, T, n_cap, node_off, node_row, lengths_out, label_out, emo_out,
               counts};
    hipLaunchKernelGGL(cim_meta_cap_kernel, dim3(1), dim3(META_THREADS), 0, (hipStream_t)stream, p);
    ERC_LAUNCH_CHECK("cim_meta_cap");
    return ERC_OK;
}

extern "C" int erc_cim_attn_fwd(float* merged, const int32_t* node_off, int B, int T, float* Pbuf, void* stream) {
    ERC_REQUIRE(merged && node_off && Pbuf, "cim_attn_fwd: null pointer");
    ERC_REQUIRE(B > 0 && T > 0, "cim_attn_fwd: bad sizes B=%d T=%d", B, T);
    ERC_REQUIRE(T <= CIM_MAX_T, "cim_attn_fwd: dialogues of up to %d utterances fit the LDS (batch T=%d)", CIM_MAX_T, T);
    ERC_REQUIRE(((uintptr_t)merged & 15) == 0, "cim_attn_fwd: merged must be 16-byte aligned");
    const int64_t bytes = lds_floats(T) * 4;
    ERC_REQUIRE(set_lds((const void*)cim_attn_fwd_kernel, bytes), "cim_attn_fwd: %lld bytes of LDS refused", (long long)bytes);
    hipLaunchKernelGGL(cim_attn_fwd_kernel, dim3(B, 6), dim3(FWD_THREADS), bytes, (hipStream_t)stream, merged, node_off, T, B, Pbuf);
    ERC_LAUNCH_CHECK("cim_attn_fwd");
    return ERC_OK;
}

extern "C" int erc_cim_attn_bwd(const float* merged, float* dmerged, const int32_t* node_off, int B, int T, const float* Pbuf,
                                float mask_scale, void* stream) {
    ERC_REQUIRE(merged && dmerged && node_off && Pbuf, "cim_attn_bwd: null pointer");
    ERC_REQUIRE(B > 0 && T > 0, "cim_attn_bwd: bad sizes B=%d T=%d", B, T);
    ERC_REQUIRE(T <= CIM_MAX_T, "cim_attn_bwd: dialogues of up to %d utterances fit the LDS (batch T=%d)", CIM_MAX_T, T);
    ERC_REQUIRE((((uintptr_t)merged | (uintptr_t)dmerged) & 15) == 0, "cim_attn_bwd: operands must be 16-byte aligned");
    const int64_t bytes = lds_floats(T) * 4;
    ERC_REQUIRE(set_lds((const void*)cim_attn_bwd_kernel, bytes), "cim_attn_bwd: %lld bytes of LDS refused", (long long)bytes);
    hipLaunchKernelGGL(cim_attn_bwd_kernel, dim3(B), dim3(BWD_THREADS), bytes, (hipStream_t)stream, merged, dmerged, node_off, T, B,
                       Pbuf, mask_scale);
    ERC_LAUNCH_CHECK("cim_attn_bwd");
    return ERC_OK;
}

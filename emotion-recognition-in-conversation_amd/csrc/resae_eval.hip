// Evaluation of MMIN's missing-modality model under missing modalities (erc_amd/mmin_miss.py, --eval_missing): the inference mode
// of the residual autoencoder (the kernel of csrc/resae_dev.h with LATENTS = true: the latents alone), the expansion of a batch's
// features into the six patterns of track_mm/mmin_miss.py:345-360 and the per-pattern scoring.  The reference evaluates
// full-modality only (track_mm/mmin_miss.py:368); the masking restated here is MMINMissCollate's (track_mm/mmin_miss.py:328-337).
#include "resae_dev.h"

// the latents of ResidualAE.forward (mmin_models.py:187-199) alone: what MMINMissModule's classifier reads (mmin_miss.py:103-106)
extern "C" int erc_resae_latents(const ErcResaeJob* job_host, int n_blocks, void* stream) {
    Jobs P;
    int max_b = 0;
    if (int e = fill("resae_latents", P, job_host, 1, n_blocks, FILL_LATENTS, max_b)) return e;
    hipLaunchKernelGGL(resae_fwd_kernel<true>, dim3(erc_cdiv(max_b, R), 1), dim3(NTH), 0, (hipStream_t)stream, P, n_blocks);
    ERC_LAUNCH_CHECK("resae_latents");
    return ERC_OK;
}

// ------------------------------------------------------------------------------------------ evaluation under missing modalities
// MMINMissCollate zeroes a missing modality's input (track_mm/mmin_miss.py:328-337, patterns :345-360) and the zero input still
// runs through its encoder, so its 128 feature columns are one row that depends on the weights alone (audio: and on the batch's
// padded length).  The features of a batch under n_cond patterns are therefore a column-block selection between the batch's
// full-modality features and that row.
namespace {

constexpr int MAX_COND = 8, SCORE_MAXC = 16, SCORE_TH = 256;

struct Patterns {
    int keep[MAX_COND];      // bit 0: visual kept, bit 1: text kept, bit 2: audio kept (the columns of MISSING_TYPES)
};

// Capacity form (erc_mmin_miss_expand_cap: one captured step for every batch of a bucket): B is the bucket's B_cap, the audio
// columns of a removed modality come from row clamp(counts[1], 1, t_rows - 1) of a table of zero-input features per padded
// length (zfeat = that table), the visual and text columns from zvt [256].
struct ExpandExact {
    static constexpr bool CAP = false;
};
struct ExpandCap {
    static constexpr bool CAP = true;
    const float* zvt;
    const int32_t* counts;
    int t_rows;
};

// one thread per 16 bytes of out; feature blocks: audio 0:128, visual 128:256, text 256:384
template <class MODE>
__global__ __launch_bounds__(256) void miss_expand_kernel(const float* __restrict__ feat, const int ldf, const float* __restrict__ zfeat,
                                                          const Patterns pat, const int n_cond, const int B, float* __restrict__ out,
                                                          const int ldo, const MODE mode) {
    constexpr int Q = D / 4;      // 16-byte pieces per row
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)n_cond * B * Q) return;
    const int q = (int)(e % Q);
    const int64_t row = e / Q;
    const int c = (int)(row / B), b = (int)(row % B);
    const int blk = q / (L2 / 4);                            // 0 audio, 1 visual, 2 text
    const int bit = blk == 0 ? 2 : blk - 1;
    const bool keep = (pat.keep[c] >> bit) & 1;
    const float* zsrc = zfeat + 4 * q;
    if constexpr (MODE::CAP) {
        const int ta = min(max(mode.counts[1], 1), mode.t_rows - 1);
        zsrc = blk == 0 ? zfeat + (int64_t)ta * L2 + 4 * q : mode.zvt + (4 * q - L2);
    }
    const f4 v = keep ? *(const f4*)(feat + (int64_t)b * ldf + 4 * q) : *(const f4*)zsrc;
    *(f4*)(out + row * ldo + 4 * q) = v;
}

// workgroup c scores block c of the logits: per row the first index of the maximum (erc_rows_score's rule) and the cross entropy
// in double; thread t takes rows t, t + 256, .. in order, the threads' sums are added in a fixed tree.  cm block c and
// loss_sum[c] belong to this workgroup alone: plain read-modify-write, no atomics on global memory.
// CAP (erc_mmin_miss_score_cap): block c starts at row c * B (B = the bucket's B_cap) and rows b < clamp(counts[0], 0, B) are
// scored, by the same code in the same order: the bits of the exact form at that B on the same rows.
template <bool CAP>
__global__ __launch_bounds__(SCORE_TH) void miss_score_kernel(const float* __restrict__ logits, const int ld, const int64_t* __restrict__ labels,
                                                              const int B, const int C, int64_t* __restrict__ cm,
                                                              double* __restrict__ loss_sum, const int32_t* __restrict__ counts) {
    __shared__ int s_cm[SCORE_MAXC * SCORE_MAXC];
    __shared__ double s_loss[SCORE_TH];
    __shared__ int s_cnt[SCORE_TH];
    const int tid = threadIdx.x, c = blockIdx.x;
    s_cm[tid] = 0;      // 256 threads = SCORE_MAXC^2 cells
    __syncthreads();
    double sum = 0.0;
    int cnt = 0;
    int Bdev = B;
    if constexpr (CAP) Bdev = min(max(counts[0], 0), B);
    for (int b = tid; b < Bdev; b += SCORE_TH) {
        const float* z = logits + ((int64_t)c * B + b) * ld;
        float mx = z[0];
        for (int k = 1; k < C; ++k) mx = fmaxf(mx, z[k]);
        int am = -1;
        for (int k = C - 1; k >= 0; --k)
            if (z[k] == mx) am = k;
        const int64_t y = labels[b];
        if (am < 0 || y < 0 || y >= C) continue;      // not counted: erc_rows_score's rows
        atomicAdd(&s_cm[(int)y * C + am], 1);
        double se = 0.0;
        for (int k = 0; k < C; ++k) se += exp((double)z[k] - (double)mx);
        sum += ((double)mx + log(se)) - (double)z[y];
        ++cnt;
    }
    s_loss[tid] = sum;
    s_cnt[tid] = cnt;
    __syncthreads();
    for (int o = SCORE_TH / 2; o > 0; o >>= 1) {
        if (tid < o) {
            s_loss[tid] += s_loss[tid + o];
            s_cnt[tid] += s_cnt[tid + o];
        }
        __syncthreads();
    }
    if (tid < C * C && s_cm[tid] > 0) cm[(int64_t)c * C * C + tid] += s_cm[tid];
    if (tid == 0 && s_cnt[0] > 0) loss_sum[c] += s_loss[0] / (double)s_cnt[0];
}
static_assert(SCORE_MAXC * SCORE_MAXC == SCORE_TH, "one histogram cell per thread");

}  // namespace

extern "C" int erc_mmin_miss_max_cond(void) { return MAX_COND; }

extern "C" int erc_mmin_miss_expand(const float* feat, int ldf, const float* zfeat, const int32_t* patterns_host, int n_cond, int B,
                                    float* out, int ldo, void* stream) {
    ERC_REQUIRE(feat && zfeat && patterns_host && out, "mmin_miss_expand: null pointer");
    ERC_REQUIRE(n_cond >= 1 && n_cond <= MAX_COND && B > 0, "mmin_miss_expand: n_cond=%d (1..%d) B=%d", n_cond, MAX_COND, B);
    ERC_REQUIRE((int64_t)n_cond * B < ((int64_t)1 << 31), "mmin_miss_expand: n_cond * B = %lld rows", (long long)n_cond * B);
    ERC_REQUIRE(ldf >= D && ldo >= D && ldf % 4 == 0 && ldo % 4 == 0, "mmin_miss_expand: ldf=%d / ldo=%d below %d or no multiple of 4",
                ldf, ldo, D);
    ERC_REQUIRE(aligned16(feat) && aligned16(zfeat) && aligned16(out), "mmin_miss_expand: feat, zfeat, out must be 16-byte aligned");
    Patterns pat{};
    for (int c = 0; c < n_cond; ++c) {
        ERC_REQUIRE(patterns_host[c] >= 0 && patterns_host[c] < 8, "mmin_miss_expand: pattern %d = %d outside [0, 8)", c, patterns_host[c]);
        pat.keep[c] = patterns_host[c];
    }
    const int64_t total = (int64_t)n_cond * B * (D / 4);
    hipLaunchKernelGGL(miss_expand_kernel<ExpandExact>, dim3(erc_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, feat, ldf, zfeat, pat,
                       n_cond, B, out, ldo, ExpandExact{});
    ERC_LAUNCH_CHECK("mmin_miss_expand");
    return ERC_OK;
}

extern "C" int erc_mmin_miss_expand_cap(const float* feat, int ldf, const float* zaudio, int t_rows, const float* zvt,
                                        const int32_t* counts, const int32_t* patterns_host, int n_cond, int B_cap, float* out, int ldo,
                                        void* stream) {
    ERC_REQUIRE(feat && zaudio && zvt && patterns_host && out, "mmin_miss_expand_cap: null pointer");
    ERC_REQUIRE(counts, "mmin_miss_expand_cap: null counts");
    ERC_REQUIRE(t_rows >= 2, "mmin_miss_expand_cap: t_rows=%d: the table has row 0 (unused) and at least row 1", t_rows);
    ERC_REQUIRE(n_cond >= 1 && n_cond <= MAX_COND && B_cap > 0, "mmin_miss_expand_cap: n_cond=%d (1..%d) B_cap=%d", n_cond, MAX_COND, B_cap);
    ERC_REQUIRE((int64_t)n_cond * B_cap < ((int64_t)1 << 31), "mmin_miss_expand_cap: n_cond * B_cap = %lld rows", (long long)n_cond * B_cap);
    ERC_REQUIRE(ldf >= D && ldo >= D && ldf % 4 == 0 && ldo % 4 == 0, "mmin_miss_expand_cap: ldf=%d / ldo=%d below %d or no multiple of 4",
                ldf, ldo, D);
    ERC_REQUIRE(aligned16(feat) && aligned16(zaudio) && aligned16(zvt) && aligned16(out),
                "mmin_miss_expand_cap: feat, zaudio, zvt, out must be 16-byte aligned");
    Patterns pat{};
    for (int c = 0; c < n_cond; ++c) {
        ERC_REQUIRE(patterns_host[c] >= 0 && patterns_host[c] < 8, "mmin_miss_expand_cap: pattern %d = %d outside [0, 8)", c,
                    patterns_host[c]);
        pat.keep[c] = patterns_host[c];
    }
    const int64_t total = (int64_t)n_cond * B_cap * (D / 4);
    hipLaunchKernelGGL(miss_expand_kernel<ExpandCap>, dim3(erc_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, feat, ldf, zaudio, pat,
                       n_cond, B_cap, out, ldo, ExpandCap{zvt, counts, t_rows});
    ERC_LAUNCH_CHECK("mmin_miss_expand_cap");
    return ERC_OK;
}

extern "C" int erc_mmin_miss_score(const float* logits, int ld, const int64_t* labels, int B, int n_cond, int C, int64_t* cm,
                                   double* loss_sum, void* stream) {
    ERC_REQUIRE(logits && labels && cm && loss_sum, "mmin_miss_score: null pointer");
    ERC_REQUIRE(n_cond >= 1 && n_cond <= MAX_COND && B > 0, "mmin_miss_score: n_cond=%d (1..%d) B=%d", n_cond, MAX_COND, B);
    ERC_REQUIRE(C > 0 && C <= erc_rows_score_max_classes() && C <= SCORE_MAXC && ld >= C, "mmin_miss_score: C=%d ld=%d (C <= %d)", C, ld,
                SCORE_MAXC);
    ERC_REQUIRE((((uintptr_t)cm | (uintptr_t)loss_sum | (uintptr_t)labels) & 7) == 0, "mmin_miss_score: labels, cm, loss_sum must be 8-byte aligned");
    hipLaunchKernelGGL(miss_score_kernel<false>, dim3(n_cond), dim3(SCORE_TH), 0, (hipStream_t)stream, logits, ld, labels, B, C, cm, loss_sum,
                       (const int32_t*)nullptr);
    ERC_LAUNCH_CHECK("mmin_miss_score");
    return ERC_OK;
}

extern "C" int erc_mmin_miss_score_cap(const float* logits, int ld, const int64_t* labels, int B_cap, const int32_t* counts, int n_cond,
                                       int C, int64_t* cm, double* loss_sum, void* stream) {
    ERC_REQUIRE(logits && labels && cm && loss_sum, "mmin_miss_score_cap: null pointer");
    ERC_REQUIRE(counts, "mmin_miss_score_cap: null counts");
    ERC_REQUIRE(n_cond >= 1 && n_cond <= MAX_COND && B_cap > 0, "mmin_miss_score_cap: n_cond=%d (1..%d) B_cap=%d", n_cond, MAX_COND, B_cap);
    ERC_REQUIRE((int64_t)n_cond * B_cap < ((int64_t)1 << 31), "mmin_miss_score_cap: n_cond * B_cap = %lld rows", (long long)n_cond * B_cap);
    ERC_REQUIRE(C > 0 && C <= erc_rows_score_max_classes() && C <= SCORE_MAXC && ld >= C, "mmin_miss_score_cap: C=%d ld=%d (C <= %d)", C, ld,
                SCORE_MAXC);
    ERC_REQUIRE((((uintptr_t)cm | (uintptr_t)loss_sum | (uintptr_t)labels) & 7) == 0,
                "mmin_miss_score_cap: labels, cm, loss_sum must be 8-byte aligned");
    hipLaunchKernelGGL(miss_score_kernel<true>, dim3(n_cond), dim3(SCORE_TH), 0, (hipStream_t)stream, logits, ld, labels, B_cap, C, cm,
                       loss_sum, counts);
    ERC_LAUNCH_CHECK("mmin_miss_score_cap");
    return ERC_OK;
}

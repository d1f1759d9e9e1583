// DialogueGCN's tail in EVAL mode, scored on the device, as ONE launch (trainer.ResidentEval): the forward half of
// dgcn_tail.hip with the counting of head.hip's head_eval_kernel behind it
//   Hc = sum of the RGCN slabs + bias                                                   (models/rgcn.py:345-355)
//   GraphConv: AGG_i = sum_{j -> i} Hc_j ; graph_out = W_rel AGG + b + W_root Hc        (dgcn_models.py:42,46)
//   Classifier on [features | graph_out]: Zc = relu(lin1 x) (eval(): no dropout), logits = lin2 Zc   (dgcn_models.py:163-170)
//   pred = first index of the maximum (torch.argmax) ; cm[label][pred] += 1             (mmbase.py:180-201)
// The layout is dgcn_tail.hip's: a workgroup of 8 wavefronts owns 16 rows and sums the Hc rows of its window (+- 10 utterances,
// clipped to the batch) from the slabs into LDS itself; the three products are v_mfma_f32_16x16x4_f32 with the A operand one
// 16-byte LDS read per lane and the weight fragments requested before the LDS-only barrier in front of their phase.  What is
// gone: labels' loss, dropout and its RNG read, the five gradient buffers, the stats exchange between workgroups.  Nothing is
// written but cm and logits; Xc is read-only (graph_out stays in LDS).  Counts are integers: a [8][8] histogram per workgroup in
// LDS, then one 64-bit vector atomic add per non-empty cell -- order-independent, hence deterministic.
// (the tile geometry and the inline product helpers are dgcn_tail_dev.h's, shared with the training kernel)
#include "dgcn_tail_dev.h"

namespace {

struct TailEvalP {
    const float* slabs; int n_slabs; int64_t slab_stride;     // RGCN partial outputs [S][N * 100]
    const float* rgcn_bias;
    const int32_t* in_ptr; const int32_t* in_src;             // CSR by target
    const float* W_rel; const float* b_rel; const float* W_root;   // [100,100] each, [out][in]
    const float* W1; const float* b1;                         // [100,300], [100]
    const float* W2; const float* b2;                         // [C,100], [C]
    const int64_t* labels;
    const int32_t* label_rows;                                // (or null) row i's label is labels[label_rows[i]]
    const int32_t* n_dev;                                     // (or null) the true row count, N below is the capacity
    const float* Xc; int ldx;                                 // [N, >= 200]: columns [0,200) read
    long long* cm;                                            // [C][C] true class x predicted class, added to
    float* logits;                                            // [N][C] or null
    int N, C;
};

// the phases meet at lds_barrier() (erc_common.h): the weight fragments of the NEXT phase stay in flight across it

__global__ __launch_bounds__(TNTH) void dgcn_tail_eval_kernel(const TailEvalP p) {
    __shared__ __attribute__((aligned(16))) float sX[TR * PX];      // [features | graph_out | 0]
    __shared__ __attribute__((aligned(16))) float sHw[TW * PH];     // Hc of the window rows
    __shared__ __attribute__((aligned(16))) float sAGG[TR * PH];
    __shared__ __attribute__((aligned(16))) float sHo[TR * PH];     // Hc of the own rows (zero padded)
    __shared__ __attribute__((aligned(16))) float sZ[TR * PH];
    __shared__ int sPtr[TR + 1];
    __shared__ int sCm[TMAXC * TMAXC];
    float (*const sPart)[TR][17] = reinterpret_cast<float (*)[TR][17]>(sHw);     // lin2 partials: after the AGG sums have read Hc
    int* const sSrc = reinterpret_cast<int*>(sZ);                   // in-edge sources of the tile's rows (Zc: later)
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = p.C, r0 = blockIdx.x * TR;
    // the grid covers p.N rows, the batch the first *n_dev of them
    const int N = p.n_dev ? __builtin_amdgcn_readfirstlane(min(max(p.n_dev[0], 0), p.N)) : p.N;
    if (r0 >= N) return;      // (uniform) no row of this tile counts: nothing else is read
    const int w0 = max(0, r0 - THL), w1 = min(N, r0 + TR + THL);
    // the 16-column tile of the 100-wide products this wavefront owns (wavefront 7: none)
    const int n1 = 16 * wave + l15;
    const bool t1 = wave < TNT, n1v = t1 && n1 < TH;
    const int n1c = min(n1, TH - 1);

    // ---- requests, in the order they are needed: the tile's CSR bounds, the feature columns and lin1's weight fragments for
    //      them (that part of lin1 does not wait for the graph), then the slabs.  Row indices are clamped to N - 1: rows at or
    //      beyond the count are never read
    int my_ptr = 0;
    if (tid <= TR) my_ptr = p.in_ptr[min(r0 + tid, N)];
    float4 xv[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {      // 16 x 77 quads of the [features | graph_out | 0] tile
        const int x = tid + TNTH * u, i = min(x / (PX / 4), TR - 1), c4 = x % (PX / 4);
        xv[u] = *reinterpret_cast<const float4*>(p.Xc + (int64_t)min(r0 + i, N - 1) * p.ldx + 4 * min(c4, TG / 4 - 1));
    }
    constexpr int NGF = 12;            // groups of 16 k that lie inside the 200 feature columns
    float4 bL1[19], bRel[7], bRoot[7];
#pragma unroll
    for (int S = 0; S < NGF; ++S) bL1[S] = wrow4(p.W1, TX, n1c, n1v, 16 * S + 4 * kq, TX);
    // window row i, column quad c4 of items x = tid and tid + 512 (900 items); up to 8 slabs per pass, all requested at once
    float4 sv[2][8];
    const int n_sl = p.n_slabs;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int x = tid + TNTH * u, i = min(x / (TH / 4), TW - 1), c4 = x % (TH / 4);
        const float* src = p.slabs + (int64_t)min(w0 + i, N - 1) * TH + 4 * c4;
#pragma unroll
        for (int s = 0; s < 8; ++s) sv[u][s] = *reinterpret_cast<const float4*>(src + min(s, n_sl - 1) * p.slab_stride);
    }
    if (tid <= TR) sPtr[tid] = my_ptr;
    if (tid < TMAXC * TMAXC) sCm[tid] = 0;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int x = tid + TNTH * u, i = x / (PX / 4), c4 = x % (PX / 4);
        if (x < TR * (PX / 4)) {
            const bool v = r0 + i < N && 4 * c4 < TG;
            *reinterpret_cast<float4*>(sX + i * PX + 4 * c4) = v ? xv[u] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    // the GraphConv weight fragments, the biases, the labels of the rows this wavefront scores
#pragma unroll
    for (int S = 0; S < 7; ++S) {
        bRel[S] = wrow4(p.W_rel, TH, n1c, n1v, 16 * S + 4 * kq, TH);
        bRoot[S] = wrow4(p.W_root, TH, n1c, n1v, 16 * S + 4 * kq, TH);
    }
    const float bias_rel = p.b_rel[n1c], bias_1 = p.b1[n1c], bias_2 = p.b2[min(l15, C - 1)];
    // scoring: wavefront w < 4 takes rows 4 (lane >> 4) + w
    const int sc_row = 4 * kq + min(wave, 3);
    const bool sc_rv = r0 + sc_row < N;
    int sc_y = -1;
    if (wave < 4) {
        const int i = min(r0 + sc_row, N - 1);
        sc_y = (int)p.labels[p.label_rows ? p.label_rows[i] : i];
    }
    lds_barrier();
    const int e_lo = sPtr[0], n_e = min(sPtr[min(TR, N - r0)] - e_lo, TR * PH);
    int my_src = 0;
    if (tid < n_e) my_src = p.in_src[e_lo + tid];
    // ---- lin1, the feature columns (while the edge list travels)
    f32x4 acc1 = {0.f, 0.f, 0.f, 0.f};
    if (t1) {
#pragma unroll
        for (int S = 0; S < NGF; ++S) {
            const float4 a = *reinterpret_cast<const float4*>(sX + l15 * PX + 16 * S + 4 * kq);
            acc1 = mfma4(a, bL1[S], acc1);
        }
    }
#pragma unroll
    for (int S = NGF; S < 19; ++S) bL1[S] = wrow4(p.W1, TX, n1c, n1v, 16 * S + 4 * kq, TX);
    // ---- Hc = sum of the slabs + bias (slab order, bias last: as erc_slab_reduce); window rows outside [0, N): 0
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int x = tid + TNTH * u, i = x / (TH / 4), c4 = x % (TH / 4);
        if (x < TW * (TH / 4)) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            if (w0 + i < w1) {
#pragma unroll
                for (int s = 0; s < 8; ++s)
                    if (s < n_sl) acc.x += sv[u][s].x, acc.y += sv[u][s].y, acc.z += sv[u][s].z, acc.w += sv[u][s].w;
                for (int s = 8; s < n_sl; ++s) {      // (more than 8 partial outputs)
                    const float4 v = *reinterpret_cast<const float4*>(p.slabs + s * p.slab_stride + (int64_t)(w0 + i) * TH + 4 * c4);
                    acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
                }
                const float4 b = *reinterpret_cast<const float4*>(p.rgcn_bias + 4 * c4);
                acc.x += b.x, acc.y += b.y, acc.z += b.z, acc.w += b.w;
            }
            *reinterpret_cast<float4*>(sHw + i * PH + 4 * c4) = acc;
        }
    }
    for (int x = tid; x < TR * (PH - TH); x += TNTH) {       // K padding of the 100-wide A tiles
        const int i = x / (PH - TH), c = TH + x % (PH - TH);
        sAGG[i * PH + c] = 0.f, sHo[i * PH + c] = 0.f;
    }
    if (tid < n_e) sSrc[tid] = my_src;
    for (int x = tid + TNTH; x < n_e; x += TNTH) sSrc[x] = p.in_src[e_lo + x];
    lds_barrier();
    // ---- AGG_i = sum over the in-edges' source rows (LDS only); the own Hc rows as an A tile
    for (int x = tid; x < TR * (TH / 4); x += TNTH) {
        const int i = x / (TH / 4), c4 = x % (TH / 4);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), own = acc;
        if (r0 + i < N) {
            const int e0 = max(sPtr[i] - e_lo, 0), e1 = min(sPtr[i + 1] - e_lo, n_e);
            for (int e = e0; e < e1; ++e) {
                const int j = min(max(sSrc[e] - w0, 0), TW - 1);
                const float4 v = *reinterpret_cast<const float4*>(sHw + j * PH + 4 * c4);
                acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
            }
            own = *reinterpret_cast<const float4*>(sHw + (r0 + i - w0) * PH + 4 * c4);
        }
        *reinterpret_cast<float4*>(sAGG + i * PH + 4 * c4) = acc;
        *reinterpret_cast<float4*>(sHo + i * PH + 4 * c4) = own;
    }
    lds_barrier();
    for (int x = tid; x < TR * (PH - TH); x += TNTH) sZ[(x / (PH - TH)) * PH + TH + x % (PH - TH)] = 0.f;   // (the edge list is done)

    // ---- GraphConv: graph_out = AGG W_rel^T + b + Hc W_root^T, into the LDS tile only
    if (t1) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = tile_product<7>(sAGG, PH, l15, kq, bRel, acc);
        acc = tile_product<7>(sHo, PH, l15, kq, bRoot, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (n1v) sX[(4 * kq + r) * PX + TG + n1] = acc[r] + bias_rel;
    }
    // request for the phase behind lin1: lin2's K group of this wavefront
    const bool cv2 = l15 < C;
    const float4 bL2 = wrow4(p.W2, TH, min(l15, C - 1), t1 && cv2, 16 * wave + 4 * kq, TH);
    lds_barrier();

    // ---- lin1 + ReLU (no dropout, no RNG read)
    if (t1) {
        f32x4 acc = acc1;
#pragma unroll
        for (int S = NGF; S < 19; ++S) {       // the graph_out columns (and the last 8 feature columns)
            const float4 a = *reinterpret_cast<const float4*>(sX + l15 * PX + 16 * S + 4 * kq);
            acc = mfma4(a, bL1[S], acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (n1v) sZ[(4 * kq + r) * PH + n1] = fmaxf(acc[r] + bias_1, 0.f);
    }
    lds_barrier();

    // ---- lin2 (K split over the wavefronts)
    {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (t1) {
            const float4 a = *reinterpret_cast<const float4*>(sZ + l15 * PH + 16 * wave + 4 * kq);
            acc = mfma4(a, bL2, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) sPart[wave][4 * kq + r][l15] = acc[r];
    }
    lds_barrier();
    // ---- logits with one class per lane, the first index of the maximum, the workgroup's histogram
    if (wave < 4) {
        const bool cv = l15 < C;
        float lg = bias_2;
#pragma unroll
        for (int w = 0; w < TNT; ++w) lg += sPart[w][sc_row][l15];
        float mx = cv ? lg : -INFINITY;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        int am = (cv && lg == mx) ? l15 : 99;      // the lowest index among equal maxima
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) am = min(am, __shfl_xor(am, o, 64));
        if (cv && sc_rv && p.logits) p.logits[(int64_t)(r0 + sc_row) * C + l15] = lg;
        if (sc_rv && l15 == 0 && sc_y >= 0 && sc_y < C && am < C) atomicAdd(&sCm[sc_y * TMAXC + am], 1);
    }
    __syncthreads();
    if (tid < TMAXC * TMAXC) {
        const int y = tid >> 3, c = tid & 7, cnt = sCm[tid];
        if (cnt > 0 && y < C && c < C) atomicAdd(reinterpret_cast<unsigned long long*>(p.cm + y * C + c), (unsigned long long)cnt);
    }
}

inline bool al16(const void* q) { return ((uintptr_t)q & 15) == 0; }

}  // namespace

extern "C" int erc_dgcn_tail_eval(const float* slabs, int n_slabs, int64_t slab_stride, const float* rgcn_bias, const int32_t* in_ptr,
                                  const int32_t* in_src, int window, const float* W_rel, const float* b_rel, const float* W_root,
                                  const float* W1, const float* b1, const float* W2, const float* b2, const int64_t* labels,
                                  const int32_t* label_rows, int n_classes, int n_rows, const int32_t* n_dev, const float* Xc,
                                  int ldx, int64_t* cm, float* logits, void* stream) {
    ERC_REQUIRE(slabs && rgcn_bias && in_ptr && in_src && W_rel && b_rel && W_root && W1 && b1 && W2 && b2 && labels && Xc && cm,
                "dgcn_tail_eval: null pointer");
    ERC_REQUIRE(n_rows >= 0 && n_rows <= erc_dgcn_tail_max_rows() && n_classes > 0 && n_classes <= TMAXC && n_slabs >= 1,
                "dgcn_tail_eval: n_rows=%d n_classes=%d n_slabs=%d unsupported (n_rows <= %d, n_classes <= %d)", n_rows, n_classes,
                n_slabs, erc_dgcn_tail_max_rows(), TMAXC);
    ERC_REQUIRE(window >= 0 && window <= THL && window <= erc_dgcn_tail_max_window(),
                "dgcn_tail_eval: window %d (the kernel holds %d rows either side)", window, THL);
    ERC_REQUIRE(ldx >= TG && ldx % 4 == 0 && slab_stride % 4 == 0, "dgcn_tail_eval: ldx=%d slab_stride=%lld", ldx, (long long)slab_stride);
    ERC_REQUIRE(al16(slabs) && al16(rgcn_bias) && al16(W_rel) && al16(W_root) && al16(W1) && al16(W2) && al16(Xc) &&
                    ((uintptr_t)cm & 7) == 0, "dgcn_tail_eval: 16-byte alignment (slabs, rgcn_bias, weights, Xc), 8-byte (cm)");
    if (n_rows == 0) return ERC_OK;      // (no rows: no launch)
    TailEvalP p;
    p.slabs = slabs; p.n_slabs = n_slabs; p.slab_stride = slab_stride; p.rgcn_bias = rgcn_bias; p.in_ptr = in_ptr; p.in_src = in_src;
    p.W_rel = W_rel; p.b_rel = b_rel; p.W_root = W_root; p.W1 = W1; p.b1 = b1; p.W2 = W2; p.b2 = b2; p.labels = labels;
    p.label_rows = label_rows; p.n_dev = n_dev; p.Xc = Xc; p.ldx = ldx; p.cm = reinterpret_cast<long long*>(cm); p.logits = logits;
    p.N = n_rows; p.C = n_classes;
    hipLaunchKernelGGL(dgcn_tail_eval_kernel, dim3(erc_cdiv(n_rows, TR)), dim3(TNTH), 0, (hipStream_t)stream, p);
    ERC_LAUNCH_CHECK("dgcn_tail_eval");
    return ERC_OK;
}

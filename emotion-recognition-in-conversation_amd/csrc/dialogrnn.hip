// DialogueRNN (track_mm/dgcnv2_models.py:235-347 DialogueRNNCell / DialogueRNN, :428-487 DialogRNNModel) for the built
// configuration: context_attention='general', listener_state=False, D_g = D_p = 150, D_e = 100.
//
// Per direction, dialogue and scan step s (u = utterance row, p = its speaker, torch GRUCell semantics, gate order r|z|n):
//     g_s  = GRU_g([u ; q[p]], g'_{s-1})              g'_s = drop(g_s)
//     c_s  = sum_{j<s} softmax_j((W_a u) . g'_j) g'_j   (c_0 = 0)
//     q[p] = drop(GRU_p([u ; c_s], q[p]))             only the speaker's party (the reference evaluates every party, :289-304)
//     e_s  = drop(GRU_e(q[p], e'_{s-1}))              emotions = drop_rec(e'_s)  (:465,470)
// The reverse direction walks a dialogue from its own last valid utterance (_reverse_seq, :445-457); padded steps are never
// run.  The u-side products W_ih^g[:, :D_m] u + b_ih^g, W_ih^p[:, :D_m] u + b_ih^p and W_a u are hoisted: GX [N, 2100],
// direction d in columns [1050 d, 1050 d + 1050) as gi_g 450 | gi_p 450 | a 150, GEMMs over the N valid rows by the caller.
//
// Form of the scan (the one of gru.hip): one workgroup of 1024 threads per (dialogue, direction), no hand-off between
// workgroups, so nothing waits.  The history of g' (110 x 150 fp32 = 66 KB) lives in LDS; the six recurrent blocks of a
// direction (345 000 floats, 1.38 MB: more than the LDS and the register file of a CU together) are streamed from L2 every
// step.  The forward reads transposed copies (erc_dialogrnn_pack: thread = a pair of gate rows, a wavefront's loads are 512
// contiguous bytes); the backward needs W^T g, for which the [rows, K] layout is the coalesced one (thread = a pair of
// columns) -- it reads contiguous copies from the same pack, so the state columns of W_ih^g / W_ih^p lose their D_m + 150 pitch.
// A step is a chain of phases separated by workgroup barriers:
//   forward   {W_gq q, W_gh g', W_ph q, W_eh e', scores} | {softmax, g gates} | c partials | c | W_pc c | p gates | W_ei q | e gates
//   backward  {e, g gate gradients} | {W_eh^T, W_ei^T, W_gh^T, W_gq^T} | {p gate gradients, d g'_{s-1}} | {W_pc^T, W_ph^T} |
//             {dc, dq[p]} | d alpha | d scores | {d a, d g'_j += alpha_j dc + dscore_j a for every j < s}
// The backward keeps g'_j (read back from the forward's save) and its gradient in LDS for the whole dialogue (2 x [110][150],
// 156 KB of the CU's 160 with the step's vectors); step s adds its attention's share to the gradient of every j < s,
// each element owned by one thread, steps in descending order: the re-association dag_rec.hip describes, with a fixed
// summation order and no atomics.  The gradient of q[party] is one LDS row per party: step s consumes the row of its
// speaker (written by the later steps of that party: next global cell + party cell) and replaces it.
#include "erc_common.h"

namespace {

constexpr int DG = 150;            // D_g = D_p
constexpr int DE = 100;            // D_e
constexpr int G3 = 450, E3 = 300;
constexpr int MAXT = 110, MAXS = 9;
constexpr int NT = 1024;
constexpr int GXW = 1050;          // hoisted columns per direction: gi_g 450 | gi_p 450 | a 150
constexpr int WT_DIR = 345000;     // packed transposed blocks per direction
constexpr int WT_GQ = 0, WT_GH = 67500, WT_PC = 135000, WT_PH = 202500, WT_EI = 270000, WT_EH = 315000;
// planes of the save buffer (ercgraft.h): plane f = [2][N][width], first float at offset(f) * 2N
constexpr int SV_GATES_G = 0, SV_GHN_G = 450, SV_GPREV = 600, SV_GPRE = 750, SV_GD = 900, SV_C = 1050, SV_GATES_P = 1200,
              SV_GHN_P = 1650, SV_QPREV = 1800, SV_QPRE = 1950, SV_QD = 2100, SV_GATES_E = 2250, SV_GHN_E = 2550, SV_EPREV = 2650,
              SV_EPRE = 2750, SV_ED = 2850, SV_ROW = 2950;
constexpr int DR_GH_G = 0, DR_GH_P = 450, DR_GI_E = 900, DR_GH_E = 1200, DR_ROW = 1500;
// parameter offsets per direction (floats from `params`)
enum { O_WIH_G, O_WHH_G, O_BHH_G, O_WIH_P, O_WHH_P, O_BHH_P, O_WIH_E, O_WHH_E, O_BIH_E, O_BHH_E, O_N };

struct DrnnP {
    const float* GX; int ldgx;
    const float* WT;
    const float* params; int64_t off[2 * O_N]; int Dm;
    const int32_t* node_off; const int32_t* node_spk;
    int B, T, S; int64_t N;
    float drop_p, drop_rec; const uint64_t* rng; uint64_t rng_stream;
    float* emo; int lde;
    float* save;
    const float* dEmo; int ldde;
    float* dGX; int lddgx;
    float* dREC;
    const int32_t* n_dev;      // capacity form of the backward: the batch's node count (device); N is then the capacity
};

// which: 0 g, 1 q[p], 2 e, 3 emotions
__device__ __forceinline__ bool kept(uint64_t seed, uint64_t off, int64_t row, int which, int u, float p) {
    return erc_uniform(seed, off, ((uint64_t)row * 4 + which) * 160 + u) >= p;
}

__device__ __forceinline__ float* plane(float* base, int off, int w, int64_t N, int d, int64_t row) {
    return base + (int64_t)off * 2 * N + ((int64_t)d * N + row) * w;
}

// rows 2 jp, 2 jp + 1 of the transposed block: out = sum_k WT[k * rows + 2 jp ..] x[k0 + k]  (8-byte loads; rows is even)
__device__ __forceinline__ f2 dot_t2(const float* __restrict__ WT, int rows, int jp, const float* x, int k0, int nk) {
    f2 acc = {0.f, 0.f};
    const f2* w = reinterpret_cast<const f2*>(WT + (int64_t)k0 * rows) + jp;
    const int pitch = rows / 2;
#pragma unroll 10
    for (int k = 0; k < nk; ++k) acc += w[k * pitch] * x[k0 + k];
    return acc;
}

// columns 2 kp, 2 kp + 1 of the row-major block [rows, ld]: out = sum_j W[(j0 + j) * ld + 2 kp ..] x[j0 + j]  (ld is even)
__device__ __forceinline__ f2 dot_n2(const float* __restrict__ W, int ld, int kp, const float* x, int j0, int nj) {
    f2 acc = {0.f, 0.f};
    const f2* w = reinterpret_cast<const f2*>(W + (int64_t)j0 * ld) + kp;
    const int pitch = ld / 2;
#pragma unroll 10
    for (int j = 0; j < nj; ++j) acc += w[j * pitch] * x[j0 + j];
    return acc;
}

constexpr int FWD_LDS_FLOATS = MAXT * DG + 1664 + 1352 + 152 + 104 + 900 + 152 + 112 + 112 + 1352 + 1800;

__global__ __launch_bounds__(NT) void drnn_fwd_kernel(DrnnP p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* hist = sm;                  // [MAXT][DG]  g' of the steps so far
    float* sA = hist + MAXT * DG;      // W_gq q 450 | W_gh g' 450 | W_ph q 450 | W_eh e' 300
    float* sQ = sA + 1664;             // [MAXS][DG]  party states
    float* sG = sQ + 1352;             // g'_{s-1}
    float* sE = sG + 152;              // e'_{s-1}
    float* sCp = sE + 104;             // [6][DG]     partial context sums
    float* sC = sCp + 900;             // c_s
    float* sSc = sC + 152;             // scores
    float* sAl = sSc + 112;            // alpha
    float* sP5 = sAl + 112;            // [3][450]    W_pc c, three thirds of k
    float* sP6 = sP5 + 1352;           // [6][300]    W_ei q, six parts of k
    const int b = blockIdx.x, d = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t N = p.N;
    const int base = p.node_off[b];
    int L = min(p.node_off[b + 1] - base, min(p.T, MAXT));
    if (base < 0 || base + L > N) L = 0;
    const float* WT = p.WT + (int64_t)d * WT_DIR;
    const int64_t* off = p.off + d * O_N;
    const float* bhg = p.params + off[O_BHH_G];
    const float* bhp = p.params + off[O_BHH_P];
    const float* bie = p.params + off[O_BIH_E];
    const float* bhe = p.params + off[O_BHH_E];
    const bool dropping = p.drop_p > 0.f, dropping_rec = p.drop_rec > 0.f;
    uint64_t roff = 0, rseed = 0;
    if (dropping || dropping_rec) roff = p.rng[0], rseed = p.rng[1] ^ (p.rng_stream + (uint64_t)d);
    const float ks = dropping ? 1.0f / (1.0f - p.drop_p) : 1.0f, ks_rec = dropping_rec ? 1.0f / (1.0f - p.drop_rec) : 1.0f;
    for (int i = tid; i < MAXS * DG; i += NT) sQ[i] = 0.f;
    if (tid < DG) sG[tid] = 0.f;
    if (tid < DE) sE[tid] = 0.f;
    __syncthreads();
    for (int s = 0; s < L; ++s) {
        const int t = d == 0 ? s : L - 1 - s;
        const int64_t row = base + t;
        const int spk = min(max(p.node_spk[row], 0), min(p.S, MAXS) - 1);
        const float* gx = p.GX + row * p.ldgx + d * GXW;
        const float* q = sQ + spk * DG;
        // ---- the four products that only need the previous state, and the attention scores over the history
        if (s > 0) {
            const float a0 = gx[900 + lane], a1 = gx[964 + lane], a2 = lane < 22 ? gx[1028 + lane] : 0.f;
            for (int j = wave; j < s; j += NT / 64) {
                const float* h = hist + j * DG;
                float v = a0 * h[lane] + a1 * h[64 + lane] + (lane < 22 ? a2 * h[128 + lane] : 0.f);
                v = wave_sum(v);
                if (lane == 0) sSc[j] = v;
            }
        }
        if (tid < 825) {               // one thread per pair of gate rows: 225 + 225 + 225 + 150
            f2 v;
            if (tid < 225) v = dot_t2(WT + WT_GQ, G3, tid, q, 0, DG);
            else if (tid < 450) v = dot_t2(WT + WT_GH, G3, tid - 225, sG, 0, DG);
            else if (tid < 675) v = dot_t2(WT + WT_PH, G3, tid - 450, q, 0, DG);
            else v = dot_t2(WT + WT_EH, E3, tid - 675, sE, 0, DE);
            sA[2 * tid] = v.x, sA[2 * tid + 1] = v.y;
        }
        __syncthreads();
        // ---- softmax (wave 0) next to the gates of the global cell (threads 256..405)
        if (wave == 0 && s > 0) {
            const float x0 = lane < s ? sSc[lane] : -INFINITY, x1 = lane + 64 < s ? sSc[lane + 64] : -INFINITY;
            const float mx = wave_max(fmaxf(x0, x1));
            const float e0 = lane < s ? expf(x0 - mx) : 0.f, e1 = lane + 64 < s ? expf(x1 - mx) : 0.f;
            const float inv = 1.0f / wave_sum(e0 + e1);
            float* al = p.save + (int64_t)SV_ROW * 2 * N + (((int64_t)d * p.B + b) * p.T + s) * p.T;
            if (lane < s) sAl[lane] = e0 * inv, al[lane] = e0 * inv;
            if (lane + 64 < s) sAl[lane + 64] = e1 * inv, al[lane + 64] = e1 * inv;
        }
        if (tid >= 256 && tid < 256 + DG) {
            const int u = tid - 256;
            const float r = sigm(gx[u] + sA[u] + sA[450 + u] + bhg[u]);
            const float z = sigm(gx[DG + u] + sA[DG + u] + sA[450 + DG + u] + bhg[DG + u]);
            const float gn = sA[450 + 2 * DG + u] + bhg[2 * DG + u];
            const float n = tanhf(gx[2 * DG + u] + sA[2 * DG + u] + r * gn);
            const float hp = sG[u];
            const float g = (1.f - z) * n + z * hp;
            const float gd = dropping ? (kept(rseed, roff, row, 0, u, p.drop_p) ? g * ks : 0.f) : g;
            float* gt = plane(p.save, SV_GATES_G, G3, N, d, row);
            gt[u] = r, gt[DG + u] = z, gt[2 * DG + u] = n;
            plane(p.save, SV_GHN_G, DG, N, d, row)[u] = gn;
            plane(p.save, SV_GPREV, DG, N, d, row)[u] = hp;
            plane(p.save, SV_GPRE, DG, N, d, row)[u] = g;
            plane(p.save, SV_GD, DG, N, d, row)[u] = gd;
            hist[s * DG + u] = gd;       // the scores of this step (j < s) are done; the context below reads j < s only
            sG[u] = gd;
        }
        __syncthreads();
        if (s > 0) {
            // ---- c_s = sum_j alpha_j g'_j: six partial sums over j, then their sum
            if (tid < 6 * DG) {
                const int part = tid / DG, k = tid % DG;
                const int per = (s + 5) / 6, j0 = part * per, j1 = min(s, j0 + per);
                float acc = 0.f;
                for (int j = j0; j < j1; ++j) acc = fmaf(sAl[j], hist[j * DG + k], acc);
                sCp[tid] = acc;
            }
            __syncthreads();
            if (tid < DG) {
                float c = sCp[tid];
#pragma unroll
                for (int q6 = 1; q6 < 6; ++q6) c += sCp[q6 * DG + tid];
                sC[tid] = c;
                plane(p.save, SV_C, DG, N, d, row)[tid] = c;
            }
            __syncthreads();
            if (tid < 675) {
                const int part = tid / 225, jp = tid % 225;
                const f2 v = dot_t2(WT + WT_PC, G3, jp, sC, part * 50, 50);
                sP5[part * G3 + 2 * jp] = v.x, sP5[part * G3 + 2 * jp + 1] = v.y;
            }
            __syncthreads();
        } else if (tid < DG) {
            plane(p.save, SV_C, DG, N, d, row)[tid] = 0.f;
        }
        // ---- party cell of the speaker
        if (tid < DG) {
            const int u = tid;
            float ir = gx[G3 + u], iz = gx[G3 + DG + u], in = gx[G3 + 2 * DG + u];
            if (s > 0) {
                ir += (sP5[u] + sP5[G3 + u]) + sP5[2 * G3 + u];
                iz += (sP5[DG + u] + sP5[G3 + DG + u]) + sP5[2 * G3 + DG + u];
                in += (sP5[2 * DG + u] + sP5[G3 + 2 * DG + u]) + sP5[2 * G3 + 2 * DG + u];
            }
            const float r = sigm(ir + sA[900 + u] + bhp[u]);
            const float z = sigm(iz + sA[900 + DG + u] + bhp[DG + u]);
            const float gn = sA[900 + 2 * DG + u] + bhp[2 * DG + u];
            const float n = tanhf(in + r * gn);
            const float hp = q[u];
            const float qn = (1.f - z) * n + z * hp;
            const float qd = dropping ? (kept(rseed, roff, row, 1, u, p.drop_p) ? qn * ks : 0.f) : qn;
            float* gt = plane(p.save, SV_GATES_P, G3, N, d, row);
            gt[u] = r, gt[DG + u] = z, gt[2 * DG + u] = n;
            plane(p.save, SV_GHN_P, DG, N, d, row)[u] = gn;
            plane(p.save, SV_QPREV, DG, N, d, row)[u] = hp;
            plane(p.save, SV_QPRE, DG, N, d, row)[u] = qn;
            plane(p.save, SV_QD, DG, N, d, row)[u] = qd;
            sQ[spk * DG + u] = qd;
        }
        __syncthreads();
        // ---- emotion cell
        if (tid < 900) {
            const int part = tid / 150, jp = tid % 150;
            const f2 v = dot_t2(WT + WT_EI, E3, jp, q, part * 25, 25);
            sP6[part * E3 + 2 * jp] = v.x, sP6[part * E3 + 2 * jp + 1] = v.y;
        }
        __syncthreads();
        if (tid < DE) {
            const int u = tid;
            float ir = bie[u], iz = bie[DE + u], in = bie[2 * DE + u];
#pragma unroll
            for (int q6 = 0; q6 < 6; ++q6) ir += sP6[q6 * E3 + u], iz += sP6[q6 * E3 + DE + u], in += sP6[q6 * E3 + 2 * DE + u];
            const float r = sigm(ir + sA[1350 + u] + bhe[u]);
            const float z = sigm(iz + sA[1350 + DE + u] + bhe[DE + u]);
            const float gn = sA[1350 + 2 * DE + u] + bhe[2 * DE + u];
            const float n = tanhf(in + r * gn);
            const float hp = sE[u];
            const float e = (1.f - z) * n + z * hp;
            const float ed = dropping ? (kept(rseed, roff, row, 2, u, p.drop_p) ? e * ks : 0.f) : e;
            float* gt = plane(p.save, SV_GATES_E, E3, N, d, row);
            gt[u] = r, gt[DE + u] = z, gt[2 * DE + u] = n;
            plane(p.save, SV_GHN_E, DE, N, d, row)[u] = gn;
            plane(p.save, SV_EPREV, DE, N, d, row)[u] = hp;
            plane(p.save, SV_EPRE, DE, N, d, row)[u] = e;
            plane(p.save, SV_ED, DE, N, d, row)[u] = ed;
            sE[u] = ed;
            p.emo[row * p.lde + d * DE + u] = dropping_rec ? (kept(rseed, roff, row, 3, u, p.drop_rec) ? ed * ks_rec : 0.f) : ed;
        }
        __syncthreads();
    }
}

constexpr int BWD_LDS_FLOATS = 2 * MAXT * DG + 1352 + 304 + 304 + 4 * 452 + 1800 + 152 + 152 + 112 + 112 + 112;   // 157 KB

// +0 over n floats at p (4-byte aligned), by thread t of nt: single floats up to the first 16-byte boundary and behind the
// last, 16-byte stores between
__device__ __forceinline__ void zero_range(float* p, int64_t n, int64_t t, int64_t nt) {
    const int64_t head = min(n, (int64_t)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2));
    const int64_t n4 = (n - head) >> 2;
    if (t < head) p[t] = 0.f;
    float4* q = reinterpret_cast<float4*>(p + head);
    for (int64_t i = t; i < n4; i += nt) q[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t done = head + 4 * n4;
    if (t < n - done) p[done + t] = 0.f;
}

constexpr int TAIL_WG = 16;            // the capacity form's tails are owned by this many workgroups, whatever B is

// +0 to the rows [*n_dev, N) of dGX (columns [0, 2100)) and of the four dREC planes of both directions: one contiguous range per
// (plane, direction), dGX too when its pitch is 2100.  Thread t of nt.
__device__ __forceinline__ void drnn_zero_tails(float* dGX, int lddgx, float* dREC, int64_t N, const int32_t* n_dev, int64_t t,
                                                int64_t nt) {
    const int64_t n = min(max((int64_t)n_dev[0], (int64_t)0), N), rows = N - n;
    if (rows <= 0) return;
    constexpr int DR_OFF[4] = {DR_GH_G, DR_GH_P, DR_GI_E, DR_GH_E}, DR_W[4] = {G3, G3, E3, E3};
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int d = 0; d < 2; ++d) zero_range(plane(dREC, DR_OFF[f], DR_W[f], N, d, n), rows * DR_W[f], t, nt);
    if (lddgx == 2 * GXW) {
        zero_range(dGX + n * lddgx, rows * 2 * GXW, t, nt);
    } else {
        for (int64_t r = n; r < N; ++r) zero_range(dGX + r * lddgx, 2 * GXW, t, nt);
    }
}

// CAP (erc_dialogrnn_scan_bwd_cap): p.N is the capacity, *p.n_dev the batch's node count.  The grid is B x (2 + k), k =
// ceil(TAIL_WG / B): of the workgroups blockIdx.y >= 2 the first TAIL_WG own the tails (drnn_zero_tails) and the others (B - 16 of
// them where B > 16: a grid is a product) end at their first branch; the B x 2 scanning workgroups run the code of the exact
// form (the test on blockIdx.y reads no kernel argument: this form compiles to the exact form's registers and scratch).
template <bool CAP>
__global__ __launch_bounds__(NT) void drnn_bwd_kernel(DrnnP p) {
    if (CAP && blockIdx.y >= 2) {
        const int w = (blockIdx.y - 2) * gridDim.x + blockIdx.x;
        if (w < TAIL_WG) drnn_zero_tails(p.dGX, p.lddgx, p.dREC, p.N, p.n_dev, (int64_t)w * NT + threadIdx.x, (int64_t)TAIL_WG * NT);
        return;
    }
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* dHist = sm;                 // [MAXT][DG]  gradient wrt g'_j
    float* hist = dHist + MAXT * DG;   // [MAXT][DG]  g'_j (scan order), read back from the forward's save
    float* sDQ = hist + MAXT * DG;     // [MAXS][DG]  gradient wrt the party states
    float* s_dgi_e = sDQ + 1352;
    float* s_dgh_e = s_dgi_e + 304;
    float* s_dgi_g = s_dgh_e + 304;
    float* s_dgh_g = s_dgi_g + 452;
    float* s_dgi_p = s_dgh_g + 452;
    float* s_dgh_p = s_dgi_p + 452;
    float* sPart = s_dgh_p + 452;      // up to 1800 partial sums of the transposed products
    float* s_dqg = sPart + 1800;       // W_gq^T dgi_g
    float* s_dc = s_dqg + 152;
    float* s_dal = s_dc + 152;
    float* s_dsc = s_dal + 112;
    float* s_al = s_dsc + 112;
    const int b = blockIdx.x, d = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t N = p.N;
    const int base = p.node_off[b];
    int L = min(p.node_off[b + 1] - base, min(p.T, MAXT));
    if (base < 0 || base + L > N) L = 0;
    const int64_t* off = p.off + d * O_N;
    const float* WN = p.WT + (int64_t)(2 + d) * WT_DIR;    // contiguous row-major copies of the recurrent blocks
    const float* Wgq = WN + WT_GQ;                         // [450, 150] = W_ih^g[:, D_m:]
    const float* Wgh = WN + WT_GH;                         // [450, 150]
    const float* Wpc = WN + WT_PC;
    const float* Wph = WN + WT_PH;
    const float* Wei = WN + WT_EI;                         // [300, 150]
    const float* Weh = WN + WT_EH;                         // [300, 100]
    const bool dropping = p.drop_p > 0.f, dropping_rec = p.drop_rec > 0.f;
    uint64_t roff = 0, rseed = 0;
    if (dropping || dropping_rec) roff = p.rng[0], rseed = p.rng[1] ^ (p.rng_stream + (uint64_t)d);
    const float ks = dropping ? 1.0f / (1.0f - p.drop_p) : 1.0f, ks_rec = dropping_rec ? 1.0f / (1.0f - p.drop_rec) : 1.0f;
    float* sv = const_cast<float*>(p.save);
    for (int i = tid; i < MAXT * DG; i += NT) dHist[i] = 0.f;
    for (int i = tid; i < MAXS * DG; i += NT) sDQ[i] = 0.f;
    for (int i = tid; i < L * DG; i += NT) {
        const int j = i / DG;
        hist[i] = plane(sv, SV_GD, DG, N, d, base + (d == 0 ? j : L - 1 - j))[i % DG];
    }
    float de_rec = 0.f, de_direct = 0.f, dq_direct = 0.f, dg_direct = 0.f;
    bool da_pending = false;
    int64_t da_row = 0;
    __syncthreads();
    for (int s = L - 1; s >= 0; --s) {
        if (da_pending && tid < DG)      // d a of the step before: its four partial sums were written ahead of that step's last barrier
            p.dGX[da_row * p.lddgx + d * GXW + 900 + tid] = (sPart[tid] + sPart[DG + tid]) + (sPart[2 * DG + tid] + sPart[3 * DG + tid]);
        da_pending = false;
        const int t = d == 0 ? s : L - 1 - s;
        const int64_t row = base + t;
        const int spk = min(max(p.node_spk[row], 0), min(p.S, MAXS) - 1);
        float* dgx = p.dGX + row * p.lddgx + d * GXW;
        // ---- gate gradients of the emotion cell and of the global cell (d g'_s is complete: only later steps add to it)
        if (tid < DE) {
            const int u = tid;
            float g = p.dEmo[row * p.ldde + d * DE + u];
            if (dropping_rec) g = kept(rseed, roff, row, 3, u, p.drop_rec) ? g * ks_rec : 0.f;
            g += de_rec;
            if (dropping) g = kept(rseed, roff, row, 2, u, p.drop_p) ? g * ks : 0.f;
            const float* gt = plane(sv, SV_GATES_E, E3, N, d, row);
            const float r = gt[u], z = gt[DE + u], n = gt[2 * DE + u];
            const float hp = plane(sv, SV_EPREV, DE, N, d, row)[u], gn = plane(sv, SV_GHN_E, DE, N, d, row)[u];
            const float dnp = g * (1.f - z) * (1.f - n * n);
            const float dzp = g * (hp - n) * z * (1.f - z);
            const float drp = dnp * gn * r * (1.f - r);
            s_dgi_e[u] = drp, s_dgi_e[DE + u] = dzp, s_dgi_e[2 * DE + u] = dnp;
            s_dgh_e[u] = drp, s_dgh_e[DE + u] = dzp, s_dgh_e[2 * DE + u] = dnp * r;
            float* gi = plane(p.dREC, DR_GI_E, E3, N, d, row);
            float* gh = plane(p.dREC, DR_GH_E, E3, N, d, row);
            gi[u] = drp, gi[DE + u] = dzp, gi[2 * DE + u] = dnp;
            gh[u] = drp, gh[DE + u] = dzp, gh[2 * DE + u] = dnp * r;
            de_direct = g * z;
        }
        if (tid >= 256 && tid < 256 + DG) {
            const int u = tid - 256;
            float g = dHist[s * DG + u];
            if (dropping) g = kept(rseed, roff, row, 0, u, p.drop_p) ? g * ks : 0.f;
            const float* gt = plane(sv, SV_GATES_G, G3, N, d, row);
            const float r = gt[u], z = gt[DG + u], n = gt[2 * DG + u];
            const float hp = plane(sv, SV_GPREV, DG, N, d, row)[u], gn = plane(sv, SV_GHN_G, DG, N, d, row)[u];
            const float dnp = g * (1.f - z) * (1.f - n * n);
            const float dzp = g * (hp - n) * z * (1.f - z);
            const float drp = dnp * gn * r * (1.f - r);
            s_dgi_g[u] = drp, s_dgi_g[DG + u] = dzp, s_dgi_g[2 * DG + u] = dnp;
            s_dgh_g[u] = drp, s_dgh_g[DG + u] = dzp, s_dgh_g[2 * DG + u] = dnp * r;
            dgx[u] = drp, dgx[DG + u] = dzp, dgx[2 * DG + u] = dnp;
            float* gh = plane(p.dREC, DR_GH_G, G3, N, d, row);
            gh[u] = drp, gh[DG + u] = dzp, gh[2 * DG + u] = dnp * r;
            dg_direct = g * z;
        }
        __syncthreads();
        // ---- W_eh^T dgh_e | W_ei^T dgi_e | W_gh^T dgh_g | W_gq^T dgi_g, three row parts each
        if (tid < 825) {               // one thread per (pair of columns, row part): 3 x (50 + 75 + 75 + 75)
            f2 v;
            int o;
            if (tid < 150) {
                const int part = tid / 50, kp = tid % 50;
                v = dot_n2(Weh, DE, kp, s_dgh_e, part * 100, 100), o = part * DE + 2 * kp;
            } else if (tid < 375) {
                const int part = (tid - 150) / 75, kp = (tid - 150) % 75;
                v = dot_n2(Wei, DG, kp, s_dgi_e, part * 100, 100), o = 300 + part * DG + 2 * kp;
            } else if (tid < 600) {
                const int part = (tid - 375) / 75, kp = (tid - 375) % 75;
                v = dot_n2(Wgh, DG, kp, s_dgh_g, part * 150, 150), o = 750 + part * DG + 2 * kp;
            } else {
                const int part = (tid - 600) / 75, kp = (tid - 600) % 75;
                v = dot_n2(Wgq, DG, kp, s_dgi_g, part * 150, 150), o = 1200 + part * DG + 2 * kp;
            }
            sPart[o] = v.x, sPart[o + 1] = v.y;
        }
        __syncthreads();
        // ---- gate gradients of the party cell; d g'_{s-1} and d q[p] from the global cell
        if (tid < DE) de_rec = de_direct + ((sPart[tid] + sPart[DE + tid]) + sPart[2 * DE + tid]);
        if (tid < DG) {
            const int u = tid;
            float g = sDQ[spk * DG + u] + ((sPart[300 + u] + sPart[450 + u]) + sPart[600 + u]);
            if (dropping) g = kept(rseed, roff, row, 1, u, p.drop_p) ? g * ks : 0.f;
            const float* gt = plane(sv, SV_GATES_P, G3, N, d, row);
            const float r = gt[u], z = gt[DG + u], n = gt[2 * DG + u];
            const float hp = plane(sv, SV_QPREV, DG, N, d, row)[u], gn = plane(sv, SV_GHN_P, DG, N, d, row)[u];
            const float dnp = g * (1.f - z) * (1.f - n * n);
            const float dzp = g * (hp - n) * z * (1.f - z);
            const float drp = dnp * gn * r * (1.f - r);
            s_dgi_p[u] = drp, s_dgi_p[DG + u] = dzp, s_dgi_p[2 * DG + u] = dnp;
            s_dgh_p[u] = drp, s_dgh_p[DG + u] = dzp, s_dgh_p[2 * DG + u] = dnp * r;
            dgx[G3 + u] = drp, dgx[G3 + DG + u] = dzp, dgx[G3 + 2 * DG + u] = dnp;
            float* gh = plane(p.dREC, DR_GH_P, G3, N, d, row);
            gh[u] = drp, gh[DG + u] = dzp, gh[2 * DG + u] = dnp * r;
            dq_direct = g * z;
        }
        if (tid >= 256 && tid < 256 + DG) {
            const int u = tid - 256;
            if (s > 0) dHist[(s - 1) * DG + u] += dg_direct + ((sPart[750 + u] + sPart[900 + u]) + sPart[1050 + u]);
            s_dqg[u] = (sPart[1200 + u] + sPart[1350 + u]) + sPart[1500 + u];
        }
        __syncthreads();
        // ---- W_pc^T dgi_p (= dc) | W_ph^T dgh_p
        if (tid < 900) {               // (pair of columns, one of six row parts) of W_pc^T | W_ph^T
            const int m = tid / 450, part = (tid % 450) / 75, kp = tid % 75;
            const f2 v = m == 0 ? dot_n2(Wpc, DG, kp, s_dgi_p, part * 75, 75) : dot_n2(Wph, DG, kp, s_dgh_p, part * 75, 75);
            sPart[m * 900 + part * DG + 2 * kp] = v.x, sPart[m * 900 + part * DG + 2 * kp + 1] = v.y;
        }
        __syncthreads();
        if (tid < DG) {
            float dc = 0.f, dh = 0.f;
#pragma unroll
            for (int q6 = 0; q6 < 6; ++q6) dc += sPart[q6 * DG + tid], dh += sPart[900 + q6 * DG + tid];
            s_dc[tid] = dc;
            sDQ[spk * DG + tid] = dq_direct + dh + s_dqg[tid];
        }
        __syncthreads();
        if (s > 0) {
            // ---- attention over the history: d alpha_j = dc . g'_j
            for (int j = wave; j < s; j += NT / 64) {
                const float* h = hist + j * DG;
                float v = s_dc[lane] * h[lane] + s_dc[64 + lane] * h[64 + lane] + (lane < 22 ? s_dc[128 + lane] * h[128 + lane] : 0.f);
                v = wave_sum(v);
                if (lane == 0) s_dal[j] = v;
            }
            __syncthreads();
            if (wave == 0) {
                const float* al = sv + (int64_t)SV_ROW * 2 * N + (((int64_t)d * p.B + b) * p.T + s) * p.T;
                const float a0 = lane < s ? al[lane] : 0.f, a1 = lane + 64 < s ? al[lane + 64] : 0.f;
                const float d0 = lane < s ? s_dal[lane] : 0.f, d1 = lane + 64 < s ? s_dal[lane + 64] : 0.f;
                const float dot = wave_sum(a0 * d0 + a1 * d1);
                if (lane < s) s_al[lane] = a0, s_dsc[lane] = a0 * (d0 - dot);
                if (lane + 64 < s) s_al[lane + 64] = a1, s_dsc[lane + 64] = a1 * (d1 - dot);
            }
            __syncthreads();
            const float* ga = p.GX + row * p.ldgx + d * GXW + 900;
            if (tid < 4 * DG) {        // d a = sum_j dscore_j g'_j: four partial sums over j, added up after the barrier
                const int part = tid / DG, k = tid % DG;
                const int per = (s + 3) / 4, j0 = part * per, j1 = min(s, j0 + per);
                float acc = 0.f;
                for (int j = j0; j < j1; ++j) acc = fmaf(s_dsc[j], hist[j * DG + k], acc);
                sPart[tid] = acc;
            } else {                   // d g'_j += alpha_j dc + dscore_j a, one owner per element
                for (int i = tid - 4 * DG; i < s * DG; i += NT - 4 * DG) {
                    const int j = i / DG, k = i % DG;
                    dHist[i] += fmaf(s_al[j], s_dc[k], s_dsc[j] * ga[k]);
                }
            }
            da_pending = true, da_row = row;
            __syncthreads();
        } else if (tid < DG) {
            dgx[900 + tid] = 0.f;
        }
    }
    // (the last step is s = 0, which has no attention: nothing is pending here)
}

// copies of the six recurrent blocks of both directions: WT[d] = W_gq^T | W_gh^T | W_pc^T | W_ph^T | W_ei^T | W_eh^T (forward) and
// WT[2 + d] = the same blocks row-major and contiguous (backward: the state columns of W_ih^g / W_ih^p without their D_m + 150 pitch)
__global__ void drnn_pack_kernel(DrnnP p) {
    const int m = blockIdx.x % 6, d = blockIdx.x / 6;
    const int64_t* off = p.off + d * O_N;
    const int ldi = p.Dm + DG;
    const float* W; int ld, rows, K, dst;
    switch (m) {
        case 0: W = p.params + off[O_WIH_G] + p.Dm; ld = ldi; rows = G3; K = DG; dst = WT_GQ; break;
        case 1: W = p.params + off[O_WHH_G]; ld = DG; rows = G3; K = DG; dst = WT_GH; break;
        case 2: W = p.params + off[O_WIH_P] + p.Dm; ld = ldi; rows = G3; K = DG; dst = WT_PC; break;
        case 3: W = p.params + off[O_WHH_P]; ld = DG; rows = G3; K = DG; dst = WT_PH; break;
        case 4: W = p.params + off[O_WIH_E]; ld = DG; rows = E3; K = DG; dst = WT_EI; break;
        default: W = p.params + off[O_WHH_E]; ld = DE; rows = E3; K = DE; dst = WT_EH; break;
    }
    float* out = const_cast<float*>(p.WT) + (int64_t)d * WT_DIR + dst;
    float* outn = const_cast<float*>(p.WT) + (int64_t)(2 + d) * WT_DIR + dst;
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < rows * K; i += gridDim.y * blockDim.x) {
        const int j = i / K, k = i % K;           // reads contiguous in k
        const float w = W[(int64_t)j * ld + k];
        out[k * rows + j] = w;
        outn[i] = w;
    }
}

// node_off, node_row (t*B + b of node node_off[b] + t) and the speaker of every node: argmax of its one-hot row
// (torch.argmax: the first index of the maximum, dgcnv2_models.py:275)
__global__ void drnn_meta_kernel(const float* onehot, int S, const int64_t* lengths, int B, int T, int n_cap, int32_t* node_off,
                                 int32_t* node_row, int32_t* node_spk) {
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
    for (int b = threadIdx.x; b <= B; b += blockDim.x) node_off[b] = min(s_off[b], n_cap);
    for (int b = 0; b < B; ++b) {
        const int o = s_off[b], L = s_off[b + 1] - o;
        for (int t = threadIdx.x; t < L; t += blockDim.x) {
            if (o + t >= n_cap) break;
            const float* r = onehot + ((int64_t)t * B + b) * S;
            int best = 0;
            for (int k = 1; k < S; ++k)
                if (r[k] > r[best]) best = k;
            node_row[o + t] = t * B + b;
            node_spk[o + t] = best;
        }
    }
}

// DialogueRNN in capacity mode (dialogrnn.py): the tables of drnn_meta_kernel for a step whose launches are sized for (B, T, n_cap)
// while the batch's own counts live on the device.  lengths [B] (int64) + onehot [T, B, S], or desc [2 B] (int32: lengths | first
// store rows; RESIDENT) + the store's speaker ids and labels [zero_store_row].  The rows are compact, so nothing but the capacity
// rows i >= n needs a filler: node_row 0 (a row of the static block) or zero_store_row, speaker 0, label 0.
__global__ void drnn_meta_cap_kernel(const float* onehot, int S, const int64_t* lengths, const int32_t* desc,
                                     const int64_t* store_speaker, const int64_t* store_label, int zero_store_row, int B, int T,
                                     int n_cap, int32_t* node_off, int32_t* node_row, int32_t* node_spk, int64_t* label_out,
                                     int32_t* counts) {
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
        counts[1] = tmax;      // the longest dialogue
    }
    __syncthreads();
    const int n = s_off[B];
    for (int b = threadIdx.x; b <= B; b += blockDim.x) node_off[b] = s_off[b];
    for (int i = threadIdx.x; i < n_cap; i += blockDim.x) {
        int row = desc ? zero_store_row : 0, spk = 0;
        int64_t lab = 0;
        if (i < n) {
            int lo = 0, hi = B;                       // the dialogue of node i: the first b with s_off[b + 1] > i
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_off[mid + 1] <= i) lo = mid + 1; else hi = mid;
            }
            const int b = min(lo, B - 1), t = i - s_off[b];
            if (desc) {
                const int64_t r = (int64_t)desc[B + b] + t;
                if (r >= 0 && r < zero_store_row) {   // a row outside the store reads the zero row, speaker 0, label 0
                    row = (int)r;
                    spk = (int)min(max(store_speaker[r], (int64_t)0), (int64_t)(S - 1));
                    if (store_label) lab = store_label[r];
                }
            } else {
                const float* r = onehot + ((int64_t)t * B + b) * S;
                int best = 0;
                for (int k = 1; k < S; ++k)
                    if (r[k] > r[best]) best = k;
                row = t * B + b, spk = best;
            }
        }
        node_row[i] = row;
        node_spk[i] = spk;
        if (label_out) label_out[i] = lab;
    }
}

// bc-LSTM / bc-GRU in capacity mode (bcrnn.py): the index tables of a step whose launches are sized for (B, T, n_cap) while the
// batch's own counts live on the device.  lengths [B] (int64) or desc [2 B] (int32: lengths | first store rows; RESIDENT).
__global__ void bcrnn_meta_kernel(const int64_t* lengths, const int32_t* desc, const int64_t* store_label, int zero_store_row,
                                  int B, int T, int n_cap, int32_t* node_off, int32_t* node_row, int32_t* pad_node, int32_t* x_row,
                                  int64_t* label_out, int32_t* counts) {
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
    // padded row t*B + b -> its node (n_cap: the zero row behind the node buffers) and, resident, its store row
    for (int i = threadIdx.x; i < B * T; i += blockDim.x) {
        const int t = i / B, b = i % B;
        const int o = s_off[b], L = s_off[b + 1] - o;
        pad_node[i] = t < L ? o + t : n_cap;
        if (x_row) x_row[i] = t < L ? desc[B + b] + t : zero_store_row;
        if (t < L) {
            node_row[o + t] = i;
            if (label_out && store_label) label_out[o + t] = store_label[desc[B + b] + t];
        }
    }
    // capacity nodes: the zero row behind the padded buffers, label 0
    for (int i = N + threadIdx.x; i < n_cap; i += blockDim.x) {
        node_row[i] = B * T;
        if (label_out && store_label) label_out[i] = 0;
    }
}

__global__ void log_softmax_kernel(const float* x, int ldx, int C, int n_rows, float* y, int ldy) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const float* xi = x + (int64_t)r * ldx;
    float mx = xi[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, xi[c]);
    float sum = 0.f;
    for (int c = 0; c < C; ++c) sum += expf(xi[c] - mx);
    const float lse = mx + logf(sum);
    for (int c = 0; c < C; ++c) y[(int64_t)r * ldy + c] = xi[c] - lse;
}

bool set_lds(const void* kernel, int64_t bytes) {
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}

int fill_offsets(DrnnP& p, const int64_t* offs_host) {
    for (int i = 0; i < 2 * O_N; ++i) {
        if (offs_host[i] < 0) return 0;
        p.off[i] = offs_host[i];
    }
    return 1;
}

}  // namespace

extern "C" int erc_dialogrnn_max_t(void) { return MAXT; }

extern "C" int64_t erc_dialogrnn_wt_floats(void) { return 4 * (int64_t)WT_DIR; }

extern "C" int64_t erc_dialogrnn_save_floats(int64_t N, int B, int T) {
    return (int64_t)SV_ROW * 2 * N + 2 * (int64_t)B * T * T;
}

extern "C" int erc_dialogrnn_meta(const float* onehot, int S, const int64_t* lengths, int B, int T, int n_cap, int32_t* node_off,
                                  int32_t* node_row, int32_t* node_spk, void* stream) {
    ERC_REQUIRE(onehot && lengths && node_off && node_row && node_spk, "dialogrnn_meta: null pointer");
    ERC_REQUIRE(B > 0 && B <= 1024 && T > 0 && S > 0 && n_cap > 0, "dialogrnn_meta: bad sizes B=%d T=%d S=%d n_cap=%d", B, T, S,
                n_cap);
    hipLaunchKernelGGL(drnn_meta_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, onehot, S, lengths, B, T, n_cap, node_off,
                       node_row, node_spk);
    ERC_LAUNCH_CHECK("dialogrnn_meta");
    return ERC_OK;
}

extern "C" int erc_bcrnn_meta_cap(const int64_t* lengths, const int32_t* desc, const int64_t* store_label, int zero_store_row,
                                  int B, int T, int n_cap, int32_t* node_off, int32_t* node_row, int32_t* pad_node, int32_t* x_row,
                                  int64_t* label_out, int32_t* counts, void* stream) {
    ERC_REQUIRE((lengths || desc) && node_off && node_row && pad_node && counts, "bcrnn_meta_cap: null pointer");
    ERC_REQUIRE(!x_row || desc, "bcrnn_meta_cap: x_row needs the resident descriptor");
    ERC_REQUIRE(!store_label || (desc && label_out), "bcrnn_meta_cap: store_label needs desc and label_out");
    ERC_REQUIRE(B > 0 && B <= 1024 && T > 0 && n_cap > 0, "bcrnn_meta_cap: bad sizes B=%d T=%d n_cap=%d", B, T, n_cap);
    hipLaunchKernelGGL(bcrnn_meta_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, lengths, desc, store_label, zero_store_row, B,
                       T, n_cap, node_off, node_row, pad_node, x_row, label_out, counts);
    ERC_LAUNCH_CHECK("bcrnn_meta_cap");
    return ERC_OK;
}

extern "C" int erc_dialogrnn_pack(const float* params, const int64_t* offs_host, int D_m, float* WT, void* stream) {
    ERC_REQUIRE(params && offs_host && WT, "dialogrnn_pack: null pointer");
    ERC_REQUIRE(D_m > 0, "dialogrnn_pack: D_m=%d", D_m);
    DrnnP p{};
    p.params = params; p.Dm = D_m; p.WT = WT;
    ERC_REQUIRE(fill_offsets(p, offs_host), "dialogrnn_pack: negative parameter offset");
    hipLaunchKernelGGL(drnn_pack_kernel, dim3(12, 16), dim3(256), 0, (hipStream_t)stream, p);
    ERC_LAUNCH_CHECK("dialogrnn_pack");
    return ERC_OK;
}

extern "C" int erc_dialogrnn_scan_fwd(const float* GX, int ldgx, const float* WT, const float* params, const int64_t* offs_host,
                                      int D_m, const int32_t* node_off, const int32_t* node_spk, int B, int T, int S, int64_t N,
                                      float drop_p, float drop_rec, const uint64_t* rng_state, uint64_t rng_stream,
                                      float* emotions, int lde, float* save, void* stream) {
    ERC_REQUIRE(GX && WT && params && offs_host && node_off && node_spk && emotions && save, "dialogrnn_scan_fwd: null pointer");
    ERC_REQUIRE(B > 0 && T > 0 && N > 0 && D_m > 0, "dialogrnn_scan_fwd: bad sizes B=%d T=%d N=%lld D_m=%d", B, T, (long long)N, D_m);
    ERC_REQUIRE(T <= MAXT, "dialogrnn_scan_fwd: the history of the global state fits %d utterances in LDS (batch T=%d)", MAXT, T);
    ERC_REQUIRE(S >= 1 && S <= MAXS, "dialogrnn_scan_fwd: n_speakers=%d (1..%d are built)", S, MAXS);
    ERC_REQUIRE(ldgx >= 2 * GXW && lde >= 2 * DE, "dialogrnn_scan_fwd: row pitches ldgx=%d lde=%d", ldgx, lde);
    ERC_REQUIRE(drop_p >= 0.f && drop_p < 1.f && drop_rec >= 0.f && drop_rec < 1.f, "dialogrnn_scan_fwd: drop_p %f / %f", drop_p,
                drop_rec);
    ERC_REQUIRE(!(drop_p > 0.f || drop_rec > 0.f) || rng_state, "dialogrnn_scan_fwd: dropout needs rng_state");
    DrnnP p{};
    p.GX = GX; p.ldgx = ldgx; p.WT = WT; p.params = params; p.Dm = D_m; p.node_off = node_off; p.node_spk = node_spk;
    p.B = B; p.T = T; p.S = S; p.N = N; p.drop_p = drop_p; p.drop_rec = drop_rec; p.rng = rng_state; p.rng_stream = rng_stream;
    p.emo = emotions; p.lde = lde; p.save = save;
    ERC_REQUIRE(fill_offsets(p, offs_host), "dialogrnn_scan_fwd: negative parameter offset");
    const int64_t bytes = (int64_t)FWD_LDS_FLOATS * 4;
    ERC_REQUIRE(set_lds((const void*)drnn_fwd_kernel, bytes), "dialogrnn_scan_fwd: %lld bytes of LDS refused", (long long)bytes);
    hipLaunchKernelGGL(drnn_fwd_kernel, dim3(B, 2), dim3(NT), bytes, (hipStream_t)stream, p);
    ERC_LAUNCH_CHECK("dialogrnn_scan_fwd");
    return ERC_OK;
}

namespace {

// both forms of the backward scan: n_dev == nullptr is the exact one (grid B x 2), else the grid has ceil(TAIL_WG / B) more rows of B
// workgroups, of which TAIL_WG own the tails
int scan_bwd_launch(const char* what, const float* GX, int ldgx, const float* WT, const float* params, const int64_t* offs_host,
                    int D_m, const int32_t* node_off, const int32_t* node_spk, int B, int T, int S, int64_t N, float drop_p,
                    float drop_rec, const uint64_t* rng_state, uint64_t rng_stream, const float* save, const float* dEmo, int ldde,
                    float* dGX, int lddgx, float* dREC, const int32_t* n_dev, void* stream) {
    ERC_REQUIRE(GX && WT && params && offs_host && node_off && node_spk && save && dEmo && dGX && dREC, "%s: null pointer", what);
    ERC_REQUIRE(B > 0 && T > 0 && N > 0 && D_m > 0, "%s: bad sizes B=%d T=%d N=%lld D_m=%d", what, B, T, (long long)N, D_m);
    ERC_REQUIRE(T <= MAXT, "%s: dialogues of up to %d utterances (batch T=%d)", what, MAXT, T);
    ERC_REQUIRE(S >= 1 && S <= MAXS, "%s: n_speakers=%d (1..%d are built)", what, S, MAXS);
    ERC_REQUIRE(ldgx >= 2 * GXW && lddgx >= 2 * GXW && ldde >= 2 * DE, "%s: row pitches ldgx=%d lddgx=%d ldde=%d", what, ldgx, lddgx,
                ldde);
    ERC_REQUIRE(drop_p >= 0.f && drop_p < 1.f && drop_rec >= 0.f && drop_rec < 1.f, "%s: drop_p %f / %f", what, drop_p, drop_rec);
    ERC_REQUIRE(!(drop_p > 0.f || drop_rec > 0.f) || rng_state, "%s: dropout needs rng_state", what);
    ERC_REQUIRE(dGX != GX, "%s: dGX must not alias GX", what);
    DrnnP p{};
    p.GX = GX; p.ldgx = ldgx; p.WT = WT; p.params = params; p.Dm = D_m; p.node_off = node_off; p.node_spk = node_spk;
    p.B = B; p.T = T; p.S = S; p.N = N; p.drop_p = drop_p; p.drop_rec = drop_rec; p.rng = rng_state; p.rng_stream = rng_stream;
    p.save = const_cast<float*>(save); p.dEmo = dEmo; p.ldde = ldde; p.dGX = dGX; p.lddgx = lddgx; p.dREC = dREC; p.n_dev = n_dev;
    ERC_REQUIRE(fill_offsets(p, offs_host), "%s: negative parameter offset", what);
    const int64_t bytes = (int64_t)BWD_LDS_FLOATS * 4;
    const void* kernel = n_dev ? (const void*)drnn_bwd_kernel<true> : (const void*)drnn_bwd_kernel<false>;
    ERC_REQUIRE(set_lds(kernel, bytes), "%s: %lld bytes of LDS refused", what, (long long)bytes);
    if (n_dev)
        hipLaunchKernelGGL(drnn_bwd_kernel<true>, dim3(B, 2 + erc_cdiv(TAIL_WG, B)), dim3(NT), bytes, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(drnn_bwd_kernel<false>, dim3(B, 2), dim3(NT), bytes, (hipStream_t)stream, p);
    ERC_LAUNCH_CHECK(what);
    return ERC_OK;
}

}  // namespace

extern "C" int erc_dialogrnn_scan_bwd(const float* GX, int ldgx, const float* WT, const float* params, const int64_t* offs_host, int D_m,
                                      const int32_t* node_off, const int32_t* node_spk, int B, int T, int S, int64_t N,
                                      float drop_p, float drop_rec, const uint64_t* rng_state, uint64_t rng_stream,
                                      const float* save, const float* dEmo, int ldde, float* dGX, int lddgx, float* dREC,
                                      void* stream) {
    return scan_bwd_launch("dialogrnn_scan_bwd", GX, ldgx, WT, params, offs_host, D_m, node_off, node_spk, B, T, S, N, drop_p, drop_rec,
                           rng_state, rng_stream, save, dEmo, ldde, dGX, lddgx, dREC, nullptr, stream);
}

extern "C" int erc_dialogrnn_scan_bwd_cap(const float* GX, int ldgx, const float* WT, const float* params, const int64_t* offs_host,
                                          int D_m, const int32_t* node_off, const int32_t* node_spk, int B, int T, int S, int64_t N,
                                          float drop_p, float drop_rec, const uint64_t* rng_state, uint64_t rng_stream,
                                          const float* save, const float* dEmo, int ldde, float* dGX, int lddgx, float* dREC,
                                          const int32_t* n_dev, void* stream) {
    ERC_REQUIRE(n_dev, "dialogrnn_scan_bwd_cap: null n_dev");
    return scan_bwd_launch("dialogrnn_scan_bwd_cap", GX, ldgx, WT, params, offs_host, D_m, node_off, node_spk, B, T, S, N, drop_p,
                           drop_rec, rng_state, rng_stream, save, dEmo, ldde, dGX, lddgx, dREC, n_dev, stream);
}

extern "C" int erc_dialogrnn_meta_cap(const float* onehot, int S, const int64_t* lengths, const int32_t* desc,
                                      const int64_t* store_speaker, const int64_t* store_label, int zero_store_row, int B, int T,
                                      int n_cap, int32_t* node_off, int32_t* node_row, int32_t* node_spk, int64_t* label_out,
                                      int32_t* counts, void* stream) {
    ERC_REQUIRE(node_off && node_row && node_spk && counts, "dialogrnn_meta_cap: null pointer");
    ERC_REQUIRE((lengths && onehot && !desc) || (desc && store_speaker && !lengths && !onehot),
                "dialogrnn_meta_cap: lengths + onehot (bucket form) or desc + store_speaker (resident form)");
    ERC_REQUIRE(!store_label || (desc && label_out), "dialogrnn_meta_cap: store_label needs desc and label_out");
    ERC_REQUIRE(!desc || zero_store_row >= 0, "dialogrnn_meta_cap: zero_store_row=%d", zero_store_row);
    ERC_REQUIRE(B > 0 && B <= 1024 && T > 0 && S > 0 && n_cap > 0, "dialogrnn_meta_cap: bad sizes B=%d T=%d S=%d n_cap=%d", B, T, S,
                n_cap);
    hipLaunchKernelGGL(drnn_meta_cap_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, onehot, S, lengths, desc, store_speaker,
                       store_label, zero_store_row, B, T, n_cap, node_off, node_row, node_spk, label_out, counts);
    ERC_LAUNCH_CHECK("dialogrnn_meta_cap");
    return ERC_OK;
}

extern "C" int erc_log_softmax_rows(const float* x, int ldx, int C, int n_rows, float* y, int ldy, void* stream) {
    ERC_REQUIRE(x && y, "log_softmax_rows: null pointer");
    ERC_REQUIRE(C > 0 && n_rows > 0 && ldx >= C && ldy >= C, "log_softmax_rows: bad sizes C=%d n_rows=%d", C, n_rows);
    hipLaunchKernelGGL(log_softmax_kernel, dim3(erc_cdiv(n_rows, 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, C, n_rows, y, ldy);
    ERC_LAUNCH_CHECK("log_softmax_rows");
    return ERC_OK;
}

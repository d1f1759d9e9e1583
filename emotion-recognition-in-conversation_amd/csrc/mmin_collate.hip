// Device collate of an MMIN batch (MMINBaseCollate, track_mm/mmin_base.py:224-251) from an utterance store that lives in HBM:
// the audio frames of all utterances as one ragged matrix [sum t_i, 130], visual [n, 50, 342], text [n, 22, 1024], labels [n].
// One launch writes a bucket's four input buffers (B_cap slots of T_cap audio frames) and counts = {B, Ta}.
//
// The batch is a descriptor of 3 B_cap int32 in device memory: frames | first frame row | sample index of every slot; a slot
// with frames == 0 is empty.  The output is cut into ROWS (B_cap T_cap audio rows of 520 bytes, B_cap Tv visual rows of 1368
// bytes, B_cap Tt text rows of 4096 bytes); a wavefront owns a row at a time and writes ALL of it, a copy of the store's row or
// zeros, so nothing of an earlier batch survives a launch, whatever that batch was.  Rows are 8-byte aligned and no more
// (520 = 8 * 65, 1368 = 8 * 171): every access is 8 bytes wide.  Workgroups share nothing and never wait for each other; the
// first wavefront of workgroup 0 also writes the labels and the two counts.
//
// What only the device knows is clamped here: frames to [0, T_cap], the first frame row so that the slot's frames stay inside
// the store, the sample index to [0, n_samples).
//
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): 35 VGPRs, no AGPRs, no scratch, no LDS, occupancy 8
// wavefronts per SIMD.
#include "erc_common.h"

namespace {
constexpr int DA = 130, DV = 342, DT = 1024;     // feature widths of the trainer (mmin_base.py:86-91)
constexpr int NTH = 256, WAVES = NTH / ERC_WAVE;

struct CollateArgs {
    const int32_t* desc;
    const float* s_audio;
    const float* s_visual;
    const float* s_text;
    const int64_t* s_label;
    float* audio;
    float* visual;
    float* text;
    int64_t* label;
    int32_t* counts;
    int64_t n_frames;
    int32_t n_samples, B_cap, T_cap, Tv, Tt;
};

// one row of `pairs` 8-byte pieces: a copy of src, or zeros where src is null (uniform over the wavefront)
__device__ __forceinline__ void put_row(f2* __restrict__ dst, const f2* __restrict__ src, int pairs, int lane) {
    if (src) {
        for (int i = lane; i < pairs; i += ERC_WAVE) dst[i] = src[i];
    } else {
        for (int i = lane; i < pairs; i += ERC_WAVE) dst[i] = f2{0.f, 0.f};
    }
}

// MASKED (erc_mmin_collate_masked): desc has a fourth block of B_cap keep bits (bit 0 visual, bit 1 text, bit 2 audio); a row of a
// modality whose bit is clear is written as zeros and the store's row is not read.  Labels and counts do not look at the bits.
template <bool MASKED>
__device__ __forceinline__ void collate_body(const CollateArgs a) {
    const int lane = threadIdx.x % ERC_WAVE, wave = threadIdx.x / ERC_WAVE;
    const int B_cap = a.B_cap, T_cap = a.T_cap;
    const int64_t rows_a = (int64_t)B_cap * T_cap, rows_v = (int64_t)B_cap * a.Tv, rows_t = (int64_t)B_cap * a.Tt;
    const int64_t rows = rows_a + rows_v + rows_t;
    for (int64_t r = (int64_t)blockIdx.x * WAVES + wave; r < rows; r += (int64_t)gridDim.x * WAVES) {
        // segment, slot and position of row r (uniform over the wavefront)
        const int seg = r < rows_a ? 0 : r < rows_a + rows_v ? 1 : 2;
        const int64_t rs = seg == 0 ? r : seg == 1 ? r - rows_a : r - rows_a - rows_v;
        const int Tseg = seg == 0 ? T_cap : seg == 1 ? a.Tv : a.Tt;
        const int b = (int)(rs / Tseg), t = (int)(rs % Tseg);
        const int frames = min(max(a.desc[b], 0), T_cap);
        bool drop = false;      // MASKED: the slot's keep bit of this segment's modality is clear
        if constexpr (MASKED) drop = !((((a.desc[3 * B_cap + b] & 7) >> (seg == 0 ? 2 : seg - 1)) & 1));
        if (seg == 0) {
            const int64_t n = min((int64_t)frames, a.n_frames);
            const int64_t first = min(max((int64_t)a.desc[B_cap + b], (int64_t)0), a.n_frames - n);
            const float* src = t < n ? a.s_audio + (first + t) * DA : nullptr;
            if constexpr (MASKED) src = drop ? nullptr : src;
            put_row(reinterpret_cast<f2*>(a.audio + rs * DA), reinterpret_cast<const f2*>(src), DA / 2, lane);
        } else {
            const int idx = min(max(a.desc[2 * B_cap + b], 0), a.n_samples - 1);
            bool have = frames > 0;
            if constexpr (MASKED) have = have && !drop;
            if (seg == 1) {
                const float* src = have ? a.s_visual + ((int64_t)idx * a.Tv + t) * DV : nullptr;
                put_row(reinterpret_cast<f2*>(a.visual + rs * DV), reinterpret_cast<const f2*>(src), DV / 2, lane);
            } else {
                const float* src = have ? a.s_text + ((int64_t)idx * a.Tt + t) * DT : nullptr;
                put_row(reinterpret_cast<f2*>(a.text + rs * DT), reinterpret_cast<const f2*>(src), DT / 2, lane);
            }
        }
    }
    if (blockIdx.x == 0 && wave == 0) {
        int nb = 0, ta = 0;
        for (int b = lane; b < B_cap; b += ERC_WAVE) {
            const int frames = min(max(a.desc[b], 0), T_cap);
            const int idx = min(max(a.desc[2 * B_cap + b], 0), a.n_samples - 1);
            a.label[b] = frames > 0 ? a.s_label[idx] : 0;
            nb += frames > 0;
            ta = max(ta, frames);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            nb += __shfl_xor(nb, o, 64);
            ta = max(ta, __shfl_xor(ta, o, 64));
        }
        if (lane == 0) {
            a.counts[0] = nb;
            a.counts[1] = ta;
        }
    }
}

__global__ __launch_bounds__(NTH) void mmin_collate_kernel(CollateArgs a) { collate_body<false>(a); }
__global__ __launch_bounds__(NTH) void mmin_collate_masked_kernel(CollateArgs a) { collate_body<true>(a); }
}  // namespace

extern "C" int erc_mmin_collate_width(int modality) { return modality == 0 ? DA : modality == 1 ? DV : modality == 2 ? DT : 0; }

template <bool MASKED>
static int collate(const char* name, const int32_t* desc, const float* store_audio, int64_t n_frames, const float* store_visual,
                   const float* store_text, const int64_t* store_label, int n_samples, int Tv, int Tt, int B_cap, int T_cap, int frames_max,
                   float* audio, float* visual, float* text, int64_t* label, int32_t* counts, void* stream) {
    ERC_REQUIRE(desc && store_audio && store_visual && store_text && store_label, "%s: null pointer (desc or the store)", name);
    ERC_REQUIRE(audio && visual && text && label && counts, "%s: null pointer (an output)", name);
    ERC_REQUIRE(B_cap > 0 && T_cap > 0 && Tv > 0 && Tt > 0, "%s: bad sizes B_cap=%d T_cap=%d Tv=%d Tt=%d", name, B_cap, T_cap, Tv, Tt);
    ERC_REQUIRE(n_samples > 0 && n_frames > 0, "%s: empty store (n_samples=%d, n_frames=%lld)", name, n_samples, (long long)n_frames);
    ERC_REQUIRE(frames_max >= 0 && frames_max <= T_cap, "%s: frames=%d > T_cap=%d", name, frames_max, T_cap);
    ERC_REQUIRE((int64_t)B_cap * T_cap <= (int64_t)1 << 30 && (int64_t)B_cap * (Tv > Tt ? Tv : Tt) <= (int64_t)1 << 30,
                "%s: B_cap=%d times T_cap=%d, Tv=%d or Tt=%d is beyond 2^30 rows", name, B_cap, T_cap, Tv, Tt);
    const uintptr_t al = (uintptr_t)store_audio | (uintptr_t)store_visual | (uintptr_t)store_text | (uintptr_t)audio |
                         (uintptr_t)visual | (uintptr_t)text;
    ERC_REQUIRE((al & 7) == 0, "%s: a feature buffer is not 8-byte aligned", name);
    CollateArgs a{desc, store_audio, store_visual, store_text, store_label, audio, visual, text, label, counts,
                  n_frames, n_samples, B_cap, T_cap, Tv, Tt};
    const int64_t rows = (int64_t)B_cap * ((int64_t)T_cap + Tv + Tt);
    const int grid = (int)(rows / WAVES + 1 < 4096 ? rows / WAVES + 1 : 4096);
    hipLaunchKernelGGL(MASKED ? mmin_collate_masked_kernel : mmin_collate_kernel, dim3(grid), dim3(NTH), 0, (hipStream_t)stream, a);
    ERC_LAUNCH_CHECK(name);
    return ERC_OK;
}

extern "C" int erc_mmin_collate(const int32_t* desc, const float* store_audio, int64_t n_frames, const float* store_visual,
                                const float* store_text, const int64_t* store_label, int n_samples, int Tv, int Tt, int B_cap,
                                int T_cap, int frames_max, float* audio, float* visual, float* text, int64_t* label,
                                int32_t* counts, void* stream) {
    return collate<false>("mmin_collate", desc, store_audio, n_frames, store_visual, store_text, store_label, n_samples, Tv, Tt, B_cap, T_cap,
                          frames_max, audio, visual, text, label, counts, stream);
}

extern "C" int erc_mmin_collate_masked(const int32_t* desc, const float* store_audio, int64_t n_frames, const float* store_visual,
                                       const float* store_text, const int64_t* store_label, int n_samples, int Tv, int Tt, int B_cap,
                                       int T_cap, int frames_max, float* audio, float* visual, float* text, int64_t* label,
                                       int32_t* counts, void* stream) {
    return collate<true>("mmin_collate_masked", desc, store_audio, n_frames, store_visual, store_text, store_label, n_samples, Tv, Tt, B_cap,
                         T_cap, frames_max, audio, visual, text, label, counts, stream);
}

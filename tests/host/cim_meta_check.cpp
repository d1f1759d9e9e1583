// Host check of erc_cim_meta_cap's index arithmetic (csrc/cim_meta.h: the functions the kernel itself calls), for a build
// with -fsanitize=address,undefined: every buffer is a heap allocation of exactly the size the header comment promises, so
// an index one past an end is reported.  Results are compared with a direct restatement.  Prints "ok <cases>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cim_meta.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
int rnd(int lo, int hi) {      // inclusive
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return lo + (int)((rng_state >> 33) % (uint64_t)(hi - lo + 1));
}

int fail(const char* what, int c) {
    std::printf("case %d: %s\n", c, what);
    return 1;
}

int run_case(int c, int B, int T, int n_cap, bool resident, bool with_emo, const std::vector<int64_t>& lens,
             const std::vector<int>& first, int U) {
    std::vector<int64_t> lengths(lens);
    std::vector<int32_t> desc(2 * B);
    for (int b = 0; b < B; ++b) desc[b] = (int32_t)lens[b], desc[B + b] = first[b];
    std::vector<int64_t> store_label(U), store_emo((size_t)U * 7);
    for (int i = 0; i < U; ++i) {
        store_label[i] = rnd(0, 5);
        for (int k = 0; k < 7; ++k) store_emo[(size_t)i * 7 + k] = rnd(0, 1);
    }
    const int tail_row = resident ? U : B * T;
    std::vector<int32_t> node_off(B + 1, -7), node_row(n_cap, -7), counts(2, -7);
    std::vector<int64_t> lengths_out(B, -7), label_out(n_cap, -7), emo_out((size_t)n_cap * 7, -7);
    std::vector<int> off(B + 1);
    CimMetaP p{resident ? nullptr : lengths.data(), resident ? desc.data() : nullptr, resident ? store_label.data() : nullptr,
               resident && with_emo ? store_emo.data() : nullptr, tail_row, B, T, n_cap, node_off.data(), node_row.data(),
               lengths_out.data(), resident ? label_out.data() : nullptr, resident && with_emo ? emo_out.data() : nullptr,
               counts.data()};
    cim_meta_prefix(p, off.data());
    for (int b = 0; b <= B; ++b) cim_meta_slot(p, off.data(), b);
    for (int i = 0; i < B * T; ++i) cim_meta_entry(p, off.data(), i);
    for (int i = off[B]; i < n_cap; ++i) cim_meta_tail(p, i);

    // restatement
    int n = 0, tmax = 0;
    for (int b = 0; b < B; ++b) {
        int64_t L = lens[b] < 0 ? 0 : (lens[b] > T ? T : lens[b]);
        if (L > n_cap - n) L = n_cap - n;
        if (node_off[b] != n || lengths_out[b] != L) return fail("node_off / lengths_out", c);
        for (int t = 0; t < L; ++t) {
            const int i = n + t;
            if (!resident) {
                if (node_row[i] != b * T + t) return fail("node_row (bucket)", c);
                continue;
            }
            const int64_t r = (int64_t)first[b] + t;
            const bool inside = r >= 0 && r < U;
            if (node_row[i] != (inside ? r : U)) return fail("node_row (resident)", c);
            if (label_out[i] != (inside ? store_label[r] : 0)) return fail("label_out", c);
            if (with_emo)
                for (int k = 0; k < 7; ++k)
                    if (emo_out[(size_t)i * 7 + k] != (inside ? store_emo[(size_t)r * 7 + k] : 0)) return fail("emo_out", c);
        }
        n += (int)L;
        tmax = (int)L > tmax ? (int)L : tmax;
    }
    if (node_off[B] != n || counts[0] != n || counts[1] != tmax) return fail("counts", c);
    for (int i = n; i < n_cap; ++i) {
        if (node_row[i] != tail_row) return fail("tail node_row", c);
        if (resident && label_out[i] != 0) return fail("tail label_out", c);
        if (resident && with_emo)
            for (int k = 0; k < 7; ++k)
                if (emo_out[(size_t)i * 7 + k] != 0) return fail("tail emo_out", c);
    }
    if (!resident)
        for (int i = 0; i < n_cap; ++i)
            if (label_out[i] != -7) return fail("the bucket form wrote a label", c);
    return 0;
}

}  // namespace

int main() {
    int cases = 0;
    // the shapes of the GPU tests: an empty slot, a one-utterance dialogue, n = 51 < n_cap; then n == n_cap
    for (int resident = 0; resident < 2; ++resident) {
        if (run_case(cases++, 4, 40, 128, resident, true, {17, 0, 1, 33}, {60, 0, 5, 7}, 100)) return 1;
        if (run_case(cases++, 4, 40, 128, resident, false, {40, 40, 40, 8}, {0, 40, 0, 80}, 100)) return 1;
        // lengths beyond T, below 0, beyond what n_cap holds; store rows before and behind the store
        if (run_case(cases++, 4, 40, 50, resident, true, {45, -3, 40, 40}, {-2, 0, 90, 99}, 100)) return 1;
        if (run_case(cases++, 1, 1, 1, resident, true, {0}, {0}, 1)) return 1;
        if (run_case(cases++, 1024, 2, 2048, resident, true, std::vector<int64_t>(1024, 2), std::vector<int>(1024, 3), 9)) return 1;
    }
    for (int k = 0; k < 400; ++k) {
        const int B = rnd(1, 9), T = rnd(1, 118), U = rnd(1, 300);
        const int n_cap = rnd(1, B * T);
        std::vector<int64_t> lens(B);
        std::vector<int> first(B);
        for (int b = 0; b < B; ++b) lens[b] = rnd(-2, T + 3), first[b] = rnd(-5, U + 5);
        if (run_case(cases++, B, T, n_cap, k & 1, k & 2, lens, first, U)) return 1;
    }
    std::printf("ok %d\n", cases);
    return 0;
}

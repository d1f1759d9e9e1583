// Host check of csrc/record_chunks.h (the functions head_fused_kernel<true, .> and cogmen_bwd_tile_kernel call to split a record
// list over their wavefronts), for a build with -fsanitize=address,undefined.  Walks the kernels' own loop -- batches of loads at
// clamped indices, masked by multiplication -- over a heap buffer of exactly n_records x slots entries, so a dereference at or
// beyond n_records is reported, and asserts that every (record, slot) with record < n_records is covered exactly once, that the
// chunks are contiguous and ordered, and that none reaches n_records or beyond.  Prints "ok <cases>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "record_chunks.h"

namespace {

int fail(const char* what, int G, int waves, int slots) {
    std::printf("G=%d waves=%d slots=%d: %s\n", G, waves, slots, what);
    return 1;
}

// batch = loads in flight per thread (16 in the head, 8 in the backward tile)
int run_case(int G, int waves, int slots, int batch) {
    // G = 0 is refused by the entry points; the arithmetic must still give empty chunks and dereference nothing
    std::vector<int> covered((size_t)G * slots, 0);
    std::vector<double> rec((size_t)G * slots);
    for (size_t i = 0; i < rec.size(); ++i) rec[i] = (double)(i % 1013) + 1.0;
    std::vector<double> sum(slots, 0.0);
    int expect_first = 0;
    for (int w = 0; w < waves; ++w) {
        const RecordChunk ch = record_chunk(G, waves, w);
        if (ch.first != expect_first) return fail("chunks are not contiguous", G, waves, slots);
        if (ch.last < ch.first || ch.last > G) return fail("chunk reaches beyond the list", G, waves, slots);
        if (w > 0 && ch.last - ch.first > record_chunk(G, waves, w - 1).last - record_chunk(G, waves, w - 1).first)
            return fail("a later chunk is longer", G, waves, slots);
        expect_first = ch.last;
        for (int lane = 0; lane < 64; ++lane) {
            const int l4 = lane < slots - 1 ? lane : slots - 1;
            double acc = 0.0;
            for (int g0 = ch.first; g0 < ch.last; g0 += batch)
                for (int j = 0; j < batch; ++j) {
                    const int g = record_chunk_index(g0 + j, G);
                    if (g < 0 || g >= G) return fail("dereference outside the list", G, waves, slots);
                    const double mk = record_chunk_mask(g0 + j, ch);
                    acc += rec[(size_t)g * slots + l4] * mk;      // the unconditional load: the sanitizer watches it
                    if (mk != 0.0 && lane < slots) {
                        if (g != g0 + j) return fail("a counted position was clamped", G, waves, slots);
                        ++covered[(size_t)g * slots + lane];
                    }
                }
            if (lane < slots) sum[lane] += acc;
        }
    }
    if (expect_first != G) return fail("the chunks do not end at the last record", G, waves, slots);
    for (size_t i = 0; i < covered.size(); ++i)
        if (covered[i] != 1) return fail("a (record, slot) is not covered exactly once", G, waves, slots);
    for (int s = 0; s < slots; ++s) {
        double want = 0.0;
        for (int g = 0; g < G; ++g) want += rec[(size_t)g * slots + s];
        if (want != sum[s]) return fail("sum", G, waves, slots);
    }
    return 0;
}

}  // namespace

int main() {
    int cases = 0;
    const int waves[2] = {8, 16}, slots[3] = {50, 57, 64}, batch[2] = {16, 8};
    for (int G = 0; G <= 600; ++G)
        for (int wi = 0; wi < 2; ++wi)
            for (int si = 0; si < 3; ++si) {
                if (run_case(G, waves[wi], slots[si], batch[wi])) return 1;
                ++cases;
            }
    std::printf("ok %d\n", cases);
    return 0;
}

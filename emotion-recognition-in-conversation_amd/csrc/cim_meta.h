// Index arithmetic of erc_cim_meta_cap (csrc/cim_attn.hip), in plain C++ so that a host program can run the very same code
// over exactly sized buffers (tests/host/cim_meta_check.cpp).  The kernel calls cim_meta_prefix from one thread and the three
// per-entry functions from all of them; a host caller runs the same four in loops.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CIM_META_HD __host__ __device__ inline
#else
#define CIM_META_HD inline
#endif

struct CimMetaP {
    const int64_t* lengths;      // bucket form [B]
    const int32_t* desc;         // resident form [2 B]: lengths | first store rows
    const int64_t* store_label;  // resident, optional [tail_row]
    const int64_t* store_emo;    // resident, optional [tail_row, 7]
    int tail_row;                // the row a tail node reads: bucket: a row of the padded block; resident: the store's zero row
    int B, T, n_cap;
    int32_t* node_off;           // [B + 1]
    int32_t* node_row;           // [n_cap]
    int64_t* lengths_out;        // [B]
    int64_t* label_out;          // [n_cap]      (resident)
    int64_t* emo_out;            // [n_cap, 7]   (resident)
    int32_t* counts;             // [2]: n, the longest dialogue
};

// off [B + 1] (the caller's scratch: LDS in the kernel): exclusive prefix sum of the lengths, each clamped to [0, T] and to what
// n_cap still holds.  The one serial part, run by one thread: its loop loads and writes nothing to global memory, so the B
// loads are independent of each other; node_off and lengths_out are cim_meta_slot's, written by all threads.  Writes counts.
CIM_META_HD void cim_meta_prefix(const CimMetaP& p, int* off) {
    int acc = 0, tmax = 0;
    for (int b = 0; b < p.B; ++b) {
        off[b] = acc;
        int64_t L = p.desc ? (int64_t)p.desc[b] : p.lengths[b];
        L = L < 0 ? 0 : (L > p.T ? p.T : L);
        const int Lc = (int)L < p.n_cap - acc ? (int)L : p.n_cap - acc;
        acc += Lc;
        tmax = Lc > tmax ? Lc : tmax;
    }
    off[p.B] = acc;
    p.counts[0] = acc;
    p.counts[1] = tmax;
}

// slot b, b <= B: node_off[b] and, b < B, the clamped length the scans read
CIM_META_HD void cim_meta_slot(const CimMetaP& p, const int* off, int b) {
    p.node_off[b] = off[b];
    if (b < p.B) p.lengths_out[b] = off[b + 1] - off[b];
}

// padded position i = b * T + t, i < B * T: where t < length[b], the entries of node off[b] + t
CIM_META_HD void cim_meta_entry(const CimMetaP& p, const int* off, int i) {
    const int b = i / p.T, t = i - b * p.T;
    const int o = off[b], L = off[b + 1] - o;
    if (t >= L) return;
    const int node = o + t;
    if (!p.desc) {
        p.node_row[node] = i;
        return;
    }
    // a store row outside [0, tail_row) reads the zero row and label 0: nothing a descriptor holds can leave the store
    int64_t row = (int64_t)p.desc[p.B + b] + t;
    const bool inside = row >= 0 && row < p.tail_row;
    if (!inside) row = p.tail_row;
    p.node_row[node] = (int32_t)row;
    if (p.label_out) p.label_out[node] = inside ? p.store_label[row] : 0;
    if (p.emo_out)
        for (int k = 0; k < 7; ++k) p.emo_out[(int64_t)node * 7 + k] = inside ? p.store_emo[row * 7 + k] : 0;
}

// tail node i, n <= i < n_cap
CIM_META_HD void cim_meta_tail(const CimMetaP& p, int i) {
    p.node_row[i] = p.tail_row;
    if (p.label_out) p.label_out[i] = 0;
    if (p.emo_out)
        for (int k = 0; k < 7; ++k) p.emo_out[(int64_t)i * 7 + k] = 0;
}

// Which workgroup records a wavefront adds up when every consumer workgroup sums every producer record (the BatchNorm tile sums in
// head_fused_kernel<true, .>, the head's records in cogmen_bwd_tile_kernel), in plain C++ so that a host program walks the very
// same arithmetic (tests/host/record_chunks_check.cpp).  A record is a contiguous run of float4 slots; one wave instruction loads a
// whole record: lane l takes slot l, wavefront w the records [first, last) of the list.
#pragma once

#if defined(__HIPCC__)
#define RECORD_CHUNKS_HD __host__ __device__ inline
#else
#define RECORD_CHUNKS_HD inline
#endif

struct RecordChunk {
    int first, last;      // records [first, last): first <= last <= n_records; empty when first == last
};

// n_records >= 0 records over n_waves >= 1 wavefronts: contiguous chunks of ceil(n_records / n_waves), in wavefront order; the
// last chunks are shorter or empty.  No chunk reaches n_records: a capacity-sized buffer may hold anything behind the list.
RECORD_CHUNKS_HD RecordChunk record_chunk(int n_records, int n_waves, int wave) {
    const int per = (n_records + n_waves - 1) / n_waves;
    const int first = wave * per < n_records ? wave * per : n_records;
    const int last = first + per < n_records ? first + per : n_records;
    return RecordChunk{first, last};
}

// The record a load of position g of a chunk dereferences: loads are unconditional, so positions at or beyond the chunk's end
// (the tail of a batch, an empty chunk) are clamped into the list and their values multiplied by record_chunk_mask = 0.
RECORD_CHUNKS_HD int record_chunk_index(int g, int n_records) { return g < n_records - 1 ? g : n_records - 1; }
RECORD_CHUNKS_HD double record_chunk_mask(int g, RecordChunk c) { return g < c.last ? 1.0 : 0.0; }

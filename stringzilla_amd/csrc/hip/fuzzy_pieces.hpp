/*
 *  fuzzy_pieces.hpp - what the kernels over the PIECES of one long text share (hip/myers_fuzzy_matches.hip: every end within a bound;
 *  hip/myers_fuzzy_occurrences.hip: one end per occurrence): the prefix sums of a wavefront, the piece a lane takes and what it walks
 *  of it, the counters of such a walk, and the grid of a walking pass.  DESIGN.md section 4.12 has the argument for the warm-up.
 */
#pragma once
#include "fuzzy_core.hpp"

namespace szs_hip {

/** Inclusive prefix sums over the 64 lanes of a wavefront. */
__device__ __forceinline__ u32 wave_prefix_u32(u32 value) {
    u32 const lane = threadIdx.x % wave_size_k;
#pragma unroll
    for (u32 offset = 1; offset < wave_size_k; offset <<= 1) {
        u32 const other = (u32)__shfl_up((int)value, offset, 64);
        if (lane >= offset) value += other;
    }
    return value;
}

/** What lane l of `chunk` walks: piece p = 64 chunk + l from `first` = p P - warm over `walked` = warm + own bytes. */
struct matches_piece_t {
    bool inside; // p < pieces
    u32 warm, first, walked;
};

__device__ __forceinline__ matches_piece_t matches_piece(u32 query_length, u32 text_length, u64 piece, u32 pieces, u32 chunk) {
    u64 const p = (u64)chunk * wave_size_k + threadIdx.x;
    matches_piece_t lane;
    lane.inside = p < pieces;
    u64 const from = lane.inside ? p * piece : 0; // below text_length: pieces = ceil(text_length / piece)
    lane.warm = from < 2u * query_length ? (u32)from : 2u * query_length;
    u32 const own = lane.inside ? (u32)(text_length - from < piece ? text_length - from : piece) : 0u;
    lane.first = (u32)from - lane.warm, lane.walked = lane.inside ? own + lane.warm : 0u; // first + walked <= text_length
    return lane;
}

/** The counters of a walk: cells and bytes as walked; the query read once a workgroup; the pair by chunk 0 of the count pass. */
__device__ __forceinline__ void matches_counted(listed_row_t const &row, bool live, u32 taken, bool with_pairs, unsigned long long *counters) {
    listed_counters_t counted;
    if (live) counted.cells = (u64)row.query_length * taken, counted.bytes = taken;
    if (threadIdx.x == 0) counted.bytes += row.query_length, counted.pairs = with_pairs;
    counted.land(counters, with_pairs);
}

/** The grid the walking passes share; false: arguments no launch takes. */
static inline bool matches_grid(szs_rerank_side_t const *queries, uint64_t first_query, uint32_t rows, void const *text, uint64_t text_length,
                                uint64_t piece, u64 &pieces, u64 &chunks) {
    if (!queries || !piece || !text || !text_length || text_length > 0xFFFFFFFFull || !rows || first_query + rows > queries->count) return false;
    pieces = (text_length + piece - 1) / piece; // below 2^32
    chunks = (pieces + wave_size_k - 1) / wave_size_k;
    return (u64)rows * chunks <= 0x7FFFFFFFull;
}

} // namespace szs_hip

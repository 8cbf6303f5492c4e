/*
 *  myers_fuzzy_occurrences.hip - ONE end per occurrence of every query inside ONE long text, and where each starts
 *  (szs_rocm_fuzzy_scan_occurrences*, host/fuzzy_scan_matches.c).  With D the unit-cost DP with a free
 *  start in the text, column j in [1, n] is an OCCURRENCE END iff
 *      D[m][j] <= bound,   D[m][j] < D[m][j - 1],   j == n or D[m][j] <= D[m][j + 1]
 *  - the first column of a valley floor of the bottom row, within the bound.  Per query the number of them in the whole text and the
 *  leftmost `limit` as (end, distance, start).  The cut and the schedule are hip/myers_fuzzy_scan.hip's; a lane's piece, the count
 *  pass, the write pass, the counters and the launch are hip/fuzzy_pieces.hpp's, shared with hip/myers_fuzzy_matches.hip; the offsets
 *  pass is that file's levenshtein_fuzzy_matches_offsets_kernel itself.  This file's own is the rule (occurrences_rule_t) with its
 *  piece, the two kernels' names - each declares the table and runs the pass under the rule - and the starts:
 *
 *  - THE TAIL COLUMN (occurrences_piece).  Piece p owns columns (p P, min(n, (p + 1) P)] and warms up min(p P, 2 m) bytes, as there; a
 *    lane whose piece is not the last walks ONE column more, (p + 1) P + 1: the right neighbour of its last owned column.  That column
 *    is exact for the reason owned columns are - it lies further from the lane's start s than they do.  The left neighbour of the
 *    first owned column is column p P, 2 m columns into the walk or s = 0: the start that attains D[m][p P] lies within m + D <= 2 m
 *    bytes of it, at or behind s, so it is exact too.  tests/test_fuzzy_scan_occurrences_model.py runs this decomposition against
 *    the rule.
 *  - THE DEFERRED DECISION (the rule's state, `column` and `behind`).  A lane keeps the scores of the two columns before the one it
 *    computes; at column c it decides column c - 1, when that column is owned.  The lane of the last piece decides column n behind
 *    the walk - no right neighbour is asked for.  The tail column is never reported: it is the first owned column of the next piece.
 *  - STARTS (levenshtein_fuzzy_occurrence_starts_kernel; launched only when the call asks for starts): one wavefront per (row, 64
 *    consecutive slots) of the (rows, limit) matrices the write pass filled, lane l slot 64 group + l.  A wavefront whose first slot
 *    is at or beyond min(counts[row], limit) returns before it builds a table.  A slot that holds 2^64 - 1 is empty and stays what the
 *    host's fill made it.  Every other slot is data read back from memory the caller can reach: distance <= m and end <= n before
 *    they address anything, else SZS_RERANK_FLAG_TAPE and a frozen lane.  The pass itself - the reversed pattern over zero phantom
 *    rows, myers_prefix_column over the window of min(end, m + distance) bytes from its last byte down, the exit once every live lane
 *    has reached its distance - is hip/fuzzy_core.hpp's, shared with hip/myers_fuzzy_spans.hip.
 *  - Every slot and every count has one writer and a value that does not depend on the order of anything: the same bytes every run.
 *  - Counters: cells and bytes as walked in every pass, tail columns and reverse windows included; one pair per row with a non-empty
 *    query, by chunk 0 of the count pass alone.
 */
#include "fuzzy_pieces.hpp"

namespace szs_hip {

/** The piece of hip/fuzzy_pieces.hpp with the tail column behind it: `walked` = warm + own + tail, first + walked <= text_length. */
struct occurrences_piece_t : matches_piece_t {
    bool tail; // the piece is not the last: column (p + 1) P + 1 is walked and never reported
};

__device__ __forceinline__ occurrences_piece_t occurrences_piece(u32 query_length, u32 text_length, u64 piece, u32 pieces, u32 chunk) {
    occurrences_piece_t lane;
    static_cast<matches_piece_t &>(lane) = matches_piece(query_length, text_length, piece, pieces, chunk);
    lane.tail = lane.inside && lane.first + lane.walked < text_length; // (the sum is at most text_length)
    lane.walked += lane.tail ? 1u : 0u;
    return lane;
}

struct occurrences_rule_t {
    using piece_t = occurrences_piece_t;

    static __device__ __forceinline__ piece_t piece(u32 query_length, u32 text_length, u64 piece, u32 pieces, u32 chunk) {
        return occurrences_piece(query_length, text_length, piece, pieces, chunk);
    }

    u32 held, left; // the score of the column before the one being computed, and of the one before that; column 0 of a walk holds m

    __device__ __forceinline__ explicit occurrences_rule_t(u32 query_length) : held(query_length), left(query_length) {}

    /** At column c: column c - 1, when it is owned. */
    template <typename on_found_t>
    __device__ __forceinline__ auto column(u32 const &warm, u32 const &bound, on_found_t const &on_found) {
        return [this, &warm, &bound, &on_found](u32 column_end, u32 score) {
            if (column_end - 1u > warm && held <= bound && held < left && held <= score) on_found(column_end - 1u, held);
            left = held, held = score;
        };
    }

    /** Behind a walk that `ended` - live and taken to its last column: the last piece ends at n, its last column has no right
     *  neighbour. */
    template <typename on_found_t>
    __device__ __forceinline__ void behind(piece_t const &lane, bool ended, u32 taken, u32 warm, u32 bound, on_found_t const &on_found) {
        if (ended && !lane.tail && taken > warm && held <= bound && held < left) on_found(taken, held);
    }
};

__global__ __launch_bounds__(64) void levenshtein_fuzzy_occurrences_count_kernel(szs_rerank_side_t const queries, u64 const first_query,
                                                                                 u32 const rows, u64 const text, u32 const text_length,
                                                                                 u64 const piece, u32 const pieces, u32 const chunks,
                                                                                 u32 const bound, u32 *__restrict__ piece_counts,
                                                                                 u32 *__restrict__ chunk_counts, u32 *flags,
                                                                                 unsigned long long *counters) {
    __shared__ __attribute__((aligned(16))) u32 fuzzy_occurrences_table[peq_layout<SZS_MYERS_SHORT_WORDS, byte_rows_k>::total_dwords];
    pieces_count_pass<occurrences_rule_t>(fuzzy_occurrences_table, queries, first_query, rows, text, text_length, piece, pieces, chunks, bound,
                                          piece_counts, chunk_counts, flags, counters);
}

__global__ __launch_bounds__(64) void levenshtein_fuzzy_occurrences_write_kernel(
    szs_rerank_side_t const queries, u64 const first_query, u32 const rows, u64 const text, u32 const text_length, u64 const piece,
    u32 const pieces, u32 const chunks, u32 const bound, u32 const limit, u32 const *__restrict__ piece_counts,
    u32 const *__restrict__ chunk_counts, u64 *__restrict__ distances, u64 *__restrict__ ends, u32 *flags, unsigned long long *counters) {
    __shared__ __attribute__((aligned(16))) u32 fuzzy_occurrences_table[peq_layout<SZS_MYERS_SHORT_WORDS, byte_rows_k>::total_dwords];
    pieces_write_pass<occurrences_rule_t>(fuzzy_occurrences_table, queries, first_query, rows, text, text_length, piece, pieces, chunks, bound,
                                          limit, piece_counts, chunk_counts, distances, ends, flags, counters);
}

template <int words_>
__device__ __forceinline__ void occurrence_starts_row(u32 *table, listed_row_t const &row, u64 text, u32 text_length, u32 limit, u32 first_slot,
                                                      u64 const *__restrict__ distances, u64 const *__restrict__ ends, u64 *__restrict__ starts,
                                                      u32 *flags, unsigned long long *counters) {
    fuzzy_reversed_table<words_, (int)wave_size_k>(table, row);
    u32 const query_length = row.query_length, rank = first_slot + threadIdx.x;
    u64 const at = row.row * limit + rank; // below rows x limit where rank < limit
    u32 window = 0, distance = 0, end = 0; // the window: T bytes that end at `end`
    bool live = rank < limit;
    if (live) {
        u64 const found = distances[at], ended = ends[at];
        if (found == ~0ull && ended == ~0ull) live = false; // an empty slot: it stays all ones
        else if (found > query_length || ended > text_length) flags[SZS_RERANK_FLAG_TAPE] = 1u, live = false; // before they address anything
        else {
            distance = (u32)found, end = (u32)ended;
            window = end < query_length + distance ? end : query_length + distance;
        }
    }
    u32 const pos = fuzzy_start_walk<words_>(table, query_length, text, end, window, distance, live);
    listed_counters_t counted;
    if (live) {
        starts[at] = end - pos;
        counted.add(query_length, window);
    }
    counted.land(counters, false);
}

__global__ __launch_bounds__(64) void levenshtein_fuzzy_occurrence_starts_kernel(szs_rerank_side_t const queries, u64 const first_query,
                                                                                 u32 const rows, u64 const text, u32 const text_length,
                                                                                 u32 const limit, u64 const *__restrict__ counts,
                                                                                 u64 const *__restrict__ distances, u64 const *__restrict__ ends,
                                                                                 u64 *__restrict__ starts, u32 *flags,
                                                                                 unsigned long long *counters) {
    __shared__ __attribute__((aligned(16))) u32 fuzzy_occurrences_table[peq_layout<SZS_MYERS_SHORT_WORDS, byte_rows_k>::total_dwords];
    u32 const r = blockIdx.x % rows, first_slot = (blockIdx.x / rows) * wave_size_k; // below `limit`: the host's grid
    u64 const counted = counts[r];
    if (first_slot >= (counted < limit ? counted : limit)) return; // no filled slot among the wavefront's
    listed_row_t const row = listed_row(queries, first_query, true, [&]() { return r; }, SZS_RERANK_LONGEST_QUERY, flags);
    u32 const length = (u32)__builtin_amdgcn_readfirstlane((int)row.query_length);
    if (!length) return; // (a row without a query counted nothing)
    listed_at_width(SZS_RERANK_WORDS_OF(length), [&](auto width) {
        occurrence_starts_row<decltype(width)::value>(fuzzy_occurrences_table, row, text, text_length, limit, first_slot, distances, ends,
                                                      starts, flags, counters);
    });
}

} // namespace szs_hip

extern "C" int szs_hip_levenshtein_fuzzy_occurrences_count(szs_rerank_side_t const *queries, uint64_t first_query, uint32_t rows,
                                                           void const *text, uint64_t text_length, uint64_t piece, uint32_t bound,
                                                           uint32_t *piece_counts, uint32_t *chunk_counts, uint32_t *flags,
                                                           unsigned long long *counters, void *stream) {
    return szs_hip::matches_launch(szs_hip::levenshtein_fuzzy_occurrences_count_kernel, piece_counts && chunk_counts && flags && counters,
                                   queries, first_query, rows, text, text_length, piece, stream, bound, piece_counts, chunk_counts, flags,
                                   counters);
}

extern "C" int szs_hip_levenshtein_fuzzy_occurrences_write(szs_rerank_side_t const *queries, uint64_t first_query, uint32_t rows,
                                                           void const *text, uint64_t text_length, uint64_t piece, uint32_t bound,
                                                           uint32_t limit, uint32_t const *piece_counts, uint32_t const *chunk_counts,
                                                           uint64_t *distances, uint64_t *ends, uint32_t *flags, unsigned long long *counters,
                                                           void *stream) {
    return szs_hip::matches_launch(szs_hip::levenshtein_fuzzy_occurrences_write_kernel,
                                   piece_counts && chunk_counts && distances && ends && limit && flags && counters, queries, first_query, rows,
                                   text, text_length, piece, stream, bound, limit, piece_counts, chunk_counts, distances, ends, flags, counters);
}

extern "C" int szs_hip_levenshtein_fuzzy_occurrence_starts(szs_rerank_side_t const *queries, uint64_t first_query, uint32_t rows,
                                                           void const *text, uint64_t text_length, uint32_t limit, uint64_t const *counts,
                                                           uint64_t const *distances, uint64_t const *ends, uint64_t *starts, uint32_t *flags,
                                                           unsigned long long *counters, void *stream) {
    using namespace szs_hip;
    if (!queries || !text || !text_length || text_length > 0xFFFFFFFFull || !rows || first_query + rows > queries->count || !limit || !counts ||
        !distances || !ends || !starts || !flags || !counters)
        return (int)hipErrorInvalidValue;
    u64 const groups = ((u64)limit + wave_size_k - 1) / wave_size_k;
    if (rows * groups > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(levenshtein_fuzzy_occurrence_starts_kernel, dim3((u32)(rows * groups)), dim3(wave_size_k), 0,
                       static_cast<hipStream_t>(stream), *queries, first_query, rows, (u64) reinterpret_cast<uintptr_t>(text), (u32)text_length,
                       limit, counts, distances, ends, starts, flags, counters);
    return (int)hipGetLastError();
}

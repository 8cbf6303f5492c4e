/*
 *  myers_fuzzy_occurrences.hip - ONE end per occurrence of every query inside ONE long text, and where each starts
 *  (szs_rocm_fuzzy_scan_occurrences*, host/fuzzy_scan_occurrences.c).  With D the unit-cost DP with a free
 *  start in the text, column j in [1, n] is an OCCURRENCE END iff
 *      D[m][j] <= bound,   D[m][j] < D[m][j - 1],   j == n or D[m][j] <= D[m][j + 1]
 *  - the first column of a valley floor of the bottom row, within the bound.  Per query the number of them in the whole text and the
 *  leftmost `limit` as (end, distance, start).  The cut, the schedule, the scratch and the two passes over a fixed capacity are
 *  hip/myers_fuzzy_matches.hip's, with "occurrence" in place of "hit"; a lane's piece, the counters and the grid are
 *  hip/fuzzy_pieces.hpp's; the offsets pass is levenshtein_fuzzy_matches_offsets_kernel itself.  This file's own:
 *
 *  - THE TAIL COLUMN.  Piece p owns columns (p P, min(n, (p + 1) P)] and warms up min(p P, 2 m) bytes, as there; a lane whose piece
 *    is not the last walks ONE column more, (p + 1) P + 1: the right neighbour of its last owned column.  That column is exact for the
 *    reason owned columns are - it lies further from the lane's start s than they do.  The left neighbour of the first owned column
 *    is column p P, 2 m columns into the walk or s = 0: the start that attains D[m][p P] lies within m + D <= 2 m bytes of it, at or
 *    behind s, so it is exact too.  tests/test_fuzzy_scan_occurrences_model.py runs this decomposition against the rule.
 *  - THE DEFERRED DECISION.  A lane keeps the scores of the two columns before the one it computes; at column c it decides column
 *    c - 1, when that column is owned.  The lane of the last piece decides column n behind the walk - no right neighbour is asked
 *    for.  The tail column is never reported: it is the first owned column of the next piece.
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
struct occurrences_piece_t {
    matches_piece_t columns;
    bool tail; // the piece is not the last: column (p + 1) P + 1 is walked and never reported
};

__device__ __forceinline__ occurrences_piece_t occurrences_piece(u32 query_length, u32 text_length, u64 piece, u32 pieces, u32 chunk) {
    occurrences_piece_t lane;
    lane.columns = matches_piece(query_length, text_length, piece, pieces, chunk);
    lane.tail = lane.columns.inside && lane.columns.first + lane.columns.walked < text_length; // (the sum is at most text_length)
    lane.columns.walked += lane.tail ? 1u : 0u;
    return lane;
}

/** One lane's walk of its piece and tail column against the row's table: `on_occurrence(column_end, score)` at every OWNED column
 *  that is an occurrence end; `keep_going()` as listed_walk asks it.  Returns the columns the lane took. */
template <int words_, typename on_occurrence_t, typename keep_going_t>
__device__ __forceinline__ u32 occurrences_walk(u32 const *table, u32 query_length, u64 text, occurrences_piece_t const &lane, bool live,
                                                u32 bound, on_occurrence_t on_occurrence, keep_going_t keep_going) {
    u32 const pad = 32u * words_ - query_length;
    u32 vp[words_], vn[words_];
#pragma unroll
    for (int w = 0; w < words_; ++w) vp[w] = rerank_bits_in_word(pad, 32u * words_, w), vn[w] = 0;
    // `held`: the score of the column before the one being computed, `left`: of the one before that; column 0 of a walk holds m
    u32 score = query_length, held = query_length, left = query_length, taken = 0;
    // (a lane that is not live still takes the zeros of listed_walk's unpredicated loop: it owns no column)
    u32 const length = live ? lane.columns.walked : 0u, warm = live ? lane.columns.warm : ~0u;
    listed_walk(
        text_stream_t(text + lane.columns.first, length), length, live,
        [&](u32 symbol, u32 column_end) {
            u32 eq[words_];
            load_match_masks<words_, byte_rows_k>(table, symbol, eq);
            u32 const top = myers_infix_column<words_>(vp, vn, eq);
            score += (top & 1u) - (top >> 1);
            taken = column_end;
            if (column_end - 1u > warm && held <= bound && held < left && held <= score) on_occurrence(column_end - 1u, held);
            left = held, held = score;
        },
        keep_going);
    // the last piece ends at n: its last column has no right neighbour (a walk that was left early owes nothing any more)
    if (live && !lane.tail && taken == length && taken > warm && held <= bound && held < left) on_occurrence(taken, held);
    return taken;
}

template <int words_>
__device__ __forceinline__ void occurrences_count_row(u32 *table, listed_row_t const &row, u64 text, u32 text_length, u64 piece, u32 pieces,
                                                      u32 chunk, u32 bound, u32 *__restrict__ piece_count, u32 *__restrict__ chunk_count,
                                                      unsigned long long *counters) {
    fuzzy_table<words_, (int)wave_size_k>(table, row);
    occurrences_piece_t const lane = occurrences_piece(row.query_length, text_length, piece, pieces, chunk);
    u32 found = 0;
    u32 const taken = occurrences_walk<words_>(
        table, row.query_length, text, lane, lane.columns.inside, bound, [&](u32, u32) { ++found; }, []() { return true; });
    piece_count[threadIdx.x] = found;
    u32 const all = (u32)wave_sum_u64(found); // <= the columns of 64 pieces, below 2^32
    if (threadIdx.x == 0) *chunk_count = all;
    matches_counted(row, lane.columns.inside, taken, chunk == 0, counters);
}

__global__ __launch_bounds__(64) void levenshtein_fuzzy_occurrences_count_kernel(szs_rerank_side_t const queries, u64 const first_query,
                                                                                 u32 const rows, u64 const text, u32 const text_length,
                                                                                 u64 const piece, u32 const pieces, u32 const chunks,
                                                                                 u32 const bound, u32 *__restrict__ piece_counts,
                                                                                 u32 *__restrict__ chunk_counts, u32 *flags,
                                                                                 unsigned long long *counters) {
    __shared__ __attribute__((aligned(16))) u32 fuzzy_occurrences_table[peq_layout<SZS_MYERS_SHORT_WORDS, byte_rows_k>::total_dwords];
    u32 const r = blockIdx.x % rows, chunk = blockIdx.x / rows; // chunk below `chunks`: the host's grid
    listed_row_t const row = listed_row(queries, first_query, true, [&]() { return r; }, SZS_RERANK_LONGEST_QUERY, flags);
    u32 const length = (u32)__builtin_amdgcn_readfirstlane((int)row.query_length); // one row a wavefront: a scalar
    u64 const cell = (u64)r * chunks + chunk; // below rows x chunks: what the host reserved, 64 piece counts a chunk
    u32 *const piece_count = piece_counts + cell * wave_size_k, *const chunk_count = chunk_counts + cell;
    if (!length) { // no query, or a flag is up and the call fails: no occurrence, nothing loaded
        piece_count[threadIdx.x] = 0;
        if (threadIdx.x == 0) *chunk_count = 0;
        return;
    }
    listed_at_width(SZS_RERANK_WORDS_OF(length), [&](auto width) {
        occurrences_count_row<decltype(width)::value>(fuzzy_occurrences_table, row, text, text_length, piece, pieces, chunk, bound,
                                                      piece_count, chunk_count, counters);
    });
}

template <int words_>
__device__ __forceinline__ void occurrences_write_row(u32 *table, listed_row_t const &row, u64 text, u32 text_length, u64 piece, u32 pieces,
                                                      u32 chunk, u32 bound, u32 limit, u32 offset, u32 found, u64 *__restrict__ distances,
                                                      u64 *__restrict__ ends, unsigned long long *counters) {
    fuzzy_table<words_, (int)wave_size_k>(table, row);
    occurrences_piece_t const lane = occurrences_piece(row.query_length, text_length, piece, pieces, chunk);
    bool const live = lane.columns.inside && found && offset < limit;
    u32 owed = live ? (found < limit - offset ? found : limit - offset) : 0u; // offset + owed <= limit
    u64 slot = row.row * limit + offset;                                        // below rows x limit while owed > 0
    u32 const taken = occurrences_walk<words_>(
        table, row.query_length, text, lane, live, bound,
        [&](u32 column_end, u32 score) {
            if (!owed) return;
            ends[slot] = (u64)lane.columns.first + column_end, distances[slot] = score;
            ++slot, --owed;
        },
        [&]() { return __ballot(owed != 0) != 0; });
    matches_counted(row, live, taken, false, counters);
}

__global__ __launch_bounds__(64) void levenshtein_fuzzy_occurrences_write_kernel(
    szs_rerank_side_t const queries, u64 const first_query, u32 const rows, u64 const text, u32 const text_length, u64 const piece,
    u32 const pieces, u32 const chunks, u32 const bound, u32 const limit, u32 const *__restrict__ piece_counts,
    u32 const *__restrict__ chunk_counts, u64 *__restrict__ distances, u64 *__restrict__ ends, u32 *flags, unsigned long long *counters) {
    __shared__ __attribute__((aligned(16))) u32 fuzzy_occurrences_table[peq_layout<SZS_MYERS_SHORT_WORDS, byte_rows_k>::total_dwords];
    u32 const r = blockIdx.x % rows, chunk = blockIdx.x / rows;
    u64 const cell = (u64)r * chunks + chunk;
    u32 const before = chunk_counts[cell]; // the occurrences of the row's chunks before this one
    if (before >= limit) return;           // every slot is taken by then
    u32 const found = piece_counts[cell * wave_size_k + threadIdx.x];
    u32 const upto = wave_prefix_u32(found);
    if (!__shfl((int)upto, (int)wave_size_k - 1, 64)) return; // a chunk without an occurrence
    listed_row_t const row = listed_row(queries, first_query, true, [&]() { return r; }, SZS_RERANK_LONGEST_QUERY, flags);
    u32 const length = (u32)__builtin_amdgcn_readfirstlane((int)row.query_length);
    if (!length) return; // (a row without a query counted nothing)
    listed_at_width(SZS_RERANK_WORDS_OF(length), [&](auto width) {
        occurrences_write_row<decltype(width)::value>(fuzzy_occurrences_table, row, text, text_length, piece, pieces, chunk, bound, limit,
                                                      before + upto - found, found, distances, ends, counters);
    });
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
    using namespace szs_hip;
    u64 pieces, chunks;
    if (!piece_counts || !chunk_counts || !flags || !counters || !matches_grid(queries, first_query, rows, text, text_length, piece, pieces, chunks))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(levenshtein_fuzzy_occurrences_count_kernel, dim3((u32)(rows * chunks)), dim3(wave_size_k), 0,
                       static_cast<hipStream_t>(stream), *queries, first_query, rows, (u64) reinterpret_cast<uintptr_t>(text), (u32)text_length,
                       piece, (u32)pieces, (u32)chunks, bound, piece_counts, chunk_counts, flags, counters);
    return (int)hipGetLastError();
}

extern "C" int szs_hip_levenshtein_fuzzy_occurrences_write(szs_rerank_side_t const *queries, uint64_t first_query, uint32_t rows,
                                                           void const *text, uint64_t text_length, uint64_t piece, uint32_t bound,
                                                           uint32_t limit, uint32_t const *piece_counts, uint32_t const *chunk_counts,
                                                           uint64_t *distances, uint64_t *ends, uint32_t *flags, unsigned long long *counters,
                                                           void *stream) {
    using namespace szs_hip;
    u64 pieces, chunks;
    if (!piece_counts || !chunk_counts || !distances || !ends || !limit || !flags || !counters ||
        !matches_grid(queries, first_query, rows, text, text_length, piece, pieces, chunks))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(levenshtein_fuzzy_occurrences_write_kernel, dim3((u32)(rows * chunks)), dim3(wave_size_k), 0,
                       static_cast<hipStream_t>(stream), *queries, first_query, rows, (u64) reinterpret_cast<uintptr_t>(text), (u32)text_length,
                       piece, (u32)pieces, (u32)chunks, bound, limit, piece_counts, chunk_counts, distances, ends, flags, counters);
    return (int)hipGetLastError();
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

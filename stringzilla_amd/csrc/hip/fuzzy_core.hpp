/*
 *  fuzzy_core.hpp - what the kernels of the semi-global distance share (hip/myers_fuzzy_find.hip: listed pairs; hip/myers_fuzzy_tile.hip:
 *  a tile of queries x candidates for the search; hip/myers_fuzzy_scan.hip and, through hip/fuzzy_pieces.hpp, hip/myers_fuzzy_matches.hip
 *  and hip/myers_fuzzy_occurrences.hip: the pieces of one long text): the Peq table with WILDCARD phantom rows and one lane's walk of
 *  its text under myers_infix_column, with the bottom-row score followed - fuzzy_infix_walk, written once; what a kernel does with
 *  (column, score) is its own.  DESIGN.md section 4.9 has the argument; hip/myers_fuzzy_find.hip's head repeats it.  And what the two
 *  reverse passes share (hip/myers_fuzzy_spans.hip; hip/myers_fuzzy_occurrences.hip): the table of the
 *  reversed pattern and one lane's walk back from an end to the start of its match.
 */
#pragma once
#include "rerank_core.hpp"

namespace szs_hip {

/** The table of `row` at `words_` words with the pattern right-aligned: every row of the table starts as the phantom mask (the bits
 *  below `pad`), the pattern's bits are scattered on top. */
template <int words_, int lanes_>
__device__ __forceinline__ void fuzzy_table(u32 *table, listed_row_t const &row) {
    u32 const pad = 32u * words_ - row.query_length; // phantom low rows of THIS row (a row without a query: all of them)
    listed_table<words_, lanes_>(table, row, [&](int w) { return rerank_bits_in_word(0, pad, w); }, [&](u32 i) { return pad + i; });
}

/** THE semi-global walk: one lane's `length` bytes at `address` against that table, `on_column(j, D[m][j])` at every column j = 1 ...
 *  of the lane's own DP - a free start at `address`.  The score starts at m and moves by hp - hn of the last row per column.
 *  `keep_going()` as listed_walk asks it.  A lane that is not `live` has `length` 0 and takes no column that counts (the zeros of
 *  listed_walk's unpredicated loop: its caller ignores what they score).  It returns nothing: a caller that wants the columns taken
 *  keeps the last `j` it saw. */
template <int words_, typename on_column_t, typename keep_going_t>
__device__ __forceinline__ void fuzzy_infix_walk(u32 const *table, u32 query_length, u64 address, u32 length, bool live, on_column_t on_column,
                                                keep_going_t keep_going) {
    u32 const pad = 32u * words_ - query_length;
    u32 vp[words_], vn[words_];
#pragma unroll
    for (int w = 0; w < words_; ++w) vp[w] = rerank_bits_in_word(pad, 32u * words_, w), vn[w] = 0;
    u32 score = query_length;
    listed_walk(
        text_stream_t(address, length), length, live,
        [&](u32 symbol, u32 column_end) {
            u32 eq[words_];
            load_match_masks<words_, byte_rows_k>(table, symbol, eq);
            u32 const top = myers_infix_column<words_>(vp, vn, eq);
            score += (top & 1u) - (top >> 1);
            on_column(column_end, score);
        },
        keep_going);
}

/** One lane's text against that table: `best` = min over j of D[m][j], `end` = the smallest j that attains it: a strictly smaller
 *  score moves `best` and `end` (the leftmost end).  A lane that is not `live` has `text_length` 0 and keeps (m, 0). */
template <int words_>
__device__ __forceinline__ void fuzzy_best_match(u32 const *table, u32 query_length, u64 address, u32 text_length, bool live, u32 &best,
                                                 u32 &end) {
    best = query_length, end = 0;
    fuzzy_infix_walk<words_>(
        table, query_length, address, text_length, live,
        [&](u32 column_end, u32 score) {
            if (score < best) best = score, end = column_end; // strictly smaller: the leftmost end
        },
        []() { return true; });
}

/** The table of the REVERSED pattern for the pass that finds a start: zero phantom rows - DP row zero of the global matrix - and byte
 *  i of the query at bit pad + (m - 1 - i): the query's last byte is the first real row. */
template <int words_, int lanes_>
__device__ __forceinline__ void fuzzy_reversed_table(u32 *table, listed_row_t const &row) {
    u32 const pad = 32u * words_ - row.query_length;
    listed_table<words_, lanes_>(table, row, [](int) { return 0u; }, [&](u32 i) { return pad + (row.query_length - 1u - i); });
}

/** One lane's reverse walk against that table: the GLOBAL unit-cost column (myers_prefix_column) over the `window` bytes that end at
 *  `address + end`, from the last byte down.  Returns the smallest t at which the bottom row is the least it gets - `distance`, when
 *  the window is min(end, m + distance) and `distance` the semi-global distance at `end` - so the match starts at end - t.  A
 *  wavefront leaves the walk once every live lane has reached its `distance`: nothing can move t then.  A lane that is not `live` has
 *  a window of 0 and returns 0. */
template <int words_>
__device__ __forceinline__ u32 fuzzy_start_walk(u32 const *table, u32 query_length, u64 address, u32 end, u32 window, u32 distance, bool live) {
    u32 const pad = 32u * words_ - query_length;
    u32 vp[words_], vn[words_];
#pragma unroll
    for (int w = 0; w < words_; ++w) vp[w] = rerank_bits_in_word(pad, 32u * words_, w), vn[w] = 0;
    u32 score = query_length, best = query_length, pos = 0;
    listed_walk(
        text_stream_backward_t(address + (end - window), window), window, live,
        [&](u32 symbol, u32 taken) {
            u32 eq[words_];
            load_match_masks<words_, byte_rows_k>(table, symbol, eq);
            u32 const top = myers_prefix_column<words_>(vp, vn, eq);
            score += (top & 1u) - (top >> 1);
            if (score < best) best = score, pos = taken; // strictly smaller: the smallest t
        },
        // a lane is open while its best is above d; with none open in the wavefront no `pos` can move any more
        [&]() { return __builtin_amdgcn_ballot_w64(live && best != distance) != 0ull; });
    return pos;
}

} // namespace szs_hip

/*
 *  fuzzy_core.hpp - what the kernels of the semi-global distance share (hip/myers_fuzzy_find.hip: listed pairs; hip/myers_fuzzy_tile.hip:
 *  a tile of queries x candidates for the search): the Peq table with WILDCARD phantom rows and one lane's walk of its text under
 *  myers_infix_column, with the bottom-row score followed.  DESIGN.md section 4.9 has the argument; hip/myers_fuzzy_find.hip's head
 *  repeats it.
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

/** One lane's text against that table: `best` = min over j of D[m][j], `end` = the smallest j that attains it.  The score starts at
 *  m, moves by hp - hn of the last row per column, and a strictly smaller score moves `best` and `end` (the leftmost end).  A lane
 *  that is not `live` has `text_length` 0 and keeps (m, 0). */
template <int words_>
__device__ __forceinline__ void fuzzy_best_match(u32 const *table, u32 query_length, u64 address, u32 text_length, bool live, u32 &best,
                                                 u32 &end) {
    u32 const pad = 32u * words_ - query_length;
    u32 vp[words_], vn[words_];
#pragma unroll
    for (int w = 0; w < words_; ++w) vp[w] = rerank_bits_in_word(pad, 32u * words_, w), vn[w] = 0;
    u32 score = query_length;
    best = query_length, end = 0;
    listed_walk(
        text_stream_t(address, text_length), text_length, live,
        [&](u32 symbol, u32 column_end) {
            u32 eq[words_];
            load_match_masks<words_, byte_rows_k>(table, symbol, eq);
            u32 const top = myers_infix_column<words_>(vp, vn, eq);
            score += (top & 1u) - (top >> 1);
            if (score < best) best = score, end = column_end; // strictly smaller: the leftmost end
        },
        []() { return true; });
}

} // namespace szs_hip

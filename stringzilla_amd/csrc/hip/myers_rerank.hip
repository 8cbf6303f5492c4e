/*
 *  myers_rerank.hip - unit-cost byte Levenshtein distances of LISTED pairs (szs_rocm_rerank*, host/rerank.c).
 *
 *  The cross-product kernels (hip/lev_myers.hip) share one Peq table among 256 lanes: one query x 256 candidates.  A rerank row is
 *  one query x the k candidates an index row names - with k = 16 that shape would leave 240 lanes idle per table.  Hence the groups
 *  of 16 / 32 / 64 lanes, one row and one table each, that hip/rerank_core.hpp lays out: rows, tables, indices, flags, the text
 *  walk and the counters are its pieces.  This kernel's own:
 *
 *  - The table is the pattern's bits over ZERO phantom rows: Eq = 0, VP = VN = 0 with +1 entering stays zero and hands HP = 1 upward
 *    - DP row zero of the global matrix.
 *  - myers_column and load_match_masks are hip/myers_core.hpp's, unchanged; distance = len(text) + popcount(VP) - popcount(VN).
 *  - Scores leave as ordinary 8-byte vector stores, straight into the caller's rows.
 */
#include "rerank_core.hpp"

namespace szs_hip {

/**
 *  The rows of one wavefront at `words_` words: every group of `lanes_` lanes builds its row's table, then scores the row's listed
 *  candidates, `lanes_` at a time.
 */
template <int words_, int lanes_>
__device__ __forceinline__ void rerank_rows(u32 *table, listed_row_t const &row, szs_rerank_side_t const &candidates,
                                            u64 const *__restrict__ indices, u64 indices_stride, u64 k, u64 *__restrict__ scores,
                                            u64 scores_stride, u32 *flags, unsigned long long *counters) {
    u32 const sub = threadIdx.x % lanes_;
    u32 const pad = 32u * words_ - row.query_length; // phantom low rows of THIS row (a row without a query: all of them)
    listed_table<words_, lanes_>(table, row, [](int) { return 0u; }, [&](u32 i) { return pad + i; });

    listed_counters_t counted;
#pragma unroll 1
    for (u64 first = 0; first < k; first += lanes_) { // uniform: every row of the call has k slots
        u64 const rank = first + sub;
        u64 const at = row.row * scores_stride + rank;
        u64 address = 0;
        u32 text_length = 0;
        bool const live = row.has_row && rank < k &&
                          listed_candidate(candidates, indices[row.row * indices_stride + rank], [&]() { scores[at] = 0; }, flags, address, text_length);

        u32 vp[words_], vn[words_];
#pragma unroll
        for (int w = 0; w < words_; ++w) vp[w] = rerank_bits_in_word(pad, 32u * words_, w), vn[w] = 0;
        listed_walk(
            text_stream_t(address, text_length), text_length, live,
            [&](u32 symbol, u32) {
                u32 eq[words_];
                load_match_masks<words_, byte_rows_k>(table, symbol, eq);
                // (the carries' xor left to the compiler: spelled as inline assembly it costs this kernel two VGPRs, and the
                // 32-lane shape its sixth wavefront per SIMD.  The compiler's form is one full-rate v_xor more per word-step -
                // 8 logic ops where the other bodies run 7 - in place of the half-rate v_alignbit that went.)
                myers_column<words_, single_pattern_t, true, false>(vp, vn, eq);
            },
            []() { return true; });

        if (live) {
            u32 distance = text_length;
#pragma unroll
            for (int w = 0; w < words_; ++w) distance += (u32)__builtin_popcount(vp[w]) - (u32)__builtin_popcount(vn[w]);
            scores[at] = distance;
            counted.add(row.query_length, text_length);
        }
    }
    counted.land(counters, true);
}

template <int lanes_>
__global__ __launch_bounds__(64) void levenshtein_rerank_kernel(szs_rerank_side_t const queries, szs_rerank_side_t const candidates,
                                                                u64 const first_query, u32 const *__restrict__ rows, u32 const rows_count,
                                                                u64 const *__restrict__ indices, u64 const indices_stride, u64 const k,
                                                                u64 *__restrict__ scores, u64 const scores_stride, u32 const table_dwords,
                                                                u32 *flags, unsigned long long *counters) {
    extern __shared__ __attribute__((aligned(16))) u32 rerank_tables[];
    listed_one_strip_rows<lanes_>(queries, first_query, rows, rows_count, rerank_tables, table_dwords, flags,
                                  [&](auto width, u32 *table, listed_row_t const &row) {
                                      rerank_rows<decltype(width)::value, lanes_>(table, row, candidates, indices, indices_stride, k, scores,
                                                                                  scores_stride, flags, counters);
                                  });
}

} // namespace szs_hip

extern "C" unsigned szs_hip_rerank_lanes(uint64_t k) { return k <= 16 ? 16u : k <= 32 ? 32u : 64u; }

extern "C" int szs_hip_levenshtein_rerank(szs_rerank_side_t const *queries, szs_rerank_side_t const *candidates, uint64_t first_query,
                                          uint32_t const *rows, uint32_t rows_count, uint64_t const *indices, uint64_t indices_stride,
                                          uint64_t k, uint64_t *scores, uint64_t scores_stride, unsigned widest, uint32_t *flags,
                                          unsigned long long *counters, void *stream) {
    using namespace szs_hip;
    if (!rows_count || !k) return 0;
    if (widest < 1 || widest > SZS_MYERS_SHORT_WORDS || !queries || !candidates || !flags || !counters) return (int)hipErrorInvalidValue;
    listed_grid_t const grid = listed_one_strip_grid(k, rows_count, widest);
    return listed_launch(k, [&](auto lanes) {
        hipLaunchKernelGGL(levenshtein_rerank_kernel<decltype(lanes)::value>, dim3(grid.grid), dim3(wave_size_k), grid.lds,
                           static_cast<hipStream_t>(stream), *queries, *candidates, first_query, rows, rows_count, indices, indices_stride, k,
                           scores, scores_stride, grid.table_dwords, flags, counters);
    });
}

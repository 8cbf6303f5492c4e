/*
 *  myers_fuzzy_find.hip - the best match of a query INSIDE each listed candidate (szs_rocm_fuzzy_find*, host/fuzzy_find.c; DESIGN.md
 *  section 4.9): distance = min over j of D[m][j] of the unit-cost DP whose row zero is all zeros (a free start in the text), and
 *  end = the smallest j that attains it.
 *
 *  Groups, rows, tables, indices, flags, the text walk and the counters are hip/rerank_core.hpp's.  The table and the walk of a lane
 *  (hip/fuzzy_core.hpp: shared with hip/myers_fuzzy_tile.hip) are this distance's own:
 *
 *  - The column is myers_infix_column (hip/myers_core.hpp): nothing enters bit 0, and the horizontal pair of the pattern's last row
 *    comes back.  The pattern is right-aligned, so that row is bit 31 of word W - 1 for every row of the wavefront.
 *  - The phantom low rows are WILDCARDS: every row of the Peq table starts as the row's phantom mask (the bits below `pad`), the
 *    pattern's bits are scattered on top.  With Eq = 1, VP = VN = 0 and nothing entering, a phantom row computes D0 = 1, HP = HN = 0,
 *    VP' = VN' = 0 and `Eq & VP` = 0 feeds no carry: it stays zero and hands h = 0 to the first real row in every column - DP row
 *    zero of the semi-global matrix.  (Rows with Eq = 0 would emit HP = 1 upward: the global distance's row zero, wrong here.)
 *  - Every lane tracks the bottom-row score: it starts at m, moves by hp - hn of the last row per column, and a strictly smaller
 *    score moves `best` and `end` (the leftmost end).  A live lane stores both as ordinary 8-byte vector stores.
 *  - `indices` NULL is the dense form: slot r is candidate r.
 */
#include "fuzzy_core.hpp"

namespace szs_hip {

template <int words_, int lanes_>
__device__ __forceinline__ void fuzzy_find_rows(u32 *table, listed_row_t const &row, szs_rerank_side_t const &candidates,
                                                u64 const *__restrict__ indices, u64 indices_stride, u64 k, u64 *__restrict__ distances,
                                                u64 *__restrict__ ends, u64 outputs_stride, u32 *flags, unsigned long long *counters) {
    u32 const sub = threadIdx.x % lanes_;
    fuzzy_table<words_, lanes_>(table, row);

    listed_counters_t counted;
#pragma unroll 1
    for (u64 first = 0; first < k; first += lanes_) { // uniform: every row of the call has k slots
        u64 const rank = first + sub, at = row.row * outputs_stride + rank;
        u64 address = 0;
        u32 text_length = 0;
        auto on_empty = [&]() {
            distances[at] = 0;
            if (ends) ends[at] = 0;
        };
        bool const live = row.has_row && rank < k &&
                          listed_candidate(candidates, indices ? indices[row.row * indices_stride + rank] : rank, on_empty, flags, address,
                                           text_length);

        u32 best, end;
        fuzzy_best_match<words_>(table, row.query_length, address, text_length, live, best, end);

        if (live) {
            distances[at] = best;
            if (ends) ends[at] = end;
            counted.add(row.query_length, text_length);
        }
    }
    counted.land(counters, true);
}

template <int lanes_>
__global__ __launch_bounds__(64) void levenshtein_fuzzy_find_kernel(szs_rerank_side_t const queries, szs_rerank_side_t const candidates,
                                                                    u64 const first_query, u32 const *__restrict__ rows,
                                                                    u32 const rows_count, u64 const *__restrict__ indices,
                                                                    u64 const indices_stride, u64 const k, u64 *__restrict__ distances,
                                                                    u64 *__restrict__ ends, u64 const outputs_stride,
                                                                    u32 const table_dwords, u32 *flags, unsigned long long *counters) {
    extern __shared__ __attribute__((aligned(16))) u32 fuzzy_find_tables[];
    listed_one_strip_rows<lanes_>(queries, first_query, rows, rows_count, fuzzy_find_tables, table_dwords, flags,
                                  [&](auto width, u32 *table, listed_row_t const &row) {
                                      fuzzy_find_rows<decltype(width)::value, lanes_>(table, row, candidates, indices, indices_stride, k,
                                                                                      distances, ends, outputs_stride, flags, counters);
                                  });
}

} // namespace szs_hip

extern "C" int szs_hip_levenshtein_fuzzy_find(szs_rerank_side_t const *queries, szs_rerank_side_t const *candidates, uint64_t first_query,
                                              uint32_t const *rows, uint32_t rows_count, uint64_t const *indices, uint64_t indices_stride,
                                              uint64_t k, uint64_t *distances, uint64_t *ends, uint64_t outputs_stride, unsigned widest,
                                              uint32_t *flags, unsigned long long *counters, void *stream) {
    using namespace szs_hip;
    if (!rows_count || !k) return 0;
    if (widest < 1 || widest > SZS_MYERS_SHORT_WORDS || !queries || !candidates || !distances || !flags || !counters)
        return (int)hipErrorInvalidValue;
    listed_grid_t const grid = listed_one_strip_grid(k, rows_count, widest);
    return listed_launch(k, [&](auto lanes) {
        hipLaunchKernelGGL(levenshtein_fuzzy_find_kernel<decltype(lanes)::value>, dim3(grid.grid), dim3(wave_size_k), grid.lds,
                           static_cast<hipStream_t>(stream), *queries, *candidates, first_query, rows, rows_count, indices, indices_stride, k,
                           distances, ends, outputs_stride, grid.table_dwords, flags, counters);
    });
}

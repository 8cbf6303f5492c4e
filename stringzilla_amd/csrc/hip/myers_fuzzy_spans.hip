/*
 *  myers_fuzzy_spans.hip - where the best match of hip/myers_fuzzy_find.hip STARTS (szs_rocm_fuzzy_find_spans*, host/fuzzy_find.c;
 *  DESIGN.md section 4.9): a second launch behind levenshtein_fuzzy_find_kernel<L> on the same stream, over the same grid, rows,
 *  indices and tables' size.  It reads the `distance` d and the `end` the first kernel wrote per pair and stores
 *      start = end - t*,  t* = the smallest t in [0, min(end, m + d)] with lev(q, c[end - t : end]) == d
 *  - the shortest best match that ends at `end`.  Such a t exists (D[m][end] = min over s of lev(q, c[s : end]) = d), none gives
 *  less (d is the minimum over all substrings), and |t - m| <= d for any t that attains d: the window is at most 2 m <= 512 bytes,
 *  whatever the candidate's length.
 *
 *  The pass is the GLOBAL unit-cost column of the REVERSED query against c[end - 1], c[end - 2], ...: D'[0][t] = t, D'[i][0] = i.
 *  Groups, rows, tables, indices, flags, the text walk and the counters are hip/rerank_core.hpp's.  This kernel's own:
 *
 *  - The table is zeroed, then the pattern's bits - byte i of the query at bit pad + (m - 1 - i).  The phantom low rows are ZERO
 *    rows, not wildcards: Eq = 0, VP = VN = 0 with +1 entering stays zero and hands HP = 1 upward - DP row zero of the global
 *    matrix, D'[0][t] = t (hip/myers_rerank.hip; tests/test_fuzzy_spans_model.py asserts that they stay zero).
 *  - The column is myers_prefix_column<W> (hip/myers_core.hpp) - myers_strip_column<W>(vp, vn, eq, 1, 0) with myers_column's
 *    materialisation: +1 enters bit 0, the horizontal pair of the last pattern row comes back.
 *  - The text is the window c[end - T, end), T = min(end, m + d), walked from its last byte down (text_stream_backward_t): group
 *    `back` is bytes [T - 4 back - 4, T - 4 back), consumed from the top byte.
 *  - Every lane tracks the bottom-row score from score = best = m, pos = 0: a strictly smaller score moves `best` and `pos` (the
 *    smallest t), start = end - pos.  A wavefront leaves the walk once every live lane has best == d: nothing can move `pos` then.
 *
 *  The candidate is derived from the index again, behind the same checks.  d and end are data the kernel reads back from memory the
 *  caller can reach, so before they address anything: d <= m and end <= the candidate's length, else SZS_RERANK_FLAG_TAPE and a
 *  frozen lane.  The counters gain m x T cells and m + T bytes per pair; pairs are counted by the first kernel only.
 */
#include "fuzzy_core.hpp"

namespace szs_hip {

/** (the table and a lane's walk are hip/fuzzy_core.hpp's fuzzy_reversed_table and fuzzy_start_walk: hip/myers_fuzzy_occurrences.hip
 *  runs the same pass over a matrix of slots in one text) */
template <int words_, int lanes_>
__device__ __forceinline__ void fuzzy_starts_rows(u32 *table, listed_row_t const &row, szs_rerank_side_t const &candidates,
                                                  u64 const *__restrict__ indices, u64 indices_stride, u64 k,
                                                  u64 const *__restrict__ distances, u64 const *__restrict__ ends, u64 *__restrict__ starts,
                                                  u64 outputs_stride, u32 *flags, unsigned long long *counters) {
    u32 const sub = threadIdx.x % lanes_;
    u32 const query_length = row.query_length;
    fuzzy_reversed_table<words_, lanes_>(table, row); // (a row without a query: phantom rows only)

    listed_counters_t counted;
#pragma unroll 1
    for (u64 first = 0; first < k; first += lanes_) { // uniform: every row of the call has k slots
        u64 const rank = first + sub, at = row.row * outputs_stride + rank;
        u64 address = 0;
        u32 text_length = 0, window = 0, distance = 0, end = 0; // the window: T bytes that end at `end`
        bool live = row.has_row && rank < k &&
                    listed_candidate(candidates, indices ? indices[row.row * indices_stride + rank] : rank, [&]() { starts[at] = 0; }, flags,
                                     address, text_length);
        if (live) {
            u64 const found = distances[at], ended = ends[at];
            if (found > query_length || ended > text_length) flags[SZS_RERANK_FLAG_TAPE] = 1u, live = false; // before they address anything
            else {
                distance = (u32)found, end = (u32)ended;
                window = end < query_length + distance ? end : query_length + distance;
            }
        }

        u32 const pos = fuzzy_start_walk<words_>(table, query_length, address, end, window, distance, live);
        if (live) {
            starts[at] = end - pos;
            counted.add(query_length, window);
        }
    }
    counted.land(counters, false);
}

template <int lanes_>
__global__ __launch_bounds__(64) void levenshtein_fuzzy_starts_kernel(szs_rerank_side_t const queries, szs_rerank_side_t const candidates,
                                                                      u64 const first_query, u32 const *__restrict__ rows,
                                                                      u32 const rows_count, u64 const *__restrict__ indices,
                                                                      u64 const indices_stride, u64 const k,
                                                                      u64 const *__restrict__ distances, u64 const *__restrict__ ends,
                                                                      u64 *__restrict__ starts, u64 const outputs_stride,
                                                                      u32 const table_dwords, u32 *flags, unsigned long long *counters) {
    extern __shared__ __attribute__((aligned(16))) u32 fuzzy_starts_tables[];
    listed_one_strip_rows<lanes_>(queries, first_query, rows, rows_count, fuzzy_starts_tables, table_dwords, flags,
                                  [&](auto width, u32 *table, listed_row_t const &row) {
                                      fuzzy_starts_rows<decltype(width)::value, lanes_>(table, row, candidates, indices, indices_stride, k,
                                                                                        distances, ends, starts, outputs_stride, flags,
                                                                                        counters);
                                  });
}

} // namespace szs_hip

extern "C" int szs_hip_levenshtein_fuzzy_starts(szs_rerank_side_t const *queries, szs_rerank_side_t const *candidates, uint64_t first_query,
                                                uint32_t const *rows, uint32_t rows_count, uint64_t const *indices, uint64_t indices_stride,
                                                uint64_t k, uint64_t const *distances, uint64_t const *ends, uint64_t *starts,
                                                uint64_t outputs_stride, unsigned widest, uint32_t *flags, unsigned long long *counters,
                                                void *stream) {
    using namespace szs_hip;
    if (!rows_count || !k) return 0;
    if (widest < 1 || widest > SZS_MYERS_SHORT_WORDS || !queries || !candidates || !distances || !ends || !starts || !flags || !counters)
        return (int)hipErrorInvalidValue;
    listed_grid_t const grid = listed_one_strip_grid(k, rows_count, widest); // the first kernel's
    return listed_launch(k, [&](auto lanes) {
        hipLaunchKernelGGL(levenshtein_fuzzy_starts_kernel<decltype(lanes)::value>, dim3(grid.grid), dim3(wave_size_k), grid.lds,
                           static_cast<hipStream_t>(stream), *queries, *candidates, first_query, rows, rows_count, indices, indices_stride, k,
                           distances, ends, starts, outputs_stride, grid.table_dwords, flags, counters);
    });
}

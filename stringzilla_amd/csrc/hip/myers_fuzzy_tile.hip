/*
 *  myers_fuzzy_tile.hip - a TILE of the semi-global distance: (a block of queries) x (a run of consecutive candidates), one 8-byte cell
 *  a pair, for the search that keeps the k best candidates of every query (szs_rocm_fuzzy_search*, host/fuzzy_search.c; DESIGN.md
 *  section 4.10).  hip/top_k.hip folds the tile as it folds an engine's.
 *
 *  The distance, its table and a lane's walk are hip/fuzzy_core.hpp's, shared with hip/myers_fuzzy_find.hip; rows, candidates, flags
 *  and counters are hip/rerank_core.hpp's.  What differs from the listed kernel is who gets a workgroup:
 *
 *  - A one-wavefront workgroup serves ONE row and a SEGMENT of the tile's columns (a multiple of 64): its 64 lanes build the row's
 *    table once, at the row's own width, and take the segment's candidates 64 at a time against it.  So the grid is rows x segments,
 *    not rows: a handful of queries over a large corpus still fills the device, and no row waits for a longer neighbour's width.
 *  - Workgroups are numbered segment-major (row = id % rows): those in flight together read the same candidates.
 *  - The candidate of a lane is a column number, not a listed index: listed_candidate with first_column + column.
 *  - Every cell of the tile is stored - a query of no bytes scores 0 in every candidate without a walk - by ordinary 8-byte vector
 *    stores; lanes beyond `columns` store nothing.  A pair whose string cannot be fetched raises its flag and stores 0.
 *  - The table is static LDS of the widest layout (8 KB): 20 workgroups a CU fit, what the registers allow (5 waves a SIMD).
 */
#include "fuzzy_core.hpp"

namespace szs_hip {

template <int words_>
__device__ __forceinline__ void fuzzy_tile_row(u32 *table, listed_row_t const &row, szs_rerank_side_t const &candidates, u64 first_column,
                                               u32 begin, u32 end, u64 *__restrict__ row_cells, u32 *flags, unsigned long long *counters) {
    fuzzy_table<words_, (int)wave_size_k>(table, row);

    listed_counters_t counted;
#pragma unroll 1
    for (u32 base = begin; base < end; base += wave_size_k) { // uniform over the wavefront
        u32 const column = base + threadIdx.x;
        u64 address = 0;
        u32 text_length = 0;
        bool const paired = row.has_row && column < end &&
                            listed_candidate(candidates, first_column + column, []() {}, flags, address, text_length);
        bool const live = paired && row.query_length; // an empty query: 0 everywhere, nothing to walk
        u32 const walked = live ? text_length : 0u;

        u32 best, match_end;
        fuzzy_best_match<words_>(table, row.query_length, address, walked, live, best, match_end);

        if (column < end) row_cells[column] = live ? best : 0u;
        if (paired) counted.add(row.query_length, walked);
    }
    counted.land(counters, true);
}

__global__ __launch_bounds__(64) void levenshtein_fuzzy_tile_kernel(szs_rerank_side_t const queries, szs_rerank_side_t const candidates,
                                                                    u64 const first_query, u32 const rows, u64 const first_column,
                                                                    u32 const columns, u32 const segment, u64 *__restrict__ cells,
                                                                    u64 const cells_stride, u32 *flags, unsigned long long *counters) {
    __shared__ __attribute__((aligned(16))) u32 fuzzy_tile_table[peq_layout<SZS_MYERS_SHORT_WORDS, byte_rows_k>::total_dwords];
    u32 const r = blockIdx.x % rows;
    u64 const begin = (u64)(blockIdx.x / rows) * segment; // below `columns`: the host launches ceil(columns / segment) segments
    u32 const end = begin + segment < columns ? (u32)(begin + segment) : columns;
    listed_row_t const row = listed_row(queries, first_query, true, [&]() { return r; }, SZS_RERANK_LONGEST_QUERY, flags);
    u32 const length = (u32)__builtin_amdgcn_readfirstlane((int)row.query_length); // one row a wavefront: a scalar
    listed_at_width(SZS_RERANK_WORDS_OF(length), [&](auto width) {
        fuzzy_tile_row<decltype(width)::value>(fuzzy_tile_table, row, candidates, first_column, (u32)begin, end, cells + (u64)r * cells_stride,
                                               flags, counters);
    });
}

} // namespace szs_hip

extern "C" int szs_hip_levenshtein_fuzzy_tile(szs_rerank_side_t const *queries, szs_rerank_side_t const *candidates, uint64_t first_query,
                                              uint32_t rows, uint64_t first_column, uint32_t columns, uint32_t segment, uint64_t *cells,
                                              uint64_t cells_stride, uint32_t *flags, unsigned long long *counters, void *stream) {
    using namespace szs_hip;
    if (!rows || !columns) return 0;
    if (!segment || segment % wave_size_k || !queries || !candidates || !cells || cells_stride < columns || !flags || !counters)
        return (int)hipErrorInvalidValue;
    if (first_query + rows > queries->count || first_column + columns > candidates->count) return (int)hipErrorInvalidValue;
    u64 const workgroups = (u64)rows * (((u64)columns + segment - 1) / segment);
    if (workgroups > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(levenshtein_fuzzy_tile_kernel, dim3((u32)workgroups), dim3(wave_size_k), 0, static_cast<hipStream_t>(stream), *queries,
                       *candidates, first_query, rows, first_column, columns, segment, cells, cells_stride, flags, counters);
    return (int)hipGetLastError();
}

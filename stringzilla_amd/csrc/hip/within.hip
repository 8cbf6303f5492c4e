/*
 *  within.hip - every candidate of every query inside a score bound, folded tile by tile out of a scored (queries x candidates)
 *  tile, on the device (host/selection.c drives it for host/within.c and host/fuzzy_search.c).
 *
 *  A cell HITS when it is <= the bound as an unsigned distance, or - `descending`, NW / SW - >= the bound as a signed score; the
 *  own column of a self-search never hits.  Every row keeps a RUNNING COUNT of the hits of the tiles folded so far, and the leftmost
 *  `limit` hits of a row land in slots 0, 1, ... of its output row in ascending candidate order - tiles arrive in that order:
 *
 *    within_count_kernel   one workgroup per (row, segment of the tile's columns): every wavefront compares, ballots and popcounts;
 *                          the workgroup leaves ONE partial count.
 *    within_store_kernel   the same grid.  The base of a segment is the row's running count plus the partials of the segments before
 *                          it; a segment whose base is already >= limit returns at once.  Otherwise it walks its cells again: the
 *                          rank of a hit is the base, the hits of the rounds before, of the wavefront chunks before it in its round
 *                          and of the lanes below it in its ballot (mbcnt) - the cell goes to slot `rank` where that is below
 *                          `limit`, by ordinary 8-byte stores.  The first segment of a row also writes the running count of the
 *                          NEXT tile - the old one plus every partial - into the other half of a two-halves buffer, which the
 *                          other segments of the launch do not read.
 *    within_finish_kernel  counts[row] and the empty pair (~0, 0) in slots [min(count, limit), limit).
 *
 *  No atomic decides a slot or a count: a result depends on the cells alone - not on the tile, the segment or any knob.  With
 *  `limit` = 0 the store pass is not launched: the count pass then ADDS to its partial, every workgroup to its own word, and the
 *  finish sums a row's partials.  Every address is 64-bit; a row, a column and a slot are compared with `rows`, `columns` and
 *  `limit` before they address anything.
 */
#include "device_common.hpp"

namespace szs_hip {

constexpr u32 within_threads_k = 256;
constexpr u32 within_waves_k = within_threads_k / wave_size_k;
constexpr u32 within_cells_per_thread_k = 4; /* loads in flight per thread before the first comparison (hip/top_k.hip's) */
constexpr u32 within_round_k = within_threads_k * within_cells_per_thread_k;

template <bool descending> __device__ __forceinline__ bool within_hit(u64 cell, u64 bound) {
    return descending ? (i64)cell >= (i64)bound : cell <= bound;
}

/** The columns [begin, end) of the tile that workgroup `segment` of its row walks; empty for a segment behind a narrow last tile. */
__device__ __forceinline__ void within_segment(u32 segment, u32 segment_columns, u32 columns, u32 &begin, u32 &end) {
    u64 const first = (u64)segment * segment_columns, last = first + segment_columns;
    begin = first < columns ? (u32)first : columns;
    end = last < columns ? (u32)last : columns;
}

/** The hits of one round of a wavefront: chunk `s` holds columns base + s * 256 + thread. */
template <bool descending>
__device__ __forceinline__ void within_round(u64 const *__restrict__ row_cells, u32 base, u32 end, u64 first_column, u64 excluded, u64 bound,
                                             u64 (&values)[within_cells_per_thread_k], bool (&hits)[within_cells_per_thread_k]) {
#pragma unroll
    for (u32 s = 0; s < within_cells_per_thread_k; ++s) {
        u32 const column = base + s * within_threads_k + threadIdx.x;
        values[s] = column < end ? row_cells[column] : 0;
    }
#pragma unroll
    for (u32 s = 0; s < within_cells_per_thread_k; ++s) {
        u32 const column = base + s * within_threads_k + threadIdx.x;
        hits[s] = column < end && first_column + column != excluded && within_hit<descending>(values[s], bound);
    }
}

template <bool descending>
__global__ __launch_bounds__(within_threads_k) void within_count_kernel(u64 const *__restrict__ cells, u64 cells_stride, u32 rows, u32 columns,
                                                                        u64 first_column, u64 self_first_row, u64 bound, u32 segments,
                                                                        u32 segment_columns, u32 *__restrict__ partials, int accumulate) {
    __shared__ u32 wave_counts[within_waves_k];
    u32 const row = blockIdx.x / segments, segment = blockIdx.x % segments;
    if (row >= rows) return;
    u32 begin, end;
    within_segment(segment, segment_columns, columns, begin, end);
    u64 const *const row_cells = cells + (u64)row * cells_stride;
    u64 const excluded = self_first_row == ~0ull ? ~0ull : self_first_row + row; /* self-search: the query's own column */

    u32 count = 0; /* of this wavefront: the same in every lane */
    for (u32 base = begin; base < end; base += within_round_k) {
        u64 values[within_cells_per_thread_k];
        bool hits[within_cells_per_thread_k];
        within_round<descending>(row_cells, base, end, first_column, excluded, bound, values, hits);
#pragma unroll
        for (u32 s = 0; s < within_cells_per_thread_k; ++s) count += (u32)__popcll(__ballot(hits[s]));
    }
    if ((threadIdx.x & 63u) == 0) wave_counts[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x != 0) return;
    u32 total = 0;
#pragma unroll
    for (u32 w = 0; w < within_waves_k; ++w) total += wave_counts[w];
    partials[blockIdx.x] = accumulate ? partials[blockIdx.x] + total : total;
}

template <bool descending>
__global__ __launch_bounds__(within_threads_k) void within_store_kernel(u64 const *__restrict__ cells, u64 cells_stride, u32 rows, u32 columns,
                                                                        u64 first_column, u64 self_first_row, u64 bound, u32 segments,
                                                                        u32 segment_columns, u32 const *__restrict__ partials,
                                                                        u64 const *__restrict__ running, u64 *__restrict__ running_next,
                                                                        u32 limit, u64 *__restrict__ indices, u64 *__restrict__ scores,
                                                                        u64 stride) {
    /* two halves, taken in turn: a round writes one while a slow wavefront may still read the round before in the other */
    __shared__ u32 chunk_counts[2][within_cells_per_thread_k][within_waves_k];
    u32 const row = blockIdx.x / segments, segment = blockIdx.x % segments;
    if (row >= rows) return;
    u32 const *const row_partials = partials + (u64)row * segments;
    u64 slot = running[row]; /* of the next hit of this segment: the same in every lane */
    for (u32 s = 0; s < segment; ++s) slot += row_partials[s];
    if (segment == 0) {
        u64 total = slot;
        for (u32 s = 0; s < segments; ++s) total += row_partials[s];
        if (threadIdx.x == 0) running_next[row] = total;
    }
    if (slot >= limit) return; /* uniform: the leftmost `limit` hits of the row lie before this segment */

    u32 begin, end;
    within_segment(segment, segment_columns, columns, begin, end);
    u64 const *const row_cells = cells + (u64)row * cells_stride;
    u64 const excluded = self_first_row == ~0ull ? ~0ull : self_first_row + row;
    u64 *const row_indices = indices + (u64)row * stride, *const row_scores = scores ? scores + (u64)row * stride : nullptr;
    u32 const wave = threadIdx.x >> 6;

    u32 parity = 0;
    for (u32 base = begin; base < end && slot < limit; base += within_round_k, parity ^= 1u) {
        u64 values[within_cells_per_thread_k];
        bool hits[within_cells_per_thread_k];
        within_round<descending>(row_cells, base, end, first_column, excluded, bound, values, hits);
        u32 below[within_cells_per_thread_k]; /* hits of the lanes below this one in its chunk */
#pragma unroll
        for (u32 s = 0; s < within_cells_per_thread_k; ++s) {
            u64 const ballot = __ballot(hits[s]);
            below[s] = __builtin_amdgcn_mbcnt_hi((u32)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((u32)ballot, 0u));
            if ((threadIdx.x & 63u) == 0) chunk_counts[parity][s][wave] = (u32)__popcll(ballot);
        }
        __syncthreads();
#pragma unroll
        for (u32 s = 0; s < within_cells_per_thread_k; ++s) {
#pragma unroll
            for (u32 w = 0; w < within_waves_k; ++w) {
                u32 const chunk = chunk_counts[parity][s][w];
                if (w == wave && hits[s]) {
                    u64 const rank = slot + below[s];
                    if (rank < limit) {
                        row_indices[rank] = first_column + base + s * within_threads_k + threadIdx.x;
                        if (row_scores) row_scores[rank] = values[s];
                    }
                }
                slot += chunk;
            }
        }
    }
}

__global__ __launch_bounds__(within_threads_k) void within_finish_kernel(u64 const *__restrict__ running, u32 const *__restrict__ partials,
                                                                         u32 segments, u32 rows, u32 limit, u64 *__restrict__ counts,
                                                                         u64 *__restrict__ indices, u64 *__restrict__ scores, u64 stride) {
    u32 const per_row = limit ? limit : 1; /* a thread per slot, and the first of a row writes its count */
    u64 const item = (u64)blockIdx.x * within_threads_k + threadIdx.x;
    if (item >= (u64)rows * per_row) return;
    u32 const row = (u32)(item / per_row), slot = (u32)(item % per_row);
    u64 count = running[row];
    for (u32 s = 0; s < segments; ++s) count += partials[(u64)row * segments + s]; /* (segments 0: the partials are in the running count) */
    if (slot == 0) counts[row] = count;
    if (slot >= limit || slot < count) return;
    indices[(u64)row * stride + slot] = ~0ull;
    if (scores) scores[(u64)row * stride + slot] = 0;
}

} // namespace szs_hip

extern "C" int szs_hip_within_fold(uint64_t const *cells, uint64_t cells_stride, uint32_t rows, uint32_t columns, uint64_t first_column,
                                   uint64_t self_first_row, uint64_t bound, int descending, uint32_t segments, uint32_t segment_columns,
                                   uint32_t *partials, uint64_t const *running, uint64_t *running_next, uint32_t limit, uint64_t *indices,
                                   uint64_t *scores, uint64_t stride, void *stream) {
    using namespace szs_hip;
    if (!rows || !columns) return 0;
    if (!cells || !partials || segments < 1 || segment_columns < 1 || (uint64_t)rows * segments > 0x7FFFFFFFull ||
        (uint64_t)segments * segment_columns < columns || limit > SZS_WITHIN_MOST)
        return (int)hipErrorInvalidValue;
    if (limit && (!running || !running_next || running == running_next || !indices || stride < limit)) return (int)hipErrorInvalidValue;
    hipStream_t const s = static_cast<hipStream_t>(stream);
    dim3 const grid(rows * segments), threads(within_threads_k);
    if (descending)
        hipLaunchKernelGGL(within_count_kernel<true>, grid, threads, 0, s, cells, cells_stride, rows, columns, first_column, self_first_row,
                           bound, segments, segment_columns, partials, limit == 0);
    else
        hipLaunchKernelGGL(within_count_kernel<false>, grid, threads, 0, s, cells, cells_stride, rows, columns, first_column, self_first_row,
                           bound, segments, segment_columns, partials, limit == 0);
    hipError_t const error = hipGetLastError();
    if (error != hipSuccess || !limit) return (int)error;
    if (descending)
        hipLaunchKernelGGL(within_store_kernel<true>, grid, threads, 0, s, cells, cells_stride, rows, columns, first_column, self_first_row,
                           bound, segments, segment_columns, partials, running, running_next, limit, indices, scores, stride);
    else
        hipLaunchKernelGGL(within_store_kernel<false>, grid, threads, 0, s, cells, cells_stride, rows, columns, first_column, self_first_row,
                           bound, segments, segment_columns, partials, running, running_next, limit, indices, scores, stride);
    return (int)hipGetLastError();
}

extern "C" int szs_hip_within_finish(uint64_t const *running, uint32_t const *partials, uint32_t segments, uint32_t rows, uint32_t limit,
                                     uint64_t *counts, uint64_t *indices, uint64_t *scores, uint64_t stride, void *stream) {
    using namespace szs_hip;
    if (!rows) return 0;
    if (!running || !counts || (segments && !partials) || limit > SZS_WITHIN_MOST || (limit && (!indices || stride < limit)))
        return (int)hipErrorInvalidValue;
    u64 const blocks = ((u64)rows * (limit ? limit : 1) + within_threads_k - 1) / within_threads_k;
    if (blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(within_finish_kernel, dim3((u32)blocks), dim3(within_threads_k), 0, static_cast<hipStream_t>(stream), running, partials,
                       segments, rows, limit, counts, indices, scores, stride);
    return (int)hipGetLastError();
}

/*
 *  top_k.hip - the k best candidates of every query, folded tile by tile out of a scored (queries x candidates) tile, on the device
 *  (host/top_k.c drives it).
 *
 *  Every entry of a list is an exact (key, index) pair of 64-bit values, compared lexicographically - never packed into one word:
 *  the key is the cell itself for the distances (ascending), and the order-reversing image of the signed score for NW / SW
 *  (descending), so "smaller pair = better" in both directions and ties go to the lower candidate index.  The sentinel
 *  (~0, ~0) loses to every real cell, whose index is always below ~0.
 *
 *    top_k_scan_kernel    one workgroup per (row, segment of the row): streams its cells, keeps those that STRICTLY beat the
 *                         current k-th pair - the row's running list's, or its own once that is better - in an LDS buffer compacted
 *                         with __ballot + mbcnt, and folds a full buffer into its sorted list of K2 = pow2(k) pairs (bitonic sort
 *                         of the buffer, one bitonic merge).  With one segment per row the list IS the row's running list.
 *    top_k_fold_kernel    one workgroup per row: merges the segments' partial lists into the row's running list.
 *    top_k_emit_kernel    the first k pairs of every running list as (index, score) rows of the caller's arrays; a sentinel becomes
 *                         index SZ_SIZE_MAX and score 0 (a row with fewer than k candidates).
 *
 *  A list in global memory is 2 * K2 words: K2 keys, then K2 indices.  Tiles arrive in ascending candidate order, so a cell that
 *  equals the running k-th score has a higher index and loses - the strict comparison IS the tie rule.
 */
#include "device_common.hpp"

namespace szs_hip {

constexpr u32 top_k_threads_k = 256;
constexpr u32 top_k_cells_per_thread_k = 4; /* loads in flight per thread before the first comparison */
constexpr u64 sign_bit_k = 0x8000000000000000ull;

/** Distances rank ascending as they are; scores rank descending: flip the sign bit (signed -> unsigned order), then invert. */
template <bool descending> __device__ __forceinline__ u64 rank_key(u64 cell) { return descending ? ~(cell ^ sign_bit_k) : cell; }
template <bool descending> __device__ __forceinline__ u64 cell_of(u64 key) { return descending ? (~key) ^ sign_bit_k : key; }

__device__ __forceinline__ bool pair_less(u64 key_a, u64 index_a, u64 key_b, u64 index_b) {
    return key_a < key_b || (key_a == key_b && index_a < index_b);
}

/** Sorts `count` (a power of two) pairs ascending; every thread of the workgroup calls it. */
__device__ void bitonic_sort(u64 *keys, u64 *indices, u32 count) {
    for (u32 size = 2; size <= count; size <<= 1)
        for (u32 stride = size >> 1; stride > 0; stride >>= 1) {
            for (u32 t = threadIdx.x; t < count / 2; t += top_k_threads_k) {
                u32 const i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i + stride; /* (stride: a power of two) */
                bool const ascending = (i & size) == 0;
                u64 const ki = keys[i], kj = keys[j], ii = indices[i], ij = indices[j];
                if (pair_less(kj, ij, ki, ii) == ascending) keys[i] = kj, keys[j] = ki, indices[i] = ij, indices[j] = ii;
            }
            __syncthreads();
        }
}

/**
 *  `list` (ascending, `width` pairs) := the `width` smallest pairs of `list` and of the ascending `other` (at least `width` pairs):
 *  min(list[i], other[width - 1 - i]) is a bitonic sequence holding exactly those, and one bitonic merge sorts it.
 */
__device__ void merge_into(u64 *keys, u64 *indices, u64 const *other_keys, u64 const *other_indices, u32 width) {
    for (u32 i = threadIdx.x; i < width; i += top_k_threads_k) {
        u64 const ko = other_keys[width - 1 - i], io = other_indices[width - 1 - i];
        if (pair_less(ko, io, keys[i], indices[i])) keys[i] = ko, indices[i] = io;
    }
    __syncthreads();
    for (u32 stride = width >> 1; stride > 0; stride >>= 1) {
        for (u32 t = threadIdx.x; t < width / 2; t += top_k_threads_k) {
            u32 const i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i + stride; /* (stride: a power of two) */
            u64 const ki = keys[i], kj = keys[j], ii = indices[i], ij = indices[j];
            if (pair_less(kj, ij, ki, ii)) keys[i] = kj, keys[j] = ki, indices[i] = ij, indices[j] = ii;
        }
        __syncthreads();
    }
}

/**
 *  LDS: list keys [width], list indices [width], buffer keys [buffer], buffer indices [buffer], then the buffer's fill count.
 *  `buffer` >= width and >= 2 * 256: a flush happens once fewer than 256 slots are left, so one round of 256 cells always fits.
 */
template <bool descending>
__global__ __launch_bounds__(top_k_threads_k) void top_k_scan_kernel(u64 const *__restrict__ cells, u64 cells_stride, u32 columns,
                                                                      u64 first_column, u64 self_first_row, u64 *__restrict__ lists,
                                                                      u64 *__restrict__ partials, u32 segments, u32 segment_columns,
                                                                      u32 k, u32 width, u32 buffer) {
    extern __shared__ __align__(16) u64 top_k_lds[];
    u64 *const list_keys = top_k_lds, *const list_indices = list_keys + width;
    u64 *const buffer_keys = list_indices + width, *const buffer_indices = buffer_keys + buffer;
    u32 *const fill = reinterpret_cast<u32 *>(buffer_indices + buffer);

    u32 const row = blockIdx.x / segments, segment = blockIdx.x % segments;
    u64 const *const running = lists + (u64)row * 2 * width;
    for (u32 i = threadIdx.x; i < width; i += top_k_threads_k) {
        bool const inherit = segment == 0;
        list_keys[i] = inherit ? running[i] : ~0ull;
        list_indices[i] = inherit ? running[width + i] : ~0ull;
    }
    if (threadIdx.x == 0) *fill = 0;
    u64 threshold_key = running[k - 1], threshold_index = running[width + k - 1];
    __syncthreads();

    u32 const begin = segment * segment_columns;
    u32 const end = begin + segment_columns < columns ? begin + segment_columns : columns;
    u64 const *const row_cells = cells + (u64)row * cells_stride;
    u64 const excluded = self_first_row == ~0ull ? ~0ull : self_first_row + row; /* self-search: the query's own column */
    u32 const lane = threadIdx.x & 63u;

    auto flush = [&](u32 count) {
        u32 sorted = width;
        while (sorted < count) sorted <<= 1;
        for (u32 i = count + threadIdx.x; i < sorted; i += top_k_threads_k) buffer_keys[i] = ~0ull, buffer_indices[i] = ~0ull;
        __syncthreads();
        bitonic_sort(buffer_keys, buffer_indices, sorted);
        merge_into(list_keys, list_indices, buffer_keys, buffer_indices, width);
        if (pair_less(list_keys[k - 1], list_indices[k - 1], threshold_key, threshold_index))
            threshold_key = list_keys[k - 1], threshold_index = list_indices[k - 1];
        if (threadIdx.x == 0) *fill = 0;
        __syncthreads();
    };

    for (u32 base = begin; base < end; base += top_k_threads_k * top_k_cells_per_thread_k) {
        u64 values[top_k_cells_per_thread_k];
#pragma unroll
        for (u32 s = 0; s < top_k_cells_per_thread_k; ++s) {
            u32 const column = base + s * top_k_threads_k + threadIdx.x;
            values[s] = column < end ? row_cells[column] : 0;
        }
#pragma unroll
        for (u32 s = 0; s < top_k_cells_per_thread_k; ++s) {
            u32 const column = base + s * top_k_threads_k + threadIdx.x;
            u64 const index = first_column + column, key = rank_key<descending>(values[s]);
            bool const keep = column < end && index != excluded && pair_less(key, index, threshold_key, threshold_index);
            u64 const kept = __ballot(keep);
            u32 const before = __builtin_amdgcn_mbcnt_hi((u32)(kept >> 32), __builtin_amdgcn_mbcnt_lo((u32)kept, 0u));
            u32 slot = 0;
            if (kept && lane == 0) slot = atomicAdd(fill, (u32)__popcll(kept));
            slot = (u32)__shfl((int)slot, 0, 64);
            if (keep) buffer_keys[slot + before] = key, buffer_indices[slot + before] = index;
            __syncthreads();
            u32 const count = *fill;
            __syncthreads();
            if (count + top_k_threads_k > buffer) flush(count);
        }
    }
    u32 const count = *fill;
    __syncthreads(); /* (no thread may reset `fill` before every thread has read it) */
    if (count) flush(count);

    u64 *const out = segments == 1 ? lists + (u64)row * 2 * width : partials + (u64)blockIdx.x * 2 * width;
    for (u32 i = threadIdx.x; i < width; i += top_k_threads_k) out[i] = list_keys[i], out[width + i] = list_indices[i];
}

/** The partial lists of a row's `segments` (the first one already holds the running list) into the running list. */
__global__ __launch_bounds__(top_k_threads_k) void top_k_fold_kernel(u64 *__restrict__ lists, u64 const *__restrict__ partials,
                                                                     u32 segments, u32 width) {
    extern __shared__ __align__(16) u64 top_k_lds[];
    u64 *const list_keys = top_k_lds, *const list_indices = list_keys + width;
    u64 *const other_keys = list_indices + width, *const other_indices = other_keys + width;
    u64 const *const first = partials + (u64)blockIdx.x * segments * 2 * width;
    for (u32 i = threadIdx.x; i < width; i += top_k_threads_k) list_keys[i] = first[i], list_indices[i] = first[width + i];
    for (u32 s = 1; s < segments; ++s) {
        u64 const *const partial = first + (u64)s * 2 * width;
        for (u32 i = threadIdx.x; i < width; i += top_k_threads_k) other_keys[i] = partial[i], other_indices[i] = partial[width + i];
        __syncthreads();
        merge_into(list_keys, list_indices, other_keys, other_indices, width);
    }
    u64 *const out = lists + (u64)blockIdx.x * 2 * width;
    for (u32 i = threadIdx.x; i < width; i += top_k_threads_k) out[i] = list_keys[i], out[width + i] = list_indices[i];
}

template <bool descending>
__global__ __launch_bounds__(top_k_threads_k) void top_k_emit_kernel(u64 const *__restrict__ lists, u32 rows, u32 k, u32 width,
                                                                     u64 *__restrict__ indices, u64 *__restrict__ scores, u64 stride) {
    u64 const item = (u64)blockIdx.x * top_k_threads_k + threadIdx.x;
    if (item >= (u64)rows * k) return;
    u32 const row = (u32)(item / k), rank = (u32)(item % k);
    u64 const key = lists[(u64)row * 2 * width + rank], index = lists[(u64)row * 2 * width + width + rank];
    bool const empty = index == ~0ull;
    indices[(u64)row * stride + rank] = index;
    if (scores) scores[(u64)row * stride + rank] = empty ? 0 : cell_of<descending>(key);
}

} // namespace szs_hip

extern "C" size_t szs_hip_top_k_width(uint32_t k) {
    uint32_t width = 1;
    while (width < k) width <<= 1;
    return width;
}

extern "C" size_t szs_hip_top_k_scan_lds_bytes(uint32_t k) {
    size_t const width = szs_hip_top_k_width(k), buffer = width > 512 ? 2 * width : 512;
    return (width + buffer) * 2 * sizeof(uint64_t) + 16;
}

extern "C" int szs_hip_top_k_scan(uint64_t const *cells, uint64_t cells_stride, uint32_t rows, uint32_t columns, uint64_t first_column,
                                  uint64_t self_first_row, uint64_t *lists, uint64_t *partials, uint32_t segments, uint32_t k,
                                  int descending, void *stream) {
    using namespace szs_hip;
    if (!rows || !columns) return 0;
    if (segments < 1 || (uint64_t)rows * segments > 0x7FFFFFFFull || k < 1 || k > SZS_TOP_K_MOST) return (int)hipErrorInvalidValue;
    u32 const width = (u32)szs_hip_top_k_width(k), buffer = width > 512 ? 2 * width : 512;
    u32 const quantum = top_k_threads_k * top_k_cells_per_thread_k;
    u32 const per_segment = (u32)((((u64)columns + segments - 1) / segments + quantum - 1) / quantum * quantum);
    size_t const lds = szs_hip_top_k_scan_lds_bytes(k);
    hipStream_t const s = static_cast<hipStream_t>(stream);
    if (descending)
        hipLaunchKernelGGL(top_k_scan_kernel<true>, dim3(rows * segments), dim3(top_k_threads_k), lds, s, cells, cells_stride, columns,
                           first_column, self_first_row, lists, partials, segments, per_segment, k, width, buffer);
    else
        hipLaunchKernelGGL(top_k_scan_kernel<false>, dim3(rows * segments), dim3(top_k_threads_k), lds, s, cells, cells_stride, columns,
                           first_column, self_first_row, lists, partials, segments, per_segment, k, width, buffer);
    hipError_t error = hipGetLastError();
    if (error != hipSuccess || segments == 1) return (int)error;
    hipLaunchKernelGGL(top_k_fold_kernel, dim3(rows), dim3(top_k_threads_k), 4 * width * sizeof(u64), s, lists, partials, segments, width);
    return (int)hipGetLastError();
}

extern "C" int szs_hip_top_k_emit(uint64_t const *lists, uint32_t rows, uint32_t k, uint64_t *indices, uint64_t *scores, uint64_t stride,
                                  int descending, void *stream) {
    using namespace szs_hip;
    if (!rows) return 0;
    u32 const width = (u32)szs_hip_top_k_width(k);
    u64 const blocks = ((u64)rows * k + top_k_threads_k - 1) / top_k_threads_k;
    if (blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    hipStream_t const s = static_cast<hipStream_t>(stream);
    if (descending)
        hipLaunchKernelGGL(top_k_emit_kernel<true>, dim3((u32)blocks), dim3(top_k_threads_k), 0, s, lists, rows, k, width, indices, scores, stride);
    else
        hipLaunchKernelGGL(top_k_emit_kernel<false>, dim3((u32)blocks), dim3(top_k_threads_k), 0, s, lists, rows, k, width, indices, scores, stride);
    return (int)hipGetLastError();
}

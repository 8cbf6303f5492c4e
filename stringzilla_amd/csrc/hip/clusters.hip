/*
 *  clusters.hip - the connected components of the graph "i ~ j iff the pair is a `within` hit", folded tile by tile out of a scored
 *  (strings x strings) tile into ONE forest of 32-bit parents, on the device (host/selection.c drives it for host/clusters.c and
 *  host/fingerprint_search.c).
 *
 *    clusters_begin_kernel   parent[i] = i: every string a root.
 *    clusters_union_kernel   hip/within.hip's count pass - one workgroup per (row, segment of the tile's columns), four cells in
 *                            flight per thread, the same compare - but a wavefront whose ballot is empty does nothing more, and a lane
 *                            with a hit and i != j runs unite(i, j).
 *    clusters_finish_kernel  labels[i] = find(i), read-only, and the number of roots: ballot and popcount per wavefront, one integer
 *                            add per workgroup - an integer sum does not depend on the order of its terms.
 *
 *  THE FOREST is lock-free with smaller-root hooking, and its INVARIANT is: every value ever stored to parent[x] is <= x, and a
 *  non-root never becomes a root again.  Both stores keep it - the halving store writes an index read BELOW parent[x] into a slot
 *  that was seen not to be a root, the compare-and-swap hooks a root under a SMALLER index and fails on anything but a root.  So
 *  every edge points strictly downward: no cycle can form, every find() walks strictly downward and ends within n steps, and every
 *  failed swap returns a parent strictly below `a`, the larger of unite()'s two indices, so that larger one falls with every turn and
 *  unite() ends within n turns - whatever other lanes, the lanes of the same wavefront included, do in between.  Nothing locks and nothing waits for
 *  another lane: a divergent wavefront cannot deadlock.  A halving store may put back an older, higher grandparent over a newer one;
 *  that index is still a node of the same tree - trees only ever merge - and still below x.  A root is hooked only under a smaller
 *  index, so the root of a finished component is its minimum: the labels depend on the hits alone, not on who arrived first.
 *
 *  MEMORY.  The forest is shared by every workgroup of every union launch of a call, and a CU's vector L1 is never refreshed by
 *  another CU's stores.  The invariant would keep a stale read correct - it is an older ancestor - but a lane fed from a stale line
 *  walks the long old paths for the rest of the launch.  So every load of `parent` in find() and unite() is a relaxed atomic load at
 *  agent scope, every halving store the matching atomic store, the swap relaxed at agent scope; it returns the parent as L2 holds
 *  it, and that value is used, not re-read.  No fence: nothing but `parent` itself is published, and the finish is a later launch on
 *  the same stream - it reads with plain loads.  Every address is 64-bit; a row, a column and a string are compared with `rows`,
 *  `columns` and `count` before they address anything.
 */
#include "device_common.hpp"

namespace szs_hip {

constexpr u32 clusters_threads_k = 256;
constexpr u32 clusters_waves_k = clusters_threads_k / wave_size_k;
constexpr u32 clusters_cells_per_thread_k = 4; /* loads in flight per thread before the first comparison (hip/within.hip's) */
constexpr u32 clusters_round_k = clusters_threads_k * clusters_cells_per_thread_k;

/** hip/within.hip's compare. */
template <bool descending> __device__ __forceinline__ bool clusters_hit(u64 cell, u64 bound) {
    return descending ? (i64)cell >= (i64)bound : cell <= bound;
}

__device__ __forceinline__ u32 parent_of(u32 *parent, u32 x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/** The root of x as the forest stands, with path halving: at most n steps, each strictly downward. */
__device__ __forceinline__ u32 clusters_find(u32 *parent, u32 x) {
    for (u32 p; (p = parent_of(parent, x)) != x; x = p) {
        u32 const g = parent_of(parent, p);
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return x;
}

/** Joins the trees of a and b: the larger root goes under the smaller.  A failed swap strictly lowers `a`. */
__device__ __forceinline__ void clusters_unite(u32 *parent, u32 a, u32 b) {
    for (;;) {
        a = clusters_find(parent, a), b = clusters_find(parent, b);
        if (a == b) return;
        if (a < b) {
            u32 const smaller = a;
            a = b, b = smaller;
        }
        u32 old = a;
        if (__hip_atomic_compare_exchange_strong(parent + a, &old, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        a = old; /* what L2 holds: a is no root any more, and its parent lies below it */
    }
}

__global__ __launch_bounds__(clusters_threads_k) void clusters_begin_kernel(u32 *__restrict__ parent, u32 count) {
    u64 const i = (u64)blockIdx.x * clusters_threads_k + threadIdx.x;
    if (i < count) parent[i] = (u32)i;
}

template <bool descending>
__global__ __launch_bounds__(clusters_threads_k) void clusters_union_kernel(u64 const *__restrict__ cells, u64 cells_stride, u32 rows,
                                                                            u32 columns, u32 first_row, u32 first_column, u64 bound,
                                                                            u32 segments, u32 segment_columns, u32 *parent) {
    u32 const row = blockIdx.x / segments, segment = blockIdx.x % segments;
    if (row >= rows) return;
    u64 const first = (u64)segment * segment_columns, last = first + segment_columns;
    u32 const begin = first < columns ? (u32)first : columns, end = last < columns ? (u32)last : columns;
    u64 const *const row_cells = cells + (u64)row * cells_stride;
    u32 const i = first_row + row;

    for (u32 base = begin; base < end; base += clusters_round_k) {
        u64 values[clusters_cells_per_thread_k];
#pragma unroll
        for (u32 s = 0; s < clusters_cells_per_thread_k; ++s) {
            u32 const column = base + s * clusters_threads_k + threadIdx.x;
            values[s] = column < end ? row_cells[column] : 0;
        }
#pragma unroll
        for (u32 s = 0; s < clusters_cells_per_thread_k; ++s) {
            u32 const column = base + s * clusters_threads_k + threadIdx.x;
            u32 const j = first_column + column;
            bool const hit = column < end && j != i && clusters_hit<descending>(values[s], bound);
            if (!__ballot(hit)) continue; /* the whole wavefront: with a useful bound almost every chunk ends here */
            if (hit) clusters_unite(parent, i, j);
        }
    }
}

__global__ __launch_bounds__(clusters_threads_k) void clusters_finish_kernel(u32 const *__restrict__ parent, u32 count,
                                                                             u64 *__restrict__ labels, unsigned long long *roots) {
    __shared__ u32 wave_roots[clusters_waves_k];
    u64 const i = (u64)blockIdx.x * clusters_threads_k + threadIdx.x;
    bool root = false;
    if (i < count) {
        u32 x = (u32)i;
        for (u32 p; (p = parent[x]) != x; x = p) {} /* strictly downward: at most `count` steps */
        labels[i] = x;
        root = x == (u32)i;
    }
    u32 const here = (u32)__popcll(__ballot(root));
    if ((threadIdx.x & 63u) == 0) wave_roots[threadIdx.x >> 6] = here;
    __syncthreads();
    if (threadIdx.x != 0) return;
    u32 total = 0;
#pragma unroll
    for (u32 w = 0; w < clusters_waves_k; ++w) total += wave_roots[w];
    if (total) atomicAdd(roots, (unsigned long long)total);
}

} // namespace szs_hip

extern "C" int szs_hip_clusters_begin(uint32_t *parent, uint32_t count, void *stream) {
    using namespace szs_hip;
    if (!count) return 0;
    if (!parent) return (int)hipErrorInvalidValue;
    u32 const blocks = (u32)(((u64)count + clusters_threads_k - 1) / clusters_threads_k);
    hipLaunchKernelGGL(clusters_begin_kernel, dim3(blocks), dim3(clusters_threads_k), 0, static_cast<hipStream_t>(stream), parent, count);
    return (int)hipGetLastError();
}

extern "C" int szs_hip_clusters_union(uint64_t const *cells, uint64_t cells_stride, uint32_t rows, uint32_t columns, uint64_t first_row,
                                      uint64_t first_column, uint64_t bound, int descending, uint32_t segments, uint32_t segment_columns,
                                      uint32_t *parent, uint32_t count, void *stream) {
    using namespace szs_hip;
    if (!rows || !columns) return 0;
    if (!cells || !parent || cells_stride < columns || segments < 1 || segment_columns < 1 || (uint64_t)rows * segments > 0x7FFFFFFFull ||
        (uint64_t)segments * segment_columns < columns || first_row + rows > count || first_column + columns > count)
        return (int)hipErrorInvalidValue; /* every row and column of the tile is a string of the forest */
    hipStream_t const s = static_cast<hipStream_t>(stream);
    dim3 const grid(rows * segments), threads(clusters_threads_k);
    if (descending)
        hipLaunchKernelGGL(clusters_union_kernel<true>, grid, threads, 0, s, cells, cells_stride, rows, columns, (u32)first_row,
                           (u32)first_column, bound, segments, segment_columns, parent);
    else
        hipLaunchKernelGGL(clusters_union_kernel<false>, grid, threads, 0, s, cells, cells_stride, rows, columns, (u32)first_row,
                           (u32)first_column, bound, segments, segment_columns, parent);
    return (int)hipGetLastError();
}

extern "C" int szs_hip_clusters_finish(uint32_t const *parent, uint32_t count, uint64_t *labels, uint64_t *clusters_count, void *stream) {
    using namespace szs_hip;
    if (!count) return 0;
    if (!parent || !labels || !clusters_count) return (int)hipErrorInvalidValue;
    u32 const blocks = (u32)(((u64)count + clusters_threads_k - 1) / clusters_threads_k);
    hipLaunchKernelGGL(clusters_finish_kernel, dim3(blocks), dim3(clusters_threads_k), 0, static_cast<hipStream_t>(stream), parent, count,
                       labels, reinterpret_cast<unsigned long long *>(clusters_count));
    return (int)hipGetLastError();
}

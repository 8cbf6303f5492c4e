/*
 *  fingerprint_matches.hip - equal dimensions of every (query, candidate) pair of MinHash fingerprints, on the device
 *  (host/fingerprint_search.c drives it):
 *
 *      M[q][c] = #{ d < D : A[q][d] == B[c][d] }      A: rows x D, B: columns x D hashes of 32 bits, row-major, strides in bytes
 *
 *  The comparison is plain equality: two 0xFFFFFFFF entries (a text shorter than the window) count as equal, as in the reference's
 *  own Jaccard snippet.  M / D estimates the Jaccard similarity of the two texts.
 *
 *  Shaped like a register-blocked SGEMM with "compare and count" in place of the multiply-add - there is no matrix-core route to an
 *  equality count, this is a VALU kernel:
 *    - a workgroup of 256 threads (16 x 16) owns a tile of (16 R) queries x 64 candidates, R = 8 or 4 rows per thread; thread
 *      (ty, tx) counts rows ty + 16 i (i < R) against columns tx + 16 j (j < 4) in R x 4 registers;
 *    - D is walked in slabs of 32 hashes staged through LDS as [row][36 dwords]: 128 bytes of a fingerprint, 16 of padding.  A slab
 *      row is filled by eight lanes with one 16-byte load and one ds_write_b128 each; the inner loop reads it back 16 bytes at a
 *      time.  With a row stride of 36 dwords the sixteen rows tx = 0 ... 15 of a ds_read_b128 lane group start at the sixteen
 *      distinct multiples of 4 banks (36 tx mod 64), and the rows of two neighbouring ty 36 banks apart: no conflicts, and the
 *      lanes that share a row are served by one broadcast.  A ds_write_b128 group of eight consecutive lanes fills one slab row,
 *      32 consecutive dwords over the 32 banks of a store: no conflicts either;
 *    - per 4 hashes of depth a thread reads R + 4 times 16 bytes and does 16 R compares (hipcc keeps every read a ds_read_b128 in
 *      <u64, 8> and splits about a third of them into narrower reads in the other instances: DESIGN.md section 4.7).  The four
 *      compares of one count become four v_cmp_eq_u32 (lane masks), two v_cndmask_b32 (a mask as 0 / 1) and two v_addc_co_u32
 *      (count + that + another mask as the carry): two lane-operations per compare, the VALU issue ceiling of this kernel;
 *    - the tail of D is padded with 0 on the query side and 1 on the candidate side - never equal - and rows beyond the edges
 *      of the matrix are staged as zeros and never written.
 *  The output cell is a template parameter: u32 cells with a byte stride (the matrix call), u64 cells with a cell stride (the
 *  scratch tile that szs_hip_top_k_scan folds, descending).
 */
#include "device_common.hpp"

namespace szs_hip {

constexpr u32 matches_threads_k = 256;
constexpr u32 matches_columns_k = 64;     /* candidates of a tile: 16 threads x 4 */
constexpr u32 matches_slab_k = 32;        /* hashes of depth per LDS slab */
constexpr u32 matches_row_dwords_k = 36;  /* slab row + 4 dwords of padding: see the bank arithmetic above */

/** Stages `tile_rows` slab rows of `source` (rows `first_row` ..., dimensions `depth` ... depth + 32) into `lds`. */
template <u32 tile_rows>
__device__ __forceinline__ void stage_slab(u32 *lds, u32 const *source, u64 stride_bytes, u32 first_row, u32 rows, u32 depth,
                                           u32 dimensions, bool vector_loads, u32 padding) {
    constexpr u32 pieces = tile_rows * (matches_slab_k / 4);
#pragma unroll
    for (u32 piece = threadIdx.x; piece < pieces; piece += matches_threads_k) {
        u32 const local_row = piece / (matches_slab_k / 4), d = depth + (piece % (matches_slab_k / 4)) * 4;
        u32 const row = first_row + local_row;
        uint4 value = make_uint4(padding, padding, padding, padding);
        if (row < rows && d < dimensions) {
            u32 const *const from = reinterpret_cast<u32 const *>(reinterpret_cast<char const *>(source) + (u64)row * stride_bytes) + d;
            if (vector_loads && d + 4 <= dimensions)
                value = *reinterpret_cast<uint4 const *>(from);
            else {
                value.x = from[0];
                if (d + 1 < dimensions) value.y = from[1];
                if (d + 2 < dimensions) value.z = from[2];
                if (d + 3 < dimensions) value.w = from[3];
            }
        }
        *reinterpret_cast<uint4 *>(lds + local_row * matches_row_dwords_k + (piece % (matches_slab_k / 4)) * 4) = value;
    }
}

template <typename cell_t, u32 rows_per_thread>
__global__ __launch_bounds__(matches_threads_k, 3) void fingerprint_matches_kernel(u32 const *__restrict__ queries, u64 queries_stride,
                                                                                 u32 rows, u32 const *__restrict__ candidates,
                                                                                 u64 candidates_stride, u32 columns, u32 dimensions,
                                                                                 cell_t *__restrict__ cells, u64 cells_stride_bytes,
                                                                                 u32 vector_loads) {
    constexpr u32 tile_rows = 16 * rows_per_thread;
    __shared__ __align__(16) u32 query_slab[tile_rows * matches_row_dwords_k];
    __shared__ __align__(16) u32 candidate_slab[matches_columns_k * matches_row_dwords_k];

    u32 const tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    u32 const first_row = blockIdx.y * tile_rows, first_column = blockIdx.x * matches_columns_k;
    u32 counts[rows_per_thread][4];
#pragma unroll
    for (u32 i = 0; i < rows_per_thread; ++i)
#pragma unroll
        for (u32 j = 0; j < 4; ++j) counts[i][j] = 0;

    for (u32 depth = 0; depth < dimensions; depth += matches_slab_k) {
        if (depth) __syncthreads(); /* the previous slab has been read by everyone */
        stage_slab<tile_rows>(query_slab, queries, queries_stride, first_row, rows, depth, dimensions, vector_loads != 0, 0u);
        stage_slab<matches_columns_k>(candidate_slab, candidates, candidates_stride, first_column, columns, depth, dimensions,
                                      vector_loads != 0, 1u);
        __syncthreads();
#pragma unroll
        for (u32 d = 0; d < matches_slab_k; d += 4) {
            uint4 b[4];
#pragma unroll
            for (u32 j = 0; j < 4; ++j) b[j] = *reinterpret_cast<uint4 const *>(candidate_slab + (tx + 16 * j) * matches_row_dwords_k + d);
#pragma unroll
            for (u32 i = 0; i < rows_per_thread; ++i) {
                uint4 const a = *reinterpret_cast<uint4 const *>(query_slab + (ty + 16 * i) * matches_row_dwords_k + d);
#pragma unroll
                for (u32 j = 0; j < 4; ++j) {
                    counts[i][j] += a.x == b[j].x;
                    counts[i][j] += a.y == b[j].y;
                    counts[i][j] += a.z == b[j].z;
                    counts[i][j] += a.w == b[j].w;
                }
            }
        }
    }

#pragma unroll
    for (u32 i = 0; i < rows_per_thread; ++i) {
        u32 const row = first_row + ty + 16 * i;
        if (row >= rows) continue;
        cell_t *const out = reinterpret_cast<cell_t *>(reinterpret_cast<char *>(cells) + (u64)row * cells_stride_bytes);
#pragma unroll
        for (u32 j = 0; j < 4; ++j) {
            u32 const column = first_column + tx + 16 * j;
            if (column < columns) out[column] = (cell_t)counts[i][j];
        }
    }
}

template <typename cell_t>
static int launch_matches(u32 const *queries, u64 queries_stride, u32 rows, u32 const *candidates, u64 candidates_stride, u32 columns,
                          u32 dimensions, cell_t *cells, u64 cells_stride_bytes, void *stream) {
    if (!rows || !columns) return 0;
    if (!dimensions || queries_stride % 4 || candidates_stride % 4 || queries_stride < (u64)dimensions * 4 ||
        candidates_stride < (u64)dimensions * 4 || cells_stride_bytes % sizeof(cell_t) || cells_stride_bytes < (u64)columns * sizeof(cell_t))
        return (int)hipErrorInvalidValue;
    u32 const column_tiles = (columns + matches_columns_k - 1) / matches_columns_k;
    /* tall tiles (128 queries: half the LDS reads per compare) once they still give every CU two workgroups; else 64 */
    bool const tall = (u64)((rows + 127) / 128) * column_tiles >= 512;
    u32 const row_tiles = tall ? (rows + 127) / 128 : (rows + 63) / 64;
    if (row_tiles > 65535u) return (int)hipErrorInvalidValue;
    /* 16-byte loads need every row to start on a 16-byte boundary; anything else is read dword by dword */
    u32 const vector_loads = ((u64)(uintptr_t)queries | (u64)(uintptr_t)candidates | queries_stride | candidates_stride) % 16 == 0;
    hipStream_t const s = static_cast<hipStream_t>(stream);
    dim3 const grid(column_tiles, row_tiles);
    if (tall)
        hipLaunchKernelGGL((fingerprint_matches_kernel<cell_t, 8>), grid, dim3(matches_threads_k), 0, s, queries, queries_stride, rows,
                           candidates, candidates_stride, columns, dimensions, cells, cells_stride_bytes, vector_loads);
    else
        hipLaunchKernelGGL((fingerprint_matches_kernel<cell_t, 4>), grid, dim3(matches_threads_k), 0, s, queries, queries_stride, rows,
                           candidates, candidates_stride, columns, dimensions, cells, cells_stride_bytes, vector_loads);
    return (int)hipGetLastError();
}

} // namespace szs_hip

extern "C" int szs_hip_fingerprint_matches_u32(uint32_t const *queries, uint64_t queries_stride, uint32_t rows, uint32_t const *candidates,
                                               uint64_t candidates_stride, uint32_t columns, uint32_t dimensions, uint32_t *cells,
                                               uint64_t cells_stride_bytes, void *stream) {
    return szs_hip::launch_matches<uint32_t>(queries, queries_stride, rows, candidates, candidates_stride, columns, dimensions, cells,
                                             cells_stride_bytes, stream);
}

extern "C" int szs_hip_fingerprint_matches_u64(uint32_t const *queries, uint64_t queries_stride, uint32_t rows, uint32_t const *candidates,
                                               uint64_t candidates_stride, uint32_t columns, uint32_t dimensions, uint64_t *cells,
                                               uint64_t cells_stride, void *stream) {
    if (cells_stride > ~(uint64_t)0 / sizeof(uint64_t)) return (int)hipErrorInvalidValue;
    return szs_hip::launch_matches<uint64_t>(queries, queries_stride, rows, candidates, candidates_stride, columns, dimensions, cells,
                                             cells_stride * sizeof(uint64_t), stream);
}

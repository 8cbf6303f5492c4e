/*
 *  myers_fuzzy_matches.hip - EVERY end within a distance bound of every query inside ONE long text (szs_rocm_fuzzy_scan_matches*,
 *  host/fuzzy_scan_matches.c): a hit is a column j in [1, n] with D[m][j] <= bound, D the unit-cost DP with
 *  a free start in the text; per query the number of hits in the whole text and the leftmost `limit` of them as (end, distance).
 *  The distance, its table and a lane's walk are hip/fuzzy_core.hpp's and hip/rerank_core.hpp's; the cut of the text and the schedule
 *  are hip/myers_fuzzy_scan.hip's; a lane's piece, the count pass, the write pass, the counters and the launch are
 *  hip/fuzzy_pieces.hpp's, shared with hip/myers_fuzzy_occurrences.hip - its head has why an owned column is exact and how the two
 *  passes fill a fixed capacity.  This file's own:
 *
 *  - THE RULE (hits_rule_t): an owned column within the bound, decided where it is computed - no state between columns, no column
 *    beyond the piece, nothing behind the walk.  No column is reported that is not a hit (a lane's values are >= D[m][j]), and every
 *    hit is seen with its exact distance by the one piece that owns it.
 *  - OFFSETS (levenshtein_fuzzy_matches_offsets_kernel, between the passes of this call and of fuzzy scan occurrences'): one
 *    workgroup per row turns chunk_counts[row][*] into exclusive prefix sums in place, tile by tile with a carry, and stores
 *    counts[row] - the total, <= n < 2^32 - as 8 bytes.
 *  - The two kernels and their names: each declares the table and runs the pass of hip/fuzzy_pieces.hpp under the rule.
 */
#include "fuzzy_pieces.hpp"

namespace szs_hip {

struct hits_rule_t {
    using piece_t = matches_piece_t;

    static __device__ __forceinline__ piece_t piece(u32 query_length, u32 text_length, u64 piece, u32 pieces, u32 chunk) {
        return matches_piece(query_length, text_length, piece, pieces, chunk);
    }

    __device__ __forceinline__ explicit hits_rule_t(u32) {}

    template <typename on_found_t>
    __device__ __forceinline__ auto column(u32 const &warm, u32 const &bound, on_found_t const &on_found) {
        return [&](u32 column_end, u32 score) {
            if (column_end > warm && score <= bound) on_found(column_end, score);
        };
    }

    template <typename on_found_t>
    __device__ __forceinline__ void behind(piece_t const &, bool, u32, u32, u32, on_found_t const &) {}
};

__global__ __launch_bounds__(64) void levenshtein_fuzzy_matches_count_kernel(szs_rerank_side_t const queries, u64 const first_query,
                                                                             u32 const rows, u64 const text, u32 const text_length,
                                                                             u64 const piece, u32 const pieces, u32 const chunks,
                                                                             u32 const bound, u32 *__restrict__ piece_counts,
                                                                             u32 *__restrict__ chunk_counts, u32 *flags,
                                                                             unsigned long long *counters) {
    __shared__ __attribute__((aligned(16))) u32 fuzzy_matches_table[peq_layout<SZS_MYERS_SHORT_WORDS, byte_rows_k>::total_dwords];
    pieces_count_pass<hits_rule_t>(fuzzy_matches_table, queries, first_query, rows, text, text_length, piece, pieces, chunks, bound,
                                   piece_counts, chunk_counts, flags, counters);
}

__global__ __launch_bounds__(256) void levenshtein_fuzzy_matches_offsets_kernel(u32 const chunks, u32 *__restrict__ chunk_counts,
                                                                                u64 *__restrict__ counts) {
    constexpr u32 waves = 256 / wave_size_k;
    __shared__ u32 wave_totals[waves];
    u32 *const cells = chunk_counts + (u64)blockIdx.x * chunks; // the row's: one workgroup a row
    u32 const wave = threadIdx.x / wave_size_k, lane = threadIdx.x % wave_size_k;
    u32 carry = 0; // the hits of the tiles before: the same in every thread
    for (u32 tile = 0; tile < chunks; tile += 256) {
        u32 const at = tile + threadIdx.x;
        u32 const own = at < chunks ? cells[at] : 0u;
        u32 const upto = wave_prefix_u32(own);
        if (lane == wave_size_k - 1) wave_totals[wave] = upto;
        __syncthreads();
        u32 before = 0, total = 0;
#pragma unroll
        for (u32 w = 0; w < waves; ++w) before += w < wave ? wave_totals[w] : 0u, total += wave_totals[w];
        if (at < chunks) cells[at] = carry + before + upto - own; // exclusive: the hits of the row's chunks before this one
        carry += total;
        __syncthreads(); // the totals are read before the next tile overwrites them
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

__global__ __launch_bounds__(64) void levenshtein_fuzzy_matches_write_kernel(szs_rerank_side_t const queries, u64 const first_query,
                                                                             u32 const rows, u64 const text, u32 const text_length,
                                                                             u64 const piece, u32 const pieces, u32 const chunks,
                                                                             u32 const bound, u32 const limit,
                                                                             u32 const *__restrict__ piece_counts,
                                                                             u32 const *__restrict__ chunk_counts, u64 *__restrict__ distances,
                                                                             u64 *__restrict__ ends, u32 *flags, unsigned long long *counters) {
    __shared__ __attribute__((aligned(16))) u32 fuzzy_matches_table[peq_layout<SZS_MYERS_SHORT_WORDS, byte_rows_k>::total_dwords];
    pieces_write_pass<hits_rule_t>(fuzzy_matches_table, queries, first_query, rows, text, text_length, piece, pieces, chunks, bound, limit,
                                   piece_counts, chunk_counts, distances, ends, flags, counters);
}

} // namespace szs_hip

extern "C" int szs_hip_levenshtein_fuzzy_matches_count(szs_rerank_side_t const *queries, uint64_t first_query, uint32_t rows,
                                                       void const *text, uint64_t text_length, uint64_t piece, uint32_t bound,
                                                       uint32_t *piece_counts, uint32_t *chunk_counts, uint32_t *flags,
                                                       unsigned long long *counters, void *stream) {
    return szs_hip::matches_launch(szs_hip::levenshtein_fuzzy_matches_count_kernel, piece_counts && chunk_counts && flags && counters, queries,
                                   first_query, rows, text, text_length, piece, stream, bound, piece_counts, chunk_counts, flags, counters);
}

extern "C" int szs_hip_levenshtein_fuzzy_matches_offsets(uint32_t rows, uint64_t chunks, uint32_t *chunk_counts, uint64_t *counts,
                                                         void *stream) {
    using namespace szs_hip;
    if (!rows || !chunks || !chunk_counts || !counts || (u64)rows * chunks > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(levenshtein_fuzzy_matches_offsets_kernel, dim3(rows), dim3(256), 0, static_cast<hipStream_t>(stream), (u32)chunks,
                       chunk_counts, counts);
    return (int)hipGetLastError();
}

extern "C" int szs_hip_levenshtein_fuzzy_matches_write(szs_rerank_side_t const *queries, uint64_t first_query, uint32_t rows,
                                                       void const *text, uint64_t text_length, uint64_t piece, uint32_t bound,
                                                       uint32_t limit, uint32_t const *piece_counts, uint32_t const *chunk_counts,
                                                       uint64_t *distances, uint64_t *ends, uint32_t *flags, unsigned long long *counters,
                                                       void *stream) {
    return szs_hip::matches_launch(szs_hip::levenshtein_fuzzy_matches_write_kernel,
                                   piece_counts && chunk_counts && distances && ends && limit && flags && counters, queries, first_query, rows,
                                   text, text_length, piece, stream, bound, limit, piece_counts, chunk_counts, distances, ends, flags, counters);
}

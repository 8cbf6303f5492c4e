/*
 *  myers_fuzzy_matches.hip - EVERY end within a distance bound of every query inside ONE long text (szs_rocm_fuzzy_scan_matches*,
 *  host/fuzzy_scan_matches.c): a hit is a column j in [1, n] with D[m][j] <= bound, D the unit-cost DP with
 *  a free start in the text; per query the number of hits in the whole text and the leftmost `limit` of them as (end, distance).
 *  The distance, its table and a lane's walk are hip/fuzzy_core.hpp's and hip/rerank_core.hpp's, unchanged; the cut of the text and
 *  the schedule are hip/myers_fuzzy_scan.hip's; a lane's piece, the counters and the grid are hip/fuzzy_pieces.hpp's, shared with
 *  hip/myers_fuzzy_occurrences.hip.  This file's own is the output: a fixed capacity, filled in two passes.
 *
 *  - Piece p owns columns (p P, min(n, (p + 1) P)].  The lane that takes it walks from s = p P - warm, warm = min(p P, 2 m): its DP
 *    has a free start at s instead of at 0, so every value L[j] it sees is >= D[m][j] (fewer starts to choose from) - no column is
 *    reported that is not a hit.  For an OWNED column j - s > 2 m or s = 0, and the start that attains D[m][j] lies within
 *    m + D[m][j] <= 2 m bytes of j (section 4.9's span bound): L[j] = D[m][j], every hit is seen with its exact distance by the one
 *    piece that owns it.  A lane counts and reports owned columns only (column_end > warm): its warm-up belongs to the piece before.
 *    (A warm-up of m is NOT enough here, though it is for the minimum of section 4.11: tests/test_fuzzy_scan_matches_model.py.)
 *  - A one-wavefront workgroup serves ONE row and a CHUNK of 64 consecutive pieces, lane l piece 64 chunk + l; the grid is
 *    rows x chunks, numbered chunk-major (row = id % rows); the table is static LDS of the widest layout (8 KB).
 *  - COUNT (levenshtein_fuzzy_matches_count_kernel): every lane stores the hits of its piece as a u32 in piece_counts[row][p] - a
 *    piece's hits are <= P < 2^32 - and lane 0 the wavefront's sum in chunk_counts[row][chunk].  Lanes beyond the pieces and rows
 *    with no query store 0 and load nothing.  Every cell has one writer: no atomics, nothing to clear.
 *  - OFFSETS (levenshtein_fuzzy_matches_offsets_kernel): one workgroup per row turns chunk_counts[row][*] into exclusive prefix sums
 *    in place, tile by tile with a carry, and stores counts[row] - the total, <= n < 2^32 - as 8 bytes.
 *  - WRITE (levenshtein_fuzzy_matches_write_kernel; not launched when limit = 0): a workgroup whose chunk starts at an offset
 *    >= limit, or holds no hit, returns before it builds a table.  Otherwise the exclusive prefix of its 64 piece counts (one
 *    coalesced load, a shuffle scan) gives every lane the slot of its first hit; lanes without a hit or past the limit are not live.
 *    A live lane repeats the walk of the count pass - the same bytes, the same arithmetic, so the same hits - and stores
 *    (s + column_end, score) into slots offset, offset + 1, ... while they are below `limit`; the walk ends once every live lane has
 *    written what it owes.  The host fills both matrices with 0xFF bytes ahead of the launch: no kernel writes an empty slot.
 *  - Every slot and every count has one writer and a value that does not depend on the order of anything: the same bytes every run.
 *  - Counters: cells and bytes as walked in both passes; one pair per row with a non-empty query, by chunk 0 of the count pass alone.
 */
#include "fuzzy_pieces.hpp"

namespace szs_hip {

/** One lane's walk of its piece against the row's table: `on_hit(column_end, score)` at every OWNED column whose bottom-row score is
 *  within `bound`; `keep_going()` as listed_walk asks it.  Returns the columns the lane took. */
template <int words_, typename on_hit_t, typename keep_going_t>
__device__ __forceinline__ u32 matches_walk(u32 const *table, u32 query_length, u64 text, matches_piece_t const &lane, bool live, u32 bound,
                                            on_hit_t on_hit, keep_going_t keep_going) {
    u32 const pad = 32u * words_ - query_length;
    u32 vp[words_], vn[words_];
#pragma unroll
    for (int w = 0; w < words_; ++w) vp[w] = rerank_bits_in_word(pad, 32u * words_, w), vn[w] = 0;
    u32 score = query_length, taken = 0;
    // (a lane that is not live still takes the zeros of listed_walk's unpredicated loop: it owns no column)
    u32 const length = live ? lane.walked : 0u, warm = live ? lane.warm : ~0u;
    listed_walk(
        text_stream_t(text + lane.first, length), length, live,
        [&](u32 symbol, u32 column_end) {
            u32 eq[words_];
            load_match_masks<words_, byte_rows_k>(table, symbol, eq);
            u32 const top = myers_infix_column<words_>(vp, vn, eq);
            score += (top & 1u) - (top >> 1);
            taken = column_end;
            if (column_end > warm && score <= bound) on_hit(column_end, score);
        },
        keep_going);
    return taken;
}

template <int words_>
__device__ __forceinline__ void matches_count_row(u32 *table, listed_row_t const &row, u64 text, u32 text_length, u64 piece, u32 pieces,
                                                  u32 chunk, u32 bound, u32 *__restrict__ piece_count, u32 *__restrict__ chunk_count,
                                                  unsigned long long *counters) {
    fuzzy_table<words_, (int)wave_size_k>(table, row);
    matches_piece_t const lane = matches_piece(row.query_length, text_length, piece, pieces, chunk);
    u32 hits = 0;
    u32 const taken = matches_walk<words_>(
        table, row.query_length, text, lane, lane.inside, bound, [&](u32, u32) { ++hits; }, []() { return true; });
    piece_count[threadIdx.x] = hits;
    u32 const all = (u32)wave_sum_u64(hits); // <= the columns of 64 pieces, below 2^32
    if (threadIdx.x == 0) *chunk_count = all;
    matches_counted(row, lane.inside, taken, chunk == 0, counters);
}

__global__ __launch_bounds__(64) void levenshtein_fuzzy_matches_count_kernel(szs_rerank_side_t const queries, u64 const first_query,
                                                                             u32 const rows, u64 const text, u32 const text_length,
                                                                             u64 const piece, u32 const pieces, u32 const chunks,
                                                                             u32 const bound, u32 *__restrict__ piece_counts,
                                                                             u32 *__restrict__ chunk_counts, u32 *flags,
                                                                             unsigned long long *counters) {
    __shared__ __attribute__((aligned(16))) u32 fuzzy_matches_table[peq_layout<SZS_MYERS_SHORT_WORDS, byte_rows_k>::total_dwords];
    u32 const r = blockIdx.x % rows, chunk = blockIdx.x / rows; // chunk below `chunks`: the host's grid
    listed_row_t const row = listed_row(queries, first_query, true, [&]() { return r; }, SZS_RERANK_LONGEST_QUERY, flags);
    u32 const length = (u32)__builtin_amdgcn_readfirstlane((int)row.query_length); // one row a wavefront: a scalar
    u64 const cell = (u64)r * chunks + chunk; // below rows x chunks: what the host reserved, 64 piece counts a chunk
    u32 *const piece_count = piece_counts + cell * wave_size_k, *const chunk_count = chunk_counts + cell;
    if (!length) { // no query, or a flag is up and the call fails: no hits, nothing loaded
        piece_count[threadIdx.x] = 0;
        if (threadIdx.x == 0) *chunk_count = 0;
        return;
    }
    listed_at_width(SZS_RERANK_WORDS_OF(length), [&](auto width) {
        matches_count_row<decltype(width)::value>(fuzzy_matches_table, row, text, text_length, piece, pieces, chunk, bound, piece_count,
                                                  chunk_count, counters);
    });
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

template <int words_>
__device__ __forceinline__ void matches_write_row(u32 *table, listed_row_t const &row, u64 text, u32 text_length, u64 piece, u32 pieces,
                                                  u32 chunk, u32 bound, u32 limit, u32 offset, u32 hits, u64 *__restrict__ distances,
                                                  u64 *__restrict__ ends, unsigned long long *counters) {
    fuzzy_table<words_, (int)wave_size_k>(table, row);
    matches_piece_t const lane = matches_piece(row.query_length, text_length, piece, pieces, chunk);
    bool const live = lane.inside && hits && offset < limit;
    u32 owed = live ? (hits < limit - offset ? hits : limit - offset) : 0u; // offset + owed <= limit
    u64 slot = row.row * limit + offset;                                      // below rows x limit while owed > 0
    u32 const taken = matches_walk<words_>(
        table, row.query_length, text, lane, live, bound,
        [&](u32 column_end, u32 score) {
            if (!owed) return;
            ends[slot] = (u64)lane.first + column_end, distances[slot] = score;
            ++slot, --owed;
        },
        [&]() { return __ballot(owed != 0) != 0; });
    matches_counted(row, live, taken, false, counters);
}

__global__ __launch_bounds__(64) void levenshtein_fuzzy_matches_write_kernel(szs_rerank_side_t const queries, u64 const first_query,
                                                                             u32 const rows, u64 const text, u32 const text_length,
                                                                             u64 const piece, u32 const pieces, u32 const chunks,
                                                                             u32 const bound, u32 const limit,
                                                                             u32 const *__restrict__ piece_counts,
                                                                             u32 const *__restrict__ chunk_counts, u64 *__restrict__ distances,
                                                                             u64 *__restrict__ ends, u32 *flags, unsigned long long *counters) {
    __shared__ __attribute__((aligned(16))) u32 fuzzy_matches_table[peq_layout<SZS_MYERS_SHORT_WORDS, byte_rows_k>::total_dwords];
    u32 const r = blockIdx.x % rows, chunk = blockIdx.x / rows;
    u64 const cell = (u64)r * chunks + chunk;
    u32 const before = chunk_counts[cell]; // the hits of the row's chunks before this one
    if (before >= limit) return;           // every slot is taken by then
    u32 const hits = piece_counts[cell * wave_size_k + threadIdx.x];
    u32 const upto = wave_prefix_u32(hits);
    if (!__shfl((int)upto, (int)wave_size_k - 1, 64)) return; // a chunk without a hit
    listed_row_t const row = listed_row(queries, first_query, true, [&]() { return r; }, SZS_RERANK_LONGEST_QUERY, flags);
    u32 const length = (u32)__builtin_amdgcn_readfirstlane((int)row.query_length);
    if (!length) return; // (a row without a query counted nothing)
    listed_at_width(SZS_RERANK_WORDS_OF(length), [&](auto width) {
        matches_write_row<decltype(width)::value>(fuzzy_matches_table, row, text, text_length, piece, pieces, chunk, bound, limit,
                                                  before + upto - hits, hits, distances, ends, counters);
    });
}

} // namespace szs_hip

extern "C" int szs_hip_levenshtein_fuzzy_matches_count(szs_rerank_side_t const *queries, uint64_t first_query, uint32_t rows,
                                                       void const *text, uint64_t text_length, uint64_t piece, uint32_t bound,
                                                       uint32_t *piece_counts, uint32_t *chunk_counts, uint32_t *flags,
                                                       unsigned long long *counters, void *stream) {
    using namespace szs_hip;
    u64 pieces, chunks;
    if (!piece_counts || !chunk_counts || !flags || !counters || !matches_grid(queries, first_query, rows, text, text_length, piece, pieces, chunks))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(levenshtein_fuzzy_matches_count_kernel, dim3((u32)(rows * chunks)), dim3(wave_size_k), 0,
                       static_cast<hipStream_t>(stream), *queries, first_query, rows, (u64) reinterpret_cast<uintptr_t>(text), (u32)text_length,
                       piece, (u32)pieces, (u32)chunks, bound, piece_counts, chunk_counts, flags, counters);
    return (int)hipGetLastError();
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
    using namespace szs_hip;
    u64 pieces, chunks;
    if (!piece_counts || !chunk_counts || !distances || !ends || !limit || !flags || !counters ||
        !matches_grid(queries, first_query, rows, text, text_length, piece, pieces, chunks))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(levenshtein_fuzzy_matches_write_kernel, dim3((u32)(rows * chunks)), dim3(wave_size_k), 0,
                       static_cast<hipStream_t>(stream), *queries, first_query, rows, (u64) reinterpret_cast<uintptr_t>(text), (u32)text_length,
                       piece, (u32)pieces, (u32)chunks, bound, limit, piece_counts, chunk_counts, distances, ends, flags, counters);
    return (int)hipGetLastError();
}

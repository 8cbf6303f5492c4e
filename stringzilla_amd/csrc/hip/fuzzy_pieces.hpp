/*
 *  fuzzy_pieces.hpp - the two passes over the PIECES of one long text that fill a fixed capacity a query (hip/myers_fuzzy_matches.hip:
 *  every end within a bound; hip/myers_fuzzy_occurrences.hip: one end per occurrence), written once over a RULE, and what they are made
 *  of: the prefix sums of a wavefront, the piece a lane takes (hip/myers_fuzzy_scan.hip takes the same), the counters and the grid of
 *  a walking pass.  DESIGN.md section 4.12 has the argument for the warm-up.
 *
 *  - Piece p owns columns (p P, min(n, (p + 1) P)].  The lane that takes it walks from s = p P - warm, warm = min(p P, 2 m): its DP
 *    has a free start at s instead of at 0, so every value L[j] it sees is >= D[m][j] (fewer starts to choose from).  For an OWNED
 *    column j - s > 2 m or s = 0, and the start that attains D[m][j] lies within m + D[m][j] <= 2 m bytes of j (section 4.9's span
 *    bound): L[j] = D[m][j], every owned column is seen with its exact value by the one piece that owns it.  A lane reports owned
 *    columns only (column_end > warm): its warm-up belongs to the piece before.  (A warm-up of m is NOT enough here, though it is for
 *    the minimum of section 4.11: tests/test_fuzzy_scan_matches_model.py.)
 *  - A one-wavefront workgroup serves ONE row and a CHUNK of 64 consecutive pieces, lane l piece 64 chunk + l; the grid is
 *    rows x chunks, numbered chunk-major (row = id % rows); the table is the kernel's static LDS of the widest layout (8 KB).
 *  - THE RULE says what a lane reports - "finds" - of the columns it walks.  It is a small struct: `piece_t` and `piece(...)`, the
 *    lane's piece with whatever the rule walks beyond it; the state a lane keeps between columns, its members; `column(warm, bound,
 *    on_found)`, which hands back what is decided at a column as a callable of (column_end, score) that reaches the walk's `warm` and
 *    `bound` and the rule's state by reference - the decision then stands in the walk's own lambda, as if written there; and
 *    `behind(...)`, what is decided once the walk has ended.  Everything is inlined: a rule without state or tail costs nothing.
 *  - COUNT (pieces_count_pass): every lane stores what it found in its piece as a u32 in piece_counts[row][p] - at most P < 2^32 -
 *    and lane 0 the wavefront's sum in chunk_counts[row][chunk].  Lanes beyond the pieces and rows with no query store 0 and load
 *    nothing.  Every cell has one writer: no atomics, nothing to clear.  (Between the passes levenshtein_fuzzy_matches_offsets_kernel
 *    turns chunk_counts[row][*] into exclusive prefix sums.)
 *  - WRITE (pieces_write_pass; not launched when limit = 0): a workgroup whose chunk starts at an offset >= limit, or found nothing,
 *    returns before it builds a table.  Otherwise the exclusive prefix of its 64 piece counts (one coalesced load, a shuffle scan)
 *    gives every lane the slot of its first find; lanes without one or past the limit are not live.  A live lane repeats the walk of
 *    the count pass - the same bytes, the same arithmetic, so the same finds - and stores (s + column_end, score) into slots offset,
 *    offset + 1, ... while they are below `limit`; the walk ends once every live lane has written what it owes.  The host fills both
 *    matrices with 0xFF bytes ahead of the launch: no kernel writes an empty slot.
 *  - Every slot and every count has one writer and a value that does not depend on the order of anything: the same bytes every run.
 *  - Counters: cells and bytes as walked in both passes; one pair per row with a non-empty query, by chunk 0 of the count pass alone.
 */
#pragma once
#include "fuzzy_core.hpp"

namespace szs_hip {

/** Inclusive prefix sums over the 64 lanes of a wavefront. */
__device__ __forceinline__ u32 wave_prefix_u32(u32 value) {
    u32 const lane = threadIdx.x % wave_size_k;
#pragma unroll
    for (u32 offset = 1; offset < wave_size_k; offset <<= 1) {
        u32 const other = (u32)__shfl_up((int)value, offset, 64);
        if (lane >= offset) value += other;
    }
    return value;
}

/** What lane l of `chunk` walks: piece p = 64 chunk + l from `first` = p P - warm over `walked` = warm + own bytes. */
struct matches_piece_t {
    bool inside; // p < pieces
    u32 warm, first, walked;
};

__device__ __forceinline__ matches_piece_t matches_piece(u32 query_length, u32 text_length, u64 piece, u32 pieces, u32 chunk) {
    u64 const p = (u64)chunk * wave_size_k + threadIdx.x;
    matches_piece_t lane;
    lane.inside = p < pieces;
    u64 const from = lane.inside ? p * piece : 0; // below text_length: pieces = ceil(text_length / piece)
    lane.warm = from < 2u * query_length ? (u32)from : 2u * query_length;
    u32 const own = lane.inside ? (u32)(text_length - from < piece ? text_length - from : piece) : 0u;
    lane.first = (u32)from - lane.warm, lane.walked = lane.inside ? own + lane.warm : 0u; // first + walked <= text_length
    return lane;
}

/** The counters of a walk: cells and bytes as walked; the query read once a workgroup; the pair by chunk 0 of the count pass. */
__device__ __forceinline__ void matches_counted(listed_row_t const &row, bool live, u32 taken, bool with_pairs, unsigned long long *counters) {
    listed_counters_t counted;
    if (live) counted.cells = (u64)row.query_length * taken, counted.bytes = taken;
    if (threadIdx.x == 0) counted.bytes += row.query_length, counted.pairs = with_pairs;
    counted.land(counters, with_pairs);
}

/** One lane's walk of its piece under `rule_t`: `on_found(column_end, score)` at every column the rule reports; `keep_going()` as
 *  listed_walk asks it.  Returns the columns the lane took. */
template <int words_, typename rule_t, typename on_found_t, typename keep_going_t>
__device__ __forceinline__ u32 pieces_walk(u32 const *table, u32 query_length, u64 text, typename rule_t::piece_t const &lane, bool live,
                                           u32 bound, on_found_t const &on_found, keep_going_t keep_going) {
    // (a lane that is not live still takes the zeros of listed_walk's unpredicated loop: it owns no column)
    u32 const length = live ? lane.walked : 0u, warm = live ? lane.warm : ~0u;
    rule_t rule(query_length);
    u32 taken = 0;
    auto at_column = rule.column(warm, bound, on_found);
    fuzzy_infix_walk<words_>(
        table, query_length, text + lane.first, length, live, [&](u32 column_end, u32 score) { taken = column_end, at_column(column_end, score); },
        keep_going);
    rule.behind(lane, live && taken == length, taken, warm, bound, on_found); // (a walk that was left early owes nothing any more)
    return taken;
}

template <int words_, typename rule_t>
__device__ __forceinline__ void pieces_count_row(u32 *table, listed_row_t const &row, u64 text, u32 text_length, u64 piece, u32 pieces,
                                                 u32 chunk, u32 bound, u32 *__restrict__ piece_count, u32 *__restrict__ chunk_count,
                                                 unsigned long long *counters) {
    fuzzy_table<words_, (int)wave_size_k>(table, row);
    typename rule_t::piece_t const lane = rule_t::piece(row.query_length, text_length, piece, pieces, chunk);
    u32 found = 0;
    u32 const taken = pieces_walk<words_, rule_t>(
        table, row.query_length, text, lane, lane.inside, bound, [&](u32, u32) { ++found; }, []() { return true; });
    piece_count[threadIdx.x] = found;
    u32 const all = (u32)wave_sum_u64(found); // <= the columns of 64 pieces, below 2^32
    if (threadIdx.x == 0) *chunk_count = all;
    matches_counted(row, lane.inside, taken, chunk == 0, counters);
}

/** The body of a count kernel: `table` is the kernel's LDS, peq_layout<SZS_MYERS_SHORT_WORDS, byte_rows_k>::total_dwords of it. */
template <typename rule_t>
__device__ __forceinline__ void pieces_count_pass(u32 *table, szs_rerank_side_t const &queries, u64 first_query, u32 rows, u64 text,
                                                  u32 text_length, u64 piece, u32 pieces, u32 chunks, u32 bound,
                                                  u32 *__restrict__ piece_counts, u32 *__restrict__ chunk_counts, u32 *flags,
                                                  unsigned long long *counters) {
    u32 const r = blockIdx.x % rows, chunk = blockIdx.x / rows; // chunk below `chunks`: the host's grid
    listed_row_t const row = listed_row(queries, first_query, true, [&]() { return r; }, SZS_RERANK_LONGEST_QUERY, flags);
    u32 const length = (u32)__builtin_amdgcn_readfirstlane((int)row.query_length); // one row a wavefront: a scalar
    u64 const cell = (u64)r * chunks + chunk; // below rows x chunks: what the host reserved, 64 piece counts a chunk
    u32 *const piece_count = piece_counts + cell * wave_size_k, *const chunk_count = chunk_counts + cell;
    if (!length) { // no query, or a flag is up and the call fails: nothing found, nothing loaded
        piece_count[threadIdx.x] = 0;
        if (threadIdx.x == 0) *chunk_count = 0;
        return;
    }
    listed_at_width(SZS_RERANK_WORDS_OF(length), [&](auto width) {
        pieces_count_row<decltype(width)::value, rule_t>(table, row, text, text_length, piece, pieces, chunk, bound, piece_count, chunk_count,
                                                         counters);
    });
}

template <int words_, typename rule_t>
__device__ __forceinline__ void pieces_write_row(u32 *table, listed_row_t const &row, u64 text, u32 text_length, u64 piece, u32 pieces,
                                                 u32 chunk, u32 bound, u32 limit, u32 offset, u32 found, u64 *__restrict__ distances,
                                                 u64 *__restrict__ ends, unsigned long long *counters) {
    fuzzy_table<words_, (int)wave_size_k>(table, row);
    typename rule_t::piece_t const lane = rule_t::piece(row.query_length, text_length, piece, pieces, chunk);
    bool const live = lane.inside && found && offset < limit;
    u32 owed = live ? (found < limit - offset ? found : limit - offset) : 0u; // offset + owed <= limit
    u64 slot = row.row * limit + offset;                                        // below rows x limit while owed > 0
    u32 const taken = pieces_walk<words_, rule_t>(
        table, row.query_length, text, lane, live, bound,
        [&](u32 column_end, u32 score) {
            if (!owed) return;
            ends[slot] = (u64)lane.first + column_end, distances[slot] = score;
            ++slot, --owed;
        },
        [&]() { return __ballot(owed != 0) != 0; });
    matches_counted(row, live, taken, false, counters);
}

/** The body of a write kernel, behind the offsets pass: chunk_counts[row][chunk] is what the row's chunks before this one found. */
template <typename rule_t>
__device__ __forceinline__ void pieces_write_pass(u32 *table, szs_rerank_side_t const &queries, u64 first_query, u32 rows, u64 text,
                                                  u32 text_length, u64 piece, u32 pieces, u32 chunks, u32 bound, u32 limit,
                                                  u32 const *__restrict__ piece_counts, u32 const *__restrict__ chunk_counts,
                                                  u64 *__restrict__ distances, u64 *__restrict__ ends, u32 *flags,
                                                  unsigned long long *counters) {
    u32 const r = blockIdx.x % rows, chunk = blockIdx.x / rows;
    u64 const cell = (u64)r * chunks + chunk;
    u32 const before = chunk_counts[cell];
    if (before >= limit) return; // every slot is taken by then
    u32 const found = piece_counts[cell * wave_size_k + threadIdx.x];
    u32 const upto = wave_prefix_u32(found);
    if (!__shfl((int)upto, (int)wave_size_k - 1, 64)) return; // a chunk that found nothing
    listed_row_t const row = listed_row(queries, first_query, true, [&]() { return r; }, SZS_RERANK_LONGEST_QUERY, flags);
    u32 const length = (u32)__builtin_amdgcn_readfirstlane((int)row.query_length);
    if (!length) return; // (a row without a query counted nothing)
    listed_at_width(SZS_RERANK_WORDS_OF(length), [&](auto width) {
        pieces_write_row<decltype(width)::value, rule_t>(table, row, text, text_length, piece, pieces, chunk, bound, limit,
                                                         before + upto - found, found, distances, ends, counters);
    });
}

/** The grid the walking passes share; false: arguments no launch takes. */
static inline bool matches_grid(szs_rerank_side_t const *queries, uint64_t first_query, uint32_t rows, void const *text, uint64_t text_length,
                                uint64_t piece, u64 &pieces, u64 &chunks) {
    if (!queries || !piece || !text || !text_length || text_length > 0xFFFFFFFFull || !rows || first_query + rows > queries->count) return false;
    pieces = (text_length + piece - 1) / piece; // below 2^32
    chunks = (pieces + wave_size_k - 1) / wave_size_k;
    return (u64)rows * chunks <= 0x7FFFFFFFull;
}

/** The launch of a walking pass: rows x chunks workgroups of one wavefront.  `kernel` takes the queries, the first row, the rows, the
 *  text, its length, the piece, the pieces and the chunks, then `arguments` as they are; `valid` false refuses them. */
template <typename kernel_t, typename... arguments_t>
static inline int matches_launch(kernel_t kernel, bool valid, szs_rerank_side_t const *queries, uint64_t first_query, uint32_t rows,
                                 void const *text, uint64_t text_length, uint64_t piece, void *stream, arguments_t... arguments) {
    u64 pieces, chunks;
    if (!valid || !matches_grid(queries, first_query, rows, text, text_length, piece, pieces, chunks)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((u32)(rows * chunks)), dim3(wave_size_k), 0, static_cast<hipStream_t>(stream), *queries, first_query, rows,
                       (u64) reinterpret_cast<uintptr_t>(text), (u32)text_length, piece, (u32)pieces, (u32)chunks, arguments...);
    return (int)hipGetLastError();
}

} // namespace szs_hip

/*
 *  myers_fuzzy_scan.hip - the semi-global distance of every query inside ONE long text (szs_rocm_fuzzy_scan*, host/fuzzy_scan.c;
 *  DESIGN.md section 4.11): distance = min over j of D[m][j], end = the smallest j that attains it.  The distance, its table and a
 *  lane's walk are hip/fuzzy_core.hpp's; rows, widths, flags and counters are hip/rerank_core.hpp's; the piece a lane takes is
 *  hip/fuzzy_pieces.hpp's matches_piece, the one the bounded scans take.  This file's own is the schedule: the text is cut into
 *  PIECES, the pieces are dealt to lanes, and the lanes' results are reduced exactly.
 *
 *  - Piece p owns columns (p P, min(n, (p + 1) P)].  The lane that takes it walks from s = p P - warm, warm = min(p P, 2 m), so its
 *    DP has a free start at s instead of at 0: every value it sees is >= the true D[m][j] (fewer starts to choose from), and equal
 *    to it once j - s >= 2 m or s = 0, because the start that attains D[m][j] lies within m + D[m][j] <= 2 m bytes of j (section
 *    4.9's span bound).  It follows (best, leftmost end) over EVERY column it walks, warm-up included, and reports (best, s + end).
 *  - The answer is the lexicographic minimum of (distance, end) over the pieces: the piece that owns the true leftmost best end j*
 *    reports exactly (d, j*); any other piece that reports d at a column e has d >= D[m][e] >= d, so e is a true best end too and
 *    e >= j*.  Where nothing occurs piece 0 reports (m, 0) and every other piece (m, s > 0).
 *  - A one-wavefront workgroup serves ONE row and a CHUNK of 64 consecutive pieces: its lanes build the row's table once, at the
 *    row's own width, and lane l takes piece 64 chunk + l.  The grid is rows x ceil(pieces / 64), numbered chunk-major
 *    (row = id % rows): workgroups in flight together read the same stretch of the text.
 *  - A lane's key is distance << 32 | end; the wavefront's minimum goes into keys[row] with ONE 64-bit atomic minimum.  The host
 *    fills `keys` with 0xFF bytes ahead of the launch; a minimum does not depend on the order of its operands, so neither does the
 *    result.
 *  - levenshtein_fuzzy_scan_emit_kernel unpacks the keys into the caller's vectors by ordinary 8-byte stores: (0, 0) for a query
 *    of no bytes, (m, 0) where no piece reported (an empty text: the host launches no scan), else (key >> 32, key & 0xFFFFFFFF).
 *  - The table is static LDS of the widest layout (8 KB), as hip/myers_fuzzy_tile.hip's.
 *  - Counters: cells and bytes as walked, warm-up included; one pair per row with a non-empty query, counted by chunk 0 alone.
 */
#include "fuzzy_pieces.hpp"

namespace szs_hip {

__device__ __forceinline__ u64 wave_min_u64(u64 value) {
#pragma unroll
    for (int offset = 32; offset >= 1; offset >>= 1) {
        u64 const other = (u64)__shfl_xor((unsigned long long)value, offset, 64);
        value = other < value ? other : value;
    }
    return value;
}

template <int words_>
__device__ __forceinline__ void fuzzy_scan_row(u32 *table, listed_row_t const &row, u64 text, u32 text_length, u64 piece, u32 pieces,
                                               u32 chunk, unsigned long long *__restrict__ keys, unsigned long long *counters) {
    fuzzy_table<words_, (int)wave_size_k>(table, row);

    matches_piece_t const lane = matches_piece(row.query_length, text_length, piece, pieces, chunk);
    bool const live = row.has_row && row.query_length && lane.inside;
    u32 const walked = live ? lane.walked : 0u;

    u32 best, match_end;
    fuzzy_best_match<words_>(table, row.query_length, text + lane.first, walked, live, best, match_end);

    u64 const key = wave_min_u64(live ? (u64)best << 32 | (lane.first + match_end) : ~0ull);
    if (threadIdx.x == 0 && key != ~0ull) atomicMin(&keys[row.row], (unsigned long long)key);

    // (not matches_counted: this kernel also runs for a row without a query, which counts no pair and no bytes)
    listed_counters_t counted;
    if (live) counted.cells = (u64)row.query_length * walked, counted.bytes = walked;
    if (live && threadIdx.x == 0) counted.bytes += row.query_length, counted.pairs = chunk == 0; // the query: read once a workgroup
    counted.land(counters, chunk == 0);
}

__global__ __launch_bounds__(64) void levenshtein_fuzzy_scan_kernel(szs_rerank_side_t const queries, u64 const first_query, u32 const rows,
                                                                    u64 const text, u32 const text_length, u64 const piece,
                                                                    u32 const pieces, unsigned long long *__restrict__ keys, u32 *flags,
                                                                    unsigned long long *counters) {
    __shared__ __attribute__((aligned(16))) u32 fuzzy_scan_table[peq_layout<SZS_MYERS_SHORT_WORDS, byte_rows_k>::total_dwords];
    u32 const r = blockIdx.x % rows, chunk = blockIdx.x / rows; // chunk below ceil(pieces / 64): the host's grid
    listed_row_t const row = listed_row(queries, first_query, true, [&]() { return r; }, SZS_RERANK_LONGEST_QUERY, flags);
    u32 const length = (u32)__builtin_amdgcn_readfirstlane((int)row.query_length); // one row a wavefront: a scalar
    listed_at_width(SZS_RERANK_WORDS_OF(length), [&](auto width) {
        fuzzy_scan_row<decltype(width)::value>(fuzzy_scan_table, row, text, text_length, piece, pieces, chunk, keys, counters);
    });
}

__global__ __launch_bounds__(256) void levenshtein_fuzzy_scan_emit_kernel(szs_rerank_side_t const queries, u64 const first_query,
                                                                          u32 const rows, unsigned long long const *__restrict__ keys,
                                                                          u64 *__restrict__ distances, u64 *__restrict__ ends, u32 *flags) {
    u32 const r = blockIdx.x * blockDim.x + threadIdx.x;
    listed_row_t const row = listed_row(queries, first_query, r < rows, [&]() { return r; }, SZS_RERANK_LONGEST_QUERY, flags);
    if (!row.has_row) return; // beyond the rows, or a flag is up and the call fails
    u64 const key = keys[r];
    bool const reported = row.query_length && key != ~0ull;
    distances[r] = reported ? key >> 32 : row.query_length;
    if (ends) ends[r] = reported ? key & 0xFFFFFFFFull : 0;
}

} // namespace szs_hip

extern "C" int szs_hip_levenshtein_fuzzy_scan(szs_rerank_side_t const *queries, uint64_t first_query, uint32_t rows, void const *text,
                                              uint64_t text_length, uint64_t piece, unsigned long long *keys, uint32_t *flags,
                                              unsigned long long *counters, void *stream) {
    using namespace szs_hip;
    if (!queries || !keys || !flags || !counters || !piece || text_length > 0xFFFFFFFFull || (text_length && !text))
        return (int)hipErrorInvalidValue;
    if (!rows || !text_length) return 0;
    if (first_query + rows > queries->count) return (int)hipErrorInvalidValue;
    u64 const pieces = (text_length + piece - 1) / piece; // below 2^32
    u64 const workgroups = (u64)rows * ((pieces + wave_size_k - 1) / wave_size_k);
    if (workgroups > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(levenshtein_fuzzy_scan_kernel, dim3((u32)workgroups), dim3(wave_size_k), 0, static_cast<hipStream_t>(stream), *queries,
                       first_query, rows, (u64) reinterpret_cast<uintptr_t>(text), (u32)text_length, piece, (u32)pieces, keys, flags, counters);
    return (int)hipGetLastError();
}

extern "C" int szs_hip_levenshtein_fuzzy_scan_emit(szs_rerank_side_t const *queries, uint64_t first_query, uint32_t rows,
                                                   unsigned long long const *keys, uint64_t *distances, uint64_t *ends, uint32_t *flags,
                                                   void *stream) {
    using namespace szs_hip;
    if (!queries || !keys || !distances || !flags) return (int)hipErrorInvalidValue;
    if (!rows) return 0;
    if (first_query + rows > queries->count) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(levenshtein_fuzzy_scan_emit_kernel, dim3((rows + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(stream),
                       *queries, first_query, rows, keys, distances, ends, flags);
    return (int)hipGetLastError();
}

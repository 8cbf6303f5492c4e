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
 *  The layout is the first kernel's; what differs:
 *
 *  - The table is rerank's: zeroed, then the pattern's bits - byte i of the query at bit pad + (m - 1 - i).  The phantom low rows are
 *    ZERO rows, not wildcards: Eq = 0, VP = VN = 0 with +1 entering stays zero and hands HP = 1 upward - DP row zero of the global
 *    matrix, D'[0][t] = t (hip/myers_rerank.hip; tests/test_fuzzy_spans_model.py asserts that they stay zero).
 *  - The column is myers_prefix_column<W> (hip/myers_core.hpp) - myers_strip_column<W>(vp, vn, eq, 1, 0) with myers_column's
 *    materialisation: +1 enters bit 0, the horizontal pair of the last pattern row comes back.
 *  - The text is the window c[end - T, end), T = min(end, m + d), walked from its last byte down (text_stream_backward_t): only
 *    aligned dwords that hold a byte of the window are loaded.
 *  - Every lane tracks the bottom-row score from score = best = m, pos = 0: a strictly smaller score moves `best` and `pos` (the
 *    smallest t), start = end - pos.  A wavefront leaves the loop once every live lane has best == d: nothing can move `pos` then.
 *
 *  Indices, flags and counters are the first kernel's: the candidate is derived from the index again, `index < count` precedes every
 *  use, a refused index or a bad tape raises the same flag words and the lane addresses nothing.  d and end are data the kernel reads
 *  back from memory the caller can reach, so before they address anything: d <= m and end <= the candidate's length, else
 *  SZS_RERANK_FLAG_TAPE and a frozen lane.  The counters gain m x T cells and m + T bytes per pair; pairs are counted by the first
 *  kernel only.
 */
#include "rerank_core.hpp"

namespace szs_hip {

template <int words_, int lanes_>
__device__ __forceinline__ void fuzzy_starts_rows(u32 *table, bool has_row, u64 row, u64 query_address, u32 query_length,
                                                  szs_rerank_side_t const &candidates, u64 const *__restrict__ indices, u64 indices_stride,
                                                  u64 k, u64 const *__restrict__ distances, u64 const *__restrict__ ends,
                                                  u64 *__restrict__ starts, u64 outputs_stride, u32 *flags, unsigned long long *counters) {
    using layout = peq_layout<words_, byte_rows_k>;
    u32 const sub = threadIdx.x % lanes_;
    u32 const pad = 32u * words_ - query_length; // phantom low rows of THIS row (a row without a query: all of them)

    // ---- Peq of the REVERSED pattern: zero, then scatter - the query's last byte is the first real row.
    for (u32 i = sub; i < layout::total_dwords / 4; i += lanes_) reinterpret_cast<uint4 *>(table)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    u8 const *pattern = reinterpret_cast<u8 const *>(query_address);
    for (u32 i = sub; i < query_length; i += lanes_) {
        u32 const position = pad + (query_length - 1u - i);
        atomicOr(&table[layout::dword_index(pattern[i], (int)(position >> 5))], 1u << (position & 31));
    }
    __syncthreads();

    u64 cells = 0, bytes = 0;
#pragma unroll 1
    for (u64 first = 0; first < k; first += lanes_) { // uniform: every row of the call has k slots
        u64 const rank = first + sub;
        bool live = has_row && rank < k;
        u64 address = 0;
        u32 window = 0, distance = 0, end = 0; // the window: T bytes that end at `end`
        if (live) {
            u64 const index = indices ? indices[row * indices_stride + rank] : rank;
            u32 text_length = 0;
            if (index == ~0ull) starts[row * outputs_stride + rank] = 0, live = false; // an empty slot: no string is touched
            else if (index >= candidates.count) flags[SZS_RERANK_FLAG_INDEX] = 1u, live = false; // never used to address anything
            else if (!rerank_fetch(candidates, index, address, text_length)) flags[SZS_RERANK_FLAG_TAPE] = 1u, live = false;
            else {
                u64 const found = distances[row * outputs_stride + rank], ended = ends[row * outputs_stride + rank];
                if (found > query_length || ended > text_length) flags[SZS_RERANK_FLAG_TAPE] = 1u, live = false; // before they address anything
                else {
                    distance = (u32)found, end = (u32)ended;
                    window = end < query_length + distance ? end : query_length + distance;
                }
            }
        }
        u32 const longest_in_wave = wave_max_u32(window);
        u32 const shortest_in_wave = ~wave_max_u32(live ? ~window : 0u); // over live lanes; none: ~0, and the longest is 0

        u32 vp[words_], vn[words_];
#pragma unroll
        for (int w = 0; w < words_; ++w) vp[w] = rerank_bits_in_word(pad, 32u * words_, w), vn[w] = 0;
        u32 score = query_length, best = query_length, pos = 0;
        auto take = [&](u32 symbol, u32 taken) {
            u32 eq[words_];
            load_match_masks<words_, byte_rows_k>(table, symbol, eq);
            u32 const top = myers_prefix_column<words_>(vp, vn, eq);
            score += (top & 1u) - (top >> 1);
            if (score < best) best = score, pos = taken; // strictly smaller: the smallest t
        };
        // a lane is open while its best is above d; with none open in the wavefront no `pos` can move any more
        auto any_open = [&]() { return __builtin_amdgcn_ballot_w64(live && best != distance) != 0ull; };

        // ---- the window, from its last byte down: group `back` is bytes [T - 4 back - 4, T - 4 back), consumed from the top byte.
        //      A lane without a window loads nothing and its symbols - zeros - are never scored into anything that is written.
        text_stream_backward_t const text(address + (end - window), window);
        u32 column = 0, back = 0, raw_high = text.raw(0);
        bool open = any_open();
        if (4 <= shortest_in_wave && longest_in_wave) { // whole groups that every live lane still has: unpredicated
            u32 ahead = text.raw(1);
            for (; open && column + 4 <= shortest_in_wave; column += 4, ++back) {
                u32 const symbols = text.splice(raw_high, ahead);
                raw_high = ahead, ahead = text.raw(back + 2);
#pragma unroll
                for (int step = 0; step < 4; ++step) take((symbols >> (8 * (3 - step))) & 0xFFu, column + step + 1);
                open = any_open();
            }
        }
        if (open && column < longest_in_wave) { // the ragged part: every column predicated on the lane's own window
            u32 next = text.raw(back + 1);
#pragma unroll 1
            for (; open && column < longest_in_wave; column += 4, ++back) {
                u32 const after = text.raw(back + 2);
                u32 const symbols = text.splice(raw_high, next);
                raw_high = next, next = after;
#pragma unroll
                for (int step = 0; step < 4; ++step)
                    if (column + step < window) take((symbols >> (8 * (3 - step))) & 0xFFu, column + step + 1);
                open = any_open();
            }
        }

        if (live) {
            starts[row * outputs_stride + rank] = end - pos;
            cells += (u64)query_length * window, bytes += (u64)query_length + window;
        }
    }
    cells = wave_sum_u64(cells), bytes = wave_sum_u64(bytes);
    if (threadIdx.x == 0 && bytes) {
        atomicAdd(&counters[1], (unsigned long long)cells);
        atomicAdd(&counters[2], (unsigned long long)bytes);
    }
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
    constexpr u32 groups = wave_size_k / lanes_;
    u32 const group = threadIdx.x / lanes_;
    u32 const slot = blockIdx.x * groups + group;
    bool has_row = slot < rows_count;
    u64 const row = has_row ? rows[slot] : 0;
    u64 query_address = 0;
    u32 query_length = 0;
    if (has_row) {
        u64 const query = first_query + row;
        if (query >= queries.count || !rerank_fetch(queries, query, query_address, query_length)) flags[SZS_RERANK_FLAG_TAPE] = 1u, has_row = false;
        else if (query_length > SZS_RERANK_LONGEST_QUERY) flags[SZS_RERANK_FLAG_UNFIT] = 1u, has_row = false; // the host's job to prevent
        if (!has_row) query_length = 0;
    }
    // every row at the width of the wavefront's longest query - a scalar, so one of the eight bodies runs and nothing diverges
    u32 const longest = (u32)__builtin_amdgcn_readfirstlane((int)wave_max_u32(query_length));
    u32 const words = longest ? (longest + 31u) / 32u : 1u;
    u32 *const table = fuzzy_starts_tables + group * table_dwords;
#define SZS_FUZZY_STARTS_BODY(W)                                                                                                    \
    case W:                                                                                                                          \
        fuzzy_starts_rows<W, lanes_>(table, has_row, row, query_address, query_length, candidates, indices, indices_stride, k,       \
                                     distances, ends, starts, outputs_stride, flags, counters);                                      \
        break;
    switch (words) {
        SZS_FUZZY_STARTS_BODY(1)
        SZS_FUZZY_STARTS_BODY(2)
        SZS_FUZZY_STARTS_BODY(3)
        SZS_FUZZY_STARTS_BODY(4)
        SZS_FUZZY_STARTS_BODY(5)
        SZS_FUZZY_STARTS_BODY(6)
        SZS_FUZZY_STARTS_BODY(7)
    default: SZS_FUZZY_STARTS_BODY(8)
    }
#undef SZS_FUZZY_STARTS_BODY
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
    unsigned const lanes = szs_hip_rerank_lanes(k), groups = wave_size_k / lanes;
    u32 const table_dwords = rerank_table_dwords(widest); // the first kernel's: at most 8 KB a row, 32 KB a workgroup
    u32 const grid = (u32)(((u64)rows_count + groups - 1) / groups);
    size_t const lds = (size_t)groups * table_dwords * sizeof(u32);
    hipStream_t const s = static_cast<hipStream_t>(stream);
#define SZS_FUZZY_STARTS_LAUNCH(L)                                                                                                 \
    hipLaunchKernelGGL(levenshtein_fuzzy_starts_kernel<L>, dim3(grid), dim3(wave_size_k), lds, s, *queries, *candidates, first_query, \
                       rows, rows_count, indices, indices_stride, k, distances, ends, starts, outputs_stride, table_dwords, flags,    \
                       counters)
    if (lanes == 16) SZS_FUZZY_STARTS_LAUNCH(16);
    else if (lanes == 32) SZS_FUZZY_STARTS_LAUNCH(32);
    else SZS_FUZZY_STARTS_LAUNCH(64);
#undef SZS_FUZZY_STARTS_LAUNCH
    return (int)hipGetLastError();
}

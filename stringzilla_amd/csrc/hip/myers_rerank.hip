/*
 *  myers_rerank.hip - unit-cost byte Levenshtein distances of LISTED pairs (szs_rocm_rerank*, host/rerank.c).
 *
 *  The cross-product kernels (hip/lev_myers.hip) share one Peq table among 256 lanes: one query x 256 candidates.  A rerank row is
 *  one query x the k candidates an index row names - with k = 16 that shape would leave 240 lanes idle per table.  Here:
 *
 *  - A GROUP of L = 16 / 32 / 64 lanes (the smallest that holds min(k, 64)) serves one row: its own Peq table in LDS
 *    (peq_layout<W, 256>), one listed candidate per lane, fetched THROUGH the index - address and length from the tape's offsets, or
 *    from a ref array in index order when the side is a callback sequence.  Rows of more than 64 candidates walk them in chunks of
 *    64 against the same table.
 *  - A workgroup is ONE wavefront of 64 / L rows: the lanes that build a table are the lanes that read it, so there is no
 *    workgroup barrier at all, and the grid comes from the rows, not from the candidates.
 *  - The pattern is right-aligned over phantom low rows (lev_myers.hip), so every row of a wavefront runs at the width W of the
 *    wavefront's longest query - a scalar choice among eight bodies.  The host deals rows by descending query length: neighbours
 *    share a width.
 *  - myers_column and load_match_masks are hip/myers_core.hpp's, unchanged; distance = len(text) + popcount(VP) - popcount(VN);
 *    lanes whose text has ended, lanes of empty slots and lanes of refused indices are frozen by EXEC.
 *  - `index < count` precedes every use of an index: a bad one addresses nothing and raises a flag in pinned host memory.  Every
 *    kind of failure has a flag word of its own and every lane stores the same 1 there: what the host reads does not depend on
 *    which lane stored last.
 *  - Scores leave as ordinary 8-byte vector stores, straight into the caller's rows.
 *  (rerank_fetch, rerank_bits_in_word and wave_sum_u64 are hip/rerank_core.hpp's, shared with hip/myers_rerank_strips.hip.)
 */
#include "rerank_core.hpp"

namespace szs_hip {

/**
 *  The rows of one wavefront at `words_` words: every group of `lanes_` lanes builds its row's table, then scores the row's listed
 *  candidates, `lanes_` at a time.  `has_row`, `row`, `query_address`, `query_length` are uniform within a group.
 */
template <int words_, int lanes_>
__device__ __forceinline__ void rerank_rows(u32 *table, bool has_row, u64 row, u64 query_address, u32 query_length,
                                            szs_rerank_side_t const &candidates, u64 const *__restrict__ indices, u64 indices_stride, u64 k,
                                            u64 *__restrict__ scores, u64 scores_stride, u32 *flags, unsigned long long *counters) {
    using layout = peq_layout<words_, byte_rows_k>;
    u32 const sub = threadIdx.x % lanes_;
    u32 const pad = 32u * words_ - query_length; // phantom low rows of THIS row (a row without a query: all of them)

    // ---- Peq: zero, then scatter the pattern's bits.  One wavefront: __syncthreads() orders its LDS traffic, no s_barrier is left.
    for (u32 i = sub; i < layout::total_dwords / 4; i += lanes_) reinterpret_cast<uint4 *>(table)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    u8 const *pattern = reinterpret_cast<u8 const *>(query_address);
    for (u32 i = sub; i < query_length; i += lanes_) {
        u32 const position = pad + i;
        atomicOr(&table[layout::dword_index(pattern[i], (int)(position >> 5))], 1u << (position & 31));
    }
    __syncthreads();

    u64 pairs = 0, cells = 0, bytes = 0;
#pragma unroll 1
    for (u64 first = 0; first < k; first += lanes_) { // uniform: every row of the call has k slots
        u64 const rank = first + sub;
        bool live = has_row && rank < k;
        u64 address = 0;
        u32 text_length = 0;
        if (live) {
            u64 const index = indices[row * indices_stride + rank];
            if (index == ~0ull) scores[row * scores_stride + rank] = 0, live = false; // an empty slot: no string is touched
            else if (index >= candidates.count) flags[SZS_RERANK_FLAG_INDEX] = 1u, live = false; // never used to address anything
            else if (!rerank_fetch(candidates, index, address, text_length)) flags[SZS_RERANK_FLAG_TAPE] = 1u, live = false, text_length = 0;
        }
        u32 const longest_in_wave = wave_max_u32(text_length);
        u32 const shortest_in_wave = ~wave_max_u32(live ? ~text_length : 0u); // over live lanes; none: ~0, and the longest is 0

        u32 vp[words_], vn[words_];
#pragma unroll
        for (int w = 0; w < words_; ++w) vp[w] = rerank_bits_in_word(pad, 32u * words_, w), vn[w] = 0;
        auto take = [&](u32 symbol) {
            u32 eq[words_];
            load_match_masks<words_, byte_rows_k>(table, symbol, eq);
            myers_column<words_>(vp, vn, eq);
        };

        // ---- the text: only aligned dwords that hold a byte of the string are loaded (text_stream_t); a lane without a text loads
        //      nothing and its symbols - zeros - are never scored into anything that is written.
        text_stream_t const text(address, text_length);
        u32 column = 0, dword = 0, raw_low = text.raw(0);
        if (4 <= shortest_in_wave && longest_in_wave) { // whole dwords that every live lane still has: unpredicated
            u32 ahead = text.raw(1);
            for (; column + 4 <= shortest_in_wave; column += 4, ++dword) {
                u32 const symbols = text.splice(raw_low, ahead);
                raw_low = ahead, ahead = text.raw(dword + 2);
#pragma unroll
                for (int step = 0; step < 4; ++step) take((symbols >> (8 * step)) & 0xFFu);
            }
        }
        if (column < longest_in_wave) { // the ragged part: every column predicated on the lane's own length
            u32 next = text.raw(dword + 1);
#pragma unroll 1
            for (; column < longest_in_wave; column += 4, ++dword) {
                u32 const after = text.raw(dword + 2);
                u32 const symbols = text.splice(raw_low, next);
                raw_low = next, next = after;
#pragma unroll
                for (int step = 0; step < 4; ++step)
                    if (column + step < text_length) take((symbols >> (8 * step)) & 0xFFu);
            }
        }

        if (live) {
            u32 distance = text_length;
#pragma unroll
            for (int w = 0; w < words_; ++w) distance += (u32)__builtin_popcount(vp[w]) - (u32)__builtin_popcount(vn[w]);
            scores[row * scores_stride + rank] = distance;
            pairs += 1, cells += (u64)query_length * text_length, bytes += (u64)query_length + text_length;
        }
    }
    pairs = wave_sum_u64(pairs), cells = wave_sum_u64(cells), bytes = wave_sum_u64(bytes);
    if (threadIdx.x == 0 && pairs) {
        atomicAdd(&counters[0], (unsigned long long)pairs), atomicAdd(&counters[1], (unsigned long long)cells);
        atomicAdd(&counters[2], (unsigned long long)bytes);
    }
}

template <int lanes_>
__global__ __launch_bounds__(64) void levenshtein_rerank_kernel(szs_rerank_side_t const queries, szs_rerank_side_t const candidates,
                                                                u64 const first_query, u32 const *__restrict__ rows, u32 const rows_count,
                                                                u64 const *__restrict__ indices, u64 const indices_stride, u64 const k,
                                                                u64 *__restrict__ scores, u64 const scores_stride, u32 const table_dwords,
                                                                u32 *flags, unsigned long long *counters) {
    extern __shared__ __attribute__((aligned(16))) u32 rerank_tables[];
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
    u32 *const table = rerank_tables + group * table_dwords;
#define SZS_RERANK_BODY(W)                                                                                                          \
    case W:                                                                                                                          \
        rerank_rows<W, lanes_>(table, has_row, row, query_address, query_length, candidates, indices, indices_stride, k, scores,     \
                               scores_stride, flags, counters);                                                                       \
        break;
    switch (words) {
        SZS_RERANK_BODY(1)
        SZS_RERANK_BODY(2)
        SZS_RERANK_BODY(3)
        SZS_RERANK_BODY(4)
        SZS_RERANK_BODY(5)
        SZS_RERANK_BODY(6)
        SZS_RERANK_BODY(7)
    default: SZS_RERANK_BODY(8)
    }
#undef SZS_RERANK_BODY
}

} // namespace szs_hip

extern "C" unsigned szs_hip_rerank_lanes(uint64_t k) { return k <= 16 ? 16u : k <= 32 ? 32u : 64u; }

extern "C" int szs_hip_levenshtein_rerank(szs_rerank_side_t const *queries, szs_rerank_side_t const *candidates, uint64_t first_query,
                                          uint32_t const *rows, uint32_t rows_count, uint64_t const *indices, uint64_t indices_stride,
                                          uint64_t k, uint64_t *scores, uint64_t scores_stride, unsigned widest, uint32_t *flags,
                                          unsigned long long *counters, void *stream) {
    using namespace szs_hip;
    if (!rows_count || !k) return 0;
    if (widest < 1 || widest > SZS_MYERS_SHORT_WORDS || !queries || !candidates || !flags || !counters) return (int)hipErrorInvalidValue;
    static_assert(peq_layout<3>::total_dwords == peq_layout<4>::total_dwords && peq_layout<5>::total_dwords == peq_layout<8>::total_dwords,
                  "a table of W words fits the table of the next even chunk count");
    unsigned const lanes = szs_hip_rerank_lanes(k), groups = wave_size_k / lanes;
    u32 const table_dwords = rerank_table_dwords(widest); // at most 8 KB a row: four rows a wavefront, 32 KB a workgroup
    u32 const grid = (u32)(((u64)rows_count + groups - 1) / groups);
    size_t const lds = (size_t)groups * table_dwords * sizeof(u32);
    hipStream_t const s = static_cast<hipStream_t>(stream);
#define SZS_RERANK_LAUNCH(L)                                                                                                       \
    hipLaunchKernelGGL(levenshtein_rerank_kernel<L>, dim3(grid), dim3(wave_size_k), lds, s, *queries, *candidates, first_query, rows, \
                       rows_count, indices, indices_stride, k, scores, scores_stride, table_dwords, flags, counters)
    if (lanes == 16) SZS_RERANK_LAUNCH(16);
    else if (lanes == 32) SZS_RERANK_LAUNCH(32);
    else SZS_RERANK_LAUNCH(64);
#undef SZS_RERANK_LAUNCH
    return (int)hipGetLastError();
}

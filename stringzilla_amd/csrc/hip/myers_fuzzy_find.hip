/*
 *  myers_fuzzy_find.hip - the best match of a query INSIDE each listed candidate (szs_rocm_fuzzy_find*, host/fuzzy_find.c; DESIGN.md
 *  section 4.9): distance = min over j of D[m][j] of the unit-cost DP whose row zero is all zeros (a free start in the text), and
 *  end = the smallest j that attains it.
 *
 *  The layout is hip/myers_rerank.hip's, unchanged: a GROUP of L = 16 / 32 / 64 lanes and one Peq table in LDS per row, one listed
 *  candidate per lane, chunks of 64, one wavefront per workgroup, the width W = 1 ... 8 of the wavefront's longest query as a scalar
 *  choice among eight bodies, rerank_fetch, text_stream_t and the unpredicated / ragged text loops.  Three things differ:
 *
 *  - The column is myers_infix_column (hip/myers_core.hpp): nothing enters bit 0, and the horizontal pair of the pattern's last row
 *    comes back.  The pattern is right-aligned, so that row is bit 31 of word W - 1 for every row of the wavefront.
 *  - The phantom low rows are WILDCARDS: every row of the Peq table starts as the row's phantom mask (the bits below `pad`), the
 *    pattern's bits are scattered on top.  With Eq = 1, VP = VN = 0 and nothing entering, a phantom row computes D0 = 1, HP = HN = 0,
 *    VP' = VN' = 0 and `Eq & VP` = 0 feeds no carry: it stays zero and hands h = 0 to the first real row in every column - DP row
 *    zero of the semi-global matrix.  (Rows with Eq = 0 would emit HP = 1 upward: the global distance's row zero, wrong here.)
 *  - Every lane tracks the bottom-row score: it starts at m, moves by hp - hn of the last row per column, and a strictly smaller
 *    score moves `best` and `end` (the leftmost end).  A live lane stores both as ordinary 8-byte vector stores.
 *
 *  Indices, flags and counters are the rerank kernel's: `index < count` precedes every use of an index, every kind of failure has a
 *  flag word of its own in pinned host memory, lanes of empty slots, refused indices and ended texts are frozen by EXEC.  `indices`
 *  NULL is the dense form: slot r is candidate r.
 */
#include "rerank_core.hpp"

namespace szs_hip {

template <int words_, int lanes_>
__device__ __forceinline__ void fuzzy_find_rows(u32 *table, bool has_row, u64 row, u64 query_address, u32 query_length,
                                                szs_rerank_side_t const &candidates, u64 const *__restrict__ indices, u64 indices_stride,
                                                u64 k, u64 *__restrict__ distances, u64 *__restrict__ ends, u64 outputs_stride, u32 *flags,
                                                unsigned long long *counters) {
    using layout = peq_layout<words_, byte_rows_k>;
    u32 const sub = threadIdx.x % lanes_;
    u32 const pad = 32u * words_ - query_length; // phantom low rows of THIS row (a row without a query: all of them)

    // ---- Peq: every row of the table is the phantom mask - a wildcard in the rows below the pattern - then the pattern's bits.
    //      dword d of the image holds word (d / (rows x chunk_words)) x chunk_words + d % chunk_words (peq_layout::dword_index).
    for (u32 i = sub; i < layout::total_dwords / 4; i += lanes_) {
        u32 const chunk_base = (4u * i / (byte_rows_k * layout::chunk_words)) * layout::chunk_words;
        reinterpret_cast<uint4 *>(table)[i] = make_uint4(rerank_bits_in_word(0, pad, (int)(chunk_base + 0 % layout::chunk_words)),
                                                         rerank_bits_in_word(0, pad, (int)(chunk_base + 1 % layout::chunk_words)),
                                                         rerank_bits_in_word(0, pad, (int)(chunk_base + 2 % layout::chunk_words)),
                                                         rerank_bits_in_word(0, pad, (int)(chunk_base + 3 % layout::chunk_words)));
    }
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
            u64 const index = indices ? indices[row * indices_stride + rank] : rank;
            if (index == ~0ull) { // an empty slot: no string is touched
                distances[row * outputs_stride + rank] = 0, live = false;
                if (ends) ends[row * outputs_stride + rank] = 0;
            }
            else if (index >= candidates.count) flags[SZS_RERANK_FLAG_INDEX] = 1u, live = false; // never used to address anything
            else if (!rerank_fetch(candidates, index, address, text_length)) flags[SZS_RERANK_FLAG_TAPE] = 1u, live = false, text_length = 0;
        }
        u32 const longest_in_wave = wave_max_u32(text_length);
        u32 const shortest_in_wave = ~wave_max_u32(live ? ~text_length : 0u); // over live lanes; none: ~0, and the longest is 0

        u32 vp[words_], vn[words_];
#pragma unroll
        for (int w = 0; w < words_; ++w) vp[w] = rerank_bits_in_word(pad, 32u * words_, w), vn[w] = 0;
        u32 score = query_length, best = query_length, end = 0;
        auto take = [&](u32 symbol, u32 column_end) {
            u32 eq[words_];
            load_match_masks<words_, byte_rows_k>(table, symbol, eq);
            u32 const top = myers_infix_column<words_>(vp, vn, eq);
            score += (top & 1u) - (top >> 1);
            if (score < best) best = score, end = column_end; // strictly smaller: the leftmost end
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
                for (int step = 0; step < 4; ++step) take((symbols >> (8 * step)) & 0xFFu, column + step + 1);
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
                    if (column + step < text_length) take((symbols >> (8 * step)) & 0xFFu, column + step + 1);
            }
        }

        if (live) {
            distances[row * outputs_stride + rank] = best;
            if (ends) ends[row * outputs_stride + rank] = end;
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
__global__ __launch_bounds__(64) void levenshtein_fuzzy_find_kernel(szs_rerank_side_t const queries, szs_rerank_side_t const candidates,
                                                                    u64 const first_query, u32 const *__restrict__ rows,
                                                                    u32 const rows_count, u64 const *__restrict__ indices,
                                                                    u64 const indices_stride, u64 const k, u64 *__restrict__ distances,
                                                                    u64 *__restrict__ ends, u64 const outputs_stride,
                                                                    u32 const table_dwords, u32 *flags, unsigned long long *counters) {
    extern __shared__ __attribute__((aligned(16))) u32 fuzzy_find_tables[];
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
    u32 *const table = fuzzy_find_tables + group * table_dwords;
#define SZS_FUZZY_FIND_BODY(W)                                                                                                      \
    case W:                                                                                                                          \
        fuzzy_find_rows<W, lanes_>(table, has_row, row, query_address, query_length, candidates, indices, indices_stride, k,         \
                                   distances, ends, outputs_stride, flags, counters);                                                \
        break;
    switch (words) {
        SZS_FUZZY_FIND_BODY(1)
        SZS_FUZZY_FIND_BODY(2)
        SZS_FUZZY_FIND_BODY(3)
        SZS_FUZZY_FIND_BODY(4)
        SZS_FUZZY_FIND_BODY(5)
        SZS_FUZZY_FIND_BODY(6)
        SZS_FUZZY_FIND_BODY(7)
    default: SZS_FUZZY_FIND_BODY(8)
    }
#undef SZS_FUZZY_FIND_BODY
}

} // namespace szs_hip

extern "C" int szs_hip_levenshtein_fuzzy_find(szs_rerank_side_t const *queries, szs_rerank_side_t const *candidates, uint64_t first_query,
                                              uint32_t const *rows, uint32_t rows_count, uint64_t const *indices, uint64_t indices_stride,
                                              uint64_t k, uint64_t *distances, uint64_t *ends, uint64_t outputs_stride, unsigned widest,
                                              uint32_t *flags, unsigned long long *counters, void *stream) {
    using namespace szs_hip;
    if (!rows_count || !k) return 0;
    if (widest < 1 || widest > SZS_MYERS_SHORT_WORDS || !queries || !candidates || !distances || !flags || !counters)
        return (int)hipErrorInvalidValue;
    unsigned const lanes = szs_hip_rerank_lanes(k), groups = wave_size_k / lanes;
    u32 const table_dwords = rerank_table_dwords(widest); // at most 8 KB a row: four rows a wavefront, 32 KB a workgroup
    u32 const grid = (u32)(((u64)rows_count + groups - 1) / groups);
    size_t const lds = (size_t)groups * table_dwords * sizeof(u32);
    hipStream_t const s = static_cast<hipStream_t>(stream);
#define SZS_FUZZY_FIND_LAUNCH(L)                                                                                                   \
    hipLaunchKernelGGL(levenshtein_fuzzy_find_kernel<L>, dim3(grid), dim3(wave_size_k), lds, s, *queries, *candidates, first_query,  \
                       rows, rows_count, indices, indices_stride, k, distances, ends, outputs_stride, table_dwords, flags, counters)
    if (lanes == 16) SZS_FUZZY_FIND_LAUNCH(16);
    else if (lanes == 32) SZS_FUZZY_FIND_LAUNCH(32);
    else SZS_FUZZY_FIND_LAUNCH(64);
#undef SZS_FUZZY_FIND_LAUNCH
    return (int)hipGetLastError();
}

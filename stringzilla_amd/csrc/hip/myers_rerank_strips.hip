/*
 *  myers_rerank_strips.hip - unit-cost byte Levenshtein distances of LISTED pairs whose query is a DOCUMENT: more than 256 and at
 *  most 65,536 bytes (szs_rocm_rerank*, host/rerank.c).  The twin of hip/myers_rerank.hip for the rows its
 *  256-row bit-vector cannot hold; groups, rows, indices, flags and counters are hip/rerank_core.hpp's.  Empty slots score 0 and
 *  touch no string; scores leave as ordinary 8-byte vector stores.  This kernel's own:
 *
 *  - STRIPS.  The query is cut into strips of equal width W = 1 ... 8 words, as few as 8 words allow (SZS_RERANK_STRIPS_OF,
 *    SZS_RERANK_STRIP_WORDS_OF: a 300-byte query is two strips of 5 words, not 8 + 2) - the sizing rule of
 *    levenshtein_myers_banded_kernel (hip/lev_myers.hip) with 8 in place of 64.  Strip count and width are those of the
 *    wavefront's longest query: scalars, so one of eight bodies runs.  Phantom low rows pad the FIRST strip; the pattern's last
 *    row is the top bit of the last strip.
 *  - Per strip the group rebuilds its table (peq_layout<W, 256>, 8 KB a row at most) from that strip's slice of the pattern and
 *    every lane walks its candidate with myers_strip_column<W> (hip/myers_core.hpp, unchanged).  The first strip enters with
 *    hp_in = 1, hn_in = 0 (DP row zero); a later strip enters with the pair the strip above parked for that column.
 *    distance = len(text) + sum over strips of popcount(VP) - popcount(VN).
 *  - A shorter row of the wavefront has more phantom rows, possibly one or more WHOLE strips of them.  Such a strip is inert:
 *    VP = VN = Eq = 0 and (hp_in, hn_in) = (1, 0) give sum = 0, D0 = 0, HP = ~0, HN = 0, hence VP' = 0 | ~(0 | ~0) = 0,
 *    VN' = ~0 & 0 = 0 and the pair leaving the last row is (1, 0) again - by induction every phantom strip hands DP row zero down
 *    unchanged and adds nothing to the sum.  tests/test_gpu_rerank_strips.py pins the case.
 *  - Loop order: chunk of candidates outside, strips inside, so a lane's parked array belongs to one candidate at a time.  The
 *    parked deltas are lev_myers.hip's format - 2 bits per text column, 16 columns to a dword - in global scratch, per workgroup
 *    [dword][64 lanes], overwritten in place by the next strip.
 *  - The grid is PERSISTENT: `workgroups` wavefronts stride over the row slots, which bounds the scratch at
 *    workgroups x 64 x parked_dwords dwords (the host sizes both: host/rerank.c).  A candidate of more than 16 x parked_dwords
 *    bytes is not scored and sets `flags[SZS_RERANK_FLAG_UNFIT]`: the parked array is never addressed past its end.
 */
#include "rerank_core.hpp"

namespace szs_hip {

constexpr u32 rerank_strip_table_dwords_k = peq_layout<SZS_RERANK_STRIP_WORDS>::total_dwords; // 8 KB: a table of any W fits

/**
 *  The rows of one wavefront as `strips` strips of `words_` words; `strips` is uniform within the wavefront.  `parked_mine`: this
 *  lane's column of the workgroup's parked array, `parked_dwords` dwords of 16 text columns each, 64 dwords apart.
 */
template <int words_, int lanes_>
__device__ __forceinline__ void rerank_strip_rows(u32 *table, u32 strips, listed_row_t const &row, szs_rerank_side_t const &candidates,
                                                  u64 const *__restrict__ indices, u64 indices_stride, u64 k, u64 *__restrict__ scores,
                                                  u64 scores_stride, u32 *parked_mine, u32 parked_dwords, u32 *flags,
                                                  unsigned long long *counters) {
    using layout = peq_layout<words_, byte_rows_k>;
    constexpr u32 strip_rows = 32u * words_;
    u32 const sub = threadIdx.x % lanes_;
    u32 const pad = strips * strip_rows - row.query_length; // phantom low rows of THIS row (a row without a query: all of them)
    u8 const *const pattern = reinterpret_cast<u8 const *>(row.query_address);

    listed_counters_t counted;
#pragma unroll 1
    for (u64 first = 0; first < k; first += lanes_) { // uniform: every row of the call has k slots
        u64 const rank = first + sub, at = row.row * scores_stride + rank;
        u64 address = 0;
        u32 text_length = 0;
        bool live = row.has_row && rank < k &&
                    listed_candidate(candidates, indices[row.row * indices_stride + rank], [&]() { scores[at] = 0; }, flags, address, text_length);
        if (live && ((u64)text_length + 15u) / 16u > parked_dwords) // the host's job to prevent: nothing is parked for it
            flags[SZS_RERANK_FLAG_UNFIT] = 1u, live = false, text_length = 0;
        u32 const longest_in_wave = wave_max_u32(text_length);
        u32 const shortest_in_wave = ~wave_max_u32(live ? ~text_length : 0u); // over live lanes; none: ~0, and the longest is 0
        text_stream_t const text(address, text_length);
        i32 delta_sum = 0;

#pragma unroll 1
        for (u32 strip = 0; strip < strips; ++strip) {
            bool const first_strip = strip == 0, last_strip = strip + 1 == strips;
            u32 const strip_base = strip * strip_rows; // the strip's first row among the strips x strip_rows rows of the wavefront
            // ---- Peq of this strip: bit b is pattern[strip_base + b - pad].  One wavefront: __syncthreads() orders its LDS traffic,
            //      no s_barrier is left; the first one keeps the previous strip's reads ahead of the zeroing.
            __syncthreads();
            for (u32 i = sub; i < layout::total_dwords / 4; i += lanes_) reinterpret_cast<uint4 *>(table)[i] = make_uint4(0, 0, 0, 0);
            __syncthreads();
            for (u32 bit = sub; bit < strip_rows; bit += lanes_) {
                u32 const position = strip_base + bit;
                if (position >= pad) atomicOr(&table[layout::dword_index(pattern[position - pad], (int)(bit >> 5))], 1u << (bit & 31));
            }
            __syncthreads();

            // phantom rows hold VP = VN = 0: a part of this strip, all of it, or none
            u32 const phantom = pad > strip_base ? (pad - strip_base < strip_rows ? pad - strip_base : strip_rows) : 0u;
            u32 vp[words_], vn[words_];
#pragma unroll
            for (int w = 0; w < words_; ++w) vp[w] = rerank_bits_in_word(phantom, strip_rows, w), vn[w] = 0;

            // Deltas of 16 columns per dword: `entering` was parked by the strip above, `leaving` collects this strip's.
            u32 entering = 0, leaving = 0;
            auto take = [&](u32 symbol, u32 column) {
                u32 eq[words_];
                load_match_masks<words_, byte_rows_k>(table, symbol, eq);
                u32 const slot = 2 * (column & 15u);
                u32 const hp_in = first_strip ? 1u : (entering >> slot) & 1u; // DP row 0 grows by one per column
                u32 const hn_in = first_strip ? 0u : (entering >> (slot + 1)) & 1u;
                leaving |= myers_strip_column<words_>(vp, vn, eq, hp_in, hn_in) << slot;
            };

            // ---- the text: only aligned dwords that hold a byte of the string are loaded (text_stream_t).  Only live lanes touch
            //      the parked array, and a live lane's groups of 16 columns lie below parked_dwords (checked above).
            u32 column = 0, dword = 0, raw_low = text.raw(0);
            if (4 <= shortest_in_wave && longest_in_wave) { // whole dwords that every live lane still has: unpredicated columns
                u32 ahead = text.raw(1);
                for (; column + 4 <= shortest_in_wave; column += 4, ++dword) {
                    u32 const symbols = text.splice(raw_low, ahead);
                    raw_low = ahead, ahead = text.raw(dword + 2);
                    if ((dword & 3u) == 0) { // a new group of 16 columns
                        if (!first_strip && live) entering = parked_mine[(u64)(dword / 4) * wave_size_k];
                        leaving = 0;
                    }
#pragma unroll
                    for (int step = 0; step < 4; ++step) take((symbols >> (8 * step)) & 0xFFu, column + step);
                    if ((dword & 3u) == 3 && !last_strip && live) parked_mine[(u64)(dword / 4) * wave_size_k] = leaving;
                }
            }
            // A main loop that stops inside a group of 16 columns parks what it has: a lane whose text ends right there never gets
            // to the tail, and a lane that does overwrites the dword with a superset of these bits.
            if ((dword & 3u) != 0 && !last_strip && live) parked_mine[(u64)(dword / 4) * wave_size_k] = leaving;
            if (column < longest_in_wave) { // the ragged part: every column predicated on the lane's own length
                u32 next = text.raw(dword + 1);
#pragma unroll 1
                for (; column < longest_in_wave; column += 4, ++dword) {
                    u32 const after = text.raw(dword + 2);
                    u32 const symbols = text.splice(raw_low, next);
                    raw_low = next, next = after;
                    if ((dword & 3u) == 0) {
                        if (!first_strip && column < text_length) entering = parked_mine[(u64)(dword / 4) * wave_size_k];
                        leaving = 0;
                    }
#pragma unroll
                    for (int step = 0; step < 4; ++step)
                        if (column + step < text_length) take((symbols >> (8 * step)) & 0xFFu, column + step);
                    // a group is parked when it is complete or when the text ends inside it
                    if (!last_strip && column < text_length && ((dword & 3u) == 3 || column + 4 >= text_length))
                        parked_mine[(u64)(dword / 4) * wave_size_k] = leaving;
                }
            }
#pragma unroll
            for (int w = 0; w < words_; ++w) delta_sum += (i32)__builtin_popcount(vp[w]) - (i32)__builtin_popcount(vn[w]);
        }

        if (live) {
            scores[at] = (u64)((i64)text_length + delta_sum);
            counted.add(row.query_length, text_length);
        }
    }
    counted.land(counters, true);
}

template <int lanes_>
__global__ __launch_bounds__(64) void levenshtein_rerank_strips_kernel(szs_rerank_side_t const queries, szs_rerank_side_t const candidates,
                                                                       u64 const first_query, u32 const *__restrict__ rows,
                                                                       u32 const rows_count, u64 const *__restrict__ indices,
                                                                       u64 const indices_stride, u64 const k, u64 *__restrict__ scores,
                                                                       u64 const scores_stride, u32 *__restrict__ parked,
                                                                       u32 const parked_dwords, u32 *flags, unsigned long long *counters) {
    constexpr u32 groups = wave_size_k / lanes_;
    __shared__ __attribute__((aligned(16))) u32 rerank_tables[groups * rerank_strip_table_dwords_k]; // 8 KB a row, 32 KB at most
    u32 const group = threadIdx.x / lanes_;
    u32 *const table = rerank_tables + group * rerank_strip_table_dwords_k;
    u32 *const parked_mine = parked + (u64)blockIdx.x * parked_dwords * wave_size_k + threadIdx.x; // [dword = 16 columns][lane]

#pragma unroll 1
    for (u64 first_slot = (u64)blockIdx.x * groups; first_slot < rows_count; first_slot += (u64)gridDim.x * groups) { // uniform
        listed_row_t const row = listed_row(queries, first_query, rows, rows_count, first_slot + group, SZS_RERANK_LONGEST_STRIPS_QUERY, flags);
        // every row at the strip count and width of the wavefront's longest query - scalars, so one of the eight bodies runs
        u32 const words = SZS_RERANK_WORDS_OF(listed_longest_query(row));
        u32 const strips = SZS_RERANK_STRIPS_OF(words);
        listed_at_width(SZS_RERANK_STRIP_WORDS_OF(words), [&](auto width) {
            rerank_strip_rows<decltype(width)::value, lanes_>(table, strips, row, candidates, indices, indices_stride, k, scores, scores_stride,
                                                              parked_mine, parked_dwords, flags, counters);
        });
    }
}

} // namespace szs_hip

extern "C" int szs_hip_levenshtein_rerank_strips(szs_rerank_side_t const *queries, szs_rerank_side_t const *candidates, uint64_t first_query,
                                                 uint32_t const *rows, uint32_t rows_count, uint64_t const *indices, uint64_t indices_stride,
                                                 uint64_t k, uint64_t *scores, uint64_t scores_stride, uint32_t workgroups, uint32_t *parked,
                                                 uint32_t parked_dwords, uint32_t *flags, unsigned long long *counters, void *stream) {
    using namespace szs_hip;
    if (!rows_count || !k) return 0;
    if (!workgroups || !parked || !parked_dwords || !queries || !candidates || !flags || !counters) return (int)hipErrorInvalidValue;
    return listed_launch(k, [&](auto lanes) {
        hipLaunchKernelGGL(levenshtein_rerank_strips_kernel<decltype(lanes)::value>, dim3(workgroups), dim3(wave_size_k), 0,
                           static_cast<hipStream_t>(stream), *queries, *candidates, first_query, rows, rows_count, indices, indices_stride, k,
                           scores, scores_stride, parked, parked_dwords, flags, counters);
    });
}

/*
 *  myers_alignments.hip - WHICH edits: the edit script of every listed pair (szs_rocm_alignments*, host/alignments.c; DESIGN.md
 *  section 4.14).  For slot (q, r): the query of m bytes against s = candidate[start : end] of t <= SZS_ALIGN_LONGEST_SPAN bytes (the
 *  whole candidate where the call gives no spans); distances = lev(q, s), lengths = L, ops = the CANONICAL script in forward order -
 *  the walk over the suffix DP S[i][j] = lev(q[i:], s[j:]) from (0, 0) that takes the first of diagonal ('=' / 'X'), 'I' (a query
 *  byte alone), 'D' (a candidate byte alone) that keeps to S.
 *
 *  On the REVERSED strings S is an ordinary prefix DP, D'[i'][j'] = S[m - i'][t - j'], and that walk is the ordinary traceback from
 *  its bottom-right corner: the pass of hip/myers_fuzzy_spans.hip - fuzzy_reversed_table, text_stream_backward_t, the global column -
 *  computes D', and a traceback of the reversed problem emits the ops in the original FORWARD order, so a lane stores them at
 *  ascending addresses without knowing L first.  Groups, rows, tables, indices, flags, the text walk and the counters are
 *  hip/rerank_core.hpp's.  This kernel's own:
 *
 *  - The column is myers_prefix_column_traced<W> (hip/myers_core.hpp): it hands out VP' and the true diagonal-zero vector D0 | VN.
 *    Both go to the lane's TRACE, one 8-byte cell per word and column, laid out [column][word][lane]: the 64 lanes of a wavefront
 *    store 512 consecutive bytes.
 *  - The traceback, per lane, from (m, t): at real row i' (bit pad + i' - 1) and column j' - diagonal iff the bytes are equal or
 *    the D0 bit is clear; else 'I' iff the VP' bit is set; else 'D'.  Row zero takes 'D's only, column zero 'I's only.  No running
 *    score: per step one 8-byte load of the lane's own trace and a byte of each string (tests/test_alignments_model.py is this rule,
 *    word by word, against the plain DP).
 *  - The trace does not grow with the call: a workgroup owns one REGION of 64 lanes x 512 columns x `widest` words x 8 bytes and
 *    reuses it for every chunk of 64 slots and every run of rows it serves - the runs blockIdx.x + i x gridDim.x.  The host sizes the
 *    grid by the regions its budget holds (host/alignments.c).  A lane reads back only what it stored itself, in program order.
 *  - A script of more than `capacity` ops leaves its slot all zero and its length L: a lane whose script MAY not fit (m + t above
 *    the capacity) walks once to count and a second time, where it fits, to store.  Past the first L bytes a slot is zero-filled.
 *
 *  `start` and `end` are data the kernel reads from memory the caller owns: start <= end <= the candidate's length before they
 *  address anything, else SZS_RERANK_FLAG_TAPE and a frozen lane; a span above SZS_ALIGN_LONGEST_SPAN bytes SZS_RERANK_FLAG_UNFIT.
 *  Every store is an ordinary vector store; every address is 64-bit.
 */
#include "fuzzy_core.hpp"

namespace szs_hip {

constexpr u32 align_columns_k = SZS_ALIGN_LONGEST_SPAN;

/** Zeros in bytes [from, capacity) of a slot: whole dwords where the slot's address allows. */
__device__ __forceinline__ void align_zero_fill(u8 *slot, u64 from, u64 capacity) {
    u64 at = from;
    for (; at < capacity && ((reinterpret_cast<u64>(slot) + at) & 3); ++at) slot[at] = 0;
    for (; at + 4 <= capacity; at += 4) *reinterpret_cast<u32 *>(slot + at) = 0u;
    for (; at < capacity; ++at) slot[at] = 0;
}

/** What the kernel reads and writes per slot: `starts` / `ends` NULL - the whole candidate; `ops` NULL - `capacity` 0. */
struct align_arrays_t {
    u64 const *indices, *starts, *ends;
    u64 inputs_stride;
    u64 *distances, *lengths;
    u64 outputs_stride;
    u8 *ops;
    u64 capacity;
};

template <int words_, int lanes_>
__device__ __forceinline__ void alignments_rows(u32 *table, listed_row_t const &row, szs_rerank_side_t const &candidates, u64 k,
                                                align_arrays_t const &arrays, uint2 *region, u32 *flags, unsigned long long *counters) {
    u32 const sub = threadIdx.x % lanes_, lane = threadIdx.x;
    u32 const query_length = row.query_length, pad = 32u * words_ - query_length;
    u8 const *const query = reinterpret_cast<u8 const *>(row.query_address);
    fuzzy_reversed_table<words_, lanes_>(table, row); // (a row without a query: phantom rows only)

    listed_counters_t counted;
#pragma unroll 1
    for (u64 first = 0; first < k; first += lanes_) { // uniform: every row of the call has k slots
        u64 const rank = first + sub, at = row.row * arrays.outputs_stride + rank, listed_at = row.row * arrays.inputs_stride + rank;
        u8 *const slot = arrays.ops ? arrays.ops + at * arrays.capacity : nullptr;
        auto const on_empty = [&]() {
            arrays.distances[at] = 0, arrays.lengths[at] = 0;
            if (slot) align_zero_fill(slot, 0, arrays.capacity);
        };
        u64 address = 0;
        u32 text_length = 0;
        bool live = row.has_row && rank < k &&
                    listed_candidate(candidates, arrays.indices ? arrays.indices[listed_at] : rank, on_empty, flags, address, text_length);
        u32 span = text_length; // t: the bytes of s, which begin at `address`
        if (live && arrays.starts) {
            u64 const start = arrays.starts[listed_at], end = arrays.ends[listed_at];
            if (start == ~0ull && end == ~0ull) on_empty(), live = false; // the empty slot of the scans' matrices
            else if (start > end || end > text_length) flags[SZS_RERANK_FLAG_TAPE] = 1u, live = false; // before they address anything
            else address += start, span = (u32)(end - start);
        }
        if (live && span > align_columns_k) flags[SZS_RERANK_FLAG_UNFIT] = 1u, live = false; // beyond the lane's trace
        if (!live) span = 0, address = 0;

        /* the forward half: D' column by column, the trace of every column parked in the lane's own cells */
        u32 vp[words_], vn[words_];
#pragma unroll
        for (int w = 0; w < words_; ++w) vp[w] = rerank_bits_in_word(pad, 32u * words_, w), vn[w] = 0;
        u32 score = query_length;
        listed_walk(
            text_stream_backward_t(address, span), span, live,
            [&](u32 symbol, u32 taken) { // taken <= the wavefront's longest span <= align_columns_k
                u32 eq[words_], diagonal_zero[words_];
                load_match_masks<words_, byte_rows_k>(table, symbol, eq);
                u32 const top = myers_prefix_column_traced<words_>(vp, vn, eq, diagonal_zero);
                score += (top & 1u) - (top >> 1);
                uint2 *const cells = region + ((u64)(taken - 1u) * words_) * wave_size_k + lane;
#pragma unroll
                for (int w = 0; w < words_; ++w) cells[(u64)w * wave_size_k] = make_uint2(vp[w], diagonal_zero[w]);
            },
            []() { return true; });
        if (live) { // (the lanes meet again before the next chunk's walk, which reduces over the wavefront)
            /* the second half: the lane's own walk from (m, t); `store` false only counts */
            u8 const *const text = reinterpret_cast<u8 const *>(address);
            auto const traceback = [&](bool store) {
                u32 rows_left = query_length, columns_left = span, emitted = 0;
                while (rows_left | columns_left) {
                    u8 op;
                    if (!rows_left) op = 'D', --columns_left;
                    else if (!columns_left) op = 'I', --rows_left;
                    else {
                        u32 const bit = pad + rows_left - 1u;
                        uint2 const cell = region[((u64)(columns_left - 1u) * words_ + (bit >> 5)) * wave_size_k + lane];
                        bool const equal = query[query_length - rows_left] == text[span - columns_left];
                        if (equal || !((cell.y >> (bit & 31u)) & 1u)) op = equal ? '=' : 'X', --rows_left, --columns_left;
                        else if ((cell.x >> (bit & 31u)) & 1u) op = 'I', --rows_left;
                        else op = 'D', --columns_left;
                    }
                    if (store) slot[emitted] = op; // emitted < L <= capacity: see below
                    ++emitted;
                }
                return emitted;
            };
            bool const certain = (u64)query_length + span <= arrays.capacity; // L <= m + t: it fits whatever it is
            u32 length = 0;
#pragma unroll 1
            for (int pass = 0; pass < 2; ++pass) { // one body for both walks
                bool const store = pass == 1;
                if (store ? (u64)length <= arrays.capacity : !certain) length = traceback(store); // (certain: `length` is still 0)
            }
            arrays.distances[at] = score, arrays.lengths[at] = length;
            if (slot) align_zero_fill(slot, (u64)length <= arrays.capacity ? length : 0, arrays.capacity);
            counted.add(query_length, span);
            counted.bytes += length;
        }
    }
    counted.land(counters, true);
}

template <int lanes_>
__global__ __launch_bounds__(64) void levenshtein_alignments_kernel(szs_rerank_side_t const queries, szs_rerank_side_t const candidates,
                                                                    u64 const first_query, u32 const *__restrict__ rows,
                                                                    u32 const rows_count, u64 const k, align_arrays_t const arrays,
                                                                    uint2 *trace, u64 const region_cells, u32 const table_dwords,
                                                                    u32 *flags, unsigned long long *counters) {
    extern __shared__ __attribute__((aligned(16))) u32 alignments_tables[];
    constexpr u32 groups = wave_size_k / lanes_;
    uint2 *const region = trace + (u64)blockIdx.x * region_cells; // this workgroup's, for every run of rows it serves
    u64 const runs = ((u64)rows_count + groups - 1) / groups;
#pragma unroll 1
    for (u64 run = blockIdx.x; run < runs; run += gridDim.x)
        listed_one_strip_rows_at<lanes_>(queries, first_query, rows, rows_count, run * groups, alignments_tables, table_dwords, flags,
                                         [&](auto width, u32 *table, listed_row_t const &row) {
                                             alignments_rows<decltype(width)::value, lanes_>(table, row, candidates, k, arrays, region, flags,
                                                                                             counters);
                                         });
}

} // namespace szs_hip

extern "C" int szs_hip_levenshtein_alignments(szs_rerank_side_t const *queries, szs_rerank_side_t const *candidates, uint64_t first_query,
                                              uint32_t const *rows, uint32_t rows_count, uint64_t const *indices, uint64_t const *starts,
                                              uint64_t const *ends, uint64_t inputs_stride, uint64_t k, uint64_t *distances,
                                              uint64_t *lengths, uint64_t outputs_stride, uint8_t *ops, uint64_t capacity, unsigned widest,
                                              void *trace, uint32_t workgroups, uint32_t *flags, unsigned long long *counters, void *stream) {
    using namespace szs_hip;
    if (!rows_count || !k) return 0;
    if (widest < 1 || widest > SZS_MYERS_SHORT_WORDS || !queries || !candidates || !distances || !lengths || !trace || !workgroups || !flags ||
        !counters || !starts != !ends || (!ops && capacity))
        return (int)hipErrorInvalidValue;
    listed_grid_t const grid = listed_one_strip_grid(k, rows_count, widest); // its tables; the grid is the trace's
    align_arrays_t const arrays = {indices, starts, ends, inputs_stride, distances, lengths, outputs_stride, ops, ops ? capacity : 0};
    u64 const region_cells = SZS_ALIGN_REGION_BYTES(widest) / sizeof(uint2);
    return listed_launch(k, [&](auto lanes) {
        hipLaunchKernelGGL(levenshtein_alignments_kernel<decltype(lanes)::value>, dim3(grid.grid < workgroups ? grid.grid : workgroups),
                           dim3(wave_size_k), grid.lds, static_cast<hipStream_t>(stream), *queries, *candidates, first_query, rows, rows_count,
                           k, arrays, static_cast<uint2 *>(trace), region_cells, grid.table_dwords, flags, counters);
    });
}

/*
 *  rerank_core.hpp - what a kernel over LISTED pairs is: the scaffold of hip/myers_rerank.hip (queries of up to 256 bytes in one
 *  bit-vector), hip/myers_rerank_strips.hip (longer queries as strips), hip/myers_fuzzy_find.hip and hip/myers_fuzzy_spans.hip.
 *  hip/myers_fuzzy_tile.hip takes the pieces - rows, widths, tables, candidates, the walk, the counters - for a grid of its own: one
 *  row and a run of consecutive candidates per workgroup.
 *
 *  - A GROUP of L = 16 / 32 / 64 lanes (the smallest that holds min(k, 64): szs_hip_rerank_lanes) serves one row - one query and
 *    the k candidates an index row names: its own Peq table in LDS (peq_layout<W, 256>), one listed candidate per lane, fetched
 *    THROUGH the index - address and length from the tape's offsets, or from a ref array in index order when the side is a callback
 *    sequence (rerank_fetch).  Rows of more than 64 candidates walk them in chunks of 64 against the same table.
 *  - A workgroup is ONE wavefront of 64 / L rows: the lanes that build a table are the lanes that read it, so there is no
 *    workgroup barrier at all, and the grid comes from the rows, not from the candidates.
 *  - The pattern is right-aligned over phantom low rows (hip/lev_myers.hip), so every row of a wavefront runs at the width W of the
 *    wavefront's longest query - a scalar choice among eight bodies (listed_at_width).  The host deals rows by descending query
 *    length: neighbours share a width.
 *  - `index < count` precedes every use of an index (listed_candidate): a bad one addresses nothing and raises a flag in pinned host
 *    memory.  Every kind of failure has a flag word of its own and every lane stores the same 1 there: what the host reads does not
 *    depend on which lane stored last.  Lanes whose text has ended, lanes of empty slots and lanes of refused indices are frozen by
 *    EXEC.
 *
 *  What differs between the kernels arrives as a template parameter or a callable - the fill word of a table, where a pattern byte
 *  lands, the stream, the column - never as a flag that says which kernel is calling.  The strips kernel keeps its own table build
 *  and text loops: it rebuilds a slice of the table per strip, and its loops park deltas at every 16th column.
 */
#pragma once
#include <type_traits>

#include "myers_core.hpp"

namespace szs_hip {

/** The bits of [from, to) that fall into word `w` (`from` differs per row of the wavefront: the rows' own phantom rows). */
__device__ __forceinline__ u32 rerank_bits_in_word(u32 from, u32 to, int w) {
    u32 const low = from > 32u * w ? from : 32u * w, high = to < 32u * w + 32u ? to : 32u * w + 32u;
    if (low >= high) return 0u;
    return (high - low == 32u ? ~0u : (1u << (high - low)) - 1u) << (low - 32u * w);
}

/** String `index` of a side, `index < side.count` checked by the caller.  False: its offsets descend, or it has 4 GiB or more. */
__device__ __forceinline__ bool rerank_fetch(szs_rerank_side_t const &side, u64 index, u64 &address, u32 &length) {
    if (side.refs) {
        szs_string_ref_t const ref = side.refs[index];
        address = ref.address, length = ref.length;
        return true;
    }
    u64 from, to;
    if (side.wide) {
        u64 const *offsets = static_cast<u64 const *>(side.offsets);
        from = offsets[index], to = offsets[index + 1];
    }
    else {
        u32 const *offsets = static_cast<u32 const *>(side.offsets);
        from = offsets[index], to = offsets[index + 1];
    }
    if (to < from || to - from > 0xFFFFFFFFull) return false;
    address = side.base + from, length = (u32)(to - from);
    return true;
}

__device__ __forceinline__ u64 wave_sum_u64(u64 value) {
#pragma unroll
    for (int offset = 32; offset >= 1; offset >>= 1) value += (u64)__shfl_xor((unsigned long long)value, offset, 64);
    return value;
}

/* ---- the row of a group -------------------------------------------------------------------------------------------------- */

/** One row as its group sees it, uniform within the group.  No row (`has_row` false): a query of no bytes, nothing is scored. */
struct listed_row_t {
    bool has_row;
    u64 row; // of the call's block: indices and outputs are addressed by it
    u64 query_address;
    u32 query_length;
};

/** The row of a group, row -> query: `row_of()` names it where the group `has_row`.  A query beyond the side, or one whose offsets
 *  descend, raises the TAPE flag; one of more than `longest_allowed` bytes the UNFIT flag (the host's job to prevent).  Either way the
 *  group has no row. */
template <typename row_of_t>
__device__ __forceinline__ listed_row_t listed_row(szs_rerank_side_t const &queries, u64 first_query, bool has_row, row_of_t row_of,
                                                   u32 longest_allowed, u32 *flags) {
    listed_row_t found = {has_row, 0, 0, 0};
    if (!found.has_row) return found;
    found.row = row_of();
    u64 const query = first_query + found.row;
    if (query >= queries.count || !rerank_fetch(queries, query, found.query_address, found.query_length))
        flags[SZS_RERANK_FLAG_TAPE] = 1u, found.has_row = false;
    else if (found.query_length > longest_allowed) flags[SZS_RERANK_FLAG_UNFIT] = 1u, found.has_row = false;
    if (!found.has_row) found.query_length = 0;
    return found;
}

/** The row in slot `slot` of `rows`: slot -> row -> query. */
__device__ __forceinline__ listed_row_t listed_row(szs_rerank_side_t const &queries, u64 first_query, u32 const *__restrict__ rows,
                                                   u32 rows_count, u64 slot, u32 longest_allowed, u32 *flags) {
    return listed_row(queries, first_query, slot < rows_count, [&]() { return rows[slot]; }, longest_allowed, flags);
}

/** The longest query of the wavefront's rows - a scalar, so one of the eight bodies runs and nothing diverges. */
__device__ __forceinline__ u32 listed_longest_query(listed_row_t const &row) {
    return (u32)__builtin_amdgcn_readfirstlane((int)wave_max_u32(row.query_length));
}

/** `body(std::integral_constant<int, W>)` for W = `words` of 1 ... 8 (more: 8): the scalar choice among the eight bodies. */
template <typename body_t>
__device__ __forceinline__ void listed_at_width(u32 words, body_t body) {
    switch (words) {
    case 1: body(std::integral_constant<int, 1>()); break;
    case 2: body(std::integral_constant<int, 2>()); break;
    case 3: body(std::integral_constant<int, 3>()); break;
    case 4: body(std::integral_constant<int, 4>()); break;
    case 5: body(std::integral_constant<int, 5>()); break;
    case 6: body(std::integral_constant<int, 6>()); break;
    case 7: body(std::integral_constant<int, 7>()); break;
    default: body(std::integral_constant<int, 8>()); break;
    }
}

/**
 *  The prologue of a kernel whose rows take ONE bit-vector (queries of at most SZS_RERANK_LONGEST_QUERY bytes): the group's row,
 *  its table among the workgroup's `tables` (`table_dwords` apart), then `body(width, table, row)` at the width of the wavefront's
 *  longest query.
 */
template <int lanes_, typename body_t>
__device__ __forceinline__ void listed_one_strip_rows(szs_rerank_side_t const &queries, u64 first_query, u32 const *__restrict__ rows,
                                                      u32 rows_count, u32 *tables, u32 table_dwords, u32 *flags, body_t body) {
    constexpr u32 groups = wave_size_k / lanes_;
    u32 const group = threadIdx.x / lanes_;
    listed_row_t const row = listed_row(queries, first_query, rows, rows_count, (u64)blockIdx.x * groups + group, SZS_RERANK_LONGEST_QUERY, flags);
    u32 const longest = listed_longest_query(row);
    u32 *const table = tables + group * table_dwords;
    listed_at_width(longest ? (longest + 31u) / 32u : 1u, [&](auto width) { body(width, table, row); });
}

/**
 *  The same prologue for a workgroup that serves MORE than one run of 64 / L rows (a grid bounded by something other than the rows:
 *  hip/myers_alignments.hip's by its trace memory): `first_slot` is the slot of the wavefront's first group, where the prologue
 *  above takes blockIdx.x x groups.  Uniform over the wavefront.
 */
template <int lanes_, typename body_t>
__device__ __forceinline__ void listed_one_strip_rows_at(szs_rerank_side_t const &queries, u64 first_query, u32 const *__restrict__ rows,
                                                         u32 rows_count, u64 first_slot, u32 *tables, u32 table_dwords, u32 *flags,
                                                         body_t body) {
    u32 const group = threadIdx.x / lanes_;
    listed_row_t const row = listed_row(queries, first_query, rows, rows_count, first_slot + group, SZS_RERANK_LONGEST_QUERY, flags);
    u32 const longest = listed_longest_query(row);
    u32 *const table = tables + group * table_dwords;
    listed_at_width(longest ? (longest + 31u) / 32u : 1u, [&](auto width) { body(width, table, row); });
}

/**
 *  The Peq table of `row` at `words_` words, built by the group's `lanes_` lanes: every dword of word w starts as `fill(w)`, then
 *  byte i of the pattern sets bit `position_of(i)` of its byte's row.  One wavefront: __syncthreads() orders its LDS traffic, no
 *  s_barrier is left.
 */
template <int words_, int lanes_, typename fill_t, typename position_of_t>
__device__ __forceinline__ void listed_table(u32 *table, listed_row_t const &row, fill_t fill, position_of_t position_of) {
    using layout = peq_layout<words_, byte_rows_k>;
    u32 const sub = threadIdx.x % lanes_;
    // dword d of the image holds word (d / (rows x chunk_words)) x chunk_words + d % chunk_words (peq_layout::dword_index)
    for (u32 i = sub; i < layout::total_dwords / 4; i += lanes_) {
        int const chunk_base = (int)((4u * i / (byte_rows_k * layout::chunk_words)) * layout::chunk_words);
        reinterpret_cast<uint4 *>(table)[i] = make_uint4(fill(chunk_base + 0 % layout::chunk_words), fill(chunk_base + 1 % layout::chunk_words),
                                                         fill(chunk_base + 2 % layout::chunk_words), fill(chunk_base + 3 % layout::chunk_words));
    }
    __syncthreads();
    u8 const *pattern = reinterpret_cast<u8 const *>(row.query_address);
    for (u32 i = sub; i < row.query_length; i += lanes_) {
        u32 const position = position_of(i);
        atomicOr(&table[layout::dword_index(pattern[i], (int)(position >> 5))], 1u << (position & 31));
    }
    __syncthreads();
}

/* ---- the candidate of a lane --------------------------------------------------------------------------------------------- */

/**
 *  The string a slot's `index` names, into `address` and `text_length`; false - and both zero - when the lane has nothing to score:
 *  an empty slot (~0: `on_empty()` writes the kernel's zeros, no string is touched), an index beyond the candidates (the INDEX flag:
 *  it is never used to address anything) or offsets that descend (the TAPE flag).
 */
template <typename on_empty_t>
__device__ __forceinline__ bool listed_candidate(szs_rerank_side_t const &candidates, u64 index, on_empty_t on_empty, u32 *flags,
                                                 u64 &address, u32 &text_length) {
    address = 0, text_length = 0;
    if (index == ~0ull) on_empty();
    else if (index >= candidates.count) flags[SZS_RERANK_FLAG_INDEX] = 1u;
    else if (!rerank_fetch(candidates, index, address, text_length)) flags[SZS_RERANK_FLAG_TAPE] = 1u, address = 0, text_length = 0;
    else return true;
    return false;
}

/**
 *  The walk of one text per lane, `length` bytes of `text` (text_stream_t, or text_stream_backward_t from the last byte down):
 *  `take(symbol, columns_taken)` per byte, the count including that byte.  Only aligned dwords that hold a byte of the text are
 *  loaded; a lane that is not `live` has `length` 0, loads nothing, and its symbols - zeros - are never scored into anything that is
 *  written.  Whole dwords that every live lane still has run unpredicated, the ragged rest predicated on the lane's own length;
 *  both loops carry one dword of look-ahead.  `keep_going()`, uniform over the wavefront, is asked once per dword: false ends the
 *  walk.
 */
template <typename stream_t, typename take_t, typename keep_going_t>
__device__ __forceinline__ void listed_walk(stream_t const &text, u32 length, bool live, take_t take, keep_going_t keep_going) {
    u32 const longest_in_wave = wave_max_u32(length);
    u32 const shortest_in_wave = ~wave_max_u32(live ? ~length : 0u); // over live lanes; none: ~0, and the longest is 0
    u32 column = 0, dword = 0, held = text.raw(0);
    bool going = keep_going();
    if (4 <= shortest_in_wave && longest_in_wave) {
        u32 ahead = text.raw(1);
        for (; going && column + 4 <= shortest_in_wave; column += 4, ++dword) {
            u32 const symbols = text.splice(held, ahead);
            held = ahead, ahead = text.raw(dword + 2);
#pragma unroll
            for (int step = 0; step < 4; ++step) take(stream_t::symbol(symbols, step), column + step + 1);
            going = keep_going();
        }
    }
    if (going && column < longest_in_wave) {
        u32 next = text.raw(dword + 1);
#pragma unroll 1
        for (; going && column < longest_in_wave; column += 4, ++dword) {
            u32 const after = text.raw(dword + 2);
            u32 const symbols = text.splice(held, next);
            held = next, next = after;
#pragma unroll
            for (int step = 0; step < 4; ++step)
                if (column + step < length) take(stream_t::symbol(symbols, step), column + step + 1);
            going = keep_going();
        }
    }
}

/* ---- the counters -------------------------------------------------------------------------------------------------------- */

/** What a lane scored: pairs, their cells and their bytes, summed over the wavefront into the call's three counters. */
struct listed_counters_t {
    u64 pairs = 0, cells = 0, bytes = 0;

    __device__ __forceinline__ void add(u32 query_length, u32 columns) {
        pairs += 1, cells += (u64)query_length * columns, bytes += (u64)query_length + columns;
    }

    /** Lane 0 adds the wavefront's sums, when there is anything to add.  `with_pairs` false: a second pass over pairs that an
     *  earlier launch has counted - cells and bytes only. */
    __device__ __forceinline__ void land(unsigned long long *counters, bool with_pairs) const {
        u64 const all_pairs = with_pairs ? wave_sum_u64(pairs) : 0, all_cells = wave_sum_u64(cells), all_bytes = wave_sum_u64(bytes);
        if (threadIdx.x != 0 || !(with_pairs ? all_pairs : all_bytes)) return;
        if (with_pairs) atomicAdd(&counters[0], (unsigned long long)all_pairs);
        atomicAdd(&counters[1], (unsigned long long)all_cells);
        atomicAdd(&counters[2], (unsigned long long)all_bytes);
    }
};

/* ---- the launch (host side) ---------------------------------------------------------------------------------------------- */

/** `launch(std::integral_constant<int, L>)` for the L = 16 / 32 / 64 lanes a row of `k` slots takes; HIP's error of the launch. */
template <typename launch_t>
inline int listed_launch(u64 k, launch_t launch) {
    unsigned const lanes = szs_hip_rerank_lanes(k);
    if (lanes == 16) launch(std::integral_constant<int, 16>());
    else if (lanes == 32) launch(std::integral_constant<int, 32>());
    else launch(std::integral_constant<int, 64>());
    return (int)hipGetLastError();
}

/** The launch of a one-strip kernel over `rows_count` rows of `k` slots whose widest query needs `widest` words: one wavefront per
 *  64 / L rows, and a table per row in dynamic LDS - at most 8 KB a row: four rows a wavefront, 32 KB a workgroup. */
struct listed_grid_t {
    u32 table_dwords, grid;
    size_t lds;
};
inline listed_grid_t listed_one_strip_grid(u64 k, u32 rows_count, unsigned widest) {
    static_assert(peq_layout<3>::total_dwords == peq_layout<4>::total_dwords && peq_layout<5>::total_dwords == peq_layout<8>::total_dwords,
                  "a table of W words fits the table of the next even chunk count");
    unsigned const groups = wave_size_k / szs_hip_rerank_lanes(k);
    u32 const table_dwords = widest == 1   ? peq_layout<1>::total_dwords
                             : widest == 2 ? peq_layout<2>::total_dwords
                             : widest <= 4 ? peq_layout<4>::total_dwords
                                           : peq_layout<8>::total_dwords;
    return {table_dwords, (u32)(((u64)rows_count + groups - 1) / groups), (size_t)groups * table_dwords * sizeof(u32)};
}

} // namespace szs_hip

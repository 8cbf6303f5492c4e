/*
 *  rerank_core.hpp - what the two rerank kernels share (hip/myers_rerank.hip: queries of up to 256 bytes in one bit-vector;
 *  hip/myers_rerank_strips.hip: longer queries as strips) and the fuzzy-find kernel (hip/myers_fuzzy_find.hip): the fetch of a string through an index, the phantom-row mask of a
 *  word, the wavefront sum of the counters.
 */
#pragma once
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

/** Dwords of one row's Peq table in a launch whose widest query needs `widest` words (a table of W words fits the table of the next
 *  even chunk count): what the one-strip kernels size their dynamic LDS by. */
inline u32 rerank_table_dwords(unsigned widest) {
    switch (widest) {
    case 1: return peq_layout<1>::total_dwords;
    case 2: return peq_layout<2>::total_dwords;
    case 3:
    case 4: return peq_layout<4>::total_dwords;
    default: return peq_layout<8>::total_dwords;
    }
}

__device__ __forceinline__ u64 wave_sum_u64(u64 value) {
#pragma unroll
    for (int offset = 32; offset >= 1; offset >>= 1) value += (u64)__shfl_xor((unsigned long long)value, offset, 64);
    return value;
}

} // namespace szs_hip

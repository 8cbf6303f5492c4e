/*
 *  myers_core.hpp - the pieces of the bit-parallel unit-cost Levenshtein kernels that more than one translation unit needs:
 *  the LDS image of the match masks, the column update on a W-word bit-vector with one carry chain, and the strip column
 *  (Hyyro's block boundary) of the kernels that spread a pattern over lanes or strips.
 *
 *  Reference semantics: levenshtein_distance_myers<char, serial>, /root/reference/include/stringzillas/similarities/serial.hpp:2073-2314
 *  (block-based there; the full-width carry chain here computes the same DP column - tests pin this).
 *  Used by hip/lev_myers.hip (one launch per width group) and hip/myers_queue.hip (one persistent launch for every width).
 */
#pragma once
#include "device_common.hpp"

namespace szs_hip {

constexpr int byte_rows_k = 256;        // Peq rows of the byte kernels: one per byte value
constexpr int rune_slots_k = 512;       // Peq rows of the rune kernels: one per slot of the open-addressing rune table
constexpr u32 rune_slot_empty_k = ~0u;  // no decoded rune has this value (4-byte sequences top out below 2^21)

/** LDS image of Peq for a W-word pattern: 16-byte rows for W >= 3 (ds_read_b128), 8 for W = 2, 4 for W = 1.
 *  A row belongs to a byte value (byte kernels) or to a slot of the rune hash table (codepoint kernels). */
template <int words_, int rows_ = byte_rows_k>
struct peq_layout {
    static constexpr int chunk_words = words_ >= 3 ? 4 : words_;             // words fetched by one LDS read
    static constexpr int chunks = (words_ + chunk_words - 1) / chunk_words;  // LDS reads per text symbol
    static constexpr int total_dwords = chunks * rows_ * chunk_words;
    /** dword index of word `w` of the mask in row `row`: [chunk][row][word in chunk] */
    __device__ static constexpr int dword_index(int row, int w) {
        return ((w / chunk_words) * rows_ + row) * chunk_words + (w % chunk_words);
    }
};

/** Slot of `rune` in the workgroup's open-addressing table, or the empty slot its probe sequence ends on - whose Peq
 *  row is all zeros, exactly the match mask of a symbol the pattern does not contain. */
__device__ __forceinline__ u32 rune_slot_hash(u32 rune) { return (rune * 2654435761u) >> 23; }
__device__ __forceinline__ u32 find_rune_slot(u32 const *keys, u32 rune) {
    u32 slot = rune_slot_hash(rune);
    for (;;) {
        u32 const key = keys[slot];
        if (key == rune || key == rune_slot_empty_k) return slot;
        slot = (slot + 1) & (rune_slots_k - 1);
    }
}

/** The match masks of `symbol`, words [first_word_, last_word_) of them: a 16-byte chunk of the row that holds none of those
 *  words is not read (myers_column's word range: with 5 or 9 words the top word is alone in its chunk). */
template <int words_, int rows_, int first_word_ = 0, int last_word_ = words_>
__device__ __forceinline__ void load_match_masks(u32 const *peq, u32 symbol, u32 (&eq)[words_]) {
    using layout = peq_layout<words_, rows_>;
    static_assert(0 <= first_word_ && first_word_ < last_word_ && last_word_ <= words_, "a word range inside the vector");
    if constexpr (layout::chunk_words == 4) {
        uint4 const *rows = reinterpret_cast<uint4 const *>(peq);
#pragma unroll
        for (int chunk = 0; chunk < layout::chunks; ++chunk) {
            if (chunk * 4 + 4 <= first_word_ || chunk * 4 >= last_word_) continue;
            uint4 const row = rows[chunk * rows_ + symbol];
            // A range that begins inside the chunk still takes it in ONE ds_read_b128 (its first word is "used" by an empty
            // statement): left to itself the compiler reads the words above `first_word_` with a ds_read2_b32 and a ds_read_b32,
            // and pays a v_or for the second address.
            if (chunk * 4 < first_word_) asm volatile("" : : "v"(row.x));
            if (chunk * 4 + 0 < words_) eq[chunk * 4 + 0] = row.x;
            if (chunk * 4 + 1 < words_) eq[chunk * 4 + 1] = row.y;
            if (chunk * 4 + 2 < words_) eq[chunk * 4 + 2] = row.z;
            if (chunk * 4 + 3 < words_) eq[chunk * 4 + 3] = row.w;
        }
    }
    else if constexpr (layout::chunk_words == 2) {
        uint2 const row = reinterpret_cast<uint2 const *>(peq)[symbol];
        eq[0] = row.x, eq[1] = row.y;
    }
    else { eq[0] = peq[symbol]; }
}

/** Does `ref` still describe string `ref.index` of its tape?  (szs_ref_guard_t, hip/kernels.h.) */
__device__ __forceinline__ bool ref_is_current(szs_ref_guard_t const &guard, int side, szs_string_ref_t const &ref) {
    if (ref.index >= guard.side[side].count) return false;
    u64 from, to;
    if (guard.side[side].wide) {
        u64 const *offsets = static_cast<u64 const *>(guard.side[side].offsets);
        from = offsets[ref.index], to = offsets[(u64)ref.index + 1];
    }
    else {
        u32 const *offsets = static_cast<u32 const *>(guard.side[side].offsets);
        from = offsets[ref.index], to = offsets[(u64)ref.index + 1];
    }
    return to >= from && to - from == ref.length && guard.side[side].base + from == ref.address;
}

/** No query boundary inside the bit-vector: the column of a single pattern (every mask below folds to nothing). */
struct single_pattern_t {};

/** Two patterns in one bit-vector (pad, q1, separator rows s0 s1, q2 from bit 0 up): per-word masks, uniform over the
 *  workgroup, held in one VGPR each (the operands of the column's v_bitop3s).  `separators` marks s0 and s1, `lower` s0 alone -
 *  the bit that EVERY row of a paired match-mask table holds.  See myers_column. */
template <int words_>
struct pattern_pair_t {
    u32 separators[words_], lower[words_];
};

/** r = f(a, b, c) bit by bit in ONE full-rate v_bitop3_b32; bit ((a << 2) | (b << 1) | c) of `table_` is f(a, b, c), i.e. the
 *  same expression over a = 0xF0, b = 0xCC, c = 0xAA.  Spelled out because LLVM, given the C expression, splits some of the
 *  column's functions in two or shares a subterm with a neighbour at the price of a v_or per word-step. */
template <int table_>
__device__ __forceinline__ u32 bitop3(u32 a, u32 b, u32 c) {
    u32 r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:%4" : "=v"(r) : "v"(a), "v"(b), "v"(c), "n"(table_));
    return r;
}

/** One column of the DP matrix: consumes the match masks of one text byte and updates the vertical delta vectors.
 *
 *  Hyyro's column is  D0 = (((Eq & VP) + VP) ^ VP) | Eq,  HP = VN | ~(D0 | VP),  HN = VP & D0,  VP' = HN << 1 | ~(X | HP << 1),
 *  VN' = HP << 1 & X  with X = Eq | VN.  HN << 1 is never shifted here, because the adder has it already: the carry OUT of bit i
 *  of `sum = (Eq & VP) + VP` is maj(Eq_i & VP_i, VP_i, c_i) = VP_i & (Eq_i | c_i), and since VP & VN = 0 that is HN_i = VP_i & D0_i.
 *  So HN << 1 is the vector of carries INTO each bit, sum ^ (Eq & VP) ^ VP - across words too: bit 0 of word w takes the addc's
 *  carry.  With K = Eq | VP, computed before the add:
 *      HNs = sum ^ K ^ Eq            HP = VN | ~(sum | K)     (D0 | VP == sum | K: D0 itself is not needed)
 *  Per word-step: 7 full-rate logic ops (Eq & VP, K, X, HNs, HP, VP', VN'), the addc and ONE v_alignbit (HP << 1) - 9.5 VALU
 *  with what surrounds them, two of them half-rate where the older column (both shifts) had three.
 *
 *  With two patterns in the vector (pattern_pair_t) the separator rows start with VP = VN = 0 and stay so, at no instruction:
 *  every mask is the third operand of a v_bitop3.  X~ = Eq | VN | Msep replaces X; VN' = HPs & X~ & ~Msep; and every Peq row
 *  holds the s0 bit, which K* = (Eq | VP) & ~Ms0 drops again: `Eq = 1, K* = 0` then happens at s0 and nowhere else (Eq is part
 *  of K on every other row), and HNs = (sum ^ K* ^ Eq) & ~(Eq & ~K*) is 0 there - q1's top row hands its carry to nobody.
 *  The sum never sees the bit (Eq & VP, VP = 0 at s0): s0 swallows the carry, s1 sees none and - sum = K* = 0 - gives q2's
 *  first row HPs = 1, HNs = 0: exactly DP row zero, as bit 0 of the vector gets it.
 *
 *  A word range [first_word_, last_word_) updates those words alone; the others are neither read nor written (hip/corner_cut.h
 *  says in which columns no path of the distance needs them).  A top word left out keeps its state - before its first update
 *  VP all ones, VN zero: "from the row below, straight down", a real path - and later joins the chain with the addc's carry and the
 *  HP bit of the word below, as ever.  With a bottom word left out the chain starts at `first_word_` with no carry and a 1 entering
 *  bit 0 of HPs: a horizontal delta of +1 on the frozen word's top row, "one more insertion", a real path too - what bit 0 of word
 *  0 gets, and Hyyro's block boundary (myers_strip_column with hp_in = 1, hn_in = 0).  len(text) + popcount(VP) - popcount(VN) over
 *  ALL words still is the distance: the frozen word's deltas and the +1 per column since then telescope to the same sum. */
template <int words_, typename boundary_t = single_pattern_t, bool materialise_ = true, bool spelled_carries_ = true, int first_word_ = 0,
          int last_word_ = words_>
__device__ __forceinline__ void myers_column(u32 (&vp)[words_], u32 (&vn)[words_], u32 const (&eq)[words_],
                                             boundary_t const &boundary = {}) {
    constexpr bool paired = !std::is_same<boundary_t, single_pattern_t>::value;
    static_assert(spelled_carries_ || !paired, "a pair's HNs is not a function the compiler finds by itself");
    static_assert(0 <= first_word_ && first_word_ < last_word_ && last_word_ <= words_, "a word range inside the vector");
    u32 carry = 0, hp_below = 0;
#pragma unroll
    for (int w = first_word_; w < last_word_; ++w) {
        u32 xv, kept, hn_shifted;
        if constexpr (paired) {
            xv = bitop3<0xfe>(eq[w], vn[w], boundary.separators[w]);   // Eq | VN | Msep
            kept = bitop3<0x54>(eq[w], vp[w], boundary.lower[w]);      // (Eq | VP) & ~Ms0
        }
        else
            xv = eq[w] | vn[w], kept = eq[w] | vp[w];
        u32 carry_out;
        u32 const sum = __builtin_addc(eq[w] & vp[w], vp[w], carry, &carry_out); // one link of the W-word carry chain
        carry = carry_out;
        if constexpr (paired) hn_shifted = bitop3<0x94>(sum, kept, eq[w]);      // (sum ^ K* ^ Eq) & ~(Eq & ~K*)
        else if constexpr (spelled_carries_) hn_shifted = bitop3<0x96>(sum, kept, eq[w]); // sum ^ K ^ Eq: the carries into every bit
        else hn_shifted = sum ^ kept ^ eq[w]; // (left to the compiler, which spends a v_xor more per word-step on it: hip/myers_rerank.hip
                                              // pays that full-rate op to keep its registers)
        u32 const hp = bitop3<0xf1>(vn[w], sum, kept);                          // VN | ~(sum | K)
        // Shift HP up by one row; bit 0 of word 0 takes the constant `+1` of DP row zero (and so does the first word of a range).
        u32 const hp_shifted = w == first_word_ ? ((hp << 1) | 1u) : __builtin_amdgcn_alignbit(hp, hp_below, 31);
        hp_below = hp;
        vp[w] = bitop3<0xf1>(hn_shifted, xv, hp_shifted);                       // HNs | ~(X | HPs)
        if constexpr (paired) vn[w] = bitop3<0x40>(hp_shifted, xv, boundary.separators[w]); // HPs & X~ & ~Msep
        else vn[w] = hp_shifted & xv;
        // Both new vectors materialised here: without this LLVM folds VP' into the next column's `Eq & VP` and then keeps
        // `xv | hp_shifted` AND VP' alive - one v_or more per word-step (and scratch in the fused kernel).  Not for one word,
        // nor where `materialise_` is false (the tiny-token kernel): there the barrier only splits the v_lshl_or_b32 of
        // `(hp << 1) | 1` into a shift and an or.
        if constexpr (materialise_ && words_ > 1) asm("" : "+v"(vp[w]), "+v"(vn[w]));
    }
}

/** One column of the SEMI-GLOBAL matrix (free start in the text: DP row zero is all zeros): myers_column with nothing entering
 *  bit 0, and the horizontal pair of the vector's LAST row - bit 31 of word W - 1, taken before the shift - coming back as
 *  hp | hn << 1: the change of the bottom-row score in this column (hip/myers_fuzzy_find.hip). */
template <int words_>
__device__ __forceinline__ u32 myers_infix_column(u32 (&vp)[words_], u32 (&vn)[words_], u32 const (&eq)[words_]) {
    u32 carry = 0, hp_below = 0, hn_below = 0;
#pragma unroll
    for (int w = 0; w < words_; ++w) {
        u32 const xv = eq[w] | vn[w];
        u32 carry_out;
        u32 const sum = __builtin_addc(eq[w] & vp[w], vp[w], carry, &carry_out);
        carry = carry_out;
        u32 const d0 = (sum ^ vp[w]) | eq[w];
        u32 const hp = vn[w] | ~(d0 | vp[w]);
        u32 const hn = vp[w] & d0;
        u32 const hp_shifted = w == 0 ? (hp << 1) : __builtin_amdgcn_alignbit(hp, hp_below, 31);
        u32 const hn_shifted = w == 0 ? (hn << 1) : __builtin_amdgcn_alignbit(hn, hn_below, 31);
        hp_below = hp, hn_below = hn;
        vp[w] = hn_shifted | ~(xv | hp_shifted);
        vn[w] = hp_shifted & xv;
        if constexpr (words_ > 1) asm("" : "+v"(vp[w]), "+v"(vn[w])); // as in myers_column: both new vectors materialised
    }
    return (hp_below >> 31) | ((hn_below >> 31) << 1);
}

/** One column of the GLOBAL matrix whose bottom-row score is followed (D[0][j] = j: every prefix of the text against the whole
 *  pattern): myers_column's `+1` entering bit 0, and the horizontal pair of the vector's LAST row coming back as hp | hn << 1, as in
 *  myers_infix_column - myers_strip_column(vp, vn, eq, 1, 0) with myers_column's materialisation (hip/myers_fuzzy_spans.hip). */
template <int words_>
__device__ __forceinline__ u32 myers_prefix_column(u32 (&vp)[words_], u32 (&vn)[words_], u32 const (&eq)[words_]) {
    u32 carry = 0, hp_below = 0, hn_below = 0;
#pragma unroll
    for (int w = 0; w < words_; ++w) {
        u32 const xv = eq[w] | vn[w];
        u32 carry_out;
        u32 const sum = __builtin_addc(eq[w] & vp[w], vp[w], carry, &carry_out);
        carry = carry_out;
        u32 const d0 = (sum ^ vp[w]) | eq[w];
        u32 const hp = vn[w] | ~(d0 | vp[w]);
        u32 const hn = vp[w] & d0;
        u32 const hp_shifted = w == 0 ? ((hp << 1) | 1u) : __builtin_amdgcn_alignbit(hp, hp_below, 31);
        u32 const hn_shifted = w == 0 ? (hn << 1) : __builtin_amdgcn_alignbit(hn, hn_below, 31);
        hp_below = hp, hn_below = hn;
        vp[w] = hn_shifted | ~(xv | hp_shifted);
        vn[w] = hp_shifted & xv;
        if constexpr (words_ > 1) asm("" : "+v"(vp[w]), "+v"(vn[w])); // as in myers_column: both new vectors materialised
    }
    return (hp_below >> 31) | ((hn_below >> 31) << 1);
}

/** myers_prefix_column that also hands out the column's TRACE (hip/myers_alignments.hip): `vp` leaves as VP',
 *  bit i set iff D[i][j] = D[i-1][j] + 1, and `diagonal_zero` is the TRUE diagonal-zero vector D0 | VN with VN taken before the
 *  update, bit i set iff D[i][j] = D[i-1][j-1].  The local `d0` below lacks the VN term: HP and HN do not need it (VN is or-ed into
 *  HP, and VP & VN = 0 keeps it out of HN), a traceback does - where VN is set the cell equals its diagonal neighbour whatever Eq
 *  says. */
template <int words_>
__device__ __forceinline__ u32 myers_prefix_column_traced(u32 (&vp)[words_], u32 (&vn)[words_], u32 const (&eq)[words_],
                                                          u32 (&diagonal_zero)[words_]) {
    u32 carry = 0, hp_below = 0, hn_below = 0;
#pragma unroll
    for (int w = 0; w < words_; ++w) {
        u32 const xv = eq[w] | vn[w];
        u32 carry_out;
        u32 const sum = __builtin_addc(eq[w] & vp[w], vp[w], carry, &carry_out);
        carry = carry_out;
        u32 const d0 = (sum ^ vp[w]) | eq[w];
        diagonal_zero[w] = d0 | vn[w];
        u32 const hp = vn[w] | ~(d0 | vp[w]);
        u32 const hn = vp[w] & d0;
        u32 const hp_shifted = w == 0 ? ((hp << 1) | 1u) : __builtin_amdgcn_alignbit(hp, hp_below, 31);
        u32 const hn_shifted = w == 0 ? (hn << 1) : __builtin_amdgcn_alignbit(hn, hn_below, 31);
        hp_below = hp, hn_below = hn;
        vp[w] = hn_shifted | ~(xv | hp_shifted);
        vn[w] = hp_shifted & xv;
        if constexpr (words_ > 1) asm("" : "+v"(vp[w]), "+v"(vn[w])); // as in myers_column: both new vectors materialised
    }
    return (hp_below >> 31) | ((hn_below >> 31) << 1);
}

/** One column of one strip; `hp_in` / `hn_in` are the deltas entering the strip's first row as 0 / 1 values; the bit pair
 *  leaving its last row comes back as hp | hn << 1. */
template <int words_>
__device__ __forceinline__ u32 myers_strip_column(u32 (&vp)[words_], u32 (&vn)[words_], u32 const (&eq)[words_], u32 hp_in,
                                                  u32 hn_in) {
    u32 carry = 0, hp_below = 0, hn_below = 0;
#pragma unroll
    for (int w = 0; w < words_; ++w) {
        u32 const xv = eq[w] | vn[w];
        u32 const eq_in = w == 0 ? (eq[w] | hn_in) : eq[w]; // a -1 entering from above acts like a match in the first row
        u32 carry_out;
        u32 const sum = __builtin_addc(eq_in & vp[w], vp[w], carry, &carry_out);
        carry = carry_out;
        u32 const d0 = (sum ^ vp[w]) | eq_in;
        u32 const hp = vn[w] | ~(d0 | vp[w]);
        u32 const hn = vp[w] & d0;
        u32 const hp_shifted = w == 0 ? ((hp << 1) | hp_in) : __builtin_amdgcn_alignbit(hp, hp_below, 31);
        u32 const hn_shifted = w == 0 ? ((hn << 1) | hn_in) : __builtin_amdgcn_alignbit(hn, hn_below, 31);
        hp_below = hp, hn_below = hn;
        vp[w] = hn_shifted | ~(xv | hp_shifted);
        vn[w] = hp_shifted & xv;
    }
    return (hp_below >> 31) | ((hn_below >> 31) << 1);
}

} // namespace szs_hip

/*
 *  corner_cut.h - which text columns of the short Myers bodies (hip/lev_myers.hip: myers_workgroup) may leave the TOP or the
 *  BOTTOM word of the bit-vector untouched, in plain C that the scoring workgroups and the host (szs_rocm_corner_cut_probe)
 *  both compile: one text, one arithmetic.
 *
 *  A query of m symbols (rows i = 1 ... m) against a text of n (columns j = 1 ... n), k = max(m, n): the distance is at most k,
 *  and a path through cell (i, j) costs at least |j - i| + |(n - m) - (j - i)|, so only cells with -L <= j - i <= U lie on a path
 *  of cost <= k:
 *
 *      L = floor((k - n + m) / 2)      U = floor((k + n - m) / 2)
 *
 *  Cells outside that band may hold the cost of ANY real edit path instead of the cheapest one: every value computed from
 *  them is still the cost of a real path, and the cells of an optimal path - all inside - still see exact predecessors.
 *
 *  The vector, from bit 0 up: `pad` phantom rows, the first (or only) query, and for a pair two separator rows and the second
 *  query; W words.  Columns are counted from 0: the column at index c is DP column j = c + 1.
 *
 *      head_until   columns c < head_until may skip word W - 1.  The word's lowest row is row i_low = 32 (W - 1) - base + 1 of the
 *                   query that owns it (base: that query's first vector row), and (i_low, j) is below the band while
 *                   j < i_low - L: head_until = max(0, i_low - L - 1).  L never grows with n: the SHORTEST text of a wavefront
 *                   gives the value safe for all of its lanes.  0 when the word holds a row that is not that query's.
 *      late_from    columns c >= late_from may skip word 0.  Its highest row is row i_top = 32 - pad of the first query, and
 *                   (i_top, j) is above the band once j > i_top + U: late_from = max(0, i_top + U).  U never shrinks with n: the
 *                   LONGEST text of the wavefront.  Never when the word holds a separator row or a row of the second query.
 *
 *  Vectors of fewer than three words have no phases: their two end words are all they have.
 *  Includes nothing; the includer may define SZS_CORNER_CUT_FN (the device: `__host__ __device__ static inline`).
 */
#ifndef SZS_CORNER_CUT_H_
#define SZS_CORNER_CUT_H_

#ifndef SZS_CORNER_CUT_FN
#define SZS_CORNER_CUT_FN static inline
#endif

#define SZS_CORNER_CUT_NEVER 0xFFFFFFFFu /* a `late_from` no column reaches */
#define SZS_CORNER_CUT_WORDS_LEAST 3u    /* the narrowest vector with phases */

/** L: how far below the main diagonal a path of cost <= max(m, n) can run.  floor((max(m, n) - n + m) / 2), overflow-free. */
SZS_CORNER_CUT_FN unsigned szs_corner_band_below(unsigned m, unsigned n) { return n >= m ? m / 2u : m - (n + 1u) / 2u; }

/** U: how far above it.  floor((max(m, n) + n - m) / 2), overflow-free. */
SZS_CORNER_CUT_FN unsigned szs_corner_band_above(unsigned m, unsigned n) { return n >= m ? n - (m + 1u) / 2u : n / 2u; }

/**
 *  The two phase bounds of a `words`-word vector holding `first_length` rows and, when `paired`, two separator rows and
 *  `second_length` rows above them, for texts of `n_short` ... `n_long` symbols.  A layout that does not fit has no phases.
 */
SZS_CORNER_CUT_FN void szs_corner_cut(unsigned first_length, unsigned second_length, int paired, unsigned words, unsigned n_short,
                                      unsigned n_long, unsigned *head_until, unsigned *late_from) {
    unsigned const used_rows = paired ? first_length + second_length + 2u : first_length;
    *head_until = 0u, *late_from = SZS_CORNER_CUT_NEVER;
    if (words < SZS_CORNER_CUT_WORDS_LEAST || used_rows > 32u * words) return;
    {
        unsigned const pad = 32u * words - used_rows, top_word_row = 32u * (words - 1u);
        unsigned const base = paired ? pad + first_length + 2u : pad; /* first vector row of the query that owns the top word */
        unsigned const top_length = paired ? second_length : first_length;
        if (base <= top_word_row) {
            unsigned const i_low = top_word_row - base + 1u, below = szs_corner_band_below(top_length, n_short);
            *head_until = i_low > below + 1u ? i_low - below - 1u : 0u;
        }
        if (pad + first_length >= 32u) { /* word 0: phantom rows and rows of the first query, nothing else */
            unsigned const above = szs_corner_band_above(first_length, n_long);
            if (pad <= 32u) *late_from = above <= SZS_CORNER_CUT_NEVER - 32u ? above + (32u - pad) : SZS_CORNER_CUT_NEVER;
            else *late_from = above > pad - 32u ? above - (pad - 32u) : 0u;
        }
    }
}

#endif /* SZS_CORNER_CUT_H_ */

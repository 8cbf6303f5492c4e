"""The DP corners no path can reach (csrc/hip/corner_cut.h; hip/myers_core.hpp: myers_column's word range; hip/lev_myers.hip: the head
and late loops of myers_workgroup) - no GPU.

A query of m rows against a text of n columns, k = max(m, n): a path through cell (i, j) costs at least |j - i| + |(n - m) - (j - i)|,
so every path of cost <= k stays inside -L <= j - i <= U with L = (k - n + m) // 2 and U = (k + n - m) // 2.  The kernel leaves the TOP
word of the bit-vector alone in the columns c < head_until, and the BOTTOM word in the columns c >= late_from (columns counted from 0).

A word-wise model of exactly the kernel's column (tests/test_carry_column_model.py's formulas) over a word range, driven by the two
bounds that `szs_rocm_corner_cut_probe` gives - the header the kernel compiles - and scored against the oracle: with the bounds used
column by column (the tightest band they allow), and as the kernel's loops use them (8 columns an iteration, handing over at iteration
boundaries; 4 in the ragged tail).
"""
import random
from collections import defaultdict

import numpy as np
import pytest

from stringzilla_amd import _abi

WORD = 0xFFFFFFFF
NEVER = _abi.CORNER_CUT_NEVER
QUERY_LENGTHS = (65, 95, 96, 97, 128, 129, 160, 255, 256)
ALPHABETS = (b"a", b"ab", bytes(range(32, 127)))  # 1, 2 and 95 letters
OUTSIDE = bytes(range(1, 32))  # letters no query holds
BATCH = 8  # text columns of one iteration of the head, main and late loops (SZS_MYERS_SHORT_TEXT_DWORDS = 2)


def bits_in_word(low_bit, high_bit, w):
    low, high = max(low_bit, 32 * w), min(high_bit, 32 * w + 32)
    if low >= high:
        return 0
    return (WORD if high - low == 32 else (1 << (high - low)) - 1) << (low - 32 * w)


def range_column(vp, vn, eq, separators, s0, first_word, last_word):
    """myers_column<..., first_word, last_word>: words outside the range are neither read nor written; the first word of the range takes
    no carry and a 1 into bit 0 of HP << 1."""
    carry, hp_below = 0, 0
    for w in range(first_word, last_word):
        xv = eq[w] | vn[w] | separators[w]
        total = (eq[w] & vp[w]) + vp[w] + carry
        total, carry = total & WORD, total >> 32
        k = (eq[w] | vp[w]) & ~s0[w] & WORD
        hn_shifted = (total ^ k ^ eq[w]) & ~(eq[w] & ~k) & WORD
        hp = (vn[w] | ~(total | k)) & WORD
        hp_shifted = ((hp << 1) | (1 if w == first_word else hp_below >> 31)) & WORD
        hp_below = hp
        vp[w] = (hn_shifted | ~(xv | hp_shifted)) & WORD
        vn[w] = hp_shifted & xv & ~separators[w] & WORD


def band(m, n):
    k = max(m, n)
    return (k - n + m) // 2, (k + n - m) // 2


def ranges_of(columns, words, head_until, late_from, n_short, as_built):
    """The word range of every text column of one lane.  `as_built`: myers_workgroup's loops for a wavefront whose shortest text has
    `n_short` columns; else the bounds column by column."""
    if not as_built:
        return [(0, words - 1) if c < head_until else (1, words) if c >= late_from else (0, words) for c in range(columns)]
    out, column = [], 0
    if BATCH <= n_short:
        while column + BATCH <= min(head_until, n_short):
            out += [(0, words - 1)] * BATCH
            column += BATCH
        while column + BATCH <= n_short and column < late_from:
            out += [(0, words)] * BATCH
            column += BATCH
        while column + BATCH <= n_short:
            out += [(1, words)] * BATCH
            column += BATCH
    while column < columns:  # the ragged tail: a dword at a time, the range decided at its first column
        out += [(1, words) if column >= late_from else (0, words)] * 4
        column += 4
    return out[:columns]


class Vector:
    """The layout of myers_workgroup: `pad` phantom rows, the first query, and for a pair two separator rows and the second query."""

    def __init__(self, first, second, words):
        self.words, self.first, self.second = words, first, second
        used = len(first) + (len(second) + 2 if second is not None else 0)
        self.pad = 32 * words - used
        assert self.pad >= 0
        self.second_row = self.pad + len(first) + 2
        if second is not None:
            self.separators = [bits_in_word(self.second_row - 2, self.second_row, w) for w in range(words)]
            self.s0 = [bits_in_word(self.second_row - 2, self.second_row - 1, w) for w in range(words)]
        else:
            self.separators = self.s0 = [0] * words
        blank = list(self.s0)  # a pair: every row of the table holds the s0 bit
        self.peq = defaultdict(lambda: blank)
        for base, string in ((self.pad, first), (self.second_row, second or b"")):
            for i, c in enumerate(string):
                if c not in self.peq:
                    self.peq[c] = list(blank)
                self.peq[c][(base + i) >> 5] |= 1 << ((base + i) & 31)

    def bounds(self, n_short, n_long):
        return _abi.corner_cut_probe(len(self.first), None if self.second is None else len(self.second), self.words, n_short, n_long)

    def distances(self, text, n_short, n_long, as_built):
        """One lane of a wavefront whose texts have n_short ... n_long columns.  (first distance, second distance or None, word-steps skipped)"""
        words = self.words
        assert n_short <= len(text) <= n_long
        head_until, late_from = self.bounds(n_short, n_long)
        vp = [bits_in_word(self.pad, 32 * words, w) & ~self.separators[w] for w in range(words)]
        vn = [0] * words
        skipped = 0
        for c, (first_word, last_word) in zip(text, ranges_of(len(text), words, head_until, late_from, n_short, as_built)):
            range_column(vp, vn, self.peq[c], self.separators, self.s0, first_word, last_word)
            skipped += words - (last_word - first_word)
        assert not any(p & n for p, n in zip(vp, vn))
        count = lambda vector, low, high: sum(bin(vector[w] & bits_in_word(low, high, w)).count("1") for w in range(words))
        low, high = self.pad, self.pad + len(self.first)
        one = len(text) + count(vp, low, high) - count(vn, low, high)
        if self.second is None:
            assert one == len(text) + sum(bin(p).count("1") - bin(n).count("1") for p, n in zip(vp, vn))  # the kernel's sum: all words
            return one, None, skipped
        return one, len(text) + count(vp, self.second_row, 32 * words) - count(vn, self.second_row, 32 * words), skipped


def _letters(rng, count, alphabet):
    return bytes(rng.choice(alphabet) for _ in range(count))


def _slack(rng, length):
    """(n_short, n_long) of the wavefront a text of `length` sits in: up to 6 away on either side, both tight one time in four."""
    if rng.random() < 0.25:
        return length, length
    return max(0, length - rng.randint(0, 6)), length + rng.randint(0, 6)


def adversarial(query, rng):
    """Texts whose only optimal paths run along the band's edges, one step inside and two (m = n: L = U = m // 2): the query without its
    first `a` letters and `a` foreign ones behind it (the path leaves row zero `a` rows down), the mirror image (it reaches the last row
    `a` columns early); then d = k exactly, and d = 0."""
    m = len(query)
    below, above = band(m, m)
    texts = []
    for a in (below - 2, below - 1, below):
        texts.append(query[a:] + _letters(rng, a, OUTSIDE))
    for a in (above - 2, above - 1, above):
        texts.append(_letters(rng, a, OUTSIDE) + query[: m - a])
    texts += [_letters(rng, n, OUTSIDE) for n in (m - 7, m, m + 9)]  # all different
    texts.append(query)
    return texts


@pytest.mark.parametrize("length", QUERY_LENGTHS)
def test_single_queries_score_what_the_oracle_scores(oracle, length):
    """Texts of 1 ... 300 bytes over each alphabet, and the adversarial family; the vector at its own width and one word wider (either
    pad an extra word allows); the wavefront's shortest and longest text up to 6 columns away from this one."""
    rng = random.Random(length)
    skipped = 0
    for alphabet in ALPHABETS:
        query = _letters(rng, length, alphabet)
        texts = [_letters(rng, n, alphabet) for n in range(1, 301)]
        # (edited copies, rotations, prefixes and suffixes: texts CLOSE to the query, whose paths hug the diagonal and its parallels)
        for _ in range(12):
            cut, shift = rng.randint(0, length), rng.randint(1, length - 1)
            texts += [query[:cut], query[cut:], query[shift:] + query[:shift],
                      bytes(c if rng.random() < 0.9 else rng.choice(alphabet) for c in query)]
        texts += adversarial(query, rng)
        expected = oracle.levenshtein([query], texts)
        for extra in (0, 1):
            vector = Vector(query, None, (length + 31) // 32 + extra)
            for j, text in enumerate(texts):
                n_short, n_long = _slack(rng, len(text))
                for as_built in (False, True):
                    got, _, saved = vector.distances(text, n_short, n_long, as_built)
                    assert got == int(expected[0, j]), (length, extra, len(alphabet), len(text), n_short, n_long, as_built, got)
                    skipped += saved
    assert skipped  # (the phases were not empty)


# (first length, second length, words): where the separator rows sit, and which end word has a phase
PAIRS = {
    "separator_in_word_1": (40, 150, 6),          # no phantom row, s0 at bit 40: both phases
    "separator_in_a_middle_word": (140, 120, 9),  # s0 at bit 166: word 5 of 9
    "separator_in_word_W_minus_2": (240, 38, 9),  # s0 at bit 248: word 7, the top word all the second query's
    "separator_in_the_top_word": (160, 20, 6),    # s0 at bit 170: word 5 of 6 - head_until must be 0
    "separator_in_word_0": (10, 170, 6),          # pad + m1 = 20 < 32, s0 at bit 20 - no late phase
    "ten_words": (159, 159, 10),                  # no phantom row, s0 on bit 31 of word 4
    "extra_word": (100, 90, 7),                   # pad 32: word 0 all phantom rows
}


@pytest.mark.parametrize("case", sorted(PAIRS))
def test_pairs_score_what_the_oracle_scores(oracle, case):
    l1, l2, words = PAIRS[case]
    rng = random.Random(case)
    pad = 32 * words - (l1 + l2 + 2)
    s0_word = (pad + l1) >> 5
    assert pad >= 0
    assert {"separator_in_word_1": s0_word == 1, "separator_in_a_middle_word": 1 < s0_word < words - 2,
            "separator_in_word_W_minus_2": s0_word == words - 2, "separator_in_the_top_word": s0_word == words - 1,
            "separator_in_word_0": s0_word == 0 and pad + l1 < 32, "ten_words": words == 10, "extra_word": pad >= 32}[case]
    for alphabet in ALPHABETS:
        first, second = _letters(rng, l1, alphabet), _letters(rng, l2, alphabet)
        vector = Vector(first, second, words)
        texts = [_letters(rng, n, alphabet) for n in range(0, 301, 3)] + adversarial(first, rng) + adversarial(second, rng)
        expected = oracle.levenshtein([first, second], texts)
        for j, text in enumerate(texts):
            n_short, n_long = _slack(rng, len(text))
            head_until, late_from = vector.bounds(n_short, n_long)
            if case == "separator_in_the_top_word":
                assert head_until == 0
            if case == "separator_in_word_0":
                assert late_from == NEVER
            for as_built in (False, True):
                one, two, _ = vector.distances(text, n_short, n_long, as_built)
                assert (one, two) == (int(expected[0, j]), int(expected[1, j])), (case, len(text), n_short, n_long, as_built, one, two)


def test_a_word_left_out_may_rejoin_the_chain(oracle):
    """Inside the columns where an end word MAY be left out, any mixture of leaving it out and updating it is exact: the tail of a
    wavefront whose texts end below `head_until` runs at full width, a build with the per-dword loop between the late loop and the tail
    (SZS_MYERS_MID_LOOP) goes back to full width after the late loop, and a frozen bottom word that is updated again resumes from
    "insertions since the freeze" - a real path."""
    rng = random.Random(11)
    for length, second_length, words in ((128, None, 4), (160, None, 5), (97, None, 5), (100, 88, 6), (140, 120, 9)):
        first = _letters(rng, length, ALPHABETS[2])
        second = None if second_length is None else _letters(rng, second_length, ALPHABETS[2])
        vector = Vector(first, second, words)
        texts = adversarial(first, rng) + (adversarial(second, rng) if second else []) + [_letters(rng, n, ALPHABETS[2]) for n in (40, 130, 200, 300)]
        expected = oracle.levenshtein([first] + ([second] if second else []), texts)
        for j, text in enumerate(texts):
            head_until, late_from = vector.bounds(len(text), len(text))
            for _ in range(4):
                vp = [bits_in_word(vector.pad, 32 * words, w) & ~vector.separators[w] for w in range(words)]
                vn = [0] * words
                for c, letter in enumerate(text):
                    leave_out = rng.random() < 0.6
                    first_word, last_word = (0, words - 1) if c < head_until and leave_out else (1, words) if c >= late_from and leave_out else (0, words)
                    range_column(vp, vn, vector.peq[letter], vector.separators, vector.s0, first_word, last_word)
                count = lambda bits, low, high: sum(bin(bits[w] & bits_in_word(low, high, w)).count("1") for w in range(words))
                rows = [(vector.pad, vector.pad + length)] + ([(vector.second_row, 32 * words)] if second else [])
                got = [len(text) + count(vp, low, high) - count(vn, low, high) for low, high in rows]
                assert got == [int(expected[q, j]) for q in range(len(rows))], (length, second_length, len(text), got)


def test_the_bounds_are_the_band_of_the_end_words():
    """The probe against the arithmetic of the issue, spelled out in Python: singles and pairs, extra pad words, any text lengths."""
    rng = random.Random(5)
    for _ in range(20000):
        words = rng.randint(1, 10)
        paired = rng.random() < 0.5
        room = 32 * words - (2 if paired else 0)
        l1 = rng.randint(0, room)
        l2 = rng.randint(0, room - l1) if paired else None
        if rng.random() < 0.5:  # the layouts the kernels build: less than a word of phantom rows
            l1 = max(l1, room - (l2 or 0) - 31)
        n_short = rng.choice((rng.randint(0, 330), rng.randint(0, 40)))
        n_long = n_short + rng.choice((0, rng.randint(0, 12), rng.randint(0, 300)))
        pad = room - l1 - (l2 or 0)
        head_until, late_from = 0, NEVER
        if words >= 3:
            base, m = (pad + l1 + 2, l2) if paired else (pad, l1)
            if base <= 32 * (words - 1):
                i_low = 32 * (words - 1) - base + 1
                head_until = max(0, i_low - band(m, n_short)[0] - 1)
            if pad + l1 >= 32:
                late_from = max(0, 32 - pad + band(l1, n_long)[1])
        assert _abi.corner_cut_probe(l1, l2, words, n_short, n_long) == (head_until, late_from), (l1, l2, words, n_short, n_long)


def test_the_bounds_move_the_safe_way():
    rng = random.Random(6)
    for _ in range(4000):
        words = rng.randint(1, 10)
        paired = rng.random() < 0.5
        room = 32 * words - (2 if paired else 0)
        l2 = rng.randint(0, min(room, 160)) if paired else None
        l1 = rng.randint(max(0, room - (l2 or 0) - rng.choice((31, 63))), room - (l2 or 0))
        lengths = sorted(rng.randint(0, 330) for _ in range(3))
        heads = [_abi.corner_cut_probe(l1, l2, words, n, lengths[2])[0] for n in lengths]
        lates = [_abi.corner_cut_probe(l1, l2, words, lengths[0], n)[1] for n in lengths]
        assert heads == sorted(heads), (l1, l2, words, lengths, heads)  # head_until never grows when n_short shrinks
        assert lates == sorted(lates), (l1, l2, words, lengths, lates)  # late_from never shrinks when n_long grows
        for n_short in lengths:
            head_until, late_from = _abi.corner_cut_probe(l1, l2, words, n_short, lengths[2])
            if words < 3:
                assert (head_until, late_from) == (0, NEVER)
            assert head_until <= late_from, (l1, l2, words, n_short, lengths[2], head_until, late_from)


def test_a_layout_that_does_not_fit_is_refused():
    with pytest.raises(_abi.StringZillasError):
        _abi.corner_cut_probe(97, None, 3, 10, 10)
    with pytest.raises(_abi.StringZillasError):
        _abi.corner_cut_probe(60, 35, 3, 10, 10)  # 60 + 35 + 2 rows
    with pytest.raises(_abi.StringZillasError):
        _abi.corner_cut_probe(96, None, 3, 11, 10)  # the shortest text longer than the longest


def test_the_phases_are_not_empty_on_the_headline_batch():
    """The model batch of tests/test_pair_rule_host.py (1024 query lengths U[96,160], numpy default_rng(2)), paired by the rule the
    sorter chooses, against 1024 candidate lengths of the same distribution, sorted and taken in wavefronts of 64 as the launch takes
    them: the share of word-steps that the loops as built (8 columns an iteration, one end word a side) leave out.

    The interval is reasoned, not read off the code.  A single of m = n = 128 in 4 words skips the top word for 96 - 64 - 1 = 31 columns
    and the bottom one from column 32 + 64 on: 3 + 4 iterations of 16, a quarter of the word-steps of those iterations, 11 % in all.  A
    paired vector has one cuttable corner per query where a single has two, twice the words, and the corner of a query of ~128 rows
    covers at most 64 columns of ~128: at most (64 / 128) / 9 = 5.6 % a side, 11 % for both if no column were lost to the 8-column
    grain, to the rows of the end words that reach into the band (the corner is a triangle: on average half of those 64 columns) and
    to the spread of a wavefront's lengths.  Half of the bound, less one iteration in eight a side: 3 % ... 7 %."""
    lengths = np.random.default_rng(2).integers(96, 161, 1024)
    rule, total_words, pairs = _abi.pair_rule_probe(lengths)
    ranked = sorted((int(x) for x in lengths), reverse=True)
    texts = sorted(int(x) for x in np.random.default_rng(3).integers(96, 161, 1024))
    waves = [texts[i:i + 64] for i in range(0, len(texts), 64)]
    words_of = lambda length: (length + 31) // 32 if length else 1
    steps = skipped = slot_words = 0
    for a, b in pairs:
        first, second = ranked[int(a)], (ranked[int(b)] if b >= 0 else None)
        shared = (first + second + 2 + 31) // 32 if second is not None else None
        if second is not None and shared <= min(10, words_of(first) + words_of(second)):
            vectors = [(first, second, shared)]
        else:
            vectors = [(length, None, words_of(length)) for length in (first, second) if length is not None]
        for l1, l2, words in vectors:
            slot_words += words
            for wave in waves:
                head_until, late_from = _abi.corner_cut_probe(l1, l2, words, wave[0], wave[-1])
                # (the loops know the wavefront's shortest text alone: a lane's ranges are the longest lane's, cut at its own length)
                ranges = ranges_of(wave[-1], words, head_until, late_from, wave[0], as_built=True)
                left_out = np.cumsum([0] + [words - (last_word - first_word) for first_word, last_word in ranges])
                skipped += int(sum(left_out[n] for n in wave))
                steps += sum(wave) * words
    assert slot_words == total_words
    share = skipped / steps
    print(f"rule {rule}: {skipped} of {steps} word-steps skipped, {100 * share:.2f} %")
    assert 0.03 <= share <= 0.07, share

"""A Python model of `myers_infix_column` (csrc/hip/myers_core.hpp) with the wildcard phantom rows of csrc/hip/myers_fuzzy_find.hip,
word by word as the kernel runs it, against the plain semi-global DP - runs anywhere.

The pattern is right-aligned in W 32-bit words over `pad` = 32 W - m phantom low rows.  Every row of the match table starts as the
phantom mask (a wildcard in the rows below the pattern), the vectors start with VP = the real rows, VN = 0, nothing enters bit 0,
and the horizontal pair of the last row - bit 31 of word W - 1 - moves the bottom-row score."""
import random

import numpy as np
import pytest

MASK = 0xFFFFFFFF


def semi_global(query, texts):
    """(distances, ends) of `query` inside every text: D[0][j] = 0, D[i][0] = i, unit costs; the smallest j of the minimum of row m."""
    m, pattern, rows = len(query), np.frombuffer(query, np.uint8), np.arange(len(query) + 1)
    lengths = np.array([len(text) for text in texts])
    padded = np.zeros((len(texts), max(lengths.max(initial=0), 1)), np.uint8)
    for at, text in enumerate(texts):
        padded[at, :len(text)] = np.frombuffer(text, np.uint8)
    column = np.tile(rows, (len(texts), 1))
    best, end = column[:, m].copy(), np.zeros(len(texts), np.int64)
    for j in range(1, int(lengths.max(initial=0)) + 1):
        step = np.zeros_like(column)
        step[:, 1:] = np.minimum(column[:, :-1] + (pattern[None, :] != padded[:, j - 1, None]), column[:, 1:] + 1)
        column = np.minimum.accumulate(step - rows, axis=1) + rows  # the insertions down the column
        better = (j <= lengths) & (column[:, m] < best)
        best[better], end[better] = column[better, m], j
    return best, end


def bits_in_word(low, high, w):
    """The bits of [low, high) that fall into word w (rerank_bits_in_word)."""
    low, high = max(low, 32 * w), min(high, 32 * w + 32)
    return 0 if low >= high else ((1 << (high - low)) - 1) << (low - 32 * w)


def model(query, text, words):
    """(distance, end, phantom rows stayed zero) as the kernel computes them at `words` words."""
    m, pad = len(query), 32 * words - len(query)
    assert pad >= 0
    phantom = [bits_in_word(0, pad, w) for w in range(words)]
    table = {}
    for symbol in set(text) | set(query):
        table[symbol] = list(phantom)
    for i, symbol in enumerate(query):
        table[symbol][(pad + i) >> 5] |= 1 << ((pad + i) & 31)
    vp, vn = [bits_in_word(pad, 32 * words, w) for w in range(words)], [0] * words
    score, best, end, inert = m, m, 0, True
    for column, symbol in enumerate(text):
        eq = table[symbol]
        carry = hp_below = hn_below = 0
        for w in range(words):
            xv = eq[w] | vn[w]
            total = (eq[w] & vp[w]) + vp[w] + carry
            carry, total = total >> 32, total & MASK
            d0 = (total ^ vp[w]) | eq[w]
            hp = (vn[w] | ~(d0 | vp[w])) & MASK
            hn = vp[w] & d0
            hp_shifted = ((hp << 1) | (hp_below >> 31 if w else 0)) & MASK  # nothing enters bit 0
            hn_shifted = ((hn << 1) | (hn_below >> 31 if w else 0)) & MASK
            hp_below, hn_below = hp, hn
            vp[w] = (hn_shifted | ~(xv | hp_shifted)) & MASK
            vn[w] = hp_shifted & xv
        score += (hp_below >> 31) - (hn_below >> 31)  # the last row: bit 31 of the last word, before the shift
        if score < best:
            best, end = score, column + 1
        inert = inert and all((vp[w] | vn[w]) & phantom[w] == 0 for w in range(words))
    return best, end, inert


def check(query, texts, words):
    want_distance, want_end = semi_global(query, texts)
    for at, text in enumerate(texts):
        distance, end, inert = model(query, text, words)
        assert (distance, end) == (want_distance[at], want_end[at]), (query, text, words)
        assert inert, (query, text, words)


def pattern_lengths(words):
    return sorted({m for m in (0, 1, 31, 32, 33, 32 * words - 1, 32 * words) if m <= 32 * words})


@pytest.mark.parametrize("words", range(1, 9))
@pytest.mark.parametrize("alphabet", [b"ab", bytes(range(256)), b"\x00\xff"], ids=["ab", "bytes", "00ff"])
def test_random_texts_at_every_word_boundary(words, alphabet):
    rng = random.Random(words * 7 + len(alphabet))
    for m in pattern_lengths(words):
        query = bytes(rng.choice(alphabet) for _ in range(m))
        lengths = [0, 1, 2, max(m - 1, 0), m, m + 1] + [rng.randint(0, 80) for _ in range(6)]  # texts shorter than the pattern too
        check(query, [bytes(rng.choice(alphabet) for _ in range(n)) for n in lengths], words)


def edited(rng, query, edit, alphabet):
    at = rng.randrange(len(query))
    other = bytes([next(b for b in alphabet if b != query[at])])
    return {"exact": query, "substitution": query[:at] + other + query[at + 1:], "insertion": query[:at] + other + query[at:],
            "deletion": query[:at] + query[at + 1:]}[edit]


@pytest.mark.parametrize("words", range(1, 9))
@pytest.mark.parametrize("edit", ["exact", "substitution", "insertion", "deletion"])
def test_planted_occurrences(words, edit):
    rng = random.Random(words * 31 + len(edit))
    for m in (m for m in pattern_lengths(words) if m):
        for alphabet in (b"abcd", b"\x00\xff\x01\xfe"):
            query = bytes(rng.choice(alphabet) for _ in range(m))
            occurrence = edited(rng, query, edit, alphabet)
            before, after = (bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 40))) for _ in range(2))
            texts = [occurrence + after, before + occurrence + after, before + occurrence]  # at the start, in the middle, at the end
            check(query, texts, words)
            for text in texts:
                assert model(query, text, words)[0] <= (edit != "exact")
            if edit == "exact":
                assert model(query, occurrence + after, words)[:2] == (0, m)


def test_by_hand():
    assert model(b"ab", b"abababab", 1)[:2] == (0, 2)  # the leftmost end
    assert model(b"xyz", b"abababab", 1)[:2] == (3, 0)  # nothing of it occurs: the empty substring
    assert model(b"", b"abc", 1)[:2] == (0, 0)
    assert model(b"abc", b"", 2)[:2] == (3, 0)
    assert model(b"survey", b"surgery", 1)[:2] == (2, 5)  # "surge": v -> g, y dropped - before "surgery" (g -> v, r dropped) ends
    distances, ends = semi_global(b"survey", [b"surgery", b"", b"xxsurveyxx"])
    assert distances.tolist() == [2, 6, 0] and ends.tolist() == [5, 0, 8]

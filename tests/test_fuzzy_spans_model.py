"""A Python model of the reverse pass of csrc/hip/myers_fuzzy_spans.hip - `myers_prefix_column` (csrc/hip/myers_core.hpp) over the
REVERSED query with ZERO phantom rows, word by word as the kernel runs it - against brute force - runs anywhere.

The forward call gives `d` and `end` (the semi-global DP below).  The reverse pass is the GLOBAL column: D'[0][t] = t, D'[i][0] = i,
for the reversed query against c[end - 1], c[end - 2], ... over T = min(end, m + d) columns.  The table is rerank's - zero, then byte
i of the query at bit pad + (m - 1 - i) - the vectors start with VP = the real rows, VN = 0, `+1` enters bit 0 in every column, and
the horizontal pair of the last row - bit 31 of word W - 1 - moves the bottom-row score from `score = best = m, pos = 0`; a strictly
smaller score moves `best` and `pos`; start = end - pos.  The reference is `lev(q, c[s:end])` over every start `s`."""
import random

import numpy as np
import pytest

MASK = 0xFFFFFFFF


def semi_global(query, text):
    """(distance, end) of `query` inside `text`: D[0][j] = 0, D[i][0] = i, unit costs; the smallest j of the minimum of row m."""
    m, pattern, rows = len(query), np.frombuffer(query, np.uint8), np.arange(len(query) + 1)
    column = rows.copy()
    best, end = int(column[m]), 0
    for j, symbol in enumerate(text, 1):
        step = np.zeros_like(column)
        step[1:] = np.minimum(column[:-1] + (pattern != symbol), column[1:] + 1)
        column = np.minimum.accumulate(step - rows) + rows  # the insertions down the column
        if column[m] < best:
            best, end = int(column[m]), j
    return best, end


def distances_of_every_start(query, text, end):
    """lev(query, text[s:end]) for s = end, end - 1, ... 0: the last row of the global DP of the reversed strings, column by column."""
    m, pattern, rows = len(query), np.frombuffer(query[::-1], np.uint8), np.arange(len(query) + 1)
    column, last_row = rows.copy(), [len(query)]
    for t in range(1, end + 1):
        step = np.empty_like(column)
        step[0] = t
        step[1:] = np.minimum(column[:-1] + (pattern != text[end - t]), column[1:] + 1)
        column = np.minimum.accumulate(step - rows) + rows
        last_row.append(int(column[m]))
    return last_row  # last_row[t] = lev(query, text[end - t:end])


def bits_in_word(low, high, w):
    """The bits of [low, high) that fall into word w (rerank_bits_in_word)."""
    low, high = max(low, 32 * w), min(high, 32 * w + 32)
    return 0 if low >= high else ((1 << (high - low)) - 1) << (low - 32 * w)


def model(query, text, distance, end, words):
    """(best, start, phantom rows stayed zero) as the kernel computes them at `words` words from the forward pass's (distance, end)."""
    m, pad = len(query), 32 * words - len(query)
    assert pad >= 0
    phantom = [bits_in_word(0, pad, w) for w in range(words)]
    table = {symbol: [0] * words for symbol in set(text) | set(query)}
    for i, symbol in enumerate(query):
        position = pad + (m - 1 - i)  # the reversed query: its last byte is the first real row
        table[symbol][position >> 5] |= 1 << (position & 31)
    vp, vn = [bits_in_word(pad, 32 * words, w) for w in range(words)], [0] * words
    score, best, pos, inert = m, m, 0, True
    for t in range(min(end, m + distance)):
        eq = table[text[end - 1 - t]]
        carry = hp_below = hn_below = 0
        for w in range(words):
            xv = eq[w] | vn[w]
            total = (eq[w] & vp[w]) + vp[w] + carry
            carry, total = total >> 32, total & MASK
            d0 = (total ^ vp[w]) | eq[w]
            hp = (vn[w] | ~(d0 | vp[w])) & MASK
            hn = vp[w] & d0
            hp_shifted = ((hp << 1) | (hp_below >> 31 if w else 1)) & MASK  # +1 enters bit 0: D'[0][t] = t
            hn_shifted = ((hn << 1) | (hn_below >> 31 if w else 0)) & MASK
            hp_below, hn_below = hp, hn
            vp[w] = (hn_shifted | ~(xv | hp_shifted)) & MASK
            vn[w] = hp_shifted & xv
        score += (hp_below >> 31) - (hn_below >> 31)  # the last row: bit 31 of the last word, before the shift
        if score < best:
            best, pos = score, t + 1
        inert = inert and all((vp[w] | vn[w]) & phantom[w] == 0 for w in range(words))
    return best, end - pos, inert


def span(query, text, words):
    """(distance, start, end) through the model, checked against brute force on the way."""
    distance, end = semi_global(query, text)
    best, start, inert = model(query, text, distance, end, words)
    by_start = distances_of_every_start(query, text, end)
    assert min(by_start) == distance, (query, text)  # no start gives less, one gives d
    assert best == distance, (query, text, words)
    assert inert, (query, text, words)
    assert start == end - by_start.index(distance), (query, text, words)  # the LARGEST start that attains d: the shortest match
    assert end - start <= len(query) + distance and abs((end - start) - len(query)) <= distance, (query, text, words)
    assert 0 <= start <= end
    return distance, start, end


def pattern_lengths(words):
    return sorted({m for m in (0, 1, 31, 32, 33, 32 * words - 1, 32 * words) if m <= 32 * words})


@pytest.mark.parametrize("words", range(1, 9))
@pytest.mark.parametrize("alphabet", [b"ab", bytes(range(256)), b"\x00\xff"], ids=["ab", "bytes", "00ff"])
def test_random_texts_at_every_word_boundary(words, alphabet):
    rng = random.Random(words * 11 + len(alphabet))
    for m in pattern_lengths(words):
        query = bytes(rng.choice(alphabet) for _ in range(m))
        lengths = [0, 1, 2, max(m - 1, 0), m, m + 1] + [rng.randint(0, 80) for _ in range(4)]  # texts shorter than the pattern too
        for n in lengths:
            span(query, bytes(rng.choice(alphabet) for _ in range(n)), words)


def edited(rng, query, edit, alphabet):
    at = rng.randrange(len(query))
    other = bytes([next(b for b in alphabet if b != query[at])])
    return {"exact": query, "substitution": query[:at] + other + query[at + 1:], "insertion": query[:at] + other + query[at:],
            "deletion": query[:at] + query[at + 1:]}[edit]


@pytest.mark.parametrize("words", range(1, 9))
@pytest.mark.parametrize("edit", ["exact", "substitution", "insertion", "deletion"])
def test_planted_occurrences(words, edit):
    rng = random.Random(words * 37 + len(edit))
    for m in (m for m in pattern_lengths(words) if m):
        for alphabet in (b"abcd", b"\x00\xff\x01\xfe"):
            query = bytes(rng.choice(alphabet) for _ in range(m))
            occurrence = edited(rng, query, edit, alphabet)
            before, after = (bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 40))) for _ in range(2))
            texts = [occurrence + after, before + occurrence + after, before + occurrence]  # at the start, in the middle, at the end
            for text in texts:
                distance, start, end = span(query, text, words)
                assert distance <= (edit != "exact")
            if edit == "exact":
                assert span(query, occurrence + after, words) == (0, 0, m)  # the window is clipped by `end`


def test_by_hand():
    assert span(b"survey", b"surgery", 1) == (2, 0, 5)  # "surge": v -> g, y dropped
    assert span(b"ab", b"abababab", 1) == (0, 0, 2)  # the leftmost end, and its start
    assert span(b"xyz", b"abab", 1) == (3, 0, 0)  # nothing of it occurs: the empty substring at 0
    assert span(b"", b"abc", 1) == (0, 0, 0)
    assert span(b"abc", b"", 2) == (3, 0, 0)
    assert span(b"survey", b"xxsurveyxx", 1) == (0, 2, 8)
    assert span(b"abcd", b"xxabdxx", 1) == (1, 2, 5)  # one deletion: t* = m - 1
    assert span(b"abcd", b"xxabxcdxx", 1) == (1, 2, 7)  # one insertion: t* = m + 1

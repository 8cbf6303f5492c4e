"""The Myers column that takes HN << 1 from the adder's carries (hip/myers_core.hpp: myers_column; hip/lev_myers.hip: the paired bodies).

A word-wise model of exactly the kernel's formulas - 32-bit words, one `addc` chain over the W words, a funnel shift for HP only:

    K   = (Eq | VP) & ~Ms0                     sum = (Eq & VP) + VP + carry
    HNs = (sum ^ K ^ Eq) & ~(Eq & ~K)          HP  = VN | ~(sum | K)
    X~  = Eq | VN | Msep                       VP' = HNs | ~(X~ | HPs)        VN' = HPs & X~ & ~Msep

with Ms0 = Msep = 0 for a single pattern, and for a pair the s0 bit in EVERY row of the match-mask table - scored against the oracle,
and HNs compared bit for bit with the older column's (VP & D0 & ~Mtop) << 1 on random states.
"""
import random
from collections import defaultdict

import pytest

WORD = 0xFFFFFFFF
WIDTHS = (1, 2, 3, 4, 5, 8, 9, 10)


def bits_in_word(low_bit, high_bit, w):
    """hip/lev_myers.hip: bits_in_word - the bits of [low_bit, high_bit) that fall into word w."""
    low, high = max(low_bit, 32 * w), min(high_bit, 32 * w + 32)
    if low >= high:
        return 0
    return (WORD if high - low == 32 else (1 << (high - low)) - 1) << (low - 32 * w)


def carry_column(vp, vn, eq, separators, s0):
    """myers_column: one column on lists of W words, in place.  Returns HNs (the carries into every bit) for the identity test."""
    carry, hp_below, carries = 0, 0, []
    for w in range(len(vp)):
        xv = eq[w] | vn[w] | separators[w]
        total = (eq[w] & vp[w]) + vp[w] + carry
        total, carry = total & WORD, total >> 32
        k = (eq[w] | vp[w]) & ~s0[w] & WORD
        hn_shifted = (total ^ k ^ eq[w]) & ~(eq[w] & ~k) & WORD
        hp = (vn[w] | ~(total | k)) & WORD
        hp_shifted = ((hp << 1) | (1 if w == 0 else hp_below >> 31)) & WORD
        hp_below = hp
        vp[w] = (hn_shifted | ~(xv | hp_shifted)) & WORD
        vn[w] = hp_shifted & xv & ~separators[w] & WORD
        carries.append(hn_shifted)
    return carries


def older_column(vp, vn, eq, separators, tops):
    """The column before this one: D0 spelled out, HN = VP & D0 & ~Mtop, both horizontal vectors shifted."""
    carry, hp_below, hn_below, shifted = 0, 0, 0, []
    for w in range(len(vp)):
        xv = eq[w] | vn[w] | separators[w]
        total = (eq[w] & vp[w]) + vp[w] + carry
        total, carry = total & WORD, total >> 32
        d0 = (total ^ vp[w]) | eq[w]
        hp = (vn[w] | ~(d0 | vp[w])) & WORD
        hn = vp[w] & d0 & ~tops[w] & WORD
        hp_shifted = ((hp << 1) | (1 if w == 0 else hp_below >> 31)) & WORD
        hn_shifted = ((hn << 1) | (0 if w == 0 else hn_below >> 31)) & WORD
        hp_below, hn_below = hp, hn
        vp[w] = (hn_shifted | ~(xv | hp_shifted)) & WORD
        vn[w] = hp_shifted & xv & ~separators[w] & WORD
        shifted.append(hn_shifted)
    return shifted


def single_distance(query, text, words):
    """The single-pattern body of myers_workgroup for one lane."""
    pad = 32 * words - len(query)
    assert pad >= 0
    none = [0] * words
    peq = defaultdict(lambda: [0] * words)
    for i, c in enumerate(query):
        peq[c][(pad + i) >> 5] |= 1 << ((pad + i) & 31)
    vp, vn = [bits_in_word(pad, 32 * words, w) for w in range(words)], [0] * words
    for c in text:
        carry_column(vp, vn, peq[c], none, none)
        assert not any(p & n for p, n in zip(vp, vn))
    return len(text) + sum(bin(p).count("1") - bin(n).count("1") for p, n in zip(vp, vn))


def pair_distances(first, second, text, words):
    """The paired body: pad rows, `first`, the separator rows s0 s1, `second` - every row of the table holds the s0 bit."""
    l1, l2 = len(first), len(second)
    pad = 32 * words - (l1 + l2 + 2)
    assert pad >= 0
    second_row = pad + l1 + 2
    separators = [bits_in_word(second_row - 2, second_row, w) for w in range(words)]
    s0 = [bits_in_word(second_row - 2, second_row - 1, w) for w in range(words)]
    peq = defaultdict(lambda: list(s0))  # the table is filled with the s0 mask, not with zeros
    for i, c in enumerate(first):
        peq[c][(pad + i) >> 5] |= 1 << ((pad + i) & 31)
    for i, c in enumerate(second):
        peq[c][(second_row + i) >> 5] |= 1 << ((second_row + i) & 31)
    vp = [bits_in_word(pad, 32 * words, w) & ~separators[w] for w in range(words)]
    vn = [0] * words
    for c in text:
        carry_column(vp, vn, peq[c], separators, s0)
        assert not any(p & n for p, n in zip(vp, vn))
        assert not any((p | n) & m for p, n, m in zip(vp, vn, separators))  # the separator rows stay inert
    count = lambda vector, low, high: sum(bin(vector[w] & bits_in_word(low, high, w)).count("1") for w in range(words))
    return (len(text) + count(vp, pad, pad + l1) - count(vn, pad, pad + l1),
            len(text) + count(vp, second_row, 32 * words) - count(vn, second_row, 32 * words))


@pytest.fixture(scope="module")
def texts():
    rng = random.Random(19)
    some = [bytes(rng.choice(b"ab") for _ in range(rng.randint(0, 70))) for _ in range(10)]
    return some + [b"", b"a", b"a" * 64, b"a" * 33, b"b" * 40, b"a" * 330]


def _letters(rng, count, alphabet):
    return bytes(rng.choice(alphabet) for _ in range(count))


@pytest.mark.parametrize("words", WIDTHS)
def test_single_patterns_score_what_the_oracle_scores(oracle, texts, words):
    rng = random.Random(words)
    queries = []
    for length in (32 * words - 31, 32 * words):  # the shortest query of this width, and the one that leaves no phantom row
        queries += [_letters(rng, length, b"ab"), b"a" * length, _letters(rng, length, bytes(range(97, 123)))]
    queries.append(_letters(rng, rng.randint(32 * words - 31, 32 * words), b"ab"))
    if words == 1:
        queries.append(b"")
    expected = oracle.levenshtein(queries, texts)
    for i, query in enumerate(queries):
        for j, text in enumerate(texts):
            assert single_distance(query, text, words) == int(expected[i, j]), (len(query), words, len(text))


def _pairs_of(words, rng):
    """(first length, second length) of one width: s0 on bit 31 with s1 on bit 0 of the next word, s0 on bit 0, s0 mid-word, pad = 0,
    an empty first and an empty second query.  s0 sits at bit 32 W - 2 - (second length)."""
    room = 32 * words - 2
    pairs = [(0, rng.randint(0, room)), (rng.randint(1, room), 0), (0, room), (room, 0), (0, 0)]
    for second in {31, 30, 13, 63, 62, 95, 129, 158, 159} | {rng.randint(0, room) for _ in range(3)}:
        if second <= room:
            pairs.append((rng.randint(0, room - second), second))  # anywhere in the vector
            pairs.append((room - second, second))                  # pad = 0
    return pairs


@pytest.mark.parametrize("words", WIDTHS)
def test_pairs_score_what_the_oracle_scores(oracle, texts, words):
    rng = random.Random(100 + words)
    for l1, l2 in _pairs_of(words, rng):
        for alphabet in (b"a", b"ab"):
            first, second = _letters(rng, l1, alphabet), _letters(rng, l2, alphabet)
            expected = oracle.levenshtein([first, second], texts)
            for j, text in enumerate(texts):
                got = pair_distances(first, second, text, words)
                assert got == (int(expected[0, j]), int(expected[1, j])), (l1, l2, words, len(text))


def test_one_carry_through_every_word_boundary(oracle):
    """ "a" * L against "a" * M: Eq = VP = all ones in the first column, so one carry ripples through all W words of the add - and every
    bit of HNs comes from it."""
    vp, vn, none = [WORD] * 10, [0] * 10, [0] * 10
    assert carry_column(vp, vn, [WORD] * 10, none, none) == [WORD & ~1] + [WORD] * 9
    for length, columns in ((320, 64), (289, 7), (320, 320), (65, 100)):
        expected = oracle.levenshtein([b"a" * length], [b"a" * columns])
        assert single_distance(b"a" * length, b"a" * columns, (length + 31) // 32) == int(expected[0, 0]) == abs(length - columns)


def test_the_carries_are_the_older_columns_shifted_negative_deltas():
    """The identity itself: on any state with VP & VN == 0, HNs == (VP & D0) << 1 across the whole vector, and with it VP' and VN'."""
    rng = random.Random(7)
    for _ in range(3000):
        words = rng.choice(WIDTHS)
        # (sparse, dense and plain random words: long carry runs need dense VP and Eq)
        draw = lambda: rng.getrandbits(32) | (rng.getrandbits(32) if rng.random() < 0.4 else 0) if rng.random() < 0.8 else WORD
        eq = [draw() for _ in range(words)]
        vp = [draw() for _ in range(words)]
        vn = [draw() & ~p & WORD for p in vp]
        none = [0] * words
        new_vp, new_vn, old_vp, old_vn = list(vp), list(vn), list(vp), list(vn)
        carries = carry_column(new_vp, new_vn, eq, none, none)
        shifted = older_column(old_vp, old_vn, eq, none, none)
        assert carries == shifted and new_vp == old_vp and new_vn == old_vn, (words, eq, vp, vn)


def test_the_identity_holds_with_two_patterns_in_the_vector():
    """The same with the separator rows inside: the older column masks q1's top row out of HN and keeps s0 out of Eq; this one
    holds s0 in every Eq and masks it out of K.  States as the kernel can reach them: VP = VN = 0 on separator and phantom rows."""
    rng = random.Random(8)
    for _ in range(3000):
        words = rng.choice(WIDTHS)
        room = 32 * words - 2
        l1 = rng.randint(0, room)
        l2 = rng.choice((rng.randint(0, room - l1), room - l1))
        pad = room - l1 - l2
        second_row = pad + l1 + 2
        rows = [bits_in_word(pad, pad + l1, w) | bits_in_word(second_row, 32 * words, w) for w in range(words)]
        separators = [bits_in_word(second_row - 2, second_row, w) for w in range(words)]
        s0 = [bits_in_word(second_row - 2, second_row - 1, w) for w in range(words)]
        tops = [bits_in_word(second_row - 3, second_row - 2, w) if l1 else 0 for w in range(words)]
        draw = lambda: rng.getrandbits(32) | (rng.getrandbits(32) if rng.random() < 0.5 else 0)
        eq = [draw() & rows[w] for w in range(words)]
        vp = [draw() & rows[w] for w in range(words)]
        vn = [draw() & rows[w] & ~vp[w] for w in range(words)]
        new_vp, new_vn, old_vp, old_vn = list(vp), list(vn), list(vp), list(vn)
        carries = carry_column(new_vp, new_vn, [e | m for e, m in zip(eq, s0)], separators, s0)
        shifted = older_column(old_vp, old_vn, eq, separators, tops)
        assert carries == shifted and new_vp == old_vp and new_vn == old_vn, (words, l1, l2)
        assert not any((p | n) & m for p, n, m in zip(new_vp, new_vn, separators))

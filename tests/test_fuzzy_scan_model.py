"""Fuzzy scan's piece rule (hip/myers_fuzzy_scan.hip) as a plain Python model against the plain DP - runs
anywhere.  The text is cut into pieces of P bytes; the lane of piece p walks from s = p P - warm, warm = min(p P, 2 m), follows
(best, leftmost end) over every column it walks and reports (best, s + end); the answer is the lexicographic minimum over the pieces.
The inputs must also be able to SEE a warm-up that is too short: with m - 1 bytes some of them give a wrong answer."""
import random

import pytest

from stringzilla_amd import _abi

PIECES = (1, 2, 3, 5, 8, 16, 64)
CASES = 3000


def last_row(query, text):
    """D[m][0 .. n] of the unit-cost DP with a free start in the text."""
    m = len(query)
    column, row = list(range(m + 1)), [m]
    for symbol in text:
        step = [0] * (m + 1)
        for i in range(1, m + 1):
            step[i] = min(column[i - 1] + (query[i - 1] != symbol), column[i] + 1, step[i - 1] + 1)
        column = step
        row.append(column[m])
    return row


def best_match(query, text):
    """(min over j of D[m][j], the smallest j that attains it)."""
    row = last_row(query, text)
    best = min(row)
    return best, row.index(best)


def pieces_model(query, text, piece, warm_up):
    """The minimum over the pieces of (best, s + end), each lane's DP started at s = p P - min(p P, warm_up(m))."""
    m, n = len(query), len(text)
    if m == 0:
        return 0, 0  # the emit's fixed result: no lane walks
    answer = (m, 0)  # no piece at all: an empty text
    reports = []
    for p in range(-(-n // piece)):
        warm = min(p * piece, max(warm_up(m), 0))
        s = p * piece - warm
        best, end = best_match(query, text[s:min(n, (p + 1) * piece)])
        reports.append((best, s + end))
    return min(reports) if reports else answer


def cases():
    rng = random.Random(20240611)
    for number in range(CASES):
        alphabet = b"abcd"[:rng.randint(2, 4)]
        m, n, piece = rng.randint(0, 12), rng.randint(0, 90), rng.choice(PIECES)
        query = bytes(rng.choice(alphabet) for _ in range(m))
        text = bytearray(rng.choice(alphabet) for _ in range(n))
        if number % 2 and m and n >= m:  # planted: a copy with up to two edits, somewhere - often across a piece boundary
            copy = bytearray(query)
            for _ in range(rng.randint(0, 2)):
                at = rng.randrange(len(copy)) if copy else 0
                kind = rng.randint(0, 2)
                if kind == 0 and copy:
                    copy[at] = rng.choice(alphabet)
                elif kind == 1 and copy:
                    del copy[at]
                else:
                    copy.insert(at, rng.choice(alphabet))
            at = rng.randint(0, n - len(copy)) if n >= len(copy) else 0
            text[at:at + len(copy)] = copy
            text = text[:n]
        yield query, bytes(text), piece


@pytest.fixture(scope="module")
def inputs():
    return list(cases())


def test_the_rule_is_exact_with_a_warm_up_of_2m(inputs):
    assert len(inputs) == CASES and {piece for _, _, piece in inputs} == set(PIECES)
    assert any(len(query) == 0 for query, _, _ in inputs) and any(len(text) == 0 for _, text, _ in inputs)
    wrong = [(query, text, piece) for query, text, piece in inputs
             if pieces_model(query, text, piece, lambda m: 2 * m) != best_match(query, text)]
    assert not wrong, wrong[:3]


def test_the_inputs_can_see_a_warm_up_that_is_too_short(inputs):
    wrong = sum(pieces_model(query, text, piece, lambda m: m - 1) != best_match(query, text) for query, text, piece in inputs)
    assert wrong >= 1


def test_fixed_results():
    assert pieces_model(b"", b"abc", 2, lambda m: 2 * m) == (0, 0)
    assert pieces_model(b"abc", b"", 2, lambda m: 2 * m) == (3, 0)
    assert pieces_model(b"abc", b"xyzxyzxyz", 2, lambda m: 2 * m) == (3, 0)  # nothing occurs: piece 0 wins with end 0


@pytest.fixture
def piece_knob():
    yield
    _abi.tuning_set("fuzzy_scan_piece", None)


@pytest.mark.parametrize("n, longest, piece", [(0, 5, 64), (1, 0, 64), (5000, 40, 64), (5000, 256, 64), (5000, 256, 128), (4096 * 3, 100, 4096),
                                               (4096 * 3 + 1, 256, 4096), (100000, 31, 192)])
def test_the_probe_counts_the_walked_bytes_as_the_model_does(piece_knob, n, longest, piece):
    _abi.tuning_set("fuzzy_scan_piece", piece)
    got_piece, pieces, _, walked = _abi.fuzzy_scan_probe(3, longest, n)
    assert got_piece == piece and pieces == -(-n // piece)
    assert walked == n + sum(min(p * piece, 2 * longest) for p in range(pieces))

"""Fuzzy scan occurrences on the GPU (`szs_rocm_fuzzy_scan_occurrences*`, `_Engine.fuzzy_scan_occurrences`):
the count of every query and its leftmost occurrences - end, distance, start - against the NumPy DP of
tests/test_gpu_fuzzy_scan_matches.py (the last row D[m][j] of the semi-global DP, every column of it) with the rule applied to it,
a reverse global DP for the starts, and against `fuzzy_scan_matches` and `fuzzy_scan` on the same GPU.  The text has about 9000
bytes; the `fuzzy_scan_piece` knob at 64 makes that 141 pieces, three workgroups a row."""
import ctypes
import random

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi
from test_gpu_fuzzy_scan_matches import (EMPTY, N, PIECES, QUERY_LENGTHS, UNTOUCHED, TwoBlocks, _last_rows, _mutated, last_rows,
                                         on_device_outputs, same)

pytestmark = pytest.mark.gpu


def occurrence_ends(row, bound):
    """The rule over one bottom row D[m][0 ... n]: the columns j in [1, n] that are occurrence ends, ascending."""
    here, left = row[1:], row[:-1]
    right_ok = np.ones(len(here), bool)  # column n has no right neighbour
    right_ok[:-1] = here[:-1] <= here[1:]
    return np.flatnonzero((here <= bound) & (here < left) & right_ok) + 1


def reverse_rows(query, text, ends, distances):
    """For every (end, distance) the bottom row of the GLOBAL DP of the reversed query against text[end - T:end] reversed,
    T = min(end, m + distance): row[i][t] = lev(query, text[end - t:end]) for t <= T.  Returns (rows, windows)."""
    windows = [min(int(end), len(query) + int(distance)) for end, distance in zip(ends, distances)]
    backwards = [bytes(text[int(end) - window:int(end)])[::-1] for end, window in zip(ends, windows)]
    return _last_rows([query[::-1]] * len(backwards), backwards, free_start=False), windows


def starts_of(query, text, ends, distances):
    """start = end - t*, t* the smallest t <= min(end, m + distance) with lev(query, text[end - t:end]) == distance."""
    if not len(ends):
        return np.zeros(0, np.uint64)
    rows, windows = reverse_rows(query, text, ends, distances)
    found = []
    for row, window, end, distance in zip(rows, windows, ends, distances):
        attained = np.flatnonzero(row[:window + 1] == distance)
        assert len(attained)  # D[m][end] is the minimum over all starts: some window attains it
        found.append(int(end) - int(attained[0]))
    return np.array(found, np.uint64)


class Oracle:
    """Every occurrence of every query in one text per bound - computed once a bound, read-only - and the call's outputs cut from it."""

    def __init__(self, queries, text):
        self.queries, self.text, self.last, self._full, self._starts = queries, text, last_rows(queries, text), {}, {}

    def full(self, bound):
        """Per query the ends and distances of ALL its occurrences."""
        bound = min(bound, 256)
        if bound not in self._full:
            rows = []
            for q, query in enumerate(self.queries):
                ends = occurrence_ends(self.last[q], bound) if query and len(self.text) else np.zeros(0, np.int64)
                rows.append((ends.astype(np.uint64), self.last[q, ends].astype(np.uint64)))
            self._full[bound] = rows
        return self._full[bound]

    def expected(self, bound, limit, starts=True):
        """(counts, distances, starts, ends) as the call returns them - without the starts a triple."""
        bound = min(bound, 256)
        rows = self.full(bound)
        counts = np.array([len(ends) for ends, _ in rows], np.uint64)
        distances, begins, ends = (np.full((len(rows), limit), EMPTY, np.uint64) for _ in range(3))
        for q, (row_ends, row_distances) in enumerate(rows):
            kept = min(limit, len(row_ends))
            ends[q, :kept], distances[q, :kept] = row_ends[:kept], row_distances[:kept]
            if starts and (bound, q, kept) not in self._starts:  # the reverse DP of the kept slots only
                self._starts[bound, q, kept] = starts_of(self.queries[q], self.text, row_ends[:kept], row_distances[:kept])
            if starts:
                begins[q, :kept] = self._starts[bound, q, kept]
        return (counts, distances, begins, ends) if starts else (counts, distances, ends)


def walked_cells(queries, n, piece):
    """What one forward pass counts: m x the bytes walked - per piece its own bytes, min(p P, 2 m) ahead of them and, where the piece
    is not the last, one tail column."""
    pieces = -(-n // piece)
    return sum(len(query) * sum(min(p * piece, 2 * len(query)) + min(piece, n - p * piece) + (p + 1 < pieces) for p in range(pieces))
               for query in queries)


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return szs.DeviceScope(gpu_device=0)


@pytest.fixture(scope="module")
def engine(gpu):
    return szs.LevenshteinDistances(capabilities=gpu)


@pytest.fixture
def piece():
    """Sets the `fuzzy_scan_piece` knob; restores the automatic rule afterwards."""
    yield lambda value: _abi.tuning_set("fuzzy_scan_piece", value)
    _abi.tuning_set("fuzzy_scan_piece", None)


@pytest.fixture(scope="module")
def planted():
    """The text of tests/test_gpu_fuzzy_scan_matches.py's `planted`, built the same way - a query of every length, one more that is
    planted nowhere, N bytes over ACGT with copies of every query under 0 to 3 edits, four a query in turn - with two exact copies of
    its own: query 33 ENDS at column 4096, so its right neighbour lies in the next piece at every piece size, and query 64 ends at
    column 8193, so its left neighbour lies in the piece before.  One more: query 65 with its last byte replaced, ending at column
    6000 - columns 5999 (the last byte deleted) and 6000 (replaced) both hold 1, a plateau at every bound from 1."""
    rng = random.Random(412)
    alphabet = b"ACGT"
    queries = [bytes(rng.choice(alphabet) for _ in range(length)) for length in QUERY_LENGTHS]
    queries.append(bytes(rng.choice(alphabet) for _ in range(48)))  # planted nowhere
    text = bytearray(rng.choice(alphabet) for _ in range(N))
    at = 5
    for turn in range(4):
        for query in queries[1:-1]:
            copy = _mutated(rng, query, alphabet, (turn + len(query)) % 4)
            text[at:at + len(copy)] = copy
            at += len(copy) + 23
        at += 300
    assert 4096 < at < 5900
    text[4096 - 33:4096] = queries[4]
    text[8193 - 64:8193] = queries[5]
    text[6000 - 65:6000] = queries[6][:-1] + bytes(letter for letter in alphabet if letter != queries[6][-1])[:1]
    return Oracle(queries, bytes(text[:N]))


@pytest.mark.parametrize("max_distance", [0, 1, 3])
@pytest.mark.parametrize("value", PIECES, ids=lambda value: f"piece-{value}")
def test_every_width_and_piece(gpu, engine, piece, planted, value, max_distance):
    queries, text, last = planted.queries, planted.text, planted.last
    piece(value)
    size = value or 4096
    assert _abi.fuzzy_scan_probe(len(queries), 256, len(text))[:2] == (size, -(-N // size))
    limit = N  # at least the largest count
    want = planted.expected(max_distance, limit)
    counts, _, _, ends = want
    # what the oracle must hold for this to have tested the cut.  Counted over the queries of more than one byte - except, at a bound
    # of 0, the plateau and the hit that is no occurrence: both need D[m][j] = D[m][j + 1] = 0 or D[m][j - 1] = D[m][j] = 0, two exact
    # copies one byte apart, which only a query of one repeated byte has; there the one-byte query supplies them.
    longer = [q for q, query in enumerate(queries) if len(query) > 1]
    reported = [(q, int(j)) for q in longer for j in ends[q, :int(counts[q])]]
    assert any(j % size == 0 and j < N for _, j in reported)  # the right neighbour is the next piece's first column
    assert any(j % size == 1 and j > 1 for _, j in reported)  # the left neighbour is the piece before's last column
    flat = longer if max_distance else [q for q, query in enumerate(queries) if query]
    assert any(j < N and last[q, j] == last[q, j + 1] for q in flat for j in map(int, ends[q, :int(counts[q])]))  # a plateau
    assert any(int((last[q, 1:] <= max_distance).sum()) > counts[q] for q in flat)  # a hit column that is not an occurrence
    assert any(counts[q] == 0 for q in longer)
    if size == 64:
        assert any(len({(j - 1) // (64 * size) for r, j in reported if r == q}) >= 2 for q in longer)

    got = engine.fuzzy_scan_occurrences(queries, text, max_distance, limit=limit, device=gpu)
    assert [array.shape for array in got] == [(len(queries),)] + [(len(queries), limit)] * 3
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert same(got, want), [np.argwhere(g != w)[:4] for g, w in zip(got, want)]
    for q in range(len(queries)):  # the empty slots are all ones
        assert all((matrix[q, int(got[0][q]):] == EMPTY).all() for matrix in got[1:])
    without = engine.fuzzy_scan_occurrences(queries, text, max_distance, limit=limit, starts=False, device=gpu)
    assert same(without, (want[0], want[1], want[3]))


@pytest.mark.parametrize("max_distance", [0, 2, 5])
def test_spans(gpu, engine, piece, planted, max_distance):
    """Every reported slot on its own terms: lev(query, text[start:end]) == distance, and no shorter window that ends there has it."""
    queries, text = planted.queries, planted.text
    piece(128)
    counts, distances, starts, ends = engine.fuzzy_scan_occurrences(queries, text, max_distance, limit=200, device=gpu)
    checked = 0
    for q, query in enumerate(queries):
        kept = min(int(counts[q]), 200)
        if not kept:
            continue
        rows, windows = reverse_rows(query, text, ends[q, :kept], distances[q, :kept])
        for row, window, start, end, distance in zip(rows, windows, starts[q, :kept], ends[q, :kept], distances[q, :kept]):
            taken = int(end) - int(start)
            assert 0 <= taken <= window and row[taken] == distance and (row[:taken] != distance).all(), (q, int(end))
            checked += len(query) > 1
    assert checked >= 10


@pytest.mark.parametrize("max_distance", [0, 2, 5])
def test_agreement_with_matches_and_fuzzy_scan(gpu, engine, piece, planted, max_distance):
    queries, text = planted.queries, planted.text
    piece(128)
    limit = N  # every occurrence of every row is kept
    scan_distances, scan_starts, scan_ends = engine.fuzzy_scan(queries, text, device=gpu, starts=True)
    hit_counts, hit_distances, hit_ends = engine.fuzzy_scan_matches(queries, text, max_distance, limit=N, device=gpu)
    counts, distances, starts, ends = engine.fuzzy_scan_occurrences(queries, text, max_distance, limit=limit, device=gpu)
    compared = 0
    for q, query in enumerate(queries):
        kept = min(int(counts[q]), limit)
        hits = {(int(j), int(d)) for j, d in zip(hit_ends[q, :int(hit_counts[q])], hit_distances[q, :int(hit_counts[q])])}
        assert {(int(j), int(d)) for j, d in zip(ends[q, :kept], distances[q, :kept])} <= hits, q  # every occurrence is a hit
        assert counts[q] <= hit_counts[q]
        if not query:  # the scan gives a query of no bytes (0, 0), the empty match; here it has no occurrence
            assert counts[q] == 0
            continue
        if scan_distances[q] <= max_distance and scan_distances[q] < len(query):
            assert 0 < counts[q] <= limit
            best = int(np.argmin(distances[q, :kept]))  # the first of the smallest: the leftmost occurrence of minimum distance
            assert (int(distances[q, best]), int(starts[q, best]), int(ends[q, best])) == \
                (int(scan_distances[q]), int(scan_starts[q]), int(scan_ends[q])), q
            compared += 1
        elif scan_distances[q] == len(query):  # nothing better than m anywhere: no occurrence
            assert counts[q] == 0
    assert compared >= 3


@pytest.mark.parametrize("limit", [0, 1, 3, 7])
def test_capacity(gpu, engine, piece, planted, limit):
    queries, text = planted.queries, planted.text
    rows = len(queries)
    piece(64)
    for max_distance in (0, 1):
        full = planted.expected(max_distance, N)[0]
        assert (full > 7).any() and (full == 0).any() and ((full > 0) & (full <= 3)).any()  # rows above, without and within the limits
        want = planted.expected(max_distance, limit)
        assert np.array_equal(want[0], full)  # the counts are full, whatever the limit
        got = engine.fuzzy_scan_occurrences(queries, text, max_distance, limit=limit, device=gpu)
        assert same(got, want), [np.argwhere(g != w)[:4] for g, w in zip(got, want)]
        assert engine.last_call_profile().launches == (4 if limit else 2)
        got = engine.fuzzy_scan_occurrences(queries, text, max_distance, limit=limit, starts=False, device=gpu)
        assert same(got, (want[0], want[1], want[3]))
        assert engine.last_call_profile().launches == (3 if limit else 2)
    if limit:
        return
    # the counting form: the matrices are never touched - (rows, 0) arrays through Python, NULL through the raw ABI
    out = (np.full(rows, UNTOUCHED, np.uint64),) + tuple(np.full((rows, 0), UNTOUCHED, np.uint64) for _ in range(3))
    assert engine.fuzzy_scan_occurrences(queries, text, 1, limit=0, device=gpu, out=out) is out
    assert np.array_equal(out[0], full) and all(matrix.shape == (rows, 0) for matrix in out[1:])
    import torch

    on_device = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    tape, error, counts = szs.Strs(queries)._tape(0), ctypes.c_char_p(), np.full(rows, UNTOUCHED, np.uint64)
    status = _abi.lib.szs_rocm_fuzzy_scan_occurrences_u32tape(engine.handle, gpu.handle, ctypes.byref(tape), on_device.data_ptr(), len(text), 1,
                                                              0, counts.ctypes.data, None, None, None, ctypes.byref(error))
    assert status == 0, error.value
    assert np.array_equal(counts, full)
    assert engine.last_call_profile().launches == 2


def test_any_bound_is_taken(gpu, engine, piece, planted):
    """A bound of 256 and of 2^64 - 1: every valley floor of the bottom row, whatever its depth - none for the query planted nowhere
    only if its row never leaves m, which the oracle decides."""
    queries, text = planted.queries, planted.text
    for value in (64, None):
        piece(value)
        want = planted.expected(256, 100)
        assert (want[0] > 100).any()
        assert same(engine.fuzzy_scan_occurrences(queries, text, 256, limit=100, device=gpu), want)
        assert same(engine.fuzzy_scan_occurrences(queries, text, 2**64 - 1, limit=100, device=gpu), want)


def test_edges(gpu, engine, piece):
    rng = random.Random(7)
    query = bytes(rng.choice(b"ACGT") for _ in range(40))
    queries = [query, b"", b"G", query[:9]]
    for value in (64, None):
        piece(value)
        # an empty text: no occurrence, no launch, zeros and ones
        got = engine.fuzzy_scan_occurrences(queries, b"", 3, limit=4, device=gpu)
        assert same(got, (np.zeros(4, np.uint64),) + (np.full((4, 4), EMPTY),) * 3)
        profile = engine.last_call_profile()
        assert profile.launches == 0 and profile.pairs == 0 and profile.cells == 0
        assert same(engine.fuzzy_scan_occurrences(queries, b"", 3, limit=0, device=gpu)[:1], (np.zeros(4, np.uint64),))
        # a text shorter than the query; a text of exactly k pieces and one byte more; an occurrence at j = n; one at j = 1
        filler = bytes(rng.choice(b"ACGT") for _ in range(5 * 64 + 1))
        texts = [query[:17], b"G", filler[:5 * 64], filler, filler[:5 * 64 - 40] + query, filler[:5 * 64 + 1 - 40] + query,
                 b"G" + filler[:200], query[-1:] + filler[:64]]
        for text in texts:
            oracle = Oracle(queries, text)
            for max_distance in (0, 2, 39, 256, 2**64 - 1):
                want = oracle.expected(max_distance, len(text))
                got = engine.fuzzy_scan_occurrences(queries, text, max_distance, limit=len(text), device=gpu)
                assert same(got, want), (len(text), max_distance)
        counts, _, starts, ends = Oracle(queries, texts[4]).expected(0, 8)
        assert counts[0] == 1 and ends[0, 0] == len(texts[4]) == 5 * 64 and starts[0, 0] == 5 * 64 - 40  # at j = n, a multiple of the piece
        assert Oracle(queries, texts[5]).expected(0, 8)[3][0, 0] == 5 * 64 + 1
        assert Oracle(queries, texts[6]).expected(0, 8)[3][2, 0] == 1  # "G" at j = 1
    got = engine.fuzzy_scan_occurrences([], b"ACGT", 1, limit=3, device=gpu)
    assert [array.shape for array in got] == [(0,), (0, 3), (0, 3), (0, 3)]
    got = engine.fuzzy_scan_occurrences([b"", b""], b"ACGT", 1, limit=3, device=gpu)  # queries of no bytes only
    assert same(got, (np.zeros(2, np.uint64),) + (np.full((2, 3), EMPTY),) * 3)


def test_outputs_and_memory_kinds(gpu, engine, piece, planted):
    import torch

    queries, text = planted.queries, planted.text
    rows, limit = len(queries), 5
    piece(128)
    want = planted.expected(2, limit)
    assert same(engine.fuzzy_scan_occurrences(queries, text, 2, limit=limit, device=gpu), want)  # returned arrays

    def as_numpy(array):
        return array if isinstance(array, np.ndarray) else array.cpu().numpy().view(np.uint64)

    on_device = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    for text_form in (text, on_device):
        for make in (lambda *shape: np.full(shape, UNTOUCHED, np.uint64),             # plain host memory: staged and copied home
                     lambda *shape: torch.full(shape, 7, dtype=torch.int64).cuda(),   # on the device: written where it is
                     lambda *shape: torch.full(shape, 7, dtype=torch.int64).pin_memory()):
            out = (make(rows),) + tuple(make(rows, limit) for _ in range(3))
            assert engine.fuzzy_scan_occurrences(queries, text_form, 2, limit=limit, device=gpu, out=out) is out
            assert same([as_numpy(array) for array in out], want), type(text_form)
            out = (make(rows),) + tuple(make(rows, limit) for _ in range(2))
            assert engine.fuzzy_scan_occurrences(queries, text_form, 2, limit=limit, starts=False, device=gpu, out=out) is out
            assert same([as_numpy(array) for array in out], (want[0], want[1], want[3]))
    out = (np.full(rows, UNTOUCHED, np.uint64), torch.full((rows, limit), 7, dtype=torch.int64).cuda(),
           np.full((rows, limit), UNTOUCHED, np.uint64), torch.full((rows, limit), 7, dtype=torch.int64).pin_memory())
    engine.fuzzy_scan_occurrences(queries, on_device, 2, limit=limit, device=gpu, out=out)  # one of every kind in one call
    assert same([as_numpy(array) for array in out], want)
    assert same(engine.fuzzy_scan_occurrences(szs.Strs(queries, wide_offsets=True), on_device, 2, limit=limit, device=gpu), want)  # u64 tape

    # the callback sequence through the raw ABI, and a text the device cannot read
    q32 = szs.Strs(queries)
    q32._tape(0)
    data, offsets = q32._device[1].data_ptr(), q32.offsets
    sequence = _abi.Sequence(None, rows, _abi.MEMBER_START(lambda handle, i: data + int(offsets[i])),
                             _abi.MEMBER_LENGTH(lambda handle, i: int(offsets[i + 1] - offsets[i])))
    four, error = [np.full(rows, UNTOUCHED, np.uint64)] + [np.full((rows, limit), UNTOUCHED, np.uint64) for _ in range(3)], ctypes.c_char_p()
    status = _abi.lib.szs_rocm_fuzzy_scan_occurrences(engine.handle, gpu.handle, ctypes.byref(sequence), on_device.data_ptr(), len(text), 2, limit,
                                                      *(array.ctypes.data for array in four), ctypes.byref(error))
    assert status == 0, error.value
    assert same(four, want)
    host_text = np.frombuffer(text, np.uint8).copy()
    status = _abi.lib.szs_rocm_fuzzy_scan_occurrences(engine.handle, gpu.handle, ctypes.byref(sequence), host_text.ctypes.data, len(text), 2,
                                                      limit, *(array.ctypes.data for array in four), ctypes.byref(error))
    assert _abi.STATUS_NAMES[status] == "unknown" and error.value and same(four, want)  # nothing written

    # a query of 257 bytes among valid ones: refused before anything is launched, the sentinels intact
    out = (np.full(3, UNTOUCHED, np.uint64),) + tuple(np.full((3, limit), UNTOUCHED, np.uint64) for _ in range(3))
    with pytest.raises(szs.StringZillasError) as refused:
        engine.fuzzy_scan_occurrences([b"AC", b"A" * 257, b"ACGT"], text, 2, limit=limit, device=gpu, out=out)
    assert refused.value.status_name == "unexpected_dimensions" and "256" in str(refused.value)
    assert all((array == UNTOUCHED).all() for array in out)
    assert same(engine.fuzzy_scan_occurrences(queries, text, 2, limit=limit, device=gpu), want)  # and the call afterwards


@pytest.fixture(scope="module")
def two_blocks():
    """tests/test_gpu_fuzzy_scan_matches.py's case with (counts, distances, starts, ends) of the occurrences: the rule and the reverse
    DP over each window, shifted by the window's offset."""
    case = TwoBlocks()
    per_pattern = []
    for p, pattern in enumerate(case.patterns):
        ends, distances, starts = [], [], []
        for offset, window, last in case.windows:
            hits = np.flatnonzero(last[p, 1:] <= case.BOUND) + 1
            assert not len(hits) or (case.EDGE < hits[0] and hits[-1] <= len(window) - case.EDGE)  # what makes the windows exact
            found = occurrence_ends(last[p], case.BOUND)
            begins = starts_of(pattern, window, found, last[p, found])
            ends.append(found + offset), distances.append(last[p, found]), starts.append(begins.astype(np.int64) + offset)
        per_pattern.append(tuple(np.concatenate(column).astype(np.uint64) for column in (distances, starts, ends)))
    return case, case.per_row(per_pattern)


@pytest.mark.parametrize("starts", [True, False], ids=["starts", "no-starts"])
def test_two_blocks_through_the_scratch_cap(gpu, engine, piece, two_blocks, starts):
    """Outputs in device memory, written where they are: the second block's rows, queries and scratch begin where the first's end."""
    import torch

    case, want = two_blocks
    piece(case.PIECE)
    assert _abi.fuzzy_scan_probe(case.ROWS, 8, case.N)[:2] == (case.PIECE, case.N // case.PIECE)
    if not starts:
        want = (want[0], want[1], want[3])
    on_device = torch.frombuffer(bytearray(case.text), dtype=torch.uint8).cuda()
    out = on_device_outputs(case.ROWS, case.LIMIT, len(want) - 1)
    assert engine.fuzzy_scan_occurrences(case.queries, on_device, case.BOUND, limit=case.LIMIT, starts=starts, device=gpu, out=out) is out
    assert engine.last_call_profile().launches == 2 * (4 if starts else 3)
    got = [array.cpu().numpy().view(np.uint64) for array in out]
    assert np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])[:8]
    assert same(got, want), [np.argwhere(g != w)[:4] for g, w in zip(got, want)]  # every filled slot, and all ones behind them
    for matrix in got[1:]:
        assert all((matrix[r, int(count):] == EMPTY).all() for r, count in enumerate(want[0]) if count < case.LIMIT)


@pytest.mark.parametrize("starts", [True, False], ids=["starts", "no-starts"])
def test_two_blocks_through_the_staging_budget(gpu, engine, piece, planted, starts):
    """Outputs in plain host memory: with 2^17 slots a row a staged block is 128 MiB / (2^17 x 8) = 128 rows, and 130 queries leave 2
    for a second one.  128 mod 11 = 7: rows r and r - 128 never hold the same query."""
    rows, limit = 130, 1 << 17
    piece(64)
    want = planted.expected(1, N, starts=starts)
    want = [array[[r % len(planted.queries) for r in range(rows)]] for array in want]
    counts = want[0]
    most = int(counts.max())
    assert 0 < most < limit and counts[128] != counts[0] and counts[129] != counts[1]
    queries = [planted.queries[r % len(planted.queries)] for r in range(rows)]
    got = (np.full(rows, UNTOUCHED, np.uint64),) + tuple(np.full((rows, limit), UNTOUCHED, np.uint64) for _ in want[1:])
    assert engine.fuzzy_scan_occurrences(queries, planted.text, 1, limit=limit, starts=starts, device=gpu, out=got) is got
    assert engine.last_call_profile().launches == 2 * (4 if starts else 3)
    assert np.array_equal(got[0], counts), np.flatnonzero(got[0] != counts)[:8]
    for matrix, wanted in zip(got[1:], want[1:]):
        assert np.array_equal(matrix[:, :most], wanted[:, :most]), np.argwhere(matrix[:, :most] != wanted[:, :most])[:4]
        assert (matrix[:, most:] == EMPTY).all()


def test_determinism_and_the_profile(gpu, engine, piece, planted):
    queries, text = planted.queries, planted.text
    filled = sum(1 for query in queries if query)
    for value in (64, 4096):
        piece(value)
        once = walked_cells(queries, len(text), value)
        for limit, starts, launches in ((0, True, 2), (16, False, 3), (16, True, 4)):
            first = engine.fuzzy_scan_occurrences(queries, text, 3, limit=limit, starts=starts, device=gpu)
            profile = engine.last_call_profile()
            again = engine.fuzzy_scan_occurrences(queries, text, 3, limit=limit, starts=starts, device=gpu)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
            assert profile.launches == launches and profile.pairs == filled and profile.longest_query == 256
            # the counting form walks the text once; the write pass at most once more, the starts at most limit x (m + 3) bytes a row
            reverse = sum(len(query) * 16 * (len(query) + 3) for query in queries) if starts else 0
            assert (profile.cells == once) if not limit else (once < profile.cells <= 2 * once + reverse)
            assert engine.last_call_profile().cells == profile.cells
            assert profile.kernel_milliseconds > 0 and profile.host_milliseconds >= profile.kernel_milliseconds

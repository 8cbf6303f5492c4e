"""Fuzzy scan matches on the GPU (`szs_rocm_fuzzy_scan_matches*`, `_Engine.fuzzy_scan_matches`): the count of
every query and its leftmost hits against the plain NumPy DP below - the last row D[m][j] of the semi-global DP, every column of it -
and against `engine.fuzzy_scan` on the same GPU.  The text has about 9000 bytes; the `fuzzy_scan_piece` knob at 64 makes that 141
pieces, three workgroups a row."""
import ctypes
import random

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi

pytestmark = pytest.mark.gpu

UNTOUCHED = 0x5A5A5A5A5A5A5A5A
EMPTY = np.uint64(2**64 - 1)
QUERY_LENGTHS = (0, 1, 31, 32, 33, 64, 65, 128, 255, 256)  # every word boundary of the kernel's eight widths
PIECES = (64, 128, 4096, None)
N = 9001


def _last_rows(queries, texts, free_start):
    """D[m_q][j] of the unit-cost DP of every query against ITS text, for j = 0 ... the longest text: a (queries, columns + 1) matrix.
    Row zero is 0 (a free start in the text) or j (the global DP).  The rows below a query's own do not reach into it."""
    count, deepest = len(queries), max(max((len(query) for query in queries), default=0), 1)
    lengths = np.array([len(query) for query in queries])
    widest = max((len(text) for text in texts), default=0)
    patterns, padded = np.zeros((count, deepest), np.uint8), np.zeros((count, max(widest, 1)), np.uint8)
    for at, (query, text) in enumerate(zip(queries, texts)):
        patterns[at, :len(query)] = np.frombuffer(query, np.uint8)
        padded[at, :len(text)] = np.frombuffer(text, np.uint8)
    rows = np.arange(deepest + 1)
    column = np.tile(rows, (count, 1))
    last = np.zeros((count, widest + 1), np.int64)
    last[:, 0] = lengths
    for j in range(1, widest + 1):
        step = np.full_like(column, 0 if free_start else j)
        step[:, 1:] = np.minimum(column[:, :-1] + (patterns != padded[:, j - 1, None]), column[:, 1:] + 1)
        column = np.minimum.accumulate(step - rows, axis=1) + rows  # the insertions down the column
        last[:, j] = column[np.arange(count), lengths]
    return last


def last_rows(queries, text):
    last = _last_rows(list(queries), [bytes(text)] * len(queries), free_start=True)
    last.setflags(write=False)
    return last


def expected(queries, last, bound, limit):
    """(counts, distances, ends) as the call returns them, from the last rows: a query of no bytes has no hit, column 0 never is one."""
    counts = np.zeros(len(queries), np.uint64)
    distances, ends = np.full((len(queries), limit), EMPTY, np.uint64), np.full((len(queries), limit), EMPTY, np.uint64)
    for q, query in enumerate(queries):
        if not query:
            continue
        hits = np.flatnonzero(last[q, 1:] <= bound) + 1
        counts[q] = len(hits)
        kept = hits[:limit]
        ends[q, :len(kept)], distances[q, :len(kept)] = kept, last[q, kept]
    return counts, distances, ends


def same(got, want):
    return len(got) == len(want) and all(g.dtype == np.uint64 and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def walked_cells(queries, n, piece):
    """What one pass counts: m x the bytes walked - the text, and min(p P, 2 m) ahead of every piece."""
    pieces = -(-n // piece)
    return sum(len(query) * (n + sum(min(p * piece, 2 * len(query)) for p in range(pieces))) for query in queries)


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


def _mutated(rng, query, alphabet, edits):
    copy = bytearray(query)
    for _ in range(edits):
        kind, at = rng.randint(0, 2), rng.randrange(len(copy)) if copy else 0
        if kind == 0 and copy:
            copy[at] = rng.choice(alphabet)
        elif kind == 1 and len(copy) > 1:
            del copy[at]
        else:
            copy.insert(at, rng.choice(alphabet))
    return bytes(copy)


@pytest.fixture(scope="module")
def planted():
    """A query of every length, one more that is planted nowhere, a text of N bytes over ACGT with copies of every query under 0 to 3
    edits - four a query in turn, 23 bytes between one copy and the next (every alignment against the 64-byte pieces, most of them
    across a multiple of 64, the last turn behind column 4096), then one of query 33 that ends 10 bytes behind column 4096 and one of
    query 64 that ends 5 bytes behind column 8192 - and the DP's last rows."""
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
    assert 4096 + 10 < at < 8192 - 64
    text[4096 + 10 - 33:4096 + 10] = queries[4]
    text[8192 + 5 - 64:8192 + 5] = queries[5]
    text = bytes(text[:N])
    return queries, text, last_rows(queries, text)


@pytest.mark.parametrize("max_distance", [0, 1, 3])
@pytest.mark.parametrize("value", PIECES, ids=lambda value: f"piece-{value}")
def test_every_width_and_piece(gpu, engine, piece, planted, value, max_distance):
    queries, text, last = planted
    piece(value)
    size = value or 4096
    assert _abi.fuzzy_scan_probe(len(queries), 256, len(text))[:2] == (size, -(-N // size))
    limit = N  # at least the largest count
    want = expected(queries, last, max_distance, limit)
    got = engine.fuzzy_scan_matches(queries, text, max_distance, limit=limit, device=gpu)
    assert [array.shape for array in got] == [(len(queries),), (len(queries), limit), (len(queries), limit)]
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert same(got, want), [np.argwhere(g != w)[:4] for g, w in zip(got, want)]
    for q in range(len(queries)):  # the empty slots are all ones
        assert (got[1][q, int(got[0][q]):] == EMPTY).all() and (got[2][q, int(got[0][q]):] == EMPTY).all()
    # what the oracle must hold for this to have tested the cut: a row without a hit, a row with hits in two chunks of 64 pieces,
    # a hit within 2 m behind a piece boundary - where only the warm-up gives the lane the start of its match
    counts, _, ends = want
    assert any(counts[q] == 0 for q, query in enumerate(queries) if query)
    chunk = 64 * size
    if N > chunk:
        assert any(len({(int(j) - 1) // chunk for j in ends[q, :int(counts[q])]}) >= 2 for q in range(len(queries)))
    assert any(0 < int(j) - (int(j) - 1) // size * size <= 2 * len(queries[q]) and int(j) > size
               for q in range(len(queries)) if len(queries[q]) > 1 for j in ends[q, :int(counts[q])])


@pytest.mark.parametrize("limit", [0, 1, 3, 7])
def test_capacity(gpu, engine, piece, planted, limit):
    queries, text, last = planted
    rows = len(queries)
    piece(64)
    for max_distance in (0, 1):
        full = expected(queries, last, max_distance, N)[0]
        assert (full > limit).any() and (full == 0).any()  # rows above and below the limit ...
        # ... and rows with hits within it (at a bound of 1 the columns next to a copy are hits too: no such row has fewer than 4)
        assert not limit or ((full > 0) & (full <= limit)).any() or (max_distance == 1 and limit < 4)
        want = expected(queries, last, max_distance, limit)
        assert np.array_equal(want[0], full)  # the counts are full, whatever the limit
        got = engine.fuzzy_scan_matches(queries, text, max_distance, limit=limit, device=gpu)
        assert same(got, want), [np.argwhere(g != w)[:4] for g, w in zip(got, want)]
    if limit:
        return
    # the counting form: the matrices are never touched - (rows, 0) arrays through Python, NULL through the raw ABI
    out = (np.full(rows, UNTOUCHED, np.uint64), np.full((rows, 0), UNTOUCHED, np.uint64), np.full((rows, 0), UNTOUCHED, np.uint64))
    assert engine.fuzzy_scan_matches(queries, text, 1, limit=0, device=gpu, out=out) is out
    assert np.array_equal(out[0], full) and out[1].shape == out[2].shape == (rows, 0)
    import torch

    on_device = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    tape, error, counts = szs.Strs(queries)._tape(0), ctypes.c_char_p(), np.full(rows, UNTOUCHED, np.uint64)
    status = _abi.lib.szs_rocm_fuzzy_scan_matches_u32tape(engine.handle, gpu.handle, ctypes.byref(tape), on_device.data_ptr(), len(text), 1, 0,
                                                          counts.ctypes.data, None, None, ctypes.byref(error))
    assert status == 0, error.value
    assert np.array_equal(counts, full)
    assert engine.last_call_profile().launches == 2


def test_every_column_a_hit(gpu, engine, piece, planted):
    """A bound of 256: the prefix runs across every piece, and every chunk behind the first returns before it builds a table."""
    queries, text, last = planted
    for value in (64, None):
        piece(value)
        counts, distances, ends = engine.fuzzy_scan_matches(queries, text, 256, limit=100, device=gpu)
        for q, query in enumerate(queries):
            if not query:
                assert counts[q] == 0 and (distances[q] == EMPTY).all() and (ends[q] == EMPTY).all()
                continue
            assert counts[q] == N and np.array_equal(ends[q], np.arange(1, 101, dtype=np.uint64))
            assert np.array_equal(distances[q], last[q, 1:101].astype(np.uint64))
    assert same(engine.fuzzy_scan_matches(queries, text, 2**64 - 1, limit=100, device=gpu), (counts, distances, ends))  # any bound is taken


@pytest.mark.parametrize("max_distance", [0, 2, 5])
def test_agreement_with_fuzzy_scan(gpu, engine, piece, planted, max_distance):
    queries, text, _ = planted
    piece(128)
    limit = 512
    scan_distances, scan_ends = engine.fuzzy_scan(queries, text, device=gpu)
    counts, distances, ends = engine.fuzzy_scan_matches(queries, text, max_distance, limit=limit, device=gpu)
    compared = 0
    for q, query in enumerate(queries):
        if not query:  # the scan gives a query of no bytes (0, 0), the empty match; here it has no hit
            assert counts[q] == 0
            continue
        assert (counts[q] > 0) == (scan_distances[q] <= max_distance), q
        if 0 < counts[q] <= limit and scan_ends[q] >= 1:
            kept = int(counts[q])
            best = int(np.argmin(distances[q, :kept]))  # the first of the smallest: the leftmost hit of minimum distance
            assert (int(distances[q, best]), int(ends[q, best])) == (int(scan_distances[q]), int(scan_ends[q])), q
            compared += 1
    assert compared >= 3


def test_edges(gpu, engine, piece):
    rng = random.Random(7)
    query = bytes(rng.choice(b"ACGT") for _ in range(40))
    queries = [query, b"", b"G", query[:9]]
    for value in (64, None):
        piece(value)
        # an empty text: no hit, no launch, zeros and ones
        got = engine.fuzzy_scan_matches(queries, b"", 3, limit=4, device=gpu)
        assert same(got, (np.zeros(4, np.uint64), np.full((4, 4), EMPTY), np.full((4, 4), EMPTY)))
        profile = engine.last_call_profile()
        assert profile.launches == 0 and profile.pairs == 0 and profile.cells == 0
        assert same(engine.fuzzy_scan_matches(queries, b"", 3, limit=0, device=gpu)[:1], (np.zeros(4, np.uint64),))
        # a text shorter than the query; a text of exactly k pieces and one byte more; a hit at j = n; a hit at j = 1
        filler = bytes(rng.choice(b"ACGT") for _ in range(5 * 64 + 1))
        texts = [query[:17], b"G", filler[:5 * 64], filler, filler[:5 * 64 - 40] + query, filler[:5 * 64 + 1 - 40] + query,
                 b"G" + filler[:200], query[-1:] + filler[:64]]
        for text in texts:
            last = last_rows(queries, text)
            for max_distance in (0, 2, 39):
                want = expected(queries, last, max_distance, len(text))
                got = engine.fuzzy_scan_matches(queries, text, max_distance, limit=len(text), device=gpu)
                assert same(got, want), (len(text), max_distance)
        last = last_rows(queries, texts[4])
        counts, _, ends = expected(queries, last, 0, 8)
        assert counts[0] == 1 and ends[0, 0] == len(texts[4]) == 5 * 64  # the one exact copy ends at j = n, a multiple of the piece
        assert expected(queries, last_rows(queries, texts[5]), 0, 8)[2][0, 0] == 5 * 64 + 1
        assert expected(queries, last_rows(queries, texts[6]), 0, 8)[2][2, 0] == 1  # "G" at j = 1
    got = engine.fuzzy_scan_matches([], b"ACGT", 1, limit=3, device=gpu)
    assert [array.shape for array in got] == [(0,), (0, 3), (0, 3)]


def test_outputs_and_memory_kinds(gpu, engine, piece, planted):
    import torch

    queries, text, last = planted
    rows, limit = len(queries), 5
    piece(128)
    want = expected(queries, last, 2, limit)
    assert same(engine.fuzzy_scan_matches(queries, text, 2, limit=limit, device=gpu), want)  # returned arrays

    def as_numpy(array):
        return array if isinstance(array, np.ndarray) else array.cpu().numpy().view(np.uint64)

    on_device = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    for text_form in (text, np.frombuffer(text, np.uint8), on_device):
        for make in (lambda *shape: np.full(shape, UNTOUCHED, np.uint64),             # plain host memory: staged and copied home
                     lambda *shape: torch.full(shape, 7, dtype=torch.int64).cuda(),   # on the device: written where it is
                     lambda *shape: torch.full(shape, 7, dtype=torch.int64).pin_memory()):
            out = (make(rows), make(rows, limit), make(rows, limit))
            assert engine.fuzzy_scan_matches(queries, text_form, 2, limit=limit, device=gpu, out=out) is out
            assert same([as_numpy(array) for array in out], want), type(text_form)
    out = (np.full(rows, UNTOUCHED, np.uint64), torch.full((rows, limit), 7, dtype=torch.int64).cuda(), np.full((rows, limit), UNTOUCHED, np.uint64))
    engine.fuzzy_scan_matches(queries, on_device, 2, limit=limit, device=gpu, out=out)  # one on the device among staged ones
    assert same([as_numpy(array) for array in out], want)
    assert same(engine.fuzzy_scan_matches(szs.Strs(queries, wide_offsets=True), on_device, 2, limit=limit, device=gpu), want)  # a u64 tape

    # the callback sequence through the raw ABI, and a text the device cannot read
    q32 = szs.Strs(queries)
    q32._tape(0)
    data, offsets = q32._device[1].data_ptr(), q32.offsets
    sequence = _abi.Sequence(None, rows, _abi.MEMBER_START(lambda handle, i: data + int(offsets[i])),
                             _abi.MEMBER_LENGTH(lambda handle, i: int(offsets[i + 1] - offsets[i])))
    triple, error = [np.full(rows, UNTOUCHED, np.uint64)] + [np.full((rows, limit), UNTOUCHED, np.uint64) for _ in range(2)], ctypes.c_char_p()
    status = _abi.lib.szs_rocm_fuzzy_scan_matches(engine.handle, gpu.handle, ctypes.byref(sequence), on_device.data_ptr(), len(text), 2, limit,
                                                  *(array.ctypes.data for array in triple), ctypes.byref(error))
    assert status == 0, error.value
    assert same(triple, want)
    host_text = np.frombuffer(text, np.uint8).copy()
    status = _abi.lib.szs_rocm_fuzzy_scan_matches(engine.handle, gpu.handle, ctypes.byref(sequence), host_text.ctypes.data, len(text), 2, limit,
                                                  *(array.ctypes.data for array in triple), ctypes.byref(error))
    assert _abi.STATUS_NAMES[status] == "unknown" and error.value and same(triple, want)  # nothing written

    # a query of 257 bytes among valid ones: refused before anything is launched, the sentinels intact
    out = (np.full(3, UNTOUCHED, np.uint64), np.full((3, limit), UNTOUCHED, np.uint64), np.full((3, limit), UNTOUCHED, np.uint64))
    with pytest.raises(szs.StringZillasError) as refused:
        engine.fuzzy_scan_matches([b"AC", b"A" * 257, b"ACGT"], text, 2, limit=limit, device=gpu, out=out)
    assert refused.value.status_name == "unexpected_dimensions" and "256" in str(refused.value)
    assert all((array == UNTOUCHED).all() for array in out)
    assert same(engine.fuzzy_scan_matches(queries, text, 2, limit=limit, device=gpu), want)  # and the call afterwards


class TwoBlocks:
    """What makes the scratch cap cut a call in two, and its oracle.  At a piece of 64 a text of 2^20 bytes has 256 chunks, a row's
    scratch is 256 x 65 x 4 = 66,560 bytes and a block floor(2^28 / 66,560) = 4,032 rows: 4,037 queries leave 5 for a second block.
    The queries cycle through 37 patterns of 4 to 8 bytes over ACGT; 4,032 mod 37 = 36, so rows r and r - 4,032 never hold the same
    pattern - the last five hold patterns 36, 0, 1, 2 and 3.  The text is the filler byte `x` but for two windows of 2,000 bytes with
    copies under 0 or 1 edits: one across column 4096 - a chunk boundary - and one that ends 30 bytes before the text does.  On filler
    the DP's column is 0 ... m again after m bytes and m > the bound, so the hits of the text are those of the windows, shifted:
    `windows` holds (offset, patterns' last rows over the window's bytes)."""
    ROWS, BLOCK, PATTERNS, N, PIECE, BOUND, LIMIT, EDGE = 4037, 4032, 37, 1 << 20, 64, 1, 4, 8

    def __init__(self):
        rng = random.Random(1812)
        alphabet = b"ACGT"
        once = [2, 5, 36]  # of the last five rows' patterns 36 and 2 are planted once a window, 0 and 3 often, 1 nowhere
        often = [p for p in range(self.PATTERNS) if p % 3 == 0 and p not in once]
        self.patterns = []
        while len(self.patterns) < self.PATTERNS:  # (8 bytes where a count is to stay small: no other copy comes within the bound)
            length = 8 if len(self.patterns) in once + [1] else rng.randint(4, 8)
            pattern = bytes(rng.choice(alphabet) for _ in range(length))
            if pattern not in self.patterns:
                self.patterns.append(pattern)
        self.queries = [self.patterns[r % self.PATTERNS] for r in range(self.ROWS)]
        text = bytearray(b"x" * self.N)
        self.windows = []
        for offset in (4096 - 1000, self.N - 30 - 2000):
            at, end = offset + 2 * self.EDGE, offset + 2000 - 2 * self.EDGE
            for p in once:  # one copy, its first byte replaced by filler: one hit at distance 1, fewer than the limit in all
                text[at:at + len(self.patterns[p])] = b"x" + self.patterns[p][1:]
                at += len(self.patterns[p]) + 11
            while at + 10 < end:
                copy = _mutated(rng, self.patterns[rng.choice(often)], alphabet, rng.randint(0, 1))
                text[at:at + len(copy)] = copy
                at += len(copy) + rng.randint(3, 11)
            window = bytes(text[offset:offset + 2000])
            assert window[:self.EDGE] == window[-self.EDGE:] == b"x" * self.EDGE
            self.windows.append((offset, window, last_rows(self.patterns, window)))
        assert text[4090:4102].count(b"x") < 12  # planted bytes on both sides of the chunk boundary
        self.text = bytes(text)

    def per_row(self, per_pattern):
        """Rows of (ends, distances, ...) per pattern, each ascending in the text, as the call's (counts, matrices ...) per query: the
        leftmost LIMIT of every row."""
        width = len(per_pattern[0])
        counts = np.array([len(per_pattern[r % self.PATTERNS][0]) for r in range(self.ROWS)], np.uint64)
        matrices = [np.full((self.ROWS, self.LIMIT), EMPTY, np.uint64) for _ in range(width)]
        for r in range(self.ROWS):
            for matrix, values in zip(matrices, per_pattern[r % self.PATTERNS]):
                matrix[r, :min(len(values), self.LIMIT)] = values[:self.LIMIT]
        # what the oracle must hold: rows above, below and without the limit in both blocks, and a second block that differs from
        # what the first block's rows - a wrong first row - would give
        for rows in (slice(0, self.BLOCK), slice(self.BLOCK, self.ROWS)):
            assert (counts[rows] > self.LIMIT).any() and (counts[rows] == 0).any() and ((counts[rows] > 0) & (counts[rows] < self.LIMIT)).any()
        assert all(not np.array_equal(matrices[-1][self.BLOCK + r], matrices[-1][r]) for r in range(self.ROWS - self.BLOCK))  # the ends
        return (counts, *matrices)

    def expected(self):
        """(counts, distances, ends) of fuzzy scan matches."""
        per_pattern = []
        for p in range(self.PATTERNS):
            ends, distances = [], []
            for offset, window, last in self.windows:
                hits = np.flatnonzero(last[p, 1:] <= self.BOUND) + 1
                assert not len(hits) or (self.EDGE < hits[0] and hits[-1] <= len(window) - self.EDGE)  # what makes the windows exact
                ends.append(hits + offset), distances.append(last[p, hits])
            per_pattern.append((np.concatenate(distances).astype(np.uint64), np.concatenate(ends).astype(np.uint64)))
        return self.per_row(per_pattern)


@pytest.fixture(scope="module")
def two_blocks():
    return TwoBlocks()


def on_device_outputs(rows, limit, matrices):
    import torch

    return (torch.full((rows,), 7, dtype=torch.int64).cuda(),) + tuple(torch.full((rows, limit), 7, dtype=torch.int64).cuda() for _ in range(matrices))


def test_two_blocks_through_the_scratch_cap(gpu, engine, piece, two_blocks):
    """Outputs in device memory, written where they are: the second block's rows, queries and scratch begin where the first's end."""
    import torch

    case = two_blocks
    piece(case.PIECE)
    assert _abi.fuzzy_scan_probe(case.ROWS, 8, case.N)[:2] == (case.PIECE, case.N // case.PIECE)
    want = case.expected()
    on_device = torch.frombuffer(bytearray(case.text), dtype=torch.uint8).cuda()
    out = on_device_outputs(case.ROWS, case.LIMIT, 2)
    assert engine.fuzzy_scan_matches(case.queries, on_device, case.BOUND, limit=case.LIMIT, device=gpu, out=out) is out
    assert engine.last_call_profile().launches == 2 * 3
    got = [array.cpu().numpy().view(np.uint64) for array in out]
    assert np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])[:8]
    assert same(got, want), [np.argwhere(g != w)[:4] for g, w in zip(got, want)]  # every filled slot, and all ones behind them
    for matrix in got[1:]:
        assert all((matrix[r, int(count):] == EMPTY).all() for r, count in enumerate(want[0]) if count < case.LIMIT)


def test_two_blocks_through_the_staging_budget(gpu, engine, piece, planted):
    """Outputs in plain host memory: with 2^17 slots a row a staged block is 128 MiB / (2^17 x 8) = 128 rows, and 130 queries leave 2
    for a second one.  128 mod 11 = 7: rows r and r - 128 never hold the same query."""
    queries, text, last = planted
    rows, limit = 130, 1 << 17
    queries, last = [queries[r % len(queries)] for r in range(rows)], last[[r % len(queries) for r in range(rows)]]
    piece(64)
    counts, distances, ends = expected(queries, last, 1, N)
    most = int(counts.max())
    assert 0 < most < limit and counts[128] != counts[0] and counts[129] != counts[1]
    got = (np.full(rows, UNTOUCHED, np.uint64), np.full((rows, limit), UNTOUCHED, np.uint64), np.full((rows, limit), UNTOUCHED, np.uint64))
    assert engine.fuzzy_scan_matches(queries, text, 1, limit=limit, device=gpu, out=got) is got
    assert engine.last_call_profile().launches == 2 * 3
    assert np.array_equal(got[0], counts), np.flatnonzero(got[0] != counts)[:8]
    for matrix, want in zip(got[1:], (distances, ends)):
        assert np.array_equal(matrix[:, :most], want[:, :most]), np.argwhere(matrix[:, :most] != want[:, :most])[:4]
        assert (matrix[:, most:] == EMPTY).all()


def test_determinism_and_the_profile(gpu, engine, piece, planted):
    queries, text, last = planted
    filled = sum(1 for query in queries if query)
    for value in (64, 4096):
        piece(value)
        for limit, launches in ((0, 2), (16, 3)):
            first = engine.fuzzy_scan_matches(queries, text, 3, limit=limit, device=gpu)
            profile = engine.last_call_profile()
            again = engine.fuzzy_scan_matches(queries, text, 3, limit=limit, device=gpu)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
            assert profile.launches == launches and profile.pairs == filled and profile.longest_query == 256
            once = walked_cells(queries, len(text), value)
            assert once <= profile.cells <= 2 * once
            assert profile.cells == once or limit  # the counting form walks the text once
            assert engine.last_call_profile().cells == profile.cells
            assert profile.kernel_milliseconds > 0 and profile.host_milliseconds >= profile.kernel_milliseconds

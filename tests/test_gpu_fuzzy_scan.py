"""Fuzzy scan on the GPU (`szs_rocm_fuzzy_scan*`, `_Engine.fuzzy_scan`): every distance, start and end of
every query inside ONE text against two oracles - the plain NumPy DP below (the semi-global DP for (distance, end), then the global DP
of the reversed query over text[:end] reversed for the start: the smallest t that attains the distance) and the existing
`engine.fuzzy_find(queries, [text], starts=True)` on the same GPU, bit for bit.  Texts are a few KB; the `fuzzy_scan_piece` knob at 64
makes that a hundred pieces and more than one workgroup a row."""
import ctypes
import functools
import random

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi, matrices

pytestmark = pytest.mark.gpu

UNTOUCHED = 0x5A5A5A5A5A5A5A5A
QUERY_LENGTHS = (0, 1, 31, 32, 33, 64, 65, 128, 255, 256)  # every word boundary of the kernel's eight widths
PIECES = (64, 128, 4096, None)


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


def oracle(queries, text):
    """(distances, starts, ends) of every query inside `text`, uint64 vectors - computed once per input, read-only."""
    return _oracle(tuple(queries), bytes(text))


@functools.lru_cache(maxsize=None)
def _oracle(queries, text):
    last = _last_rows(queries, [text] * len(queries), free_start=True)
    best = last.min(axis=1)
    end = (last == best[:, None]).argmax(axis=1)  # the smallest j that attains it
    heads = [text[:int(e)][::-1] for e in end]
    back_rows = _last_rows([query[::-1] for query in queries], heads, free_start=False)
    back = np.zeros(len(queries), np.int64)
    for q, e in enumerate(end):
        row = back_rows[q, :int(e) + 1]
        assert row.min() == best[q]  # some start attains d, none gives less
        back[q] = int((row == best[q]).argmax())  # the smallest t: the shortest match
    triple = tuple(vector.astype(np.uint64) for vector in (best, end - back, end))
    for vector in triple:
        vector.setflags(write=False)
    return triple


def same(got, want):
    return len(got) == len(want) and all(g.dtype == np.uint64 and np.array_equal(g, w) for g, w in zip(got, want))


def walked_cells(queries, n, piece):
    """What the scan counts: m x the bytes walked - the text, and min(p P, 2 m) ahead of every piece."""
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


def _widths(alphabet, seed, n):
    """Two queries of every length, interleaved (0 next to 256, 1 next to 255 ...), a text of `n` bytes with a mutated copy of every
    query planted 240 bytes apart - at every alignment against the 64-byte pieces - and the DP's triple."""
    rng = random.Random(seed)
    ascending = [bytes(rng.choice(alphabet) for _ in range(length)) for length in QUERY_LENGTHS for _ in range(2)]
    queries = []
    while ascending:
        queries.append(ascending.pop(0))
        if ascending:
            queries.append(ascending.pop())
    text = bytearray(rng.choice(alphabet) for _ in range(n))
    for at, query in enumerate(queries):
        copy = _mutated(rng, query, alphabet, rng.randint(0, 1 + len(query) // 16))
        text[7 + 240 * at:7 + 240 * at + len(copy)] = copy
    text = bytes(text[:n])
    return queries, text, oracle(queries, text)


@pytest.fixture(scope="module")
def widths_acgt():
    return _widths(b"ACGT", 51, 5000)


@pytest.fixture(scope="module")
def widths_bytes():
    return _widths(bytes(range(256)), 53, 5000)


def _find(engine, gpu, queries, text):
    """The existing route: the whole text as the one candidate of the dense form, column 0."""
    return tuple(matrix[:, 0] for matrix in engine.fuzzy_find(queries, [text], device=gpu, starts=True))


def test_every_width_against_both_oracles(gpu, engine, piece, widths_acgt):
    queries, text, want = widths_acgt
    piece(64)
    assert _abi.fuzzy_scan_probe(len(queries), 256, len(text))[:3] == (64, 79, 2 * len(queries))  # two chunks: the fold crosses workgroups
    got = engine.fuzzy_scan(queries, text, device=gpu, starts=True)
    assert all(vector.shape == (len(queries),) for vector in got)
    assert same(got, want), [np.flatnonzero(g != w)[:8] for g, w in zip(got, want)]
    assert same(got, _find(engine, gpu, queries, text))
    plain = engine.fuzzy_scan(queries, text, device=gpu)  # without starts: the same distances and ends
    assert same(plain, (want[0], want[2]))


def _planted(query, at, n=5000, filler=b"x"):
    text = bytearray(filler * n)
    text[at:at + len(query)] = query
    return bytes(text)


@pytest.mark.parametrize("end", [5 * 64 - 1, 5 * 64, 5 * 64 + 1, 5 * 64 + 20, 64 * 64 - 1, 64 * 64, 64 * 64 + 1, 64 * 64 + 24],
                         ids=["before", "at", "behind", "straddles-pieces", "before-chunk", "at-chunk", "behind-chunk", "straddles-chunks"])
def test_boundaries_of_pieces_and_chunks(gpu, engine, piece, end):
    rng = random.Random(end)
    query = bytes(rng.choice(b"ACGT") for _ in range(40))
    piece(64)
    text = _planted(query, end - 40)
    got = engine.fuzzy_scan([query], text, device=gpu, starts=True)
    assert [int(vector[0]) for vector in got] == [0, end - 40, end]  # by hand: the one exact copy
    broken = bytearray(text)
    broken[end - 20] = ord("x")  # one substitution inside the copy: nothing ends earlier at distance 1
    got = engine.fuzzy_scan([query], bytes(broken), device=gpu, starts=True)
    assert [int(vector[0]) for vector in got] == [1, end - 40, end]
    assert same(got, oracle([query], bytes(broken)))


def test_ties_go_to_the_leftmost_end(gpu, engine, piece):
    rng = random.Random(3)
    query = bytes(rng.choice(b"ACGT") for _ in range(40))
    piece(64)
    text = bytearray(_planted(query, 3 * 64 + 8))  # the same exact copy in pieces 3 and 70
    text[70 * 64 + 10:70 * 64 + 50] = query
    got = engine.fuzzy_scan([query], bytes(text), device=gpu, starts=True)
    assert [int(vector[0]) for vector in got] == [0, 200, 240]
    text[200 + 13] = text[70 * 64 + 10 + 29] = ord("x")  # one error each, and nothing better
    got = engine.fuzzy_scan([query], bytes(text), device=gpu, starts=True)
    assert [int(vector[0]) for vector in got] == [1, 200, 240]
    assert same(got, oracle([query], bytes(text))) and same(got, _find(engine, gpu, [query], bytes(text)))
    text[200:240] = b"x" * 40  # the left one gone: the right one is found
    got = engine.fuzzy_scan([query], bytes(text), device=gpu, starts=True)
    assert [int(vector[0]) for vector in got] == [1, 70 * 64 + 10, 70 * 64 + 50]


@pytest.mark.parametrize("value", PIECES)
def test_nothing_occurs_and_the_fixed_results(gpu, engine, piece, value):
    piece(value)
    queries = [b"ACGT" * 10, b"", b"G", b"TTGACA" * 40]
    for text in (b"x" * 5000, b"x" * (3 * 64), b"x" * 8192, b"x", b""):
        got = engine.fuzzy_scan(queries, text, device=gpu, starts=True)
        assert [vector.tolist() for vector in got] == [[40, 0, 1, 240], [0] * 4, [0] * 4], len(text)  # (m, 0, 0); the empty query (0, 0, 0)
    # a text shorter than the query, a text of one byte, a text of exactly k P bytes
    for text in (b"ACG", b"G", bytes(random.Random(9).choice(b"ACGT") for _ in range(3 * 64)), bytes(random.Random(10).choice(b"ACGT") for _ in range(8192))):
        got = engine.fuzzy_scan(queries, text, device=gpu, starts=True)
        assert same(got, oracle(queries, text)), len(text)
        assert same(got, _find(engine, gpu, queries, text)), len(text)
    got = engine.fuzzy_scan([], b"ACGT", device=gpu, starts=True)
    assert [vector.shape for vector in got] == [(0,)] * 3


def test_every_byte_value(gpu, engine, piece, widths_bytes):
    queries, text, want = widths_bytes
    queries = list(queries) + [b"\x00" * 9, b"\x00\xff\x80\x7f" * 5, bytes(range(128, 256))]
    text = text[:1000] + b"\x00" * 8 + text[1000:3000] + b"\x00\xff\x80\x7f" * 4 + b"\x80" + bytes(range(130, 256)) + text[3000:]
    want = oracle(queries, text)
    piece(64)
    got = engine.fuzzy_scan(queries, text, device=gpu, starts=True)
    assert same(got, want), [np.flatnonzero(g != w)[:8] for g, w in zip(got, want)]
    assert same(got, _find(engine, gpu, queries, text))


def test_the_knob_changes_no_result(gpu, engine, piece, widths_acgt):
    queries, text, want = widths_acgt
    for value in PIECES:
        piece(value)
        assert same(engine.fuzzy_scan(queries, text, device=gpu, starts=True), want), value
        assert same(engine.fuzzy_scan(queries, text, device=gpu), (want[0], want[2])), value


def test_memory_kinds(gpu, engine, piece, widths_acgt):
    import torch

    queries, text, want = widths_acgt
    rows = len(queries)
    piece(128)

    def as_numpy(vector):
        return vector if isinstance(vector, np.ndarray) else vector.cpu().numpy().view(np.uint64)

    on_device = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    for text_form in (text, bytearray(text), np.frombuffer(text, np.uint8), torch.frombuffer(bytearray(text), dtype=torch.uint8), on_device):
        for make in (lambda: np.full(rows, UNTOUCHED, np.uint64), lambda: torch.full((rows,), 7, dtype=torch.int64).cuda(),
                     lambda: torch.full((rows,), 7, dtype=torch.int64).pin_memory()):
            out = tuple(make() for _ in range(3))
            assert engine.fuzzy_scan(queries, text_form, device=gpu, out=out, starts=True) is out
            assert same([as_numpy(vector) for vector in out], want), type(text_form)
        out = np.full(rows, UNTOUCHED, np.uint64), torch.full((rows,), 7, dtype=torch.int64).cuda()  # one staged, one not
        engine.fuzzy_scan(queries, text_form, device=gpu, out=out)
        assert same([as_numpy(vector) for vector in out], (want[0], want[2]))
    wide = szs.Strs(queries, wide_offsets=True)  # a u64 tape
    assert same(engine.fuzzy_scan(wide, on_device, device=gpu, starts=True), want)

    # the C entries: `ends` NULL, and the callback sequence
    q32 = szs.Strs(queries)
    tape = q32._tape(0)
    error, distances = ctypes.c_char_p(), np.full(rows, UNTOUCHED, np.uint64)
    status = _abi.lib.szs_rocm_fuzzy_scan_u32tape(engine.handle, gpu.handle, ctypes.byref(tape), on_device.data_ptr(), len(text),
                                                  distances.ctypes.data, None, ctypes.byref(error))
    assert status == 0, error.value
    assert np.array_equal(distances, want[0])
    data, offsets = q32._device[1].data_ptr(), q32.offsets
    sequence = _abi.Sequence(None, rows, _abi.MEMBER_START(lambda handle, i: data + int(offsets[i])),
                             _abi.MEMBER_LENGTH(lambda handle, i: int(offsets[i + 1] - offsets[i])))
    triple = [np.full(rows, UNTOUCHED, np.uint64) for _ in range(3)]
    status = _abi.lib.szs_rocm_fuzzy_scan_spans(engine.handle, gpu.handle, ctypes.byref(sequence), on_device.data_ptr(), len(text),
                                                *(vector.ctypes.data for vector in triple), ctypes.byref(error))
    assert status == 0, error.value
    assert same(triple, want)
    host_text = np.frombuffer(text, np.uint8).copy()  # plain host memory: not a text the device can read
    status = _abi.lib.szs_rocm_fuzzy_scan_spans(engine.handle, gpu.handle, ctypes.byref(sequence), host_text.ctypes.data, len(text),
                                                *(vector.ctypes.data for vector in triple), ctypes.byref(error))
    assert _abi.STATUS_NAMES[status] == "unknown" and error.value and same(triple, want)  # nothing written


def test_refusals_and_the_calls_afterwards(gpu, engine, piece):
    queries, text = [b"ACGT", b"AC", b"GATTACA"], b"TTGATTACCAACGGT" * 20
    piece(64)
    before = engine.fuzzy_find(queries, [text], device=gpu, starts=True)
    out = tuple(np.full(3, UNTOUCHED, np.uint64) for _ in range(3))
    with pytest.raises(szs.StringZillasError) as refused:  # one query beyond the bit-vector, among valid ones
        engine.fuzzy_scan([b"AC", b"A" * 257, b"ACGT"], text, device=gpu, out=out, starts=True)
    assert refused.value.status_name == "unexpected_dimensions" and "256" in str(refused.value)
    assert all((vector == UNTOUCHED).all() for vector in out)
    got = engine.fuzzy_scan([b"AC", b"A" * 256, b"ACGT"], text, device=gpu, starts=True)
    assert same(got, oracle([b"AC", b"A" * 256, b"ACGT"], text))
    after = engine.fuzzy_find(queries, [text], device=gpu, starts=True)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert same(engine.fuzzy_scan(queries, text, device=gpu, starts=True), tuple(matrix[:, 0] for matrix in before))

    table = matrices.blosum62()
    for other in (szs.LevenshteinDistances(0, 2, 3, 1, capabilities=gpu), szs.LevenshteinDistancesUTF8(capabilities=gpu),
                  szs.NeedlemanWunschScores(*table, open=-4, extend=-4, capabilities=gpu)):
        with pytest.raises(szs.StringZillasError) as refused:
            other.fuzzy_scan(queries, text, device=gpu, out=out, starts=True)
        assert refused.value.status_name == "unknown"
        assert all((vector == UNTOUCHED).all() for vector in out)


def test_the_profile(gpu, engine, piece, widths_acgt):
    queries, text, want = widths_acgt
    filled = sum(1 for query in queries if query)
    for value in (64, 4096):
        piece(value)
        engine.fuzzy_scan(queries, text, device=gpu)
        profile = engine.last_call_profile()
        assert profile.launches == 2 and profile.pairs == filled and profile.longest_query == 256
        assert profile.cells == walked_cells(queries, len(text), value)
        assert profile.kernel_milliseconds > 0 and profile.host_milliseconds >= profile.kernel_milliseconds
        engine.fuzzy_scan(queries, text, device=gpu, starts=True)
        profile = engine.last_call_profile()
        assert profile.launches == 3 and profile.pairs == filled
        windows = sum(len(query) * min(int(e), len(query) + int(d)) for query, d, e in zip(queries, want[0], want[2]))
        assert profile.cells == walked_cells(queries, len(text), value) + windows

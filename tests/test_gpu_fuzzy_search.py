"""Fuzzy search on the GPU (`szs_rocm_fuzzy_search*`, `_Engine.fuzzy_search`): the k candidates with the
smallest semi-global distance per query, against the plain DP below - D[0][j] = 0, D[i][0] = i, unit costs; distance = the minimum of
the last row, end = the smallest j that attains it, start = the shortest match that ends there - and a stable sort on (distance, index)."""
import ctypes
import random

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi, matrices

pytestmark = pytest.mark.gpu

EMPTY = np.uint64(2**64 - 1)
UNTOUCHED = 0x5A5A5A5A5A5A5A5A
QUERY_LENGTHS = (0, 1, 31, 32, 33, 64, 65, 128, 255, 256)  # every word boundary of the kernel's eight widths


def _columns(pattern, texts, lengths, free_start):
    """The last row of the unit-cost DP of `pattern` against every text, column by column: yields (j, D[m][j] per text)."""
    m, rows = len(pattern), np.arange(len(pattern) + 1)
    padded = np.zeros((len(texts), max(int(lengths.max(initial=0)), 1)), np.uint8)
    for at, text in enumerate(texts):
        padded[at, :len(text)] = np.frombuffer(text, np.uint8)
    column = np.tile(rows, (len(texts), 1))
    for j in range(1, int(lengths.max(initial=0)) + 1):
        step = np.full_like(column, 0 if free_start else j)  # row zero: free start in the text, or D[0][j] = j
        step[:, 1:] = np.minimum(column[:, :-1] + (pattern[None, :] != padded[:, j - 1, None]), column[:, 1:] + 1)
        column = np.minimum.accumulate(step - rows, axis=1) + rows  # the insertions down the column
        yield j, column[:, m]


def spans(query, texts):
    """(distances, starts, ends) of `query` inside every text, vectorised over the texts (as tests/test_gpu_fuzzy_spans.py)."""
    m, pattern = len(query), np.frombuffer(query, np.uint8)
    lengths = np.array([len(text) for text in texts], dtype=np.int64)
    best, end = np.full(len(texts), m, np.int64), np.zeros(len(texts), np.int64)
    for j, last in _columns(pattern, texts, lengths, free_start=True):
        better = (j <= lengths) & (last < best)
        best[better], end[better] = last[better], j
    heads = [text[:int(e)][::-1] for text, e in zip(texts, end)]  # c[:end] reversed, against the reversed query
    least, back = np.full(len(texts), m, np.int64), np.zeros(len(texts), np.int64)
    for t, last in _columns(pattern[::-1], heads, end, free_start=False):
        better = (t <= end) & (last < least)
        least[better], back[better] = last[better], t  # strictly smaller: the smallest t, the shortest match
    assert np.array_equal(least, best)
    return best, end - back, end


def dense(queries, candidates):
    """The (queries x candidates) matrices of distances, starts and ends, read-only."""
    if not candidates:
        return tuple(np.zeros((len(queries), 0), np.uint64) for _ in range(3))
    triples = [spans(query, candidates) for query in queries]
    parts = tuple(np.array([triple[part] for triple in triples], dtype=np.uint64).reshape(len(queries), len(candidates)) for part in range(3))
    for matrix in parts:
        matrix.setflags(write=False)
    return parts


def select(want, k, skip_own=False):
    """(indices, distances, starts, ends) of the k best columns per row: a stable sort on the distance, so ties go to the lower index;
    `skip_own`: the self form, row q never lists column q.  Missing slots: (2^64 - 1, 0, 0, 0)."""
    rows, count = want[0].shape
    out = [np.full((rows, k), EMPTY, np.uint64)] + [np.zeros((rows, k), np.uint64) for _ in range(3)]
    for q in range(rows):
        order = np.argsort(want[0][q], kind="stable")
        if skip_own:
            order = order[order != q]
        order = order[:k]
        out[0][q, :len(order)] = order
        for part in range(3):
            out[1 + part][q, :len(order)] = want[part][q, order]
    return tuple(out)


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


def without_starts(quad):
    return quad[0], quad[1], quad[3]


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return szs.DeviceScope(gpu_device=0)


@pytest.fixture(scope="module")
def engine(gpu):
    return szs.LevenshteinDistances(capabilities=gpu)


def _widths(alphabet, seed):
    """Two queries of every length, short and long interleaved; 8 candidates of 0 ... 9 bytes and 142 of U[0, 300] - 150, no multiple of
    64, odd lengths first so that most start at odd tape offsets; one longest query planted whole inside candidate 11."""
    rng = random.Random(seed)
    ascending = [bytes(rng.choice(alphabet) for _ in range(length)) for length in QUERY_LENGTHS for _ in range(2)]
    queries = []
    while ascending:
        queries.append(ascending.pop(0))
        if ascending:
            queries.append(ascending.pop())
    lengths = [1, 3, 0, 4, 5, 7, 8, 9] + [rng.randint(0, 300) for _ in range(142)]
    candidates = [bytes(rng.choice(alphabet) for _ in range(length)) for length in lengths]
    assert len(queries[1]) == 256
    candidates[11] = candidates[10][:20] + queries[1] + candidates[10][20:40]
    return queries, candidates, dense(queries, candidates)


@pytest.fixture(scope="module")
def widths_ab():
    return _widths(b"ab", 41)


@pytest.fixture(scope="module")
def widths_bytes():
    return _widths(bytes(range(256)), 43)


@pytest.fixture
def knobs():
    yield
    _abi.tuning_set("top_k_tile", None)
    _abi.tuning_set("fuzzy_search_segment", None)


@pytest.mark.parametrize("k", [1, 3, 16, 64])
@pytest.mark.parametrize("alphabet", ["ab", "bytes"])
def test_widths(gpu, engine, widths_ab, widths_bytes, alphabet, k):
    queries, candidates, want = widths_ab if alphabet == "ab" else widths_bytes
    got = engine.fuzzy_search(queries, candidates, k=k, device=gpu)
    assert len(got) == 3 and all(matrix.dtype == np.uint64 and matrix.shape == (len(queries), k) for matrix in got)
    expected = without_starts(select(want, k))
    for name, g, w in zip(("indices", "distances", "ends"), got, expected):
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:8])
    assert got[0][1, 0] == 11 and got[1][1, 0] == 0  # the planted query: its text comes first, distance 0
    empty = [q for q, query in enumerate(queries) if not query]
    assert empty and all(got[0][q].tolist() == list(range(k)) and not got[1][q].any() and not got[2][q].any() for q in empty)


@pytest.mark.parametrize("tile", [64, 100])
def test_tiles_and_segments(gpu, engine, knobs, widths_ab, tile):
    queries, candidates, want = widths_ab
    untiled = engine.fuzzy_search(queries, candidates, k=16, device=gpu, starts=True)
    one_tile = engine.last_call_profile()
    assert same(untiled, select(want, 16))
    _abi.tuning_set("top_k_tile", tile)
    _abi.tuning_set("fuzzy_search_segment", 64)
    block, planned_tile, segment, workgroups = _abi.fuzzy_search_probe(len(queries), len(candidates), 16)
    assert (planned_tile, segment) == (tile, 64) and workgroups == len(queries) * -(-tile // 64)  # several segments, a partial chunk
    tiled = engine.fuzzy_search(queries, candidates, k=16, device=gpu, starts=True)
    profile = engine.last_call_profile()
    assert same(tiled, untiled)
    tiles = -(-len(candidates) // tile)
    assert tiles > 1 and profile.launches == one_tile.launches + 2 * (tiles - 1)  # a scoring launch and a scan per tile
    assert profile.pairs == one_tile.pairs and profile.cells == one_tile.cells  # the knobs change no count either
    for k in (1, 64):
        assert same(engine.fuzzy_search(queries, candidates, k=k, device=gpu), without_starts(select(want, k)))


def test_scan_segments_share_a_row(gpu, engine, knobs):
    """3 x 8,200 at the automatic sizes: one tile whose rows the scan splits into two segments (8200 // 4096), at column 5,120.  Strings
    over two letters: every row's ties at the best distance run across that boundary, and the merge of the segments' lists must still
    give them to the lower index."""
    rng = random.Random(77)
    queries = [bytes(rng.choice(b"ab") for _ in range(length)) for length in (1, 4, 6)]
    candidates = [bytes(rng.choice(b"ab") for _ in range(rng.randint(0, 10))) for _ in range(8200)]
    block, tile, _, _ = _abi.fuzzy_search_probe(len(queries), len(candidates), 16)
    assert (block, tile) == (3, 8200)  # one tile of at least 2 x 4096 columns, few rows: the scan takes segments
    cells = dense(queries, candidates)
    assert all((row[:5120] == row.min()).sum() > 16 and (row[5120:] == row.min()).sum() > 16 for row in cells[0])  # full lists of ties on both sides
    want = select(cells, 16)
    got = engine.fuzzy_search(queries, candidates, k=16, device=gpu, starts=True)
    for name, g, w in zip(("indices", "distances", "starts", "ends"), got, want):
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:8])


def test_ties_and_empty_slots(gpu, engine):
    rng = random.Random(12)
    text = bytes(rng.choice(b"ACGT") for _ in range(90))
    candidates = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(40, 120))) for _ in range(70)]
    copies = sorted(rng.sample(range(70), 40))
    for at in copies:
        candidates[at] = text
    queries = [text[30:60], text[10:40] + b"T", bytes(rng.choice(b"ACGT") for _ in range(25)), b"", b"G"]
    want = dense(queries, candidates)
    got = engine.fuzzy_search(queries, candidates, k=16, device=gpu)
    assert same(got, without_starts(select(want, 16)))
    assert got[0][0].tolist() == copies[:16] and not got[1][0].any()  # 40 equal texts: the lower indices, in order
    assert (got[2][0] == 60).all()

    few = candidates[:5]
    got = engine.fuzzy_search(queries, few, k=16, device=gpu, starts=True)
    assert same(got, select(dense(queries, few), 16))
    assert (got[0][:, 5:] == EMPTY).all() and (got[0][:, :5] != EMPTY).all()  # 11 empty slots: (2^64 - 1, 0, 0, 0)
    assert all(not matrix[:, 5:].any() for matrix in got[1:])

    none = engine.fuzzy_search(queries, [], k=4, device=gpu, starts=True)  # no candidates at all
    assert (none[0] == EMPTY).all() and all(not matrix.any() for matrix in none[1:])
    assert engine.last_call_profile().pairs == 0


def test_self_form(gpu, engine):
    rng = random.Random(21)
    strings = [bytes(rng.choice(b"ab") for _ in range(rng.randint(0, 70))) for _ in range(37)]
    strings[5] = strings[9]  # a duplicate at another index counts
    want = dense(strings, strings)
    for k in (1, 8, 40):  # 40: more than the 36 others
        got = engine.fuzzy_search(strings, k=k, device=gpu, starts=True)
        assert same(got, select(want, k, skip_own=True)), k
        assert not (got[0] == np.arange(len(strings), dtype=np.uint64)[:, None]).any()  # never the own index, whose distance is 0
    assert got[1][5, 0] == 0 and got[1][9, 0] == 0  # the twins find each other
    profile = engine.last_call_profile()
    lone = engine.fuzzy_search([b"abc"], k=3, device=gpu, starts=True)  # one query, searched in nothing else
    assert (lone[0] == EMPTY).all() and all(not matrix.any() for matrix in lone[1:])
    assert profile.pairs == len(strings) ** 2 + len(strings) * (len(strings) - 1)  # the own column is scored, and skipped by the scan; the winners


def _c_call(name, engine, gpu, queries, candidates, k, indices, distances, starts, ends, stride):
    """One C-ABI call over tapes / sequences that the caller keeps alive; pointers as integers or None."""
    error = ctypes.c_char_p()
    status = getattr(_abi.lib, name)(engine.handle, gpu.handle, ctypes.byref(queries), None if candidates is None else ctypes.byref(candidates),
                                     k, indices, distances, starts, ends, stride, ctypes.byref(error))
    return status, error.value


@pytest.fixture(scope="module")
def small():
    rng = random.Random(8)
    queries = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 90))) for _ in range(9)] + [b""]
    candidates = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 300))) for _ in range(75)]
    return queries, candidates, dense(queries, candidates)


def test_spans_and_the_winners_pass(gpu, engine, small):
    queries, candidates, want = small
    rows, count, k = len(queries), len(candidates), 7
    indices, distances, starts, ends = engine.fuzzy_search(queries, candidates, k=k, device=gpu, starts=True)
    with_spans = engine.last_call_profile()
    assert same((indices, distances, starts, ends), select(want, k))
    assert same((distances, starts, ends), engine.fuzzy_find(queries, candidates, indices, device=gpu, starts=True))  # bit for bit
    plain = engine.fuzzy_search(queries, candidates, k=k, device=gpu)
    with_ends = engine.last_call_profile()
    assert same(plain, (indices, distances, ends))
    assert same(plain[1:], engine.fuzzy_find(queries, candidates, indices, device=gpu))

    # without `ends` (the C call: the Python method always asks for them) no winners pass is launched
    keep = [szs.Strs(queries).to_device(0), szs.Strs(candidates).to_device(0)]
    q32, c32 = (strs._tape(0) for strs in keep)
    bare = [np.full((rows, k), UNTOUCHED, np.uint64) for _ in range(2)]
    status, message = _c_call("szs_rocm_fuzzy_search_u32tape", engine, gpu, q32, c32, k, bare[0].ctypes.data, bare[1].ctypes.data, None, None, k)
    assert status == 0, message
    assert same(bare, (indices, distances))
    profile = engine.last_call_profile()
    cells = sum(len(q) for q in queries) * sum(len(c) for c in candidates)
    assert profile.launches == 3 and profile.pairs == rows * count and profile.cells == cells  # one tile: scoring, scan, emit
    assert with_ends.launches == 4 and with_ends.pairs == rows * count + rows * k  # ... and fuzzy find's launch on the winners
    assert with_spans.launches == 5 and with_spans.pairs == with_ends.pairs and with_spans.cells > with_ends.cells > cells


def test_forms_and_placement(gpu, engine, small):
    import torch

    queries, candidates, want = small
    rows, k, stride = len(queries), 6, 9
    expected = select(want, k)
    keep = [szs.Strs(queries).to_device(0), szs.Strs(candidates).to_device(0), szs.Strs(queries, wide_offsets=True).to_device(0),
            szs.Strs(candidates, wide_offsets=True).to_device(0)]
    q32, c32, q64, c64 = (strs._tape(0) for strs in keep)

    def sequence_of(strings):  # sz_sequence_t callbacks, each string at its own device address
        tensors = [torch.tensor(list(s), dtype=torch.uint8, device="cuda") for s in strings]
        addresses, lengths = [t.data_ptr() for t in tensors], [len(s) for s in strings]
        get_start = _abi.MEMBER_START(lambda handle, i: addresses[i])
        get_length = _abi.MEMBER_LENGTH(lambda handle, i: lengths[i])
        keep.extend([tensors, get_start, get_length])
        return _abi.Sequence(None, len(strings), get_start, get_length)

    for name, q, c in (("szs_rocm_fuzzy_search_u32tape", q32, c32), ("szs_rocm_fuzzy_search_u64tape", q64, c64),
                       ("szs_rocm_fuzzy_search", sequence_of(queries), sequence_of(candidates))):
        out = [np.full((rows, stride), UNTOUCHED, np.uint64) for _ in range(4)]
        status, message = _c_call(name, engine, gpu, q, c, k, *(array.ctypes.data for array in out), stride)
        assert status == 0, (name, message)
        assert same([array[:, :k] for array in out], expected), name  # the three forms agree: each equals the oracle
        assert all((array[:, k:] == UNTOUCHED).all() for array in out), name  # row_stride > k: the padding is untouched
        status, message = _c_call(name, engine, gpu, q, None, k, *(array.ctypes.data for array in out), stride)  # the self form
        assert status == 0, (name, message)
        assert same([array[:, :k] for array in out], select(dense(queries, queries), k, skip_own=True)), name

    def as_numpy(array):
        return array if isinstance(array, np.ndarray) else array.cpu().numpy().view(np.uint64)

    for where in ("device", "pinned", "numpy"):
        wide = [np.full((rows, stride), UNTOUCHED, dtype=np.uint64) for _ in range(4)]
        if where == "device":
            wide = [torch.from_numpy(array.view(np.int64)).cuda() for array in wide]
        elif where == "pinned":
            wide = [torch.from_numpy(array.view(np.int64)).pin_memory() for array in wide]
        out = tuple(array[:, :k] for array in wide)
        assert engine.fuzzy_search(queries, candidates, k=k, device=gpu, out=out, starts=True) is out
        wide = [as_numpy(array) for array in wide]
        assert same([array[:, :k] for array in wide], expected), where
        assert all((array[:, k:] == UNTOUCHED).all() for array in wide), where
    # indices and distances on the device, ends in host memory: the winners pass stages what it has to
    out = [np.full((rows, k), UNTOUCHED, dtype=np.uint64) for _ in range(3)]
    out = tuple(torch.from_numpy(array.view(np.int64)).cuda() if part < 2 else array for part, array in enumerate(out))
    engine.fuzzy_search(queries, candidates, k=k, device=gpu, out=out)
    assert same([as_numpy(array) for array in out], without_starts(expected))


def test_refusals_on_a_real_engine(gpu, engine):
    queries, candidates = [b"ACGT", b"AC", b"GATTACA"], [b"ACG", b"T", b"", b"GATT"]
    good = engine.fuzzy_search(queries, candidates, k=2, device=gpu, starts=True)
    assert same(good, select(dense(queries, candidates), 2))
    out = tuple(np.full((3, 2), UNTOUCHED, np.uint64) for _ in range(4))
    with pytest.raises(szs.StringZillasError) as refused:  # one query beyond the bit-vector, among valid ones
        engine.fuzzy_search([b"AC", b"A" * 257, b"ACGT"], candidates, k=2, device=gpu, out=out, starts=True)
    assert refused.value.status_name == "unexpected_dimensions" and "256" in str(refused.value)
    assert all((array == UNTOUCHED).all() for array in out)
    assert same(engine.fuzzy_search([b"AC", b"A" * 256, b"ACGT"], candidates, k=2, device=gpu)[:1],
                select(dense([b"AC", b"A" * 256, b"ACGT"], candidates), 2)[:1])  # 256 bytes are taken

    table = matrices.blosum62()
    for other in (szs.LevenshteinDistances(0, 2, 3, 1, capabilities=gpu), szs.LevenshteinDistancesUTF8(capabilities=gpu),
                  szs.NeedlemanWunschScores(*table, open=-4, extend=-4, capabilities=gpu)):
        with pytest.raises(szs.StringZillasError) as refused:
            other.fuzzy_search(queries, candidates, k=2, device=gpu, out=out, starts=True)
        assert refused.value.status_name == "unknown"
        assert all((array == UNTOUCHED).all() for array in out)

    # the engine goes on, and so do the calls it had before
    assert same(engine.fuzzy_search(queries, candidates, k=2, device=gpu, starts=True), good)
    distances, ends = engine.fuzzy_find(queries, candidates, good[0], device=gpu)
    assert np.array_equal(distances, good[1]) and np.array_equal(ends, good[3])
    assert engine.last_call_profile().launches == 1

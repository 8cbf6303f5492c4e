"""Fuzzy search within a bound on the GPU (`szs_rocm_fuzzy_search_within*`, `_Engine.fuzzy_search_within`):
every candidate whose semi-global distance is at most `max_distance`, against the plain DP of tests/within_cases.py - the hits of a row
among ALL candidates, the leftmost `limit` in ascending candidate index with `fuzzy_find`'s own distances, starts and ends."""
import ctypes
import random

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi

import within_cases as cases

pytestmark = pytest.mark.gpu

EMPTY, UNTOUCHED = cases.EMPTY, cases.UNTOUCHED
NAMES = ("counts", "indices", "distances", "starts", "ends")


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return szs.DeviceScope(gpu_device=0)


@pytest.fixture(scope="module")
def engine(gpu):
    return szs.LevenshteinDistances(capabilities=gpu)


@pytest.fixture
def knobs():
    yield
    _abi.tuning_set("top_k_tile", None)
    _abi.tuning_set("fuzzy_search_segment", None)


def _edited(rng, text, edits):
    text = bytearray(text)
    for _ in range(edits):
        at = rng.randrange(len(text))
        kind = rng.choice("XID")
        if kind == "X":
            text[at] = rng.choice([b for b in b"ACGT" if b != text[at]])
        elif kind == "I":
            text.insert(at, rng.choice(b"ACGT"))
        elif len(text) > 1:
            del text[at]
    return bytes(text)


@pytest.fixture(scope="module")
def corpus():
    """Two queries of every length, short and long interleaved; 150 ACGT candidates of 0 ... 300 bytes - no multiple of 64 - of which
    every fifth from the tenth on holds a copy of some query with 0 ... 3 edits; the matrices of the DP, computed once."""
    rng = random.Random(47)
    ascending = [bytes(rng.choice(b"ACGT") for _ in range(length)) for length in cases.QUERY_LENGTHS for _ in range(2)]
    queries = []
    while ascending:
        queries.append(ascending.pop(0))
        if ascending:
            queries.append(ascending.pop())
    lengths = [1, 3, 0, 4, 5, 7, 8, 9] + [rng.randint(0, 300) for _ in range(142)]
    candidates = [bytes(rng.choice(b"ACGT") for _ in range(length)) for length in lengths]
    planted = [query for query in queries if len(query) >= 31][:-2]  # 14 of the 16, over 28 candidates: two copies each; two stay unmatched
    for i, at in enumerate(range(10, 150, 5)):
        head = candidates[at][:rng.randint(0, 20)]
        candidates[at] = (head + _edited(rng, planted[i % len(planted)], (i + i // len(planted)) % 4) + candidates[at][len(head):])[:300]
    return queries, candidates, cases.dense(queries, candidates)


def _check(got, want, note):
    assert len(got) == len(want), note
    for name, g, w in zip(NAMES if len(want) == 5 else NAMES[:3] + NAMES[4:], got, want):
        assert g.dtype == np.uint64 and g.shape == w.shape and np.array_equal(g, w), (note, name, np.argwhere(g != w)[:8])


def _without_starts(five):
    return five[:3] + five[4:]


@pytest.mark.parametrize("starts", [False, True])
@pytest.mark.parametrize("max_distance", [0, 1, 3, 256, 2**40])
def test_widths_bounds_and_limits(gpu, engine, corpus, max_distance, starts):
    queries, candidates, want = corpus
    for limit in (0, 1, 64):
        expected = cases.expected_fuzzy_within(want, max_distance, limit)
        got = engine.fuzzy_search_within(queries, candidates, max_distance=max_distance, limit=limit, starts=starts, device=gpu)
        _check(got, expected if starts else _without_starts(expected), (max_distance, limit, starts))
        if limit:  # the rows feed fuzzy find directly, empty slots included: the same distances, starts and ends, bit for bit
            found = engine.fuzzy_find(queries, candidates, got[1], device=gpu, starts=True)
            assert cases.same(found if starts else (found[0], found[2]), got[2:]), (max_distance, limit, starts)
    counts = expected[0]
    empty = [q for q, query in enumerate(queries) if not query]
    assert empty and all(counts[q] == len(candidates) for q in empty)  # a query of no bytes hits every candidate
    if max_distance >= 256:
        assert (counts == len(candidates)).all()  # no distance exceeds the query's length
    else:
        assert (counts == 0).any() and (counts > 0).any() and (max_distance == 0 or ((counts > 1) & (counts < 64)).any())


def test_self_form(gpu, engine):
    rng = random.Random(21)
    strings = [bytes(rng.choice(b"ab") for _ in range(rng.randint(0, 70))) for _ in range(37)]
    strings[5] = strings[9]  # a duplicate at another index counts
    want = cases.dense(strings, strings)
    for max_distance in (0, 2):
        for limit in (0, 1, 8, 40):  # 40: more than the 36 others
            got = engine.fuzzy_search_within(strings, max_distance=max_distance, limit=limit, starts=True, device=gpu)
            _check(got, cases.expected_fuzzy_within(want, max_distance, limit, skip_own=True), (max_distance, limit))
            assert not (got[1] == np.arange(len(strings), dtype=np.uint64)[:, None]).any()  # never the own index, whose distance is 0
    assert 9 in got[1][5].tolist() and 5 in got[1][9].tolist()  # the twins find each other
    lone = engine.fuzzy_search_within([b"abc"], max_distance=3, limit=3, starts=True, device=gpu)  # one query, searched in nothing else
    assert lone[0].tolist() == [0] and (lone[1] == EMPTY).all() and all(not matrix.any() for matrix in lone[2:])


@pytest.mark.parametrize("tile, segment", [(64, 64), (100, 64), (150, 128), (1, None), (None, 64)])
def test_knobs_change_no_byte(gpu, engine, knobs, corpus, tile, segment):
    queries, candidates, want = corpus
    untiled = engine.fuzzy_search_within(queries, candidates, max_distance=3, limit=16, starts=True, device=gpu)
    one_tile = engine.last_call_profile()
    _check(untiled, cases.expected_fuzzy_within(want, 3, 16), "automatic")
    _abi.tuning_set("top_k_tile", tile)
    _abi.tuning_set("fuzzy_search_segment", segment)
    assert _abi.within_probe(len(queries), len(candidates), 16)[1] == (tile or len(candidates))
    tiled = engine.fuzzy_search_within(queries, candidates, max_distance=3, limit=16, starts=True, device=gpu)
    profile = engine.last_call_profile()
    assert all(g.tobytes() == w.tobytes() for g, w in zip(tiled, untiled))
    tiles = -(-len(candidates) // (tile or len(candidates)))
    assert profile.launches == one_tile.launches + 3 * (tiles - 1)  # a scoring launch, a count pass and a store pass per tile
    assert profile.pairs == one_tile.pairs and profile.cells == one_tile.cells  # the knobs change no count either
    counted = engine.fuzzy_search_within(queries, candidates, max_distance=3, limit=0, device=gpu)
    assert np.array_equal(counted[0], untiled[0]) and engine.last_call_profile().launches == 2 * tiles + 1  # no store pass, no winners


def test_profile_counts_every_launch(gpu, engine, corpus):
    queries, candidates, want = corpus
    rows, count, limit = len(queries), len(candidates), 7
    expected = cases.expected_fuzzy_within(want, 3, limit)
    held = int(np.minimum(expected[0], limit).sum())
    cells = sum(len(q) for q in queries) * sum(len(c) for c in candidates)
    five = engine.fuzzy_search_within(queries, candidates, max_distance=3, limit=limit, starts=True, device=gpu)
    with_spans = engine.last_call_profile()
    four = engine.fuzzy_search_within(queries, candidates, max_distance=3, limit=limit, device=gpu)
    with_ends = engine.last_call_profile()
    _check(five, expected, "spans")
    _check(four, _without_starts(expected), "ends")
    # one tile: scoring, count, store, finish - and fuzzy find's launch on the stored rows, whose empty slots are no pairs
    assert with_ends.launches == 5 and with_ends.pairs == rows * count + held and with_ends.cells > cells
    assert with_spans.launches == 6 and with_spans.pairs == with_ends.pairs and with_spans.cells > with_ends.cells

    # without `ends` (the C call: the Python method always asks for them) no winners pass is launched
    keep = [szs.Strs(queries).to_device(0), szs.Strs(candidates).to_device(0)]
    q32, c32 = (strs._tape(0) for strs in keep)
    bare = [np.full(rows, UNTOUCHED, np.uint64)] + [np.full((rows, limit + 2), UNTOUCHED, np.uint64) for _ in range(2)]
    error = ctypes.c_char_p()
    status = _abi.lib.szs_rocm_fuzzy_search_within_u32tape(engine.handle, gpu.handle, ctypes.byref(q32), ctypes.byref(c32), 3, limit,
                                                           bare[0].ctypes.data, bare[1].ctypes.data, bare[2].ctypes.data, None, None, limit + 2,
                                                           ctypes.byref(error))
    assert status == 0, error.value
    assert cases.same([bare[0], bare[1][:, :limit], bare[2][:, :limit]], expected[:3])
    assert all((array[:, limit:] == UNTOUCHED).all() for array in bare[1:])  # row_stride > limit: the padding is untouched
    profile = engine.last_call_profile()
    assert profile.launches == 4 and profile.pairs == rows * count and profile.cells == cells
    counted = engine.fuzzy_search_within(queries, candidates, max_distance=3, limit=0, device=gpu)
    profile = engine.last_call_profile()
    assert np.array_equal(counted[0], expected[0]) and all(matrix.shape == (rows, 0) for matrix in counted[1:])
    assert profile.launches == 3 and profile.pairs == rows * count  # scoring, count, finish


def test_forms_and_placement(gpu, engine):
    import torch

    rng = random.Random(8)
    queries = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 90))) for _ in range(9)] + [b""]
    candidates = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 300))) for _ in range(75)]
    rows, limit, stride, bound = len(queries), 6, 9, 20
    expected = cases.expected_fuzzy_within(cases.dense(queries, candidates), bound, limit)
    own = cases.expected_fuzzy_within(cases.dense(queries, queries), bound, limit, skip_own=True)
    assert (expected[0] > limit).any() and (expected[0] < limit).any()
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

    error = ctypes.c_char_p()
    for name, q, c in (("szs_rocm_fuzzy_search_within_u32tape", q32, c32), ("szs_rocm_fuzzy_search_within_u64tape", q64, c64),
                       ("szs_rocm_fuzzy_search_within", sequence_of(queries), sequence_of(candidates))):
        for pool, want in ((c, expected), (None, own)):
            counts, out = np.full(rows, UNTOUCHED, np.uint64), [np.full((rows, stride), UNTOUCHED, np.uint64) for _ in range(4)]
            status = getattr(_abi.lib, name)(engine.handle, gpu.handle, ctypes.byref(q), None if pool is None else ctypes.byref(pool), bound, limit,
                                             counts.ctypes.data, *(array.ctypes.data for array in out), stride, ctypes.byref(error))
            assert status == 0, (name, error.value)
            assert cases.same([counts] + [array[:, :limit] for array in out], want), name  # the three forms agree: each equals the DP
            assert all((array[:, limit:] == UNTOUCHED).all() for array in out), name

    def as_numpy(array):
        return array if isinstance(array, np.ndarray) else array.cpu().numpy().view(np.uint64)

    for where in ("device", "pinned", "numpy"):
        counts, wide = np.full(rows, UNTOUCHED, np.uint64), [np.full((rows, stride), UNTOUCHED, dtype=np.uint64) for _ in range(4)]
        if where == "device":
            counts, wide = torch.from_numpy(counts.view(np.int64)).cuda(), [torch.from_numpy(array.view(np.int64)).cuda() for array in wide]
        elif where == "pinned":
            counts, wide = torch.from_numpy(counts.view(np.int64)).pin_memory(), [torch.from_numpy(array.view(np.int64)).pin_memory() for array in wide]
        out = (counts,) + tuple(array[:, :limit] for array in wide)
        assert engine.fuzzy_search_within(queries, candidates, max_distance=bound, limit=limit, starts=True, device=gpu, out=out) is out
        wide = [as_numpy(array) for array in wide]
        assert cases.same([as_numpy(counts)] + [array[:, :limit] for array in wide], expected), where
        assert all((array[:, limit:] == UNTOUCHED).all() for array in wide), where
    # counts and ends in host memory, indices and distances on the device: every pass stages what it has to
    out = [np.full(rows, UNTOUCHED, np.uint64)] + [np.full((rows, limit), UNTOUCHED, dtype=np.uint64) for _ in range(3)]
    out = tuple(torch.from_numpy(array.view(np.int64)).cuda() if part in (1, 2) else array for part, array in enumerate(out))
    engine.fuzzy_search_within(queries, candidates, max_distance=bound, limit=limit, device=gpu, out=out)
    assert cases.same([as_numpy(array) for array in out], _without_starts(expected))


def test_refusals_on_a_real_engine(gpu, engine):
    from stringzilla_amd import matrices

    queries, candidates = [b"ACGT", b"AC", b"GATTACA"], [b"ACG", b"T", b"", b"GATT"]
    good = engine.fuzzy_search_within(queries, candidates, max_distance=1, limit=2, starts=True, device=gpu)
    _check(good, cases.expected_fuzzy_within(cases.dense(queries, candidates), 1, 2), "small")
    out = (np.full(3, UNTOUCHED, np.uint64),) + tuple(np.full((3, 2), UNTOUCHED, np.uint64) for _ in range(4))
    with pytest.raises(szs.StringZillasError) as refused:  # one query beyond the bit-vector, among valid ones
        engine.fuzzy_search_within([b"AC", b"A" * 257, b"ACGT"], candidates, max_distance=1, limit=2, device=gpu, out=out, starts=True)
    assert refused.value.status_name == "unexpected_dimensions" and "256" in str(refused.value)
    assert all((array == UNTOUCHED).all() for array in out)
    taken = [b"AC", b"A" * 256, b"ACGT"]  # 256 bytes are taken
    _check(engine.fuzzy_search_within(taken, candidates, max_distance=255, limit=2, starts=True, device=gpu),
           cases.expected_fuzzy_within(cases.dense(taken, candidates), 255, 2), "256 bytes")

    table = matrices.blosum62()
    for other in (szs.LevenshteinDistances(0, 2, 3, 1, capabilities=gpu), szs.LevenshteinDistancesUTF8(capabilities=gpu),
                  szs.NeedlemanWunschScores(*table, open=-4, extend=-4, capabilities=gpu)):
        with pytest.raises(szs.StringZillasError) as refused:
            other.fuzzy_search_within(queries, candidates, max_distance=1, limit=2, device=gpu, out=out, starts=True)
        assert refused.value.status_name == "unknown"
        assert all((array == UNTOUCHED).all() for array in out)

    none = engine.fuzzy_search_within(queries, [], max_distance=1, limit=4, starts=True, device=gpu)  # no candidates at all
    assert not none[0].any() and (none[1] == EMPTY).all() and all(not matrix.any() for matrix in none[2:])
    assert engine.last_call_profile().pairs == 0
    # the engine goes on, and so do the calls it had before
    assert cases.same(engine.fuzzy_search_within(queries, candidates, max_distance=1, limit=2, starts=True, device=gpu), good)
    distances, ends = engine.fuzzy_find(queries, candidates, good[1], device=gpu)
    assert np.array_equal(distances, good[2]) and np.array_equal(ends, good[4])
    assert engine.last_call_profile().launches == 1

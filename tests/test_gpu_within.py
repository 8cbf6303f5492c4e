"""Bounded search on the GPU (`szs_rocm_within*`, `_Engine.within`) against numpy over the oracle's full
matrix (tests/within_cases.py): the hits of every row among ALL candidates, the leftmost `limit` of them in ascending candidate index,
the empty pair behind them."""
import ctypes
import functools
import random

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi, matrices

import within_cases as cases

pytestmark = pytest.mark.gpu

EMPTY, UNTOUCHED = cases.EMPTY, cases.UNTOUCHED
FAMILIES = ["levenshtein", "levenshtein_affine", "levenshtein_utf8", "needleman_wunsch", "smith_waterman"]
LIMITS = (0, 1, 5, 64, 200)


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return szs.DeviceScope(gpu_device=0)


@pytest.fixture
def tile_knob():
    previous = _abi._knob_values["top_k_tile"]
    yield lambda value: _abi.tuning_set("top_k_tile", value)
    _abi.tuning_set("top_k_tile", previous)


def _rand(rng, count, lo, hi, alphabet):
    return [bytes(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(count)]


def _utf8_strings(rng, count):
    pieces = ["a", "b", "é", "ж", "中", "😀", "ß"]
    return ["".join(rng.choice(pieces) for _ in range(rng.randint(1, 30))).encode() for _ in range(count)]


def _family(name, gpu):
    """(engine, oracle function of (queries, candidates), descending, alphabet of the random strings)"""
    if name == "levenshtein":
        return szs.LevenshteinDistances(capabilities=gpu), lambda o, q, c: o.levenshtein(q, c), False, b"ACGT"
    if name == "levenshtein_affine":
        return (szs.LevenshteinDistances(0, 2, 3, 1, capabilities=gpu), lambda o, q, c: o.levenshtein(q, c, 0, 2, 3, 1), False, b"abcdef")
    if name == "levenshtein_utf8":
        return szs.LevenshteinDistancesUTF8(capabilities=gpu), lambda o, q, c: o.levenshtein_utf8(q, c), False, None
    if name == "needleman_wunsch":
        table = matrices.blosum62()
        return (szs.NeedlemanWunschScores(*table, open=-4, extend=-4, capabilities=gpu),
                lambda o, q, c: o.needleman_wunsch(q, c, *table, -4, -4), True, b"ARNDCQEGHILKMFPSTWYV")
    table = matrices.nuc44()
    return (szs.SmithWatermanScores(*table, open=-4, extend=-1, capabilities=gpu),
            lambda o, q, c: o.smith_waterman(q, c, *table, -4, -1), True, b"ACGT")


def _check(got, want, note):
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint64 and got[2].dtype == want[2].dtype, note
    for name, g, w in zip(("counts", "indices", "scores"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (note, name, np.argwhere(g != w)[:8])


@functools.lru_cache(maxsize=None)
def _strings(family, alphabet):
    """37 queries x 150 candidates - the last chunk of 64 columns is partial - with lengths that spread the scores of a row."""
    rng = random.Random(len(family))
    if alphabet is None:
        return _utf8_strings(rng, 37), _utf8_strings(rng, 150)
    queries = _rand(rng, 37, 1, 40, alphabet)
    queries[5], queries[6] = queries[5][:1], queries[6] * 3  # a very short and a very long query: rows of many and of no hits
    return queries, _rand(rng, 150, 1, 40, alphabet)


@pytest.mark.parametrize("family", FAMILIES)
def test_families(gpu, oracle, family):
    engine, score, descending, alphabet = _family(family, gpu)
    queries, candidates = _strings(family, alphabet)
    full = score(oracle, queries, candidates)
    signed = full.astype(np.int64)
    bounds = sorted({int(np.quantile(signed, q, method="nearest")) for q in (0.02, 0.25, 0.5, 0.9)} | {int(signed.min()), int(signed.max())})
    # beyond both ends: a negative bound on a distance engine - no hits - and a bound no score reaches (NW, SW) or every distance does
    bounds = [-5, -1] + bounds + [int(signed.max()) + 1] if not descending else [int(signed.min()) - 1] + bounds + [int(signed.max()) + 1]
    seen = set()
    for bound in bounds:
        for limit in LIMITS:
            want = cases.expected_within(full, bound, descending, limit, dtype=engine._dtype)
            got = engine.within(queries, candidates, bound=bound, limit=limit, device=gpu)
            _check(got, want, (family, bound, limit))
            seen |= {"none"} if (want[0] == 0).any() else set()
            seen |= {"all"} if (want[0] == len(candidates)).any() else set()
            seen |= {"more"} if limit and ((want[0] > limit) & (want[0] < len(candidates))).any() else set()
            seen |= {"fewer"} if limit and ((want[0] > 0) & (want[0] < limit)).any() else set()
    assert seen == {"none", "all", "more", "fewer"}, seen  # the bounds reach every kind of row
    nothing = cases.expected_within(full, bounds[0] if descending else bounds[-1], descending, 5)[0]
    assert (nothing == len(candidates)).all()
    unreachable = engine.within(queries, candidates, bound=bounds[-1] if descending else -1, limit=5, device=gpu)
    assert not unreachable[0].any() and (unreachable[1] == EMPTY).all() and not unreachable[2].any()


@pytest.mark.parametrize("family", ["levenshtein", "smith_waterman"])
def test_self_form_excludes_the_diagonal(gpu, oracle, family):
    rng = random.Random(5)
    engine, score, descending, alphabet = _family(family, gpu)
    strings = _rand(rng, 17, 1, 12, alphabet)
    strings[3] = strings[9] = strings[11]  # duplicates at other indices still count
    full = score(oracle, strings, strings)
    diagonal = full.astype(np.int64).diagonal()
    for bound in sorted({int(diagonal.min()), int(diagonal.max()), int(np.median(full.astype(np.int64)))}):  # the diagonal would hit
        for limit in (0, 3, 20):
            want = cases.expected_within(full, bound, descending, limit, self_search=True, dtype=engine._dtype)
            got = engine.within(strings, None, bound=bound, limit=limit, device=gpu)
            _check(got, want, (family, bound, limit))
            assert not (got[1] == np.arange(len(strings), dtype=np.uint64)[:, None]).any()
    twins = engine.within(strings, None, bound=int(full[3, 3]), limit=len(strings), device=gpu)
    assert {9, 11} <= set(twins[1][3].tolist()) and 3 not in twins[1][3].tolist()
    lone = engine.within(strings[:1], None, bound=int(full[0, 0]), limit=3, device=gpu)  # one query, searched in nothing else
    assert lone[0].tolist() == [0] and (lone[1] == EMPTY).all() and not lone[2].any()


def test_tiling_changes_no_byte(gpu, oracle, tile_knob):
    rng = random.Random(11)
    queries, candidates = _rand(rng, 11, 1, 24, b"ab"), _rand(rng, 300, 1, 24, b"ab")
    candidates[100:140] = [queries[2]] * 40  # a run of hits that every tile size cuts somewhere else
    engine = szs.LevenshteinDistances(capabilities=gpu)
    full = oracle.levenshtein(queries, candidates)
    bound = int(np.quantile(full, 0.3, method="nearest"))
    for limit in (0, 7, 64, 300):
        want = cases.expected_within(full, bound, False, limit)
        outputs = {}
        for tile in (1, 7, 64, 65, None):
            tile_knob(tile)
            assert _abi.within_probe(len(queries), len(candidates), limit)[1] == (tile or 300)
            outputs[tile] = engine.within(queries, candidates, bound=bound, limit=limit, device=gpu)
            _check(outputs[tile], want, (tile, limit))
            tiles = -(-300 // (tile or 300))
            assert engine.last_call_profile().pairs == len(queries) * 300
            if tile in (64, 65):  # per tile: the scoring launches, the count pass and - with a limit - the store pass; one finish
                scoring = engine.last_call_profile().launches - tiles * (2 if limit else 1) - 1
                assert scoring >= tiles
        assert all(cases.same(outputs[tile], outputs[None]) and all(g.tobytes() == w.tobytes() for g, w in zip(outputs[tile], outputs[None]))
                   for tile in outputs)


def test_segments_and_edges(gpu, oracle, tile_knob):
    rng = np.random.default_rng(3)
    lengths = rng.integers(0, 9, size=9000)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(lengths.sum()))]
    offsets = np.zeros(len(lengths) + 1, dtype=np.uint32)
    np.cumsum(lengths, out=offsets[1:])
    candidates = szs.Strs.from_tape(letters, offsets)
    queries = [b"ACGTAC", b"TTTT", b"GACGTTA"]
    engine = szs.LevenshteinDistances(capabilities=gpu)
    full = oracle.levenshtein(queries, [candidates[i] for i in range(len(candidates))])
    block, tile, segments, segment_columns = _abi.within_probe(3, 9000, 64)
    assert (block, tile) == (3, 9000) and segments > 1  # few rows over a wide tile: several workgroups share a row

    def every_candidate_hits(limit):
        counts, indices, scores = engine.within(queries, candidates, bound=16, limit=limit, device=gpu)  # no distance exceeds 8
        assert (counts == 9000).all(), limit
        assert np.array_equal(indices, np.tile(np.arange(limit, dtype=np.uint64), (3, 1))), limit
        assert np.array_equal(scores, full[:, :limit]), limit

    for limit in (segment_columns - 1, segment_columns, segment_columns + 1, 8999, 9000):
        every_candidate_hits(limit)
    tile_knob(1000)  # ... and the limit on and beside the edge of a tile
    assert _abi.within_probe(3, 9000, 64)[1] == 1000
    for limit in (999, 1000, 1001, 2000):
        every_candidate_hits(limit)
    tile_knob(None)
    # hits on both sides of the segments' edge only: the second segment's base is the first one's partial count
    near = engine.within(queries, candidates, bound=2, limit=4000, device=gpu)
    _check(near, cases.expected_within(full, 2, False, 4000), "sparse hits across segments")
    assert ((near[1] != EMPTY) & (near[1] >= segment_columns)).any() and ((near[1] < segment_columns)).any()


def test_output_placement(gpu, oracle):
    import torch

    rng = random.Random(9)
    table = matrices.nuc44()
    queries, candidates = _rand(rng, 7, 5, 40, b"ACGT"), _rand(rng, 30, 5, 40, b"ACGT")
    engine = szs.SmithWatermanScores(*table, open=-4, extend=-1, capabilities=gpu)
    full = oracle.smith_waterman(queries, candidates, *table, -4, -1)
    bound, limit, stride = int(np.median(full)), 5, 9
    want = cases.expected_within(full, bound, True, limit, dtype=np.int64)
    assert (want[0] > limit).any() and (want[0] < limit).any()

    def as_numpy(array):
        return array if isinstance(array, np.ndarray) else array.cpu().numpy().view(np.uint64)

    for where in ("numpy", "pinned", "device"):
        counts = np.full(7, UNTOUCHED, dtype=np.uint64)
        wide = [np.full((7, stride), UNTOUCHED, dtype=np.uint64) for _ in range(2)]
        if where == "device":
            counts, wide = torch.from_numpy(counts.view(np.int64)).cuda(), [torch.from_numpy(array.view(np.int64)).cuda() for array in wide]
        elif where == "pinned":
            counts, wide = torch.from_numpy(counts.view(np.int64)).pin_memory(), [torch.from_numpy(array.view(np.int64)).pin_memory() for array in wide]
        out = (counts, wide[0][:, :limit], wide[1][:, :limit])
        assert engine.within(queries, candidates, bound=bound, limit=limit, device=gpu, out=out) is out
        counts, wide = as_numpy(counts), [as_numpy(array) for array in wide]
        assert np.array_equal(counts, want[0]), where
        assert np.array_equal(wide[0][:, :limit], want[1]) and np.array_equal(wide[1][:, :limit].view(np.int64), want[2]), where
        assert all((array[:, limit:] == UNTOUCHED).all() for array in wide), where  # cells [limit, row_stride) are left alone

        # scores NULL: counts and indices only; limit 0 with no matrix at all: counts only
        counts, indices = np.full(7, UNTOUCHED, dtype=np.uint64), np.full((7, stride), UNTOUCHED, dtype=np.uint64)
        if where == "device":
            counts, indices = torch.from_numpy(counts.view(np.int64)).cuda(), torch.from_numpy(indices.view(np.int64)).cuda()
        engine.within(queries, candidates, bound=bound, limit=limit, device=gpu, out=(counts, indices[:, :limit], None))
        assert np.array_equal(as_numpy(counts), want[0]) and np.array_equal(as_numpy(indices)[:, :limit], want[1]), where
        assert (as_numpy(indices)[:, limit:] == UNTOUCHED).all(), where
        fresh = torch.full((7,), 77, dtype=torch.int64, device="cuda" if where == "device" else "cpu")
        only = engine.within(queries, candidates, bound=bound, limit=0, device=gpu, out=(fresh.pin_memory() if where == "pinned" else fresh, None, None))
        assert only[1] is None and only[2] is None and np.array_equal(as_numpy(only[0]), want[0]), where


def test_input_forms(gpu, oracle, tile_knob):
    import torch

    rng = random.Random(8)
    queries, candidates = _rand(rng, 6, 1, 30, b"ACGT"), _rand(rng, 25, 1, 30, b"ACGT")
    full = oracle.levenshtein(queries, candidates)
    bound = int(np.median(full))
    want = cases.expected_within(full, bound, False, 4)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    got = engine.within(szs.Strs(queries, wide_offsets=True), szs.Strs(candidates, wide_offsets=True), bound=bound, limit=4, device=gpu)
    _check(got, want, "u64 tapes")

    keep = []

    def sequence_of(strings):  # sz_sequence_t callbacks, each string at its own device address
        tensors = [torch.tensor(list(s), dtype=torch.uint8, device="cuda") for s in strings]
        starts, lengths = [t.data_ptr() for t in tensors], [len(s) for s in strings]
        get_start = _abi.MEMBER_START(lambda handle, i: starts[i])
        get_length = _abi.MEMBER_LENGTH(lambda handle, i: lengths[i])
        keep.extend([tensors, get_start, get_length])
        return _abi.Sequence(None, len(strings), get_start, get_length)

    q_seq, c_seq = sequence_of(queries), sequence_of(candidates)
    error = ctypes.c_char_p()
    for tile in (None, 7):  # several tiles: the callbacks are re-based per tile
        tile_knob(tile)
        counts, indices, scores = np.zeros(6, np.uint64), np.zeros((6, 4), np.uint64), np.zeros((6, 4), np.uint64)
        status = _abi.lib.szs_rocm_within(engine.handle, gpu.handle, ctypes.byref(q_seq), ctypes.byref(c_seq), bound, 4, counts.ctypes.data,
                                          indices.ctypes.data, scores.ctypes.data, 4, ctypes.byref(error))
        assert status == 0, error.value
        _check((counts, indices, scores), want, ("sequences", tile))


def test_refusals_and_empty_sides(gpu):
    engine = szs.LevenshteinDistances(capabilities=gpu)
    counts, indices, scores = engine.within([b"abc", b"x"], szs.Strs([]), bound=3, limit=3, device=gpu)  # no candidates: nothing hits
    assert counts.tolist() == [0, 0] and (indices == EMPTY).all() and (scores == 0).all() and indices.shape == (2, 3)
    assert engine.last_call_profile().pairs == 0
    counts, indices, scores = engine.within(szs.Strs([]), [b"abc"], bound=3, limit=2, device=gpu)  # no queries: nothing to write
    assert counts.shape == (0,) and indices.shape == (0, 2) and scores.shape == (0, 2)

    tape = szs.Strs([b"abc", b"abd"])._tape(0)
    counts, indices = np.full(2, UNTOUCHED, dtype=np.uint64), np.full((2, 2), UNTOUCHED, dtype=np.uint64)
    error = ctypes.c_char_p()
    fingerprints = szs.Fingerprints(64, capabilities=gpu)
    status = _abi.lib.szs_rocm_within_u32tape(fingerprints.handle, gpu.handle, ctypes.byref(tape), ctypes.byref(tape), 1, 2, counts.ctypes.data,
                                              indices.ctypes.data, None, 2, ctypes.byref(error))
    assert _abi.STATUS_NAMES[status] == "unknown" and (counts == UNTOUCHED).all() and (indices == UNTOUCHED).all()
    for limit, stride in ((3, 2), (65537, 65537)):  # row_stride < limit, and a limit beyond the cap: on a real engine too
        status = _abi.lib.szs_rocm_within_u32tape(engine.handle, gpu.handle, ctypes.byref(tape), ctypes.byref(tape), 1, limit, counts.ctypes.data,
                                                  indices.ctypes.data, None, stride, ctypes.byref(error))
        assert _abi.STATUS_NAMES[status] == "unexpected_dimensions" and (counts == UNTOUCHED).all() and (indices == UNTOUCHED).all()
    got = engine.within([b"abc", b"abd"], [b"abc", b"abd"], bound=0, limit=2, device=gpu)  # the engine goes on
    assert got[0].tolist() == [1, 1] and got[1][:, 0].tolist() == [0, 1]


@pytest.mark.parametrize("family", ["levenshtein", "needleman_wunsch"])
def test_consistent_with_top_k(gpu, oracle, family):
    engine, score, descending, alphabet = _family(family, gpu)
    queries, candidates = _strings(family, alphabet)
    full = score(oracle, queries, candidates).astype(np.int64)
    for bound in (int(np.quantile(full, q, method="nearest")) for q in (0.1, 0.5, 0.9)):
        for k in (1, 5, 64):
            counts = engine.within(queries, candidates, bound=bound, limit=k, device=gpu)[0]
            indices, scores = engine.top_k(queries, candidates, k=k, device=gpu)
            inside = (scores.astype(np.int64) >= bound if descending else scores.astype(np.int64) <= bound) & (indices != EMPTY)
            assert np.array_equal(inside.sum(axis=1), np.minimum(counts, k)), (family, bound, k)

"""Top-k search on the GPU (`szs_rocm_top_k*`, `_Engine.top_k`) against numpy selection over the oracle's full matrix."""
import ctypes
import random

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi, matrices

pytestmark = pytest.mark.gpu

EMPTY = np.uint64(2**64 - 1)
UNTOUCHED = 0x5A5A5A5A5A5A5A5A


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


def expected_top_k(matrix, k, descending, self_search=False, dtype=np.uint64):
    """First k of a stable sort of each row (ties: lower index), the own index skipped in self-search, short rows completed."""
    rows = matrix.shape[0]
    indices = np.full((rows, k), EMPTY, dtype=np.uint64)
    scores = np.zeros((rows, k), dtype=dtype)
    for q in range(rows):
        row = matrix[q]
        order = np.argsort(-row.astype(np.int64) if descending else row, kind="stable")
        if self_search:
            order = order[order != q]
        order = order[:k]
        indices[q, :len(order)] = order
        scores[q, :len(order)] = row[order]
    return indices, scores


def _family(name, gpu):
    """(engine, oracle function of (queries, candidates), descending, alphabet of the random strings)"""
    if name == "levenshtein":
        return szs.LevenshteinDistances(capabilities=gpu), lambda o, q, c: o.levenshtein(q, c), False, b"ACGT"
    if name == "levenshtein_affine":
        return (szs.LevenshteinDistances(0, 2, 3, 1, capabilities=gpu), lambda o, q, c: o.levenshtein(q, c, 0, 2, 3, 1), False,
                b"abcdef")
    if name == "levenshtein_utf8":
        return szs.LevenshteinDistancesUTF8(capabilities=gpu), lambda o, q, c: o.levenshtein_utf8(q, c), False, None
    if name == "needleman_wunsch":
        table = matrices.blosum62()
        return (szs.NeedlemanWunschScores(*table, open=-4, extend=-4, capabilities=gpu),
                lambda o, q, c: o.needleman_wunsch(q, c, *table, -4, -4), True, b"ARNDCQEGHILKMFPSTWYV")
    table = matrices.nuc44()
    return (szs.SmithWatermanScores(*table, open=-4, extend=-1, capabilities=gpu),
            lambda o, q, c: o.smith_waterman(q, c, *table, -4, -1), True, b"ACGT")


def _utf8_strings(rng, count):
    pieces = ["a", "b", "é", "ж", "中", "😀", "ß"]
    return ["".join(rng.choice(pieces) for _ in range(rng.randint(1, 30))).encode() for _ in range(count)]


@pytest.mark.parametrize("family", ["levenshtein", "levenshtein_affine", "levenshtein_utf8", "needleman_wunsch", "smith_waterman"])
def test_families_and_k(gpu, oracle, family):
    rng = random.Random(len(family))
    engine, score, descending, alphabet = _family(family, gpu)
    if alphabet is None:
        queries, candidates = _utf8_strings(rng, 23), _utf8_strings(rng, 41)
    else:
        queries, candidates = _rand(rng, 23, 1, 40, alphabet), _rand(rng, 41, 1, 40, alphabet)
    full = score(oracle, queries, candidates)
    for k in (1, 7, len(candidates), len(candidates) + 3):
        indices, scores = engine.top_k(queries, candidates, k=k, device=gpu)
        want_indices, want_scores = expected_top_k(full, k, descending, dtype=engine._dtype)
        assert indices.dtype == np.uint64 and scores.dtype == engine._dtype and indices.shape == (len(queries), k)
        assert np.array_equal(indices, want_indices), (family, k)
        assert np.array_equal(scores, want_scores), (family, k)


@pytest.mark.parametrize("family", ["levenshtein", "smith_waterman"])
def test_self_search_excludes_the_diagonal(gpu, oracle, family):
    rng = random.Random(5)
    engine, score, descending, alphabet = _family(family, gpu)
    strings = _rand(rng, 17, 1, 12, alphabet)
    strings[3] = strings[9] = strings[11]  # duplicates at other indices still count
    full = score(oracle, strings, strings)
    for k in (4, len(strings) - 1, len(strings) + 2):
        indices, scores = engine.top_k(strings, None, k=k, device=gpu)
        want_indices, want_scores = expected_top_k(full, k, descending, self_search=True, dtype=engine._dtype)
        assert np.array_equal(indices, want_indices) and np.array_equal(scores, want_scores), k
    single_indices, single_scores = engine.top_k(strings[:1], None, k=3, device=gpu)
    assert (single_indices == EMPTY).all() and (single_scores == 0).all()


def test_ties_are_independent_of_tiling(gpu, oracle, tile_knob):
    rng = random.Random(11)
    words = [b"ab", b"abc", b"b", b"ba", b"abcd"]
    queries = [rng.choice(words) for _ in range(9)]
    candidates = [rng.choice(words) for _ in range(70)]
    candidates[20:40] = [b"abc"] * 20  # a long run of ties that tiles of 3 cut in many places
    engine = szs.LevenshteinDistances(capabilities=gpu)
    full = oracle.levenshtein(queries, candidates)
    outputs = []
    for tile in (1, 3, None):
        tile_knob(tile)
        for k in (5, 33):
            indices, scores = engine.top_k(queries, candidates, k=k, device=gpu)
            want_indices, want_scores = expected_top_k(full, k, False)
            assert np.array_equal(indices, want_indices) and np.array_equal(scores, want_scores), (tile, k)
            outputs.append((tile, k, indices))
    for tile, k, indices in outputs:
        assert np.array_equal(indices, next(i for t, kk, i in outputs if kk == k and t is None)), tile


def test_tile_boundary_inside_ties_nw(gpu, oracle, tile_knob):
    table = matrices.blosum62()
    engine = szs.NeedlemanWunschScores(*table, open=-4, extend=-4, capabilities=gpu)
    queries = [b"ACDEFG", b"WYV"]
    candidates = [b"ACDQ"] * 3 + [b"ACDEFG"] * 10 + [b"WWW"] * 7
    full = oracle.needleman_wunsch(queries, candidates, *table, -4, -4)
    for tile in (4, 7, None):
        tile_knob(tile)
        indices, scores = engine.top_k(queries, candidates, k=6, device=gpu)
        want_indices, want_scores = expected_top_k(full, 6, True, dtype=np.int64)
        assert np.array_equal(indices, want_indices) and np.array_equal(scores, want_scores), tile


def test_long_queries_and_chained_tiers(gpu, oracle):
    rng = random.Random(21)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    queries, candidates = _rand(rng, 3, 2100, 2600, b"ACGT"), _rand(rng, 20, 50, 3000, b"ACGT")  # beyond 2048 bytes: strips
    full = oracle.levenshtein(queries, candidates)
    indices, scores = engine.top_k(queries, candidates, k=5, device=gpu)
    want = expected_top_k(full, 5, False)
    assert np.array_equal(indices, want[0]) and np.array_equal(scores, want[1])
    query, long_candidates = _rand(rng, 1, 5000, 5000, b"ACGT"), _rand(rng, 4, 5000, 5200, b"ACGT")
    full = oracle.levenshtein(query, long_candidates)
    indices, scores = engine.top_k(query, long_candidates, k=3, device=gpu)
    want = expected_top_k(full, 3, False)
    assert np.array_equal(indices, want[0]) and np.array_equal(scores, want[1])


def test_automatic_tiling_crosses_the_device_planner_limit(gpu, oracle):
    rng = np.random.default_rng(3)
    lengths = rng.integers(3, 9, size=300_000)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(lengths.sum()))]
    offsets = np.zeros(len(lengths) + 1, dtype=np.uint32)
    np.cumsum(lengths, out=offsets[1:])
    candidates = szs.Strs.from_tape(letters, offsets)
    queries = [b"ACGTAC", b"TTTT", b"GACGTTA", b"CA"]
    engine = szs.LevenshteinDistances(capabilities=gpu)
    indices, scores = engine.top_k(queries, candidates, k=10, device=gpu)
    full = oracle.levenshtein(queries, [candidates[i] for i in range(len(candidates))])
    want = expected_top_k(full, 10, False)
    assert np.array_equal(indices, want[0]) and np.array_equal(scores, want[1])
    assert engine.last_call_profile().pairs == 4 * 300_000


def test_input_layouts(gpu, oracle):
    import torch

    rng = random.Random(8)
    queries, candidates = _rand(rng, 6, 1, 30, b"ACGT"), _rand(rng, 25, 1, 30, b"ACGT")
    full = oracle.levenshtein(queries, candidates)
    want = expected_top_k(full, 4, False)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    error = ctypes.c_char_p()

    # u32 tapes whose offsets are in host memory (bytes on the device): host-planned tiles
    def host_offsets_tape(strings):
        strs = szs.Strs(strings).to_device(0)
        return _abi.U32Tape(strs._device[1].data_ptr(), strs.offsets.ctypes.data, len(strings)), strs

    (q_tape, q_keep), (c_tape, c_keep) = host_offsets_tape(queries), host_offsets_tape(candidates)
    indices, scores = np.zeros((6, 4), np.uint64), np.zeros((6, 4), np.uint64)
    status = _abi.lib.szs_rocm_top_k_u32tape(engine.handle, gpu.handle, ctypes.byref(q_tape), ctypes.byref(c_tape), 4,
                                             indices.ctypes.data, scores.ctypes.data, 4, ctypes.byref(error))
    assert status == 0, error.value
    assert np.array_equal(indices, want[0]) and np.array_equal(scores, want[1])

    # u64 device tapes
    indices, scores = engine.top_k(szs.Strs(queries, wide_offsets=True), szs.Strs(candidates, wide_offsets=True), k=4, device=gpu)
    assert np.array_equal(indices, want[0]) and np.array_equal(scores, want[1])

    # sz_sequence_t callbacks, each string at its own device address
    keep = []

    def sequence_of(strings):
        tensors = [torch.tensor(list(s), dtype=torch.uint8, device="cuda") for s in strings]
        starts, lengths = [t.data_ptr() for t in tensors], [len(s) for s in strings]
        get_start = _abi.MEMBER_START(lambda handle, i: starts[i])
        get_length = _abi.MEMBER_LENGTH(lambda handle, i: lengths[i])
        keep.extend([tensors, get_start, get_length])
        return _abi.Sequence(None, len(strings), get_start, get_length)

    q_seq, c_seq = sequence_of(queries), sequence_of(candidates)
    for tile in (None, 7):  # several tiles: the callbacks are re-based per tile
        _abi.tuning_set("top_k_tile", tile)
        try:
            indices, scores = np.zeros((6, 4), np.uint64), np.zeros((6, 4), np.uint64)
            status = _abi.lib.szs_rocm_top_k(engine.handle, gpu.handle, ctypes.byref(q_seq), ctypes.byref(c_seq), 4, indices.ctypes.data,
                                             scores.ctypes.data, 4, ctypes.byref(error))
        finally:
            _abi.tuning_set("top_k_tile", None)
        assert status == 0, error.value
        assert np.array_equal(indices, want[0]) and np.array_equal(scores, want[1]), tile


def test_output_placement(gpu, oracle):
    import torch

    rng = random.Random(9)
    table = matrices.nuc44()
    queries, candidates = _rand(rng, 7, 5, 40, b"ACGT"), _rand(rng, 30, 5, 40, b"ACGT")
    engine = szs.SmithWatermanScores(*table, open=-4, extend=-1, capabilities=gpu)
    want = expected_top_k(oracle.smith_waterman(queries, candidates, *table, -4, -1), 5, True, dtype=np.int64)

    # numpy outputs, row stride beyond k: the padding stays as it was
    wide_indices = np.full((7, 9), UNTOUCHED, dtype=np.uint64)
    wide_scores = np.full((7, 9), UNTOUCHED, dtype=np.uint64).view(np.int64)
    engine.top_k(queries, candidates, k=5, device=gpu, out=(wide_indices[:, :5], wide_scores[:, :5]))
    assert np.array_equal(wide_indices[:, :5], want[0]) and np.array_equal(wide_scores[:, :5], want[1])
    assert (wide_indices[:, 5:] == UNTOUCHED).all() and (wide_scores[:, 5:].view(np.uint64) == UNTOUCHED).all()

    # device torch outputs, and the same with a row stride beyond k
    device_indices = torch.zeros((7, 5), dtype=torch.int64, device="cuda")
    device_scores = torch.zeros((7, 5), dtype=torch.int64, device="cuda")
    engine.top_k(queries, candidates, k=5, device=gpu, out=(device_indices, device_scores))
    assert np.array_equal(device_indices.cpu().numpy().view(np.uint64), want[0])
    assert np.array_equal(device_scores.cpu().numpy(), want[1])
    padded = torch.full((2, 7, 8), 77, dtype=torch.int64, device="cuda")
    engine.top_k(queries, candidates, k=5, device=gpu, out=(padded[0, :, :5], padded[1, :, :5]))
    assert np.array_equal(padded[0, :, :5].cpu().numpy().view(np.uint64), want[0])
    assert np.array_equal(padded[1, :, :5].cpu().numpy(), want[1])
    assert (padded[:, :, 5:] == 77).all()

    # scores NULL: indices only
    indices_only = np.full((7, 6), UNTOUCHED, dtype=np.uint64)
    engine.top_k(queries, candidates, k=5, device=gpu, out=(indices_only[:, :5], None))
    assert np.array_equal(indices_only[:, :5], want[0]) and (indices_only[:, 5] == UNTOUCHED).all()


def test_empty_sides(gpu):
    engine = szs.LevenshteinDistances(capabilities=gpu)
    indices, scores = engine.top_k([b"abc", b"x"], szs.Strs([]), k=3, device=gpu)
    assert (indices == EMPTY).all() and (scores == 0).all() and indices.shape == (2, 3)
    indices, scores = engine.top_k(szs.Strs([]), [b"abc"], k=2, device=gpu)
    assert indices.shape == (0, 2)


def test_fingerprints_handle_is_refused(gpu):
    fingerprints = szs.Fingerprints(64, capabilities=gpu)
    tape = szs.Strs([b"abc", b"abd"])._tape(0)
    indices = np.full((2, 2), UNTOUCHED, dtype=np.uint64)
    error = ctypes.c_char_p()
    status = _abi.lib.szs_rocm_top_k_u32tape(fingerprints.handle, gpu.handle, ctypes.byref(tape), ctypes.byref(tape), 2,
                                             indices.ctypes.data, None, 2, ctypes.byref(error))
    assert status != 0 and (indices == UNTOUCHED).all()

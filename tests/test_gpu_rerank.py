"""Rerank on the GPU (`szs_rocm_rerank*`, `_Engine.rerank`): every score against the oracle's cell `matrix[q, indices[q, r]]`."""
import ctypes
import random

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi, matrices

pytestmark = pytest.mark.gpu

EMPTY = np.uint64(2**64 - 1)
UNTOUCHED = 0x5A5A5A5A5A5A5A5A
QUERY_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)  # every width of the kernel, and two beyond it


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return szs.DeviceScope(gpu_device=0)


@pytest.fixture
def rerank_knob():
    previous = _abi._knob_values["rerank"]
    yield lambda value: _abi.tuning_set("rerank", value)
    _abi.tuning_set("rerank", previous)


def _rand(rng, count, lo, hi, alphabet):
    return [bytes(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(count)]


def expected(matrix, indices, dtype=np.uint64):
    """The oracle's cell for every listed index; 0 for an empty slot."""
    indices = np.asarray(indices, dtype=np.uint64)
    want = np.zeros(indices.shape, dtype=dtype)
    for q in range(indices.shape[0]):
        for r in range(indices.shape[1]):
            if indices[q, r] != EMPTY:
                want[q, r] = matrix[q, int(indices[q, r])]
    return want


@pytest.fixture(scope="module")
def widths(oracle):
    """Two queries of every length, interleaved so that neighbouring rows differ (0 next to 300, 1 next to 257 ...), ~100 candidates
    of 0 ... 160 bytes and one of 3000, and the oracle's matrix - computed once, never changed."""
    rng = random.Random(41)
    ascending = [bytes(rng.choice(b"ACGT") for _ in range(length)) for length in QUERY_LENGTHS for _ in range(2)]
    queries = []
    while ascending:
        queries.append(ascending.pop(0))
        if ascending:
            queries.append(ascending.pop())
    lengths = [0, 1, 3, 4, 5, 160] + [rng.randint(0, 160) for _ in range(94)]
    candidates = [bytes(rng.choice(b"ACGT") for _ in range(length)) for length in lengths] + [bytes(rng.choice(b"ACGT") for _ in range(3000))]
    matrix = oracle.levenshtein(queries, candidates)
    matrix.setflags(write=False)
    return queries, candidates, matrix


@pytest.mark.parametrize("k", [1, 7, 16, 17, 64, 65, 200])
def test_widths_and_routing_in_one_call(gpu, widths, rerank_knob, k):
    queries, candidates, matrix = widths
    rng = np.random.default_rng(k)
    indices = rng.integers(0, len(candidates), size=(len(queries), k), dtype=np.uint64)
    indices[:, 0] = len(candidates) - 1 if k > 1 else indices[:, 0]  # the 3000-byte candidate in every row
    want = expected(matrix, indices)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    automatic = engine.rerank(queries, candidates, indices, device=gpu)
    assert automatic.dtype == np.uint64 and automatic.shape == indices.shape
    assert np.array_equal(automatic, want), np.argwhere(automatic != want)[:8]
    rerank_knob(0)
    by_rows = engine.rerank(queries, candidates, indices, device=gpu)
    assert np.array_equal(by_rows, want), np.argwhere(by_rows != want)[:8]
    assert np.array_equal(by_rows, automatic)


def test_routes_show_in_the_profile(gpu, oracle, rerank_knob):
    rng = random.Random(64)
    queries, candidates = _rand(rng, 64, 0, 256, b"ACGT"), _rand(rng, 40, 0, 90, b"ACGT")
    indices = np.random.default_rng(2).integers(0, len(candidates), size=(64, 16), dtype=np.uint64)
    indices[5, 3] = indices[9, :4] = EMPTY
    want = expected(oracle.levenshtein(queries, candidates), indices)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    assert np.array_equal(engine.rerank(queries, candidates, indices, device=gpu), want)
    profile = engine.last_call_profile()
    assert profile.launches <= 4 and profile.pairs == int((indices != EMPTY).sum())
    assert profile.cells == sum(len(queries[q]) * len(candidates[int(i)]) for q in range(64) for i in indices[q] if i != EMPTY)
    rerank_knob(0)
    assert np.array_equal(engine.rerank(queries, candidates, indices, device=gpu), want)
    profile = engine.last_call_profile()
    assert profile.launches >= 64 and profile.pairs == int((indices != EMPTY).sum())


@pytest.mark.parametrize("knob", [None, 0])
def test_empty_slots_padding_and_duplicates(gpu, oracle, rerank_knob, knob):
    rng = random.Random(3)
    queries, candidates = _rand(rng, 9, 1, 70, b"ACGT") + [bytes(rng.choice(b"ACGT") for _ in range(280))], _rand(rng, 30, 0, 60, b"ACGT")
    k, stride = 6, 9
    wide_indices = np.full((len(queries), stride), UNTOUCHED, dtype=np.uint64)
    indices = wide_indices[:, :k]
    indices[:] = np.random.default_rng(4).integers(0, len(candidates), size=indices.shape, dtype=np.uint64)
    indices[0, 2] = indices[3, 0] = indices[3, 5] = indices[9, 1] = EMPTY  # in the middle of rows, of both routes
    indices[4, :] = EMPTY                                                    # a row that lists nothing
    indices[5, :] = 7                                                        # one candidate six times
    indices[6, 1] = indices[6, 4] = indices[6, 0]
    wide_scores = np.full((len(queries), stride), UNTOUCHED, dtype=np.uint64)
    rerank_knob(knob)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    engine.rerank(queries, candidates, indices, device=gpu, out=wide_scores[:, :k])
    want = expected(oracle.levenshtein(queries, candidates), indices)
    assert np.array_equal(wide_scores[:, :k], want)
    assert (wide_scores[:, k:] == UNTOUCHED).all() and (wide_indices[:, k:] == UNTOUCHED).all()
    assert (wide_scores[4, :k] == 0).all()


def test_descending_offsets_of_a_candidate_are_refused_by_every_kernel(gpu, oracle):
    """A listed candidate whose offsets descend: each of the four kernels refuses it before it addresses anything (the TAPE flag), the
    call reports it, and with the offset restored the same calls answer as the oracle and the plain DP do."""
    from test_gpu_fuzzy_spans import dense, listed, same

    rng = random.Random(17)
    short, long = _rand(rng, 4, 5, 40, b"ACGT"), _rand(rng, 4, 300, 400, b"ACGT")
    queries = [short[0], long[0], short[1], long[1], short[2], long[2], short[3], long[3]]  # one call, both rerank kernels
    plain = _rand(rng, 12, 10, 60, b"ACGT")
    candidates = szs.Strs(plain).to_device(0)
    indices = np.random.default_rng(17).integers(0, len(plain), size=(len(queries), 4), dtype=np.uint64)
    indices[:, 1] = 5  # every row lists candidate 5
    engine = szs.LevenshteinDistances(capabilities=gpu)
    calls = [lambda: engine.rerank(queries, candidates, indices, device=gpu),
             lambda: engine.fuzzy_find(short, candidates, indices[:4], device=gpu),
             lambda: engine.fuzzy_find(short, candidates, indices[:4], device=gpu, starts=True)]

    _, _, offsets = candidates._device
    kept = offsets[6].clone()
    offsets[6] = offsets[5] - 3  # candidate 5 now "ends" before it begins; every other string still lies inside the tape
    for call in calls:
        with pytest.raises(szs.StringZillasError) as refused:
            call()
        assert refused.value.status_name == "unexpected_dimensions" and "ascend" in str(refused.value).lower(), str(refused.value)
    offsets[6] = kept

    assert np.array_equal(calls[0](), expected(oracle.levenshtein(queries, plain), indices))  # the engine goes on
    distances, starts, ends = listed(dense(short, plain), indices[:4])
    assert same(calls[1](), (distances, ends))
    assert same(calls[2](), (distances, starts, ends))


def test_an_index_past_the_end_is_refused(gpu):
    import torch

    queries, candidates = [b"ACGT", b"AC", b"GATTACA"], [b"ACG", b"T", b"", b"GATT"]
    engine = szs.LevenshteinDistances(capabilities=gpu)
    indices = np.array([[0, 1], [2, 3], [3, 0]], dtype=np.uint64)
    assert engine.rerank(queries, candidates, indices, device=gpu).shape == (3, 2)
    indices[1, 1] = len(candidates)  # one past the end
    with pytest.raises(szs.StringZillasError) as refused:
        engine.rerank(queries, candidates, indices, device=gpu)
    assert refused.value.status_name == "unexpected_dimensions"
    on_device = torch.from_numpy(indices.view(np.int64)).cuda()  # only the kernel can read these: it checks before every use
    with pytest.raises(szs.StringZillasError) as refused:
        engine.rerank(queries, candidates, on_device, device=gpu)
    assert refused.value.status_name == "unexpected_dimensions"
    indices[1, 1] = 3
    assert np.array_equal(engine.rerank(queries, candidates, torch.from_numpy(indices.view(np.int64)).cuda(), device=gpu),
                          np.array([[1, 3], [2, 3], [3, 5]], dtype=np.uint64))  # by hand: ACGT~ACG, ACGT~T; AC~"", AC~GATT; GATTACA~GATT, ~ACG


def test_placement(gpu, oracle, rerank_knob):
    import torch

    rng = random.Random(8)
    queries = _rand(rng, 8, 1, 90, b"ACGT")
    queries[6] = bytes(rng.choice(b"ACGT") for _ in range(270))  # one row of the row route in every call
    candidates = _rand(rng, 25, 0, 90, b"ACGT")
    k = 5
    indices = np.random.default_rng(5).integers(0, len(candidates), size=(8, k), dtype=np.uint64)
    indices[2, 1] = EMPTY
    want = expected(oracle.levenshtein(queries, candidates), indices)
    engine = szs.LevenshteinDistances(capabilities=gpu)

    def placed(array, where):
        tensor = torch.from_numpy(array.view(np.int64).copy())
        return array.copy() if where == "numpy" else tensor.pin_memory() if where == "pinned" else tensor.cuda()

    def as_numpy(array):
        return array if isinstance(array, np.ndarray) else array.cpu().numpy().view(np.uint64)

    for where_indices in ("numpy", "pinned", "device"):
        for where_out in ("numpy", "pinned", "device"):
            out = placed(np.full((8, k), UNTOUCHED, dtype=np.uint64), where_out)
            returned = engine.rerank(queries, candidates, placed(indices, where_indices), device=gpu, out=out)
            assert returned is out and np.array_equal(as_numpy(out), want), (where_indices, where_out)
        assert np.array_equal(engine.rerank(queries, candidates, placed(indices, where_indices), device=gpu), want), where_indices

    # u64 tapes, and the self form: the indices refer to the queries, the own index included
    wide = engine.rerank(szs.Strs(queries, wide_offsets=True), szs.Strs(candidates, wide_offsets=True), indices, device=gpu)
    assert np.array_equal(wide, want)
    own = np.random.default_rng(6).integers(0, len(queries), size=(8, 3), dtype=np.uint64)
    own[:, 0] = np.arange(8)
    for knob in (None, 0):
        rerank_knob(knob)
        assert np.array_equal(engine.rerank(queries, None, own, device=gpu), expected(oracle.levenshtein(queries, queries), own)), knob
    rerank_knob(None)

    # u32 tapes whose offsets are in host memory (bytes on the device): the kernel reads refs built from them
    error = ctypes.c_char_p()

    def host_offsets_tape(strings):
        strs = szs.Strs(strings).to_device(0)
        return _abi.U32Tape(strs._device[1].data_ptr(), strs.offsets.ctypes.data, len(strings)), strs

    (q_tape, q_keep), (c_tape, c_keep) = host_offsets_tape(queries), host_offsets_tape(candidates)
    scores = np.zeros((8, k), np.uint64)
    status = _abi.lib.szs_rocm_rerank_u32tape(engine.handle, gpu.handle, ctypes.byref(q_tape), ctypes.byref(c_tape), indices.ctypes.data, k,
                                              scores.ctypes.data, k, ctypes.byref(error))
    assert status == 0, error.value
    assert np.array_equal(scores, want)

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
    for knob in (None, 0):
        rerank_knob(knob)
        scores = np.zeros((8, k), np.uint64)
        status = _abi.lib.szs_rocm_rerank(engine.handle, gpu.handle, ctypes.byref(q_seq), ctypes.byref(c_seq), indices.ctypes.data, k,
                                          scores.ctypes.data, k, ctypes.byref(error))
        assert status == 0, error.value
        assert np.array_equal(scores, want), knob


def _family(name, gpu):
    """(engine, oracle function of (queries, candidates), alphabet of the random strings): the engines of tests/test_gpu_top_k.py"""
    if name == "levenshtein_affine":
        return szs.LevenshteinDistances(0, 2, 3, 1, capabilities=gpu), lambda o, q, c: o.levenshtein(q, c, 0, 2, 3, 1), b"abcdef"
    if name == "levenshtein_utf8":
        return szs.LevenshteinDistancesUTF8(capabilities=gpu), lambda o, q, c: o.levenshtein_utf8(q, c), None
    if name == "needleman_wunsch":
        table = matrices.blosum62()
        return (szs.NeedlemanWunschScores(*table, open=-4, extend=-4, capabilities=gpu),
                lambda o, q, c: o.needleman_wunsch(q, c, *table, -4, -4), b"ARNDCQEGHILKMFPSTWYV")
    table = matrices.nuc44()
    return szs.SmithWatermanScores(*table, open=-4, extend=-1, capabilities=gpu), lambda o, q, c: o.smith_waterman(q, c, *table, -4, -1), b"ACGT"


def _utf8_strings(rng, count):
    pieces = ["a", "b", "é", "ж", "中", "😀", "ß"]
    return ["".join(rng.choice(pieces) for _ in range(rng.randint(1, 30))).encode() for _ in range(count)]


@pytest.mark.parametrize("family", ["levenshtein_affine", "levenshtein_utf8", "needleman_wunsch", "smith_waterman"])
def test_other_families_take_the_row_route(gpu, oracle, family):
    rng = random.Random(len(family))
    engine, score, alphabet = _family(family, gpu)
    if alphabet is None:
        queries, candidates = _utf8_strings(rng, 8), _utf8_strings(rng, 19)
    else:
        queries, candidates = _rand(rng, 8, 1, 40, alphabet), _rand(rng, 19, 1, 40, alphabet)
    indices = np.random.default_rng(7).integers(0, len(candidates), size=(8, 5), dtype=np.uint64)
    indices[1, 2] = EMPTY
    scores = engine.rerank(queries, candidates, indices, device=gpu)
    assert scores.dtype == engine._dtype
    assert np.array_equal(scores, expected(score(oracle, queries, candidates), indices, dtype=engine._dtype))
    assert engine.last_call_profile().launches >= 8


@pytest.mark.parametrize("family", ["levenshtein", "smith_waterman"])
def test_rerank_of_top_k_returns_its_scores(gpu, family):
    rng = random.Random(12)
    if family == "levenshtein":
        engine = szs.LevenshteinDistances(capabilities=gpu)
    else:
        engine = szs.SmithWatermanScores(*matrices.nuc44(), open=-4, extend=-1, capabilities=gpu)
    queries, candidates = _rand(rng, 11, 1, 60, b"ACGT"), _rand(rng, 14, 1, 60, b"ACGT")
    for k in (4, len(candidates) + 3):  # beyond the candidates: rows end in empty slots
        indices, scores = engine.top_k(queries, candidates, k=k, device=gpu)
        assert np.array_equal(engine.rerank(queries, candidates, indices, device=gpu), scores), k
    for k in (3, len(queries) + 2):
        indices, scores = engine.top_k(queries, None, k=k, device=gpu)
        assert np.array_equal(engine.rerank(queries, None, indices, device=gpu), scores), k

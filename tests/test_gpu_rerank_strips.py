"""Rerank rows whose query has more than 256 bytes (`hip/myers_rerank_strips.hip`, the STRIPS route of host/rerank.c): every score
against the oracle's cell `matrix[q, indices[q, r]]`, and against the same call routed by the `rerank` knob."""
import ctypes
import random

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi

pytestmark = pytest.mark.gpu

EMPTY = np.uint64(2**64 - 1)
UNTOUCHED = 0x5A5A5A5A5A5A5A5A
# around every strip boundary of 5 ... 8 words, two and three strips, eight and nine, and one of 17 strips
QUERY_LENGTHS = (257, 258, 287, 288, 289, 319, 320, 321, 511, 512, 513, 1000, 2047, 2048, 2049, 4100)
CANDIDATE_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129)  # around the groups of 16 parked columns and the text dwords
EVERY_BYTE = bytes(range(256))


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


def _string(rng, length, alphabet):
    return bytes(rng.choice(alphabet) for _ in range(length))


def expected(matrix, indices):
    """The oracle's cell for every listed index; 0 for an empty slot."""
    indices = np.asarray(indices, dtype=np.uint64)
    want = np.zeros(indices.shape, dtype=np.uint64)
    for q in range(indices.shape[0]):
        for r in range(indices.shape[1]):
            if indices[q, r] != EMPTY:
                want[q, r] = matrix[q, int(indices[q, r])]
    return want


@pytest.fixture(scope="module")
def documents(oracle):
    """Two queries of every length - one over ACGT, one over all 256 byte values - interleaved so that neighbouring rows differ
    (257 next to 4100, 258 next to 2049 ...); the candidates of CANDIDATE_LENGTHS, forty of 0 ... 400 bytes, one equal to a query
    and, last, one of 5000 bytes; the oracle's matrix - computed once, never changed."""
    rng = random.Random(91)
    ascending = [_string(rng, length, alphabet) for length in QUERY_LENGTHS for alphabet in (b"ACGT", EVERY_BYTE)]
    queries = []
    while ascending:
        queries.append(ascending.pop(0))
        if ascending:
            queries.append(ascending.pop())
    candidates = [_string(rng, length, b"ACGT") for length in CANDIDATE_LENGTHS]
    candidates += [_string(rng, rng.randint(0, 400), EVERY_BYTE if i % 2 else b"ACGT") for i in range(40)]
    candidates += [queries[5], _string(rng, 5000, b"ACGT")]
    matrix = oracle.levenshtein(queries, candidates)
    matrix.setflags(write=False)
    return queries, candidates, matrix


@pytest.mark.parametrize("k", [1, 16, 17, 65, 130])
def test_strip_boundaries_and_table_rows(gpu, documents, rerank_knob, k):
    queries, candidates, matrix = documents
    rng = np.random.default_rng(k)
    indices = rng.integers(0, len(candidates), size=(len(queries), k), dtype=np.uint64)
    if k > 1:
        indices[:, k // 2] = len(candidates) - 1  # the 5000-byte candidate in every row
        indices[:, 0] = len(candidates) - 2       # and the one that is a query: distance 0 in its own row
    want = expected(matrix, indices)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    automatic = engine.rerank(queries, candidates, indices, device=gpu)
    assert automatic.dtype == np.uint64 and automatic.shape == indices.shape
    assert np.array_equal(automatic, want), np.argwhere(automatic != want)[:8]
    assert engine.last_call_profile().launches == 1  # every row is a document: one launch of the strips kernel
    for knob in (1, 0):
        rerank_knob(knob)
        routed = engine.rerank(queries, candidates, indices, device=gpu)
        assert np.array_equal(routed, want), (knob, np.argwhere(routed != want)[:8])
        assert np.array_equal(routed, automatic)


def test_whole_phantom_strips(gpu, oracle):
    """One wavefront at L = 16: four rows at the 17 strips of 8 words of the 4100-byte query, so the 257-byte row is sixteen
    whole strips of phantom rows above nine rows of pattern."""
    rng = random.Random(17)
    queries = [_string(rng, length, b"ACGT") for length in (4100, 257, 2048, 300)]
    candidates = [_string(rng, length, b"ACGT") for length in (0, 1, 16, 17, 100, 255, 256, 257, 300, 640, 1000, 2048)]
    indices = np.random.default_rng(3).integers(0, len(candidates), size=(4, 16), dtype=np.uint64)
    indices[:, :len(candidates)] = np.arange(len(candidates))  # every candidate in every row
    engine = szs.LevenshteinDistances(capabilities=gpu)
    got = engine.rerank(queries, candidates, indices, device=gpu)
    want = expected(oracle.levenshtein(queries, candidates), indices)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert engine.last_call_profile().launches == 1


def test_routing_shows_in_the_profile(gpu, oracle, rerank_knob):
    rng = random.Random(64)
    queries = [_string(rng, rng.randint(300, 600), b"ACGT") for _ in range(64)]
    candidates = [_string(rng, rng.randint(0, 90), b"ACGT") for _ in range(40)]
    indices = np.random.default_rng(2).integers(0, len(candidates), size=(64, 16), dtype=np.uint64)
    indices[5, 3] = indices[9, :4] = indices[63, 15] = EMPTY
    want = expected(oracle.levenshtein(queries, candidates), indices)
    pairs = int((indices != EMPTY).sum())
    cells = sum(len(queries[q]) * len(candidates[int(i)]) for q in range(64) for i in indices[q] if i != EMPTY)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    assert np.array_equal(engine.rerank(queries, candidates, indices, device=gpu), want)
    profile = engine.last_call_profile()
    assert profile.launches <= 2 and profile.pairs == pairs and profile.cells == cells
    assert profile.longest_query == max(len(q) for q in queries)
    rerank_knob(1)
    assert np.array_equal(engine.rerank(queries, candidates, indices, device=gpu), want)
    profile = engine.last_call_profile()
    assert profile.launches >= 64 and profile.pairs == pairs


def test_all_three_routes_in_one_call(gpu, oracle):
    import torch

    rng = random.Random(5)
    lengths = [rng.choice((10, 200, 256, 257, 900)) for _ in range(23)]
    lengths[3], lengths[4], lengths[5], lengths[6] = 256, 257, 10, 900  # neighbours of different routes
    lengths.insert(11, 70000)                                            # ONE row beyond the strips kernel: the row route
    queries = [_string(rng, length, b"ACGT") for length in lengths]
    short = [_string(rng, rng.randint(0, 64), b"ACGT") for _ in range(30)]
    candidates = short + [_string(rng, rng.randint(65, 500), b"ACGT") for _ in range(10)]
    k, stride = 6, 9
    wide_indices = np.full((len(queries), stride), UNTOUCHED, dtype=np.uint64)
    indices = wide_indices[:, :k]
    indices[:] = np.random.default_rng(6).integers(0, len(candidates), size=indices.shape, dtype=np.uint64)
    indices[11] = np.random.default_rng(7).integers(0, len(short), size=k, dtype=np.uint64)  # the long row lists short candidates only
    indices[2, 1] = indices[4, 0] = indices[11, 5] = EMPTY
    matrix = np.zeros((len(queries), len(candidates)), dtype=np.uint64)
    others = [q for q in range(len(queries)) if q != 11]
    matrix[others] = oracle.levenshtein([queries[q] for q in others], candidates)
    matrix[11, :len(short)] = oracle.levenshtein([queries[11]], short)[0]
    want = expected(matrix, indices)

    engine = szs.LevenshteinDistances(capabilities=gpu)
    wide_scores = np.full((len(queries), stride), UNTOUCHED, dtype=np.uint64)
    engine.rerank(queries, candidates, indices, device=gpu, out=wide_scores[:, :k])
    assert np.array_equal(wide_scores[:, :k], want), np.argwhere(wide_scores[:, :k] != want)[:8]
    assert (wide_scores[:, k:] == UNTOUCHED).all() and (wide_indices[:, k:] == UNTOUCHED).all()
    profile = engine.last_call_profile()
    assert profile.longest_query == 70000 and profile.pairs == int((indices != EMPTY).sum())

    device_indices = torch.from_numpy(wide_indices.view(np.int64)).cuda()
    device_scores = torch.from_numpy(np.full((len(queries), stride), UNTOUCHED, dtype=np.uint64).view(np.int64)).cuda()
    engine.rerank(queries, candidates, device_indices[:, :k], device=gpu, out=device_scores[:, :k])
    landed = device_scores.cpu().numpy().view(np.uint64)
    assert np.array_equal(landed[:, :k], want) and (landed[:, k:] == UNTOUCHED).all()


def test_forms(gpu, oracle):
    import torch

    rng = random.Random(8)
    queries = [_string(rng, length, b"ACGT") for length in (300, 40, 1025, 257, 700, 256, 513, 333)]
    candidates = [_string(rng, rng.randint(0, 300), b"ACGT") for _ in range(25)]
    k = 5
    indices = np.random.default_rng(5).integers(0, len(candidates), size=(8, k), dtype=np.uint64)
    indices[0, :] = 7                                   # one candidate five times
    indices[2, 1] = indices[2, 4] = indices[2, 0]       # duplicates within a row
    indices[4, :] = EMPTY                               # a document that lists nothing
    indices[6, 2] = EMPTY
    want = expected(oracle.levenshtein(queries, candidates), indices)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    got = engine.rerank(queries, candidates, indices, device=gpu)
    assert np.array_equal(got, want) and (got[4] == 0).all()

    # the self form: the indices refer to the queries, the own index included
    own = np.random.default_rng(6).integers(0, len(queries), size=(8, 3), dtype=np.uint64)
    own[:, 0] = np.arange(8)
    assert np.array_equal(engine.rerank(queries, None, own, device=gpu), expected(oracle.levenshtein(queries, queries), own))

    # u64 tapes
    wide = engine.rerank(szs.Strs(queries, wide_offsets=True), szs.Strs(candidates, wide_offsets=True), indices, device=gpu)
    assert np.array_equal(wide, want)

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
    scores = np.zeros((8, k), np.uint64)
    status = _abi.lib.szs_rocm_rerank(engine.handle, gpu.handle, ctypes.byref(q_seq), ctypes.byref(c_seq), indices.ctypes.data, k,
                                      scores.ctypes.data, k, ctypes.byref(error))
    assert status == 0, error.value
    assert np.array_equal(scores, want)


def test_an_index_past_the_end_is_refused(gpu, oracle):
    import torch

    rng = random.Random(4)
    queries = [_string(rng, length, b"ACGT") for length in (300, 400, 500)]
    candidates = [_string(rng, length, b"ACGT") for length in (3, 70, 0, 410)]
    engine = szs.LevenshteinDistances(capabilities=gpu)
    indices = np.array([[0, 1], [2, 3], [3, 0]], dtype=np.uint64)
    want = expected(oracle.levenshtein(queries, candidates), indices)
    assert np.array_equal(engine.rerank(queries, candidates, indices, device=gpu), want)
    indices[1, 1] = len(candidates)  # one past the end, in the row of the 400-byte query
    with pytest.raises(szs.StringZillasError) as refused:
        engine.rerank(queries, candidates, indices, device=gpu)
    assert refused.value.status_name == "unexpected_dimensions"
    on_device = torch.from_numpy(indices.view(np.int64)).cuda()  # only the kernel can read these: it checks before every use
    with pytest.raises(szs.StringZillasError) as refused:
        engine.rerank(queries, candidates, on_device, device=gpu)
    assert refused.value.status_name == "unexpected_dimensions"
    indices[1, 1] = 3
    assert np.array_equal(engine.rerank(queries, candidates, torch.from_numpy(indices.view(np.int64)).cuda(), device=gpu), want)

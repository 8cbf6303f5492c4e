"""Fuzzy find on the GPU (`szs_rocm_fuzzy_find*`, `_Engine.fuzzy_find`): every distance and every end against the plain semi-global
DP below - D[0][j] = 0, D[i][0] = i, unit costs; the minimum of the last row and the smallest j that attains it."""
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


def semi_global(query, texts):
    """(distances, ends) of `query` inside every text, vectorised over the texts."""
    m, pattern, rows = len(query), np.frombuffer(query, np.uint8), np.arange(len(query) + 1)
    lengths = np.array([len(text) for text in texts])
    padded = np.zeros((len(texts), max(lengths.max(initial=0), 1)), np.uint8)
    for at, text in enumerate(texts):
        padded[at, :len(text)] = np.frombuffer(text, np.uint8)
    column = np.tile(rows, (len(texts), 1))
    best, end = column[:, m].copy(), np.zeros(len(texts), np.int64)
    for j in range(1, int(lengths.max(initial=0)) + 1):
        step = np.zeros_like(column)
        step[:, 1:] = np.minimum(column[:, :-1] + (pattern[None, :] != padded[:, j - 1, None]), column[:, 1:] + 1)
        column = np.minimum.accumulate(step - rows, axis=1) + rows  # the insertions down the column
        better = (j <= lengths) & (column[:, m] < best)
        best[better], end[better] = column[better, m], j
    return best, end


def dense(queries, candidates):
    """The (queries x candidates) matrices of distances and ends."""
    both = [semi_global(query, candidates) for query in queries]
    return (np.array([d for d, _ in both], dtype=np.uint64).reshape(len(queries), len(candidates)),
            np.array([e for _, e in both], dtype=np.uint64).reshape(len(queries), len(candidates)))


def listed(matrices_pair, indices):
    """The cells the indices list; (0, 0) for an empty slot."""
    indices = np.asarray(indices, dtype=np.uint64)
    safe = np.where(indices == EMPTY, 0, indices).astype(np.int64)
    rows = np.arange(indices.shape[0])[:, None]
    return tuple(np.where(indices == EMPTY, np.uint64(0), matrix[rows, safe]) for matrix in matrices_pair)


def _rand(rng, count, lo, hi, alphabet):
    return [bytes(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(count)]


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return szs.DeviceScope(gpu_device=0)


@pytest.fixture(scope="module")
def engine(gpu):
    return szs.LevenshteinDistances(capabilities=gpu)


def _widths(alphabet, seed):
    """Two queries of every length, interleaved so that rows of different `pad` share a wavefront (0 next to 256, 1 next to 255 ...),
    candidates of 0 ... 9 bytes and of U[0, 700] - odd lengths first, so most start at odd tape offsets - and the DP's matrices."""
    rng = random.Random(seed)
    ascending = [bytes(rng.choice(alphabet) for _ in range(length)) for length in QUERY_LENGTHS for _ in range(2)]
    queries = []
    while ascending:
        queries.append(ascending.pop(0))
        if ascending:
            queries.append(ascending.pop())
    lengths = [1, 3, 0, 4, 5, 7, 8, 9] + [rng.randint(0, 700) for _ in range(36)]
    candidates = [bytes(rng.choice(alphabet) for _ in range(length)) for length in lengths]
    candidates[11] = candidates[10][:50] + queries[1] + candidates[10][50:90]  # a longest query, whole, inside one text
    want = dense(queries, candidates)
    for matrix in want:
        matrix.setflags(write=False)
    return queries, candidates, want


@pytest.fixture(scope="module")
def widths_ab():
    return _widths(b"ab", 41)


@pytest.fixture(scope="module")
def widths_bytes():
    return _widths(bytes(range(256)), 43)


@pytest.mark.parametrize("alphabet", ["ab", "bytes"])
def test_body_widths_and_word_boundaries(gpu, engine, widths_ab, widths_bytes, alphabet):
    queries, candidates, want = widths_ab if alphabet == "ab" else widths_bytes
    distances, ends = engine.fuzzy_find(queries, candidates, device=gpu)  # dense: every query in every candidate, ONE call
    assert distances.dtype == np.uint64 and ends.dtype == np.uint64 and distances.shape == (len(queries), len(candidates))
    assert np.array_equal(distances, want[0]), np.argwhere(distances != want[0])[:8]
    assert np.array_equal(ends, want[1]), np.argwhere(ends != want[1])[:8]
    assert engine.last_call_profile().launches == 1


@pytest.mark.parametrize("k", [1, 16, 17, 33, 64, 65, 130])
def test_lanes_and_chunks(gpu, engine, widths_ab, k):
    queries, candidates, want = widths_ab
    rng = np.random.default_rng(k)
    indices = rng.integers(0, len(candidates), size=(len(queries), k), dtype=np.uint64)
    indices[:, 0] = 11  # one candidate listed in every row
    if k > 1:
        indices[3, 1] = indices[7, k - 1] = indices[5, k // 2] = EMPTY  # empty slots at the start, the end and the middle of rows
        indices[9, :] = EMPTY                                           # a row that lists nothing
        indices[12, :] = 13                                             # one candidate k times
        indices[14, 1:] = indices[14, 0]
    want_distances, want_ends = listed(want, indices)
    distances, ends = engine.fuzzy_find(queries, candidates, indices, device=gpu)
    assert distances.shape == indices.shape and ends.shape == indices.shape
    assert np.array_equal(distances, want_distances), np.argwhere(distances != want_distances)[:8]
    assert np.array_equal(ends, want_ends), np.argwhere(ends != want_ends)[:8]
    profile = engine.last_call_profile()
    assert profile.launches == 1 and profile.pairs == int((indices != EMPTY).sum())


def test_planted_matches(gpu, engine):
    rng = random.Random(5)
    queries, candidates, by_hand = [], [], []
    for m in (1, 17, 40, 64, 100, 256):
        query = bytes(rng.choice(b"abcd") for _ in range(m))
        at = rng.randrange(1, m) if m > 1 else 0  # inside: an insertion in front would leave the copy whole
        before, after = (bytes(rng.choice(b"wxyz") for _ in range(rng.randint(30, 300))) for _ in range(2))  # none of the query's bytes
        for copy, distance in ((query, 0), (query[:at] + b"w" + query[at + 1:], 1), (query[:at] + b"w" + query[at:], 1),
                               (query[:at] + query[at + 1:], 1)):
            if m == 1 and distance:  # one byte, edited, is no occurrence at all
                continue
            for text in (copy + after, before + copy + after, before + copy):  # at offset 0, in the middle, at the very end
                queries.append(query), candidates.append(text)
                by_hand.append((distance, text.index(copy) + len(copy) if not distance else None))
    queries += [b"ab", b"abcd" * 9]
    candidates += [b"abababab", b"wxyz" * 50]
    indices = np.arange(len(queries), dtype=np.uint64)[:, None]  # pair i: query i in candidate i
    distances, ends = engine.fuzzy_find(queries, candidates, indices, device=gpu)
    for pair, (distance, end) in enumerate(by_hand):
        assert distances[pair, 0] == distance, (pair, queries[pair], candidates[pair])
        if end is not None:
            assert ends[pair, 0] == end, (pair, queries[pair], candidates[pair])
    assert (distances[-2, 0], ends[-2, 0]) == (0, 2)    # the leftmost end
    assert (distances[-1, 0], ends[-1, 0]) == (36, 0)   # bytes the text does not contain: the empty substring
    for pair in range(len(queries)):                    # ... and every end, the edited copies' too, against the DP
        want = semi_global(queries[pair], [candidates[pair]])
        assert (distances[pair, 0], ends[pair, 0]) == (want[0][0], want[1][0]), pair


def _c_call(name, engine, gpu, queries, candidates, indices, k, distances, ends, stride):
    """One C-ABI call over tapes / sequences that the caller keeps alive; pointers as integers or None."""
    error = ctypes.c_char_p()
    status = getattr(_abi.lib, name)(engine.handle, gpu.handle, ctypes.byref(queries), None if candidates is None else ctypes.byref(candidates),
                                     indices, k, distances, ends, stride, ctypes.byref(error))
    return status, error.value


@pytest.fixture(scope="module")
def small():
    rng = random.Random(8)
    queries = _rand(rng, 9, 1, 90, b"ACGT") + [b""]
    candidates = _rand(rng, 25, 0, 300, b"ACGT")
    want = dense(queries, candidates)
    for matrix in want:
        matrix.setflags(write=False)
    return queries, candidates, want


def test_forms(gpu, engine, small):
    import torch

    queries, candidates, want = small
    rows, count = len(queries), len(candidates)
    # the dense form - Python `indices=None`, C `indices` NULL - equals the listed form with arange rows
    everything = np.tile(np.arange(count, dtype=np.uint64), (rows, 1))
    by_list = engine.fuzzy_find(queries, candidates, everything, device=gpu)
    by_none = engine.fuzzy_find(queries, candidates, device=gpu)
    for got in (by_list, by_none):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    keep = [szs.Strs(queries).to_device(0), szs.Strs(candidates).to_device(0), szs.Strs(queries, wide_offsets=True).to_device(0),
            szs.Strs(candidates, wide_offsets=True).to_device(0)]
    q32, c32, q64, c64 = (strs._tape(0) for strs in keep)

    # sz_sequence_t callbacks, each string at its own device address
    def sequence_of(strings):
        tensors = [torch.tensor(list(s), dtype=torch.uint8, device="cuda") for s in strings]
        starts, lengths = [t.data_ptr() for t in tensors], [len(s) for s in strings]
        get_start = _abi.MEMBER_START(lambda handle, i: starts[i])
        get_length = _abi.MEMBER_LENGTH(lambda handle, i: lengths[i])
        keep.extend([tensors, get_start, get_length])
        return _abi.Sequence(None, len(strings), get_start, get_length)

    q_seq, c_seq = sequence_of(queries), sequence_of(candidates)
    for name, q, c in (("szs_rocm_fuzzy_find_u32tape", q32, c32), ("szs_rocm_fuzzy_find_u64tape", q64, c64), ("szs_rocm_fuzzy_find", q_seq, c_seq)):
        distances, ends = np.full((rows, count), UNTOUCHED, np.uint64), np.full((rows, count), UNTOUCHED, np.uint64)
        status, message = _c_call(name, engine, gpu, q, c, None, count, distances.ctypes.data, ends.ctypes.data, count)
        assert status == 0, message
        assert np.array_equal(distances, want[0]) and np.array_equal(ends, want[1]), name
        status, message = _c_call(name, engine, gpu, q, c, None, count - 1, distances.ctypes.data, ends.ctypes.data, count)
        assert _abi.STATUS_NAMES[status] == "unexpected_dimensions", name  # dense: k is the candidates' count
        # `ends` NULL, listed indices
        picks = np.random.default_rng(3).integers(0, count, size=(rows, 5), dtype=np.uint64)
        distances = np.full((rows, 5), UNTOUCHED, np.uint64)
        status, message = _c_call(name, engine, gpu, q, c, picks.ctypes.data, 5, distances.ctypes.data, None, 5)
        assert status == 0, message
        assert np.array_equal(distances, listed(want, picks)[0]), name

    # u32 tapes whose offsets are in host memory (bytes on the device): the kernel reads refs built from them
    q_host = _abi.U32Tape(keep[0]._device[1].data_ptr(), keep[0].offsets.ctypes.data, rows)
    c_host = _abi.U32Tape(keep[1]._device[1].data_ptr(), keep[1].offsets.ctypes.data, count)
    distances, ends = np.zeros((rows, count), np.uint64), np.zeros((rows, count), np.uint64)
    status, message = _c_call("szs_rocm_fuzzy_find_u32tape", engine, gpu, q_host, c_host, None, count, distances.ctypes.data, ends.ctypes.data, count)
    assert status == 0, message
    assert np.array_equal(distances, want[0]) and np.array_equal(ends, want[1])

    # the self form: the indices refer to the queries, the own index included
    own = np.random.default_rng(6).integers(0, rows, size=(rows, 3), dtype=np.uint64)
    own[:, 0] = np.arange(rows)
    got = engine.fuzzy_find(queries, None, own, device=gpu)
    want_own = listed(dense(queries, queries), own)
    assert np.array_equal(got[0], want_own[0]) and np.array_equal(got[1], want_own[1])
    assert (got[0][:, 0] == 0).all() and (got[1][:, 0] == [len(q) for q in queries]).all()  # a query in itself


def test_placement_and_row_stride(gpu, engine, small):
    import torch

    queries, candidates, want = small
    rows, k = len(queries), 5
    indices = np.random.default_rng(5).integers(0, len(candidates), size=(rows, k), dtype=np.uint64)
    indices[2, 1] = EMPTY
    want_distances, want_ends = listed(want, indices)

    def placed(array, where):
        tensor = torch.from_numpy(array.view(np.int64).copy())
        return array.copy() if where == "numpy" else tensor.pin_memory() if where == "pinned" else tensor.cuda()

    def as_numpy(array):
        return array if isinstance(array, np.ndarray) else array.cpu().numpy().view(np.uint64)

    blank = np.full((rows, k), UNTOUCHED, dtype=np.uint64)
    for where_indices in ("numpy", "pinned", "device"):
        for where_distances, where_ends in (("numpy", "numpy"), ("pinned", "pinned"), ("device", "device"), ("numpy", "device"), ("device", "pinned")):
            out = placed(blank, where_distances), placed(blank, where_ends)
            returned = engine.fuzzy_find(queries, candidates, placed(indices, where_indices), device=gpu, out=out)
            assert returned is out, (where_indices, where_distances, where_ends)
            assert np.array_equal(as_numpy(out[0]), want_distances), (where_indices, where_distances, where_ends)
            assert np.array_equal(as_numpy(out[1]), want_ends), (where_indices, where_distances, where_ends)
        got = engine.fuzzy_find(queries, candidates, placed(indices, where_indices), device=gpu)
        assert np.array_equal(got[0], want_distances) and np.array_equal(got[1], want_ends), where_indices

    # a row stride beyond k: the cells past k stay as they were, in host and in device arrays
    stride = 9
    for where in ("numpy", "device"):
        wide = [np.full((rows, stride), UNTOUCHED, dtype=np.uint64) for _ in range(3)]
        wide[0][:, :k] = indices
        wide = [placed(array, where) for array in wide]
        engine.fuzzy_find(queries, candidates, wide[0][:, :k], device=gpu, out=(wide[1][:, :k], wide[2][:, :k]))
        wide = [as_numpy(array) for array in wide]
        assert np.array_equal(wide[1][:, :k], want_distances) and np.array_equal(wide[2][:, :k], want_ends), where
        assert all((array[:, k:] == UNTOUCHED).all() for array in wide), where
        got = engine.fuzzy_find(queries, candidates, placed(wide[0], where)[:, :k], device=gpu)  # no `out`: the stride of the indices
        assert np.array_equal(got[0], want_distances) and np.array_equal(got[1], want_ends), where


def test_refusals(gpu, engine):
    import torch

    queries, candidates = [b"ACGT", b"AC", b"GATTACA"], [b"ACG", b"T", b"", b"GATT"]
    indices = np.array([[0, 1], [2, 3], [3, 0]], dtype=np.uint64)
    distances, ends = engine.fuzzy_find(queries, candidates, indices, device=gpu)
    assert distances.tolist() == [[1, 3], [2, 1], [3, 5]] and ends.tolist() == [[3, 1], [0, 2], [4, 2]]  # by hand
    indices[1, 1] = len(candidates)  # one past the end
    with pytest.raises(szs.StringZillasError) as refused:
        engine.fuzzy_find(queries, candidates, indices, device=gpu)
    assert refused.value.status_name == "unexpected_dimensions"
    on_device = torch.from_numpy(indices.view(np.int64)).cuda()  # only the kernel can read these: it checks before every use
    with pytest.raises(szs.StringZillasError) as refused:
        engine.fuzzy_find(queries, candidates, on_device, device=gpu)
    assert refused.value.status_name == "unexpected_dimensions"
    indices[1, 1] = 3
    again = engine.fuzzy_find(queries, candidates, torch.from_numpy(indices.view(np.int64)).cuda(), device=gpu)  # and the engine goes on
    assert np.array_equal(again[0], distances) and np.array_equal(again[1], ends)

    with pytest.raises(szs.StringZillasError) as refused:  # one query beyond the bit-vector
        engine.fuzzy_find([b"AC", b"A" * 257, b"ACGT"], candidates, indices, device=gpu)
    assert refused.value.status_name == "unexpected_dimensions" and "256" in str(refused.value)
    assert engine.fuzzy_find([b"AC", b"A" * 256, b"ACGT"], candidates, indices, device=gpu)[0][1].tolist() == [256, 255]  # in "" and in "GATT"

    table = matrices.blosum62()
    for other in (szs.LevenshteinDistances(0, 2, 3, 1, capabilities=gpu), szs.LevenshteinDistancesUTF8(capabilities=gpu),
                  szs.NeedlemanWunschScores(*table, open=-4, extend=-4, capabilities=gpu)):
        out = np.full((3, 2), UNTOUCHED, np.uint64), np.full((3, 2), UNTOUCHED, np.uint64)
        with pytest.raises(szs.StringZillasError) as refused:
            other.fuzzy_find(queries, candidates, indices, device=gpu, out=out)
        assert refused.value.status_name == "unknown"
        assert (out[0] == UNTOUCHED).all() and (out[1] == UNTOUCHED).all()


def test_relations_to_rerank_and_the_profile(gpu, engine):
    rng = random.Random(64)
    queries, candidates = _rand(rng, 64, 0, 256, b"ACGT"), _rand(rng, 40, 0, 400, b"ACGT")
    indices = np.random.default_rng(2).integers(0, len(candidates), size=(64, 16), dtype=np.uint64)
    indices[5, 3] = indices[9, :4] = EMPTY
    distances, ends = engine.fuzzy_find(queries, candidates, indices, device=gpu)
    profile = engine.last_call_profile()
    assert profile.launches == 1 and profile.pairs == int((indices != EMPTY).sum())
    assert profile.cells == sum(len(queries[q]) * len(candidates[int(i)]) for q in range(64) for i in indices[q] if i != EMPTY)
    assert profile.kernel_milliseconds > 0 and profile.host_milliseconds >= profile.kernel_milliseconds
    globally = engine.rerank(queries, candidates, indices, device=gpu)
    lengths = np.array([len(q) for q in queries], dtype=np.uint64)[:, None]
    assert (distances <= np.minimum(lengths, globally)).all()  # a substring is never further than the whole, nor than nothing
    assert (ends <= np.array([[len(candidates[int(i)]) if i != EMPTY else 0 for i in row] for row in indices], dtype=np.uint64)).all()
    want = listed(dense(queries, candidates), indices)
    assert np.array_equal(distances, want[0]) and np.array_equal(ends, want[1])

"""Fuzzy find with spans on the GPU (`szs_rocm_fuzzy_find_spans*`, `_Engine.fuzzy_find(..., starts=True)`): every distance, start and
end against the plain NumPy DP below - the semi-global DP for (distance, end), then the GLOBAL DP of the
reversed query over c[:end] reversed, whose last row is lev(q, c[end - t : end]) for every t: start = end - the smallest t that
attains the distance.  The reverse DP walks ALL of c[:end], not the kernel's window of min(end, m + d) columns."""
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
    """(distances, starts, ends) of `query` inside every text, vectorised over the texts."""
    m, pattern = len(query), np.frombuffer(query, np.uint8)
    lengths = np.array([len(text) for text in texts], dtype=np.int64)
    best, end = np.full(len(texts), m, np.int64), np.zeros(len(texts), np.int64)
    for j, last in _columns(pattern, texts, lengths, free_start=True):  # `semi_global` of tests/test_gpu_fuzzy_find.py, restated
        better = (j <= lengths) & (last < best)
        best[better], end[better] = last[better], j
    heads = [text[:int(e)][::-1] for text, e in zip(texts, end)]  # c[:end] reversed, against the reversed query
    least, back = np.full(len(texts), m, np.int64), np.zeros(len(texts), np.int64)
    for t, last in _columns(pattern[::-1], heads, end, free_start=False):
        better = (t <= end) & (last < least)
        least[better], back[better] = last[better], t  # strictly smaller: the smallest t, the shortest match
    assert np.array_equal(least, best)  # some start attains d, none gives less
    assert (np.abs(back - m) <= best).all()  # |t* - m| <= d: the bound on the kernel's window
    return best, end - back, end


def dense(queries, candidates):
    """The (queries x candidates) matrices of distances, starts and ends."""
    triples = [spans(query, candidates) for query in queries]
    return tuple(np.array([triple[part] for triple in triples], dtype=np.uint64).reshape(len(queries), len(candidates)) for part in range(3))


def listed(matrices_triple, indices):
    """The cells the indices list; (0, 0, 0) for an empty slot."""
    indices = np.asarray(indices, dtype=np.uint64)
    safe = np.where(indices == EMPTY, 0, indices).astype(np.int64)
    rows = np.arange(indices.shape[0])[:, None]
    return tuple(np.where(indices == EMPTY, np.uint64(0), matrix[rows, safe]) for matrix in matrices_triple)


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want)) and len(got) == len(want)


def frozen(triple):
    for matrix in triple:
        matrix.setflags(write=False)
    return triple


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
    44 candidates of 0 ... 9 bytes and of U[0, 700] - odd lengths first, so windows begin at every byte alignment - and the DP's matrices."""
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
    return queries, candidates, frozen(dense(queries, candidates))


@pytest.fixture(scope="module")
def widths_ab():
    return _widths(b"ab", 41)


@pytest.fixture(scope="module")
def widths_bytes():
    return _widths(bytes(range(256)), 43)


def _cells(queries, candidates, indices, want):
    """What the profile's `cells` must be: m x n of the forward pass plus m x min(end, m + d) of the reverse one, over the filled slots."""
    total = 0
    for q, row in enumerate(indices):
        for r, index in enumerate(row):
            if index != EMPTY:
                m = len(queries[q])
                total += m * len(candidates[int(index)]) + m * min(int(want[2][q, r]), m + int(want[0][q, r]))
    return total


@pytest.mark.parametrize("alphabet", ["ab", "bytes"])
def test_base_batch_every_width_and_alignment(gpu, engine, widths_ab, widths_bytes, alphabet):
    queries, candidates, want = widths_ab if alphabet == "ab" else widths_bytes
    got = engine.fuzzy_find(queries, candidates, device=gpu, starts=True)  # dense: every query in every candidate
    profile = engine.last_call_profile()
    assert len(got) == 3 and all(matrix.dtype == np.uint64 and matrix.shape == (len(queries), len(candidates)) for matrix in got)
    for part, name in enumerate(("distances", "starts", "ends")):
        assert np.array_equal(got[part], want[part]), (name, np.argwhere(got[part] != want[part])[:8])
    everything = np.tile(np.arange(len(candidates), dtype=np.uint64), (len(queries), 1))
    assert profile.launches == 2 and profile.pairs == everything.size
    assert profile.cells == _cells(queries, candidates, everything, want)
    plain = engine.fuzzy_find(queries, candidates, device=gpu)  # the existing call: bit-equal distances and ends, one launch
    assert engine.last_call_profile().launches == 1
    assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[2])


def _planted():
    """A 256-byte query planted four ways, the texts around it over bytes the query does not have; by-hand (distance, start, end)."""
    rng = random.Random(9)
    query = bytes(rng.choice(b"abcd") for _ in range(256))
    before, after = (bytes(rng.choice(b"wxyz") for _ in range(length)) for length in (301, 77))
    at = 100
    deleted, inserted = query[:at] + query[at + 1:], query[:at] + b"w" + query[at:]
    texts = [query + after, before + query, before + deleted + after, before + inserted + after]
    by_hand = [(0, 0, 256),                                  # at byte 0: the window is clipped by `end`
               (0, len(before), len(before) + 256),          # at the very end of the text
               (1, len(before), len(before) + 255),          # one deletion: t* = m - 1
               (1, len(before), len(before) + 257)]          # one insertion: t* = m + 1
    return query, texts, by_hand


def test_planted_occurrences(gpu, engine):
    query, texts, by_hand = _planted()
    want = spans(query, texts)
    assert [tuple(int(part[i]) for part in want) for i in range(len(texts))] == by_hand  # the DP and the hand agree
    queries = [query] * len(texts) + [b"survey", b"ab", b"xyz"]
    candidates = texts + [b"surgery", b"abababab", b"abab"]
    indices = np.arange(len(queries), dtype=np.uint64)[:, None]  # pair i: query i in candidate i
    got = engine.fuzzy_find(queries, candidates, indices, device=gpu, starts=True)
    triples = [tuple(int(part[i, 0]) for part in got) for i in range(len(queries))]
    assert triples == by_hand + [(2, 0, 5), (0, 0, 2), (3, 0, 0)]


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
    expected = listed(want, indices)
    got = engine.fuzzy_find(queries, candidates, indices, device=gpu, starts=True)
    profile = engine.last_call_profile()
    for part, name in enumerate(("distances", "starts", "ends")):
        assert got[part].shape == indices.shape
        assert np.array_equal(got[part], expected[part]), (name, np.argwhere(got[part] != expected[part])[:8])
    assert profile.launches == 2 and profile.pairs == int((indices != EMPTY).sum())
    assert profile.cells == _cells(queries, candidates, indices, expected)
    plain = engine.fuzzy_find(queries, candidates, indices, device=gpu)
    assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[2])


@pytest.fixture(scope="module")
def small():
    rng = random.Random(8)
    queries = _rand(rng, 9, 1, 90, b"ACGT") + [b""]
    candidates = _rand(rng, 25, 0, 300, b"ACGT")
    return queries, candidates, frozen(dense(queries, candidates))


def _c_call(name, engine, gpu, queries, candidates, indices, k, distances, starts, ends, stride):
    """One C-ABI call over tapes / sequences that the caller keeps alive; pointers as integers or None."""
    error = ctypes.c_char_p()
    status = getattr(_abi.lib, name)(engine.handle, gpu.handle, ctypes.byref(queries), None if candidates is None else ctypes.byref(candidates),
                                     indices, k, distances, starts, ends, stride, ctypes.byref(error))
    return status, error.value


def test_entry_points_and_the_self_form(gpu, engine, small):
    import torch

    queries, candidates, want = small
    rows, count = len(queries), len(candidates)
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

    q_seq, c_seq = sequence_of(queries), sequence_of(candidates)
    picks = np.random.default_rng(3).integers(0, count, size=(rows, 5), dtype=np.uint64)
    results = {}
    for name, q, c in (("szs_rocm_fuzzy_find_spans_u32tape", q32, c32), ("szs_rocm_fuzzy_find_spans_u64tape", q64, c64),
                       ("szs_rocm_fuzzy_find_spans", q_seq, c_seq)):
        out = [np.full((rows, count), UNTOUCHED, np.uint64) for _ in range(3)]
        status, message = _c_call(name, engine, gpu, q, c, None, count, *(array.ctypes.data for array in out), count)  # dense
        assert status == 0, message
        assert same(out, want), name
        few = [np.full((rows, 5), UNTOUCHED, np.uint64) for _ in range(3)]
        status, message = _c_call(name, engine, gpu, q, c, picks.ctypes.data, 5, *(array.ctypes.data for array in few), 5)
        assert status == 0, message
        assert same(few, listed(want, picks)), name
        status, message = _c_call(name, engine, gpu, q, c, picks.ctypes.data, 5, few[0].ctypes.data, None, few[2].ctypes.data, 5)
        assert _abi.STATUS_NAMES[status] == "unknown" and message, name  # on a live engine too: `starts` is required
        results[name] = out + few
    first = results["szs_rocm_fuzzy_find_spans_u32tape"]
    assert all(same(other, first) for other in results.values())  # the three entry points agree with each other

    # the self form: the indices refer to the queries, the own index included
    own = np.random.default_rng(6).integers(0, rows, size=(rows, 3), dtype=np.uint64)
    own[:, 0] = np.arange(rows)
    got = engine.fuzzy_find(queries, None, own, device=gpu, starts=True)
    assert same(got, listed(dense(queries, queries), own))
    assert (got[0][:, 0] == 0).all() and (got[1][:, 0] == 0).all() and (got[2][:, 0] == [len(q) for q in queries]).all()  # a query in itself


def test_memory_kinds_and_row_stride(gpu, engine, small):
    import torch

    queries, candidates, want = small
    rows, k, stride = len(queries), 5, 9
    indices = np.random.default_rng(5).integers(0, len(candidates), size=(rows, k), dtype=np.uint64)
    indices[2, 1] = EMPTY
    expected = listed(want, indices)

    def as_numpy(array):
        return array if isinstance(array, np.ndarray) else array.cpu().numpy().view(np.uint64)

    # outputs as torch device tensors: written in place; outputs as NumPy host arrays: the staged path, all three arrays
    for where in ("device", "numpy"):
        wide = [np.full((rows, stride), UNTOUCHED, dtype=np.uint64) for _ in range(4)]
        wide[0][:, :k] = indices
        if where == "device":
            wide = [torch.from_numpy(array.view(np.int64)).cuda() for array in wide]
        out = tuple(array[:, :k] for array in wide[1:])
        returned = engine.fuzzy_find(queries, candidates, wide[0][:, :k], device=gpu, out=out, starts=True)
        assert returned is out
        wide = [as_numpy(array) for array in wide]
        assert same([array[:, :k] for array in wide[1:]], expected), where
        assert all((array[:, k:] == UNTOUCHED).all() for array in wide), where  # row_stride > k: the padding cells keep the sentinel
        assert engine.last_call_profile().launches == 2
    # host distances and ends with device starts, and the other way round: one staged output stages all three
    for on_device in ((1,), (0, 2)):
        out = [np.full((rows, k), UNTOUCHED, dtype=np.uint64) for _ in range(3)]
        out = tuple(torch.from_numpy(array.view(np.int64)).cuda() if part in on_device else array for part, array in enumerate(out))
        engine.fuzzy_find(queries, candidates, indices, device=gpu, out=out, starts=True)
        assert same([as_numpy(array) for array in out], expected), on_device
    assert same(engine.fuzzy_find(queries, candidates, wide[0][:, :k], device=gpu, starts=True), expected)  # no `out`: the indices' stride


def test_refusals_and_the_existing_call_afterwards(gpu, engine):
    import torch

    queries, candidates = [b"ACGT", b"AC", b"GATTACA"], [b"ACG", b"T", b"", b"GATT"]
    indices = np.array([[0, 1], [2, 3], [3, 0]], dtype=np.uint64)
    good = engine.fuzzy_find(queries, candidates, indices, device=gpu, starts=True)
    assert good[0].tolist() == [[1, 3], [2, 1], [3, 5]] and good[2].tolist() == [[3, 1], [0, 2], [4, 2]]  # by hand, as fuzzy_find's test
    assert good[1].tolist() == [[0, 0], [0, 1], [0, 0]]  # "ACG"; "T" for one of four; ""; "A"->"T"; "GATT"; "AC"
    indices[1, 1] = len(candidates)  # one past the end
    with pytest.raises(szs.StringZillasError) as refused:
        engine.fuzzy_find(queries, candidates, indices, device=gpu, starts=True)
    assert refused.value.status_name == "unexpected_dimensions"
    on_device = torch.from_numpy(indices.view(np.int64)).cuda()  # only the kernels can read these: both check before every use
    with pytest.raises(szs.StringZillasError) as refused:
        engine.fuzzy_find(queries, candidates, on_device, device=gpu, starts=True)
    assert refused.value.status_name == "unexpected_dimensions"
    indices[1, 1] = 3
    again = engine.fuzzy_find(queries, candidates, torch.from_numpy(indices.view(np.int64)).cuda(), device=gpu, starts=True)  # the engine goes on
    assert same(again, good)

    with pytest.raises(szs.StringZillasError) as refused:  # one query beyond the bit-vector: fuzzy_find's status and message
        engine.fuzzy_find([b"AC", b"A" * 257, b"ACGT"], candidates, indices, device=gpu, starts=True)
    assert refused.value.status_name == "unexpected_dimensions" and "256" in str(refused.value)

    table = matrices.blosum62()
    for other in (szs.LevenshteinDistances(0, 2, 3, 1, capabilities=gpu), szs.LevenshteinDistancesUTF8(capabilities=gpu),
                  szs.NeedlemanWunschScores(*table, open=-4, extend=-4, capabilities=gpu)):
        out = tuple(np.full((3, 2), UNTOUCHED, np.uint64) for _ in range(3))
        with pytest.raises(szs.StringZillasError) as refused:
            other.fuzzy_find(queries, candidates, indices, device=gpu, out=out, starts=True)
        assert refused.value.status_name == "unknown"
        assert all((array == UNTOUCHED).all() for array in out)

    # the existing call on the same engine, after all of that: one launch, the same distances and ends
    plain = engine.fuzzy_find(queries, candidates, indices, device=gpu)
    profile = engine.last_call_profile()
    assert len(plain) == 2 and np.array_equal(plain[0], good[0]) and np.array_equal(plain[1], good[2])
    assert profile.launches == 1 and profile.pairs == indices.size
    assert profile.cells == sum(len(queries[q]) * len(candidates[int(i)]) for q in range(3) for i in indices[q])

"""Alignments on the GPU (`szs_rocm_alignments*`, `_Engine.align`): every distance, length and op bit for bit
against the canonical script of the plain suffix DP (tests/alignment_cases.py, vectorised over the spans of a query), the zero tail of
every slot included."""
import ctypes
import random

import numpy as np
import pytest

import alignment_cases as cases
import stringzilla_amd as szs
from stringzilla_amd import _abi, matrices

pytestmark = pytest.mark.gpu

EMPTY = np.uint64(2**64 - 1)
UNTOUCHED = 0x5A5A5A5A5A5A5A5A
CAPACITY = 256 + 512  # what `capacity=None` comes to with these strings: every script fits


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return szs.DeviceScope(gpu_device=0)


@pytest.fixture(scope="module")
def engine(gpu):
    return szs.LevenshteinDistances(capabilities=gpu)


def scripts_of(queries, spans_per_query, capacity):
    """(distances, lengths, ops) as the call returns them for row q against `spans_per_query[q]`: a script of more than `capacity`
    ops keeps its length and leaves zeros."""
    rows, k = len(queries), len(spans_per_query[0])
    distances, lengths = np.zeros((rows, k), np.uint64), np.zeros((rows, k), np.uint64)
    ops = np.zeros((rows, k, capacity), np.uint8)
    for q, (query, spans) in enumerate(zip(queries, spans_per_query)):
        distances[q], lengths[q], scripts = cases.canonical_scripts(query, spans)
        width = min(capacity, scripts.shape[1])
        fits = lengths[q] <= capacity
        ops[q, fits, :width] = scripts[fits, :width]
    return distances, lengths, ops


def listed(want, indices):
    """The slots the indices list; (0, 0, zeros) for an empty one."""
    indices = np.asarray(indices, dtype=np.uint64)
    safe = np.where(indices == EMPTY, 0, indices).astype(np.int64)
    rows = np.arange(indices.shape[0])[:, None]
    empty = indices == EMPTY
    return (np.where(empty, np.uint64(0), want[0][rows, safe]), np.where(empty, np.uint64(0), want[1][rows, safe]),
            np.where(empty[:, :, None], np.uint8(0), want[2][rows, safe]))


def clipped(want, capacity):
    """The same slots at a smaller capacity: what fits is cut to it (its tail was zero), what does not is all zero."""
    fits = want[1] <= capacity
    return want[0], want[1], np.where(fits[:, :, None], want[2][:, :, :capacity], np.uint8(0))


def same(got, want):
    for part, name in enumerate(("distances", "lengths", "ops")):
        assert got[part].shape == want[part].shape, (name, got[part].shape, want[part].shape)
        assert np.array_equal(got[part], want[part]), (name, np.argwhere(got[part] != want[part])[:8])
    return True


def frozen(triple):
    for array in triple:
        array.setflags(write=False)
    return triple


def _widths(alphabet, seed, longest_candidate):
    """Two queries of every length, interleaved so that rows of different `pad` share a wavefront (0 next to 256, 1 next to 255 ...),
    and 40 candidates of 0 ... 9 bytes, of the last two lengths the call takes and of U[0, longest]."""
    rng = random.Random(seed)
    ascending = [bytes(rng.choice(alphabet) for _ in range(length)) for length in cases.QUERY_LENGTHS for _ in range(2)]
    queries = []
    while ascending:
        queries.append(ascending.pop(0))
        if ascending:
            queries.append(ascending.pop())
    lengths = [1, 3, 0, 4, 5, 7, 8, 9, 511, 512] + [rng.randint(0, longest_candidate) for _ in range(30)]
    candidates = [bytes(rng.choice(alphabet) for _ in range(length)) for length in lengths]
    candidates[11] = (candidates[10][:50] + queries[1] + candidates[10][50:])[:longest_candidate]  # a longest query, whole, inside one text
    candidates[12] = queries[1][:100] + queries[1][101:180] + b"b" + queries[1][180:]              # ... and one edit script away from one
    return queries, candidates


@pytest.fixture(scope="module")
def widths_ab():
    queries, candidates = _widths(b"ab", 41, 512)
    return queries, candidates, frozen(scripts_of(queries, [candidates] * len(queries), CAPACITY))


def _cells(queries, spans_per_query, filled):
    return sum(len(queries[q]) * len(spans_per_query[q][r]) for q, r in zip(*np.nonzero(filled)))


def test_every_width_dense(gpu, engine, widths_ab):
    queries, candidates, want = widths_ab
    got = engine.align(queries, candidates, device=gpu)  # dense, no spans, the capacity every script fits
    profile = engine.last_call_profile()
    assert got[0].dtype == got[1].dtype == np.uint64 and got[2].dtype == np.uint8 and got[2].shape == (len(queries), len(candidates), CAPACITY)
    assert same(got, want)
    assert profile.launches == 1 and profile.pairs == len(queries) * len(candidates)
    assert profile.cells == _cells(queries, [candidates] * len(queries), np.ones(want[0].shape, bool))
    assert profile.longest_query == 256
    for q in (1, 6):  # the scripts do what they say
        for r in (11, 12, 39):
            script = got[2][q, r, :int(got[1][q, r])].tobytes()
            assert cases.apply_script(queries[q], script, candidates[r]) == candidates[r]
            assert sum(op != ord("=") for op in script) == int(got[0][q, r])
    again = engine.align(queries, candidates, device=gpu)  # the same call twice: the same bytes
    assert same(again, got)


def test_every_width_over_all_bytes(gpu, engine):
    queries, candidates = _widths(bytes(range(256)), 43, 512)
    queries, candidates = [query for at, query in enumerate(queries) if at % 4 < 2], candidates[:24]  # one query of every length
    want = scripts_of(queries, [candidates] * len(queries), CAPACITY)
    assert max(map(len, queries)) == 256 and max(map(len, candidates)) == 512
    assert same(engine.align(queries, candidates, device=gpu), want)


def test_the_pipeline_from_spans(gpu, engine):
    """fuzzy_find(starts=True), then align on its spans: the distances agree and the script is the canonical one of c[start:end]."""
    queries, candidates = _widths(b"ab", 47, 700)
    distances, starts, ends = engine.fuzzy_find(queries, candidates, device=gpu, starts=True)
    assert int((ends - starts).max()) <= 512
    indices = np.tile(np.arange(len(candidates), dtype=np.uint64), (len(queries), 1))
    got = engine.align(queries, candidates, indices, starts=starts, ends=ends, device=gpu)
    spans = [[candidates[r][int(starts[q, r]):int(ends[q, r])] for r in range(len(candidates))] for q in range(len(queries))]
    assert got[2].shape[2] == 256 + 512
    assert same(got, scripts_of(queries, spans, 256 + 512))
    assert np.array_equal(got[0], distances)
    profile = engine.last_call_profile()
    assert profile.launches == 1 and profile.pairs == indices.size and profile.cells == _cells(queries, spans, np.ones(indices.shape, bool))
    dense = engine.align(queries, candidates, starts=starts, ends=ends, device=gpu)  # the dense form takes spans too
    assert same(dense, got)


def test_the_matrices_of_the_occurrences_go_straight_in(gpu, engine):
    rng = random.Random(5)
    words = [b"alignment", b"kernel", b"trace", b"nowhere at all", b""]
    text = bytearray(rng.choice(b"abcdefgh ") for _ in range(3000))
    for at, word in ((100, b"alignment"), (700, b"alignmnt"), (1500, b"kernel"), (1510, b"kernal"), (2200, b"traace"), (2990, b"trace")):
        text[at:at + len(word)] = word
    text = bytes(text)
    limit = 6
    counts, distances, starts, ends = engine.fuzzy_scan_occurrences(words, text, 2, limit=limit, device=gpu)
    assert counts[0] >= 2 and counts[3] == 0 and (starts[3] == EMPTY).all() and (ends[3] == EMPTY).all()
    got = engine.align(words, [text], np.zeros((len(words), limit), np.uint64), starts=starts, ends=ends, capacity=32, device=gpu)
    filled = ends != EMPTY
    assert filled.any() and not filled.all()
    spans = [[text[int(starts[q, i]):int(ends[q, i])] if filled[q, i] else b"" for i in range(limit)] for q in range(len(words))]
    want = scripts_of(words, spans, 32)
    want[0][~filled], want[1][~filled] = 0, 0  # an empty slot: (0, 0, zeros), not the query against the empty string
    want[2][~filled] = 0
    assert same(got, want)
    assert np.array_equal(got[0][filled], distances[filled])
    profile = engine.last_call_profile()
    assert profile.pairs == int(filled.sum()) and profile.cells == _cells(words, spans, filled)


@pytest.mark.parametrize("k", [1, 16, 17, 64, 65, 130])
def test_lanes_chunks_and_row_stride(gpu, engine, widths_ab, k):
    queries, candidates, want = widths_ab
    rows, stride = len(queries), k + 3
    rng = np.random.default_rng(k)
    indices = rng.integers(0, len(candidates), size=(rows, k), dtype=np.uint64)
    indices[:, 0] = 11  # one candidate listed in every row
    if k > 1:
        indices[3, 1] = indices[7, k - 1] = indices[5, k // 2] = EMPTY  # empty slots at the start, the end and the middle of rows
        indices[9, :] = EMPTY                                           # a row that lists nothing
        indices[12, :] = 13                                             # one candidate k times
        indices[14, 1:] = indices[14, 0]
    wide_indices = np.full((rows, stride), UNTOUCHED, np.uint64)
    wide_indices[:, :k] = indices
    wide = [np.full((rows, stride), UNTOUCHED, np.uint64), np.full((rows, stride), UNTOUCHED, np.uint64),
            np.full((rows, stride, CAPACITY), 0x5A, np.uint8)]
    out = tuple(array[:, :k] for array in wide)
    assert engine.align(queries, candidates, wide_indices[:, :k], device=gpu, out=out) is out  # the capacity: what `ops` holds
    profile = engine.last_call_profile()
    assert same(out, listed(want, indices))
    assert (wide[0][:, k:] == UNTOUCHED).all() and (wide[1][:, k:] == UNTOUCHED).all() and (wide[2][:, k:] == 0x5A).all()
    assert profile.launches == 1 and profile.pairs == int((indices != EMPTY).sum())
    assert profile.cells == sum(len(queries[q]) * len(candidates[int(i)]) for q in range(rows) for i in indices[q] if i != EMPTY)


def test_capacities_13_and_0(gpu, engine, widths_ab):
    queries, candidates, want = widths_ab
    got = engine.align(queries, candidates, capacity=13, device=gpu)
    assert got[2].shape == (len(queries), len(candidates), 13)
    overflowing = want[1] > 13
    assert overflowing.any() and not overflowing.all()
    assert same(got, clipped(want, 13))  # an overflowing slot: all zero, the full L in `lengths`; its neighbours intact
    assert not got[2][overflowing].any() and (got[2][~overflowing & (want[1] > 0)][:, 0] != 0).all()
    distances, lengths, ops = engine.align(queries, candidates, capacity=0, device=gpu)
    assert ops is None and np.array_equal(distances, want[0]) and np.array_equal(lengths, want[1])
    out = (np.full(want[0].shape, UNTOUCHED, np.uint64), np.full(want[0].shape, UNTOUCHED, np.uint64), None)
    engine.align(queries, candidates, device=gpu, out=out)  # `ops` None in `out`: capacity 0
    assert np.array_equal(out[0], want[0]) and np.array_equal(out[1], want[1])


@pytest.fixture(scope="module")
def small():
    rng = random.Random(8)
    queries = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 90))) for _ in range(9)] + [b""]
    candidates = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 300))) for _ in range(25)]
    return queries, candidates, frozen(scripts_of(queries, [candidates] * len(queries), 96))


def test_memory_kinds(gpu, engine, small):
    import torch

    queries, candidates, want = small
    rows, k, capacity = len(queries), 5, 96
    indices = np.random.default_rng(5).integers(0, len(candidates), size=(rows, k), dtype=np.uint64)
    indices[2, 1] = EMPTY
    expected = listed(want, indices)
    starts = np.zeros((rows, k), np.uint64)
    ends = np.array([[len(candidates[int(i)]) if i != EMPTY else 0 for i in row] for row in indices], dtype=np.uint64)  # whole candidates, as spans
    to_device = lambda array: torch.from_numpy(array.view(np.int64) if array.dtype == np.uint64 else array).cuda()
    as_numpy = lambda array: array if isinstance(array, np.ndarray) else array.cpu().numpy().view(np.uint64 if array.dtype == torch.int64 else np.uint8)

    def fresh():
        return [np.full((rows, k), UNTOUCHED, np.uint64), np.full((rows, k), UNTOUCHED, np.uint64), np.full((rows, k, capacity), 0x5A, np.uint8)]

    # outputs in NumPy host memory (staged) and in torch device tensors (written in place); indices and spans on either side
    for outputs_on_device in (False, True):
        for inputs_on_device in (False, True):
            out = tuple(to_device(array) if outputs_on_device else array for array in fresh())
            given = [to_device(array) if inputs_on_device else array for array in (indices, starts, ends)]
            assert engine.align(queries, candidates, given[0], starts=given[1], ends=given[2], device=gpu, out=out) is out
            assert same([as_numpy(array) for array in out], expected), (outputs_on_device, inputs_on_device)
    # one output on the device, the others on the host - and the other way round: one staged output stages all three
    for on_device in ((2,), (0, 1)):
        out = tuple(to_device(array) if part in on_device else array for part, array in enumerate(fresh()))
        engine.align(queries, candidates, to_device(indices), starts=starts, ends=to_device(ends), device=gpu, out=out)
        assert same([as_numpy(array) for array in out], expected), on_device


def test_entry_points_and_the_self_form(gpu, engine, small):
    import torch

    queries, candidates, want = small
    rows, count, capacity = len(queries), len(candidates), 96
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

    def c_call(name, q, c, indices, k, out):
        error = ctypes.c_char_p()
        status = getattr(_abi.lib, name)(engine.handle, gpu.handle, ctypes.byref(q), ctypes.byref(c), None if indices is None else indices.ctypes.data,
                                         k, None, None, out[0].ctypes.data, out[1].ctypes.data, None if out[2] is None else out[2].ctypes.data,
                                         capacity, k, ctypes.byref(error))
        return status, error.value

    picks = np.random.default_rng(3).integers(0, count, size=(rows, 5), dtype=np.uint64)
    for name, q, c in (("szs_rocm_alignments_u32tape", q32, c32), ("szs_rocm_alignments_u64tape", q64, c64),
                       ("szs_rocm_alignments", sequence_of(queries), sequence_of(candidates))):
        out = [np.full((rows, count), UNTOUCHED, np.uint64), np.full((rows, count), UNTOUCHED, np.uint64), np.full((rows, count, capacity), 0x5A, np.uint8)]
        status, message = c_call(name, q, c, None, count, out)  # dense
        assert status == 0, message
        assert same(out, want), name
        few = [np.full((rows, 5), UNTOUCHED, np.uint64), np.full((rows, 5), UNTOUCHED, np.uint64), np.full((rows, 5, capacity), 0x5A, np.uint8)]
        status, message = c_call(name, q, c, picks, 5, few)
        assert status == 0, message
        assert same(few, listed(want, picks)), name
        status, message = c_call(name, q, c, picks, 5, [few[0], few[1], None])  # on a live engine too: a capacity needs `ops`
        assert _abi.STATUS_NAMES[status] == "unknown" and message, name

    # the self form: the indices refer to the queries, the own index included - a query against itself is all '='
    own = np.random.default_rng(6).integers(0, rows, size=(rows, 3), dtype=np.uint64)
    own[:, 0] = np.arange(rows)
    got = engine.align(queries, None, own, device=gpu)
    assert same(got, listed(scripts_of(queries, [queries] * rows, got[2].shape[2]), own))
    assert (got[0][:, 0] == 0).all() and all(got[2][q, 0, :len(query)].tobytes() == b"=" * len(query) for q, query in enumerate(queries))


def test_the_trace_budget_changes_no_byte(gpu, engine):
    """64 rows of queries of at most 32 bytes - one word, regions of 256 KiB: at 512 KiB two workgroups serve the runs of rows between
    them, at 1 KiB - the floor - one serves them all; k = 70 makes every row two chunks of its workgroup's region."""
    rng = random.Random(12)
    queries = [bytes(rng.choice(b"abc") for _ in range(rng.randint(0, 32))) for _ in range(64)]
    candidates = [bytes(rng.choice(b"abc") for _ in range(rng.randint(0, 80))) for _ in range(30)]
    want = scripts_of(queries, [candidates] * len(queries), max(map(len, queries)) + max(map(len, candidates)))
    indices = np.random.default_rng(2).integers(0, len(candidates), size=(64, 70), dtype=np.uint64)
    assert same(engine.align(queries, candidates, device=gpu), want)
    listed_default = engine.align(queries, candidates, indices, device=gpu)
    assert same(listed_default, listed(want, indices))
    previous = _abi.tuning_set("align_trace_kib", 512)
    try:
        for kib in (512, 1):
            _abi.tuning_set("align_trace_kib", kib)
            assert same(engine.align(queries, candidates, device=gpu), want), kib
            assert same(engine.align(queries, candidates, indices, device=gpu), listed_default), kib
            assert engine.last_call_profile().launches == 1
    finally:
        _abi.tuning_set("align_trace_kib", previous)


def test_refusals_and_the_call_afterwards(gpu, engine):
    import torch

    queries, candidates = [b"ACGT", b"AC", b"GATTACA"], [b"ACG", b"T", b"", b"GATT", b"C" * 513, b"G" * 600]
    indices = np.array([[0, 1], [2, 3], [3, 0]], dtype=np.uint64)
    good = engine.align(queries, candidates, indices, device=gpu)
    assert good[0].tolist() == [[1, 3], [2, 3], [3, 5]] and good[1].tolist() == [[4, 4], [2, 4], [7, 7]]  # by hand
    assert [good[2][q, r, :int(good[1][q, r])].tobytes() for q in range(3) for r in range(2)] == [
        b"===I", b"III=", b"II", b"D=XD", b"====III", b"I=III=X"]  # the diagonal first, then 'I', then 'D' - wherever they keep to the DP
    assert good[2].shape == (3, 2, 7 + 512)

    def refused(status_name, needle, *args, **kwargs):
        with pytest.raises(szs.StringZillasError) as caught:
            engine.align(*args, device=gpu, **kwargs)
        assert caught.value.status_name == status_name and needle in str(caught.value), str(caught.value)

    spans = lambda pairs: tuple(np.array([[pair[part] for pair in row] for row in pairs], dtype=np.uint64) for part in range(2))
    over = np.array([[5, 1], [2, 3], [3, 0]], dtype=np.uint64)
    starts, ends = spans([[(0, 513), (0, 1)], [(0, 0), (0, 4)], [(0, 4), (0, 3)]])
    refused("unexpected_dimensions", "512", queries, candidates, over, starts=starts, ends=ends)  # a span of 513 bytes
    starts, ends = spans([[(88, 600), (0, 1)], [(0, 0), (0, 4)], [(0, 4), (0, 3)]])
    assert engine.align(queries, candidates, over, starts=starts, ends=ends, device=gpu)[1][0, 0] == 512  # ... one of 512 is taken
    over[0, 0] = 4
    refused("unexpected_dimensions", "512", queries, candidates, over)  # a 513-byte candidate without spans
    for bad in ((3, 2), (0, 4), (2**63, 2**63 + 1), (int(EMPTY), 0), (1, int(EMPTY))):  # start > end; end > n; only one of them empty
        starts, ends = spans([[(0, 3), (0, 1)], [(0, 0), (0, 4)], [(0, 4), bad]])
        refused("unexpected_dimensions", "", queries, candidates, indices, starts=starts, ends=ends)
        refused("unexpected_dimensions", "", queries, candidates, indices, starts=torch.from_numpy(starts.view(np.int64)).cuda(),
                ends=torch.from_numpy(ends.view(np.int64)).cuda())
    refused("unexpected_dimensions", "256", [b"AC", b"A" * 257, b"ACGT"], candidates, indices)  # a 257-byte query, before anything is launched
    indices[1, 1] = len(candidates)  # one past the end: on the host, and where only the kernel can read it
    refused("unexpected_dimensions", "index", queries, candidates, indices)
    refused("unexpected_dimensions", "index", queries, candidates, torch.from_numpy(indices.view(np.int64)).cuda())
    indices[1, 1] = 3

    table = matrices.blosum62()
    for other in (szs.LevenshteinDistances(0, 2, 3, 1, capabilities=gpu), szs.LevenshteinDistancesUTF8(capabilities=gpu),
                  szs.NeedlemanWunschScores(*table, open=-4, extend=-4, capabilities=gpu)):
        out = (np.full((3, 2), UNTOUCHED, np.uint64), np.full((3, 2), UNTOUCHED, np.uint64), np.full((3, 2, 8), 0x5A, np.uint8))
        with pytest.raises(szs.StringZillasError) as caught:
            other.align(queries, candidates, indices, device=gpu, out=out)
        assert caught.value.status_name == "unknown"
        assert (out[0] == UNTOUCHED).all() and (out[1] == UNTOUCHED).all() and (out[2] == 0x5A).all()

    again = engine.align(queries, candidates, torch.from_numpy(indices.view(np.int64)).cuda(), device=gpu)  # the engine goes on
    assert same(again, good)
    profile = engine.last_call_profile()
    assert profile.launches == 1 and profile.pairs == indices.size
    assert profile.cells == sum(len(queries[q]) * len(candidates[int(i)]) for q in range(3) for i in indices[q])

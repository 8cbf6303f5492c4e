"""The bounded searches (`szs_rocm_within*`, `szs_rocm_fuzzy_search_within*`, `_Engine.within`, `_Engine.fuzzy_search_within`;
DESIGN.md section 4.15): what is checked before a GPU is touched, how a call is cut, and a model of the device's two passes - runs
anywhere."""
import ctypes

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi

from host_fakes import _fake_engine, _no_gpu_engine

import within_cases as cases

WITHIN_SYMBOLS = ("szs_rocm_within", "szs_rocm_within_u32tape", "szs_rocm_within_u64tape")
FUZZY_SYMBOLS = ("szs_rocm_fuzzy_search_within", "szs_rocm_fuzzy_search_within_u32tape", "szs_rocm_fuzzy_search_within_u64tape")
UNTOUCHED = cases.UNTOUCHED
STAGE_BYTES = 128 << 20


def test_symbols_exported_and_bound():
    for name in WITHIN_SYMBOLS:
        function = getattr(_abi.lib, name)
        assert name in _abi.SIGNATURES and function.restype is ctypes.c_int and len(function.argtypes) == 11
        assert function.argtypes[4] is ctypes.c_ssize_t  # the bound is signed
    for name in FUZZY_SYMBOLS:
        function = getattr(_abi.lib, name)
        assert name in _abi.SIGNATURES and function.restype is ctypes.c_int and len(function.argtypes) == 13
    assert "szs_rocm_within_probe" in _abi.SIGNATURES and len(_abi.lib.szs_rocm_within_probe.argtypes) == 7
    for method in ("within", "fuzzy_search_within"):
        assert hasattr(szs.LevenshteinDistances, method) and hasattr(szs.SmithWatermanScores, method)


# ---- the refusals, in order, on memory that passes for an engine -------------------------------------------------------------------


def _call(name, engine, limit, row_stride, arrays, count=2, queries=True):
    """One C call over two strings; `arrays`: counts and the matrices in the C order, None for NULL."""
    data = np.frombuffer(b"abcabd", dtype=np.uint8).copy()
    offsets = np.array([0, 3, 6], dtype=np.uint64 if name.endswith("u64tape") else np.uint32)
    tape = (_abi.U64Tape if name.endswith("u64tape") else _abi.U32Tape)(data.ctypes.data, offsets.ctypes.data, count)
    if not name.endswith("tape"):  # the sz_sequence_t form: `count` strings behind callbacks
        get_start = _abi.MEMBER_START(lambda handle, i: data.ctypes.data + int(offsets[i]))
        get_length = _abi.MEMBER_LENGTH(lambda handle, i: int(offsets[i + 1] - offsets[i]))
        tape = _abi.Sequence(None, count, get_start, get_length)
    side = ctypes.byref(tape) if queries else None
    error = ctypes.c_char_p()
    pointers = [None if array is None else array.ctypes.data for array in arrays]
    status = getattr(_abi.lib, name)(engine, None, side, side, 2, limit, *pointers, row_stride, ctypes.byref(error))
    return _abi.STATUS_NAMES[status], error.value


def _arrays(name, columns=3):
    """counts and the matrices of `name`, every cell UNTOUCHED."""
    return [np.full(2, UNTOUCHED, np.uint64)] + [np.full((2, columns), UNTOUCHED, np.uint64) for _ in range(2 if name in WITHIN_SYMBOLS else 4)]


def _intact(arrays):
    return all(array is None or (array == UNTOUCHED).all() for array in arrays)


@pytest.mark.parametrize("name", WITHIN_SYMBOLS + FUZZY_SYMBOLS)
def test_refusals_come_in_order_and_write_nothing(name):
    good, blank = _fake_engine(), ctypes.create_string_buffer(4096)
    arrays = _arrays(name)
    # 1. the dimensions - before the engine is looked at, before the queries are
    for engine in (None, ctypes.addressof(blank), ctypes.addressof(good)):
        for limit, row_stride in ((65537, 65537), (3, 2), (1, 0)):
            for queries in (True, False):
                status, message = _call(name, engine, limit, row_stride, arrays, queries=queries)
                assert status == "unexpected_dimensions" and message and _intact(arrays), (limit, row_stride)
    # 2. the engine - before the queries, also with nothing to do
    for engine in (None, ctypes.addressof(blank)):
        for count, queries in ((2, True), (0, True), (2, False)):
            status, message = _call(name, engine, 2, 3, arrays, count=count, queries=queries)
            assert status == "unknown" and message and _intact(arrays)
    # 3. NULL queries; zero queries succeed with nothing looked at
    status, message = _call(name, ctypes.addressof(good), 2, 3, arrays, queries=False)
    assert status == "unknown" and b"ueries" in message and _intact(arrays)
    assert _call(name, ctypes.addressof(good), 2, 3, arrays, count=0)[0] == "success" and _intact(arrays)
    assert _call(name, ctypes.addressof(good), 2, 3, [None] * len(arrays), count=0)[0] == "success"
    # 4. NULL counts, then - with a limit - NULL indices
    status, message = _call(name, ctypes.addressof(good), 2, 3, [None] + arrays[1:])
    assert status == "unknown" and b"ounts" in message and _intact(arrays)
    status, message = _call(name, ctypes.addressof(good), 0, 0, [None] * len(arrays))  # limit 0 still needs the counts
    assert status == "unknown" and b"ounts" in message
    status, message = _call(name, ctypes.addressof(good), 2, 3, [arrays[0], None] + arrays[2:])
    assert status == "unknown" and b"ndices" in message and _intact(arrays)


def test_engines_each_call_takes():
    arrays = _arrays("szs_rocm_within")
    for family in (0, 1, 2, 3):  # within: every similarity engine, at any costs - the next refusal is the NULL counts
        for unit_cost in (0, 1):
            engine = _fake_engine(family, unit_cost)
            status, message = _call("szs_rocm_within_u32tape", ctypes.addressof(engine), 2, 3, [None] + arrays[1:])
            assert status == "unknown" and b"ounts" in message
    arrays = _arrays("szs_rocm_fuzzy_search_within")
    for family, unit_cost in ((0, 0), (1, 1), (2, 1), (3, 1)):  # the fuzzy family: unit-cost byte Levenshtein only
        engine = _fake_engine(family, unit_cost)
        status, message = _call("szs_rocm_fuzzy_search_within_u32tape", ctypes.addressof(engine), 2, 3, arrays)
        assert status == "unknown" and b"unit-cost" in message and _intact(arrays)


def test_fuzzy_outputs_that_need_another():
    engine = _fake_engine()
    counts, indices, distances, starts, ends = arrays = _arrays("szs_rocm_fuzzy_search_within")
    status, message = _call("szs_rocm_fuzzy_search_within_u32tape", ctypes.addressof(engine), 2, 3, [counts, indices, None, None, ends])
    assert status == "unknown" and b"distances" in message
    status, message = _call("szs_rocm_fuzzy_search_within_u32tape", ctypes.addressof(engine), 2, 3, [counts, indices, distances, starts, None])
    assert status == "unknown" and b"ends" in message
    assert _intact(arrays)


@pytest.mark.parametrize("arguments", [
    dict(), dict(bound=1.5), dict(bound=True), dict(bound=2**63), dict(bound=1, limit=-1), dict(bound=1, limit=65537), dict(bound=1, limit=2.0),
    dict(bound=1, limit=3, out=(np.zeros(2, np.uint64), np.zeros((2, 3), np.uint64))),                                # not a triple
    dict(bound=1, limit=3, out=(np.zeros(3, np.uint64), np.zeros((2, 3), np.uint64), None)),                          # a count too many
    dict(bound=1, limit=3, out=(np.zeros(2, np.uint32), np.zeros((2, 3), np.uint64), None)),                          # 4-byte counts
    dict(bound=1, limit=3, out=(np.zeros(4, np.uint64)[::2], np.zeros((2, 3), np.uint64), None)),                     # strided counts
    dict(bound=1, limit=3, out=(np.zeros(2, np.uint64), None, None)),                                                 # a limit needs indices
    dict(bound=1, limit=3, out=(np.zeros(2, np.uint64), np.zeros((2, 4), np.uint64), None)),                          # another shape
    dict(bound=1, limit=3, out=(np.zeros(2, np.uint64), np.zeros((2, 3), np.uint64), np.zeros((2, 5), np.uint64)[:, :3])),  # two strides
    dict(bound=1, limit=0, out=(np.zeros(2, np.uint64), np.zeros((2, 3), np.uint64), None)),                          # limit 0: (rows, 0) or None
])
def test_python_within_rejects_bad_arguments_before_the_library(arguments):
    with pytest.raises(ValueError):
        _no_gpu_engine().within(["abc", "abd"], ["abx", "b"], **arguments)


@pytest.mark.parametrize("arguments", [
    dict(), dict(max_distance=-1), dict(max_distance=2**64), dict(max_distance=1.0), dict(max_distance=1, limit=65537),
    dict(max_distance=1, limit=3, out=tuple([np.zeros(2, np.uint64)] + [np.zeros((2, 3), np.uint64)] * 4)),            # five without starts
    dict(max_distance=1, limit=3, starts=True, out=tuple([np.zeros(2, np.uint64)] + [np.zeros((2, 3), np.uint64)] * 3)),
    dict(max_distance=1, limit=3, out=(np.zeros(2, np.uint64), np.zeros((2, 3), np.uint64), None, np.zeros((2, 3), np.uint64))),
])
def test_python_fuzzy_search_within_rejects_bad_arguments_before_the_library(arguments):
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_search_within(["abc", "abd"], ["abx", "b"], **arguments)


# ---- the probe ------------------------------------------------------------------------------------------------------------------------


@pytest.fixture
def tile_knob():
    previous = _abi._knob_values["top_k_tile"]
    yield lambda value: _abi.tuning_set("top_k_tile", value)
    _abi.tuning_set("top_k_tile", previous)


def test_probe_block_falls_as_the_limit_grows():
    blocks = []
    for limit in (0, 1, 64, 1024, 4096, 16384, 65536):
        block, tile, segments, segment_columns = _abi.within_probe(10**6, 10**6, limit)
        assert block >= 1 and 2 * block * limit * 8 <= STAGE_BYTES  # the dense copy of a block's rows stays within the budget
        assert block * tile <= 16 << 20 and tile >= 4096  # ... and the scored tile within the scratch, still 4096 columns wide
        assert segments >= 1 and segments * segment_columns >= tile and segment_columns % 1024 == 0
        blocks.append(block)
    assert blocks == sorted(blocks, reverse=True) and blocks[-1] == STAGE_BYTES // (2 * 65536 * 8) == 128 and blocks[-1] < blocks[0]
    assert _abi.within_probe(5, 10, 65536)[0] == 5 and _abi.within_probe(0, 0, 0)[:2] == (1, 1)


def test_probe_tile_follows_the_knob(tile_knob):
    assert _abi.within_probe(37, 300, 64)[:2] == (37, 300)
    for tile in (1, 7, 64, 65):
        tile_knob(tile)
        block, planned, segments, segment_columns = _abi.within_probe(37, 300, 64)
        assert (block, planned, segments) == (37, tile, 1) and segment_columns >= tile
    tile_knob(1000)
    assert _abi.within_probe(37, 300, 64)[1] == 300  # never beyond the candidates


def test_probe_few_rows_over_a_wide_tile_take_segments():
    block, tile, segments, segment_columns = _abi.within_probe(3, 9000, 64)
    assert (block, tile) == (3, 9000) and segments > 1 and segments * segment_columns >= tile > (segments - 1) * segment_columns
    block, tile, segments, segment_columns = _abi.within_probe(4096, 9000, 64)
    assert segments == 1  # enough rows: a workgroup a row fills the device


def test_probe_refuses_a_limit_beyond_the_cap():
    assert _abi.within_probe(3, 9000, 65536)
    with pytest.raises(szs.StringZillasError) as refused:
        _abi.within_probe(3, 9000, 65537)
    assert refused.value.status_name == "unexpected_dimensions"


# ---- a model of the two passes (csrc/hip/within.hip) ----------------------------------------------------------------------------------


def model_within(matrix, bound, descending, limit, tile, segment_columns, self_search=False, row_stride=None):
    """The device's fold in plain Python: per tile a COUNT pass - one partial a (row, segment) - and a STORE pass - the base of a segment is
    the row's running count plus the partials before it; a segment whose base has reached the limit stores nothing; else hit number
    `rank` of the segment goes to slot base + rank where that is below the limit; the running count then gains the row's partials -
    and after the last tile the FINISH: the counts, and the empty pair behind the hits.  Cells the fold does not write keep UNTOUCHED."""
    rows, columns = matrix.shape
    row_stride = limit if row_stride is None else row_stride
    indices, scores = np.full((rows, row_stride), UNTOUCHED, np.uint64), np.full((rows, row_stride), UNTOUCHED, np.uint64)
    running = [0] * rows
    hits = cases.hits_of(matrix, bound, descending, self_search)
    for c0 in range(0, columns, tile):
        width = min(tile, columns - c0)
        segments = -(-tile // segment_columns)  # the geometry of a full tile, also over a narrower last one
        partials = [[int(hits[r, c0 + s * segment_columns:c0 + min((s + 1) * segment_columns, width)].sum()) for s in range(segments)]
                    for r in range(rows)]
        if limit:
            for r in range(rows):
                for s in range(segments):
                    base = running[r] + sum(partials[r][:s])
                    if base >= limit:
                        continue
                    rank = 0
                    for c in range(s * segment_columns, min((s + 1) * segment_columns, width)):
                        if hits[r, c0 + c]:
                            if base + rank < limit:
                                indices[r, base + rank], scores[r, base + rank] = c0 + c, matrix[r, c0 + c]
                            rank += 1
                    assert rank == partials[r][s]
        running = [running[r] + sum(partials[r]) for r in range(rows)]
    for r in range(rows):
        indices[r, min(running[r], limit):limit], scores[r, min(running[r], limit):limit] = cases.EMPTY, 0
    return np.array(running, np.uint64), indices, scores


@pytest.mark.parametrize("segment_columns", [1, 64, 65])
def test_model_of_the_two_passes(segment_columns):
    rng = np.random.default_rng(segment_columns)
    columns = 4 * segment_columns + 3
    matrix = rng.integers(0, 4, size=(3, columns)).astype(np.uint64)
    matrix[0] = 0  # a row whose every column hits: hit number i is column i, so the limit sits ON the segment edges below
    matrix[2, :] = 9  # ... and one without a hit
    edges = sorted({max(edge + delta, 0) for edge in range(0, columns + segment_columns, segment_columns) for delta in (-1, 0, 1)})
    for tile in (columns, 2 * segment_columns, 2 * segment_columns + 1):
        for limit in edges + [columns + 5]:
            got = model_within(matrix, 1, False, limit, tile, segment_columns, row_stride=limit + 2)
            want = cases.expected_within(matrix, 1, False, limit)
            assert np.array_equal(got[0], want[0]) and got[0][0] == columns and got[0][2] == 0
            assert np.array_equal(got[1][:, :limit], want[1]) and np.array_equal(got[2][:, :limit], want[2]), (tile, limit)
            assert (got[1][:, limit:] == UNTOUCHED).all() and (got[2][:, limit:] == UNTOUCHED).all()  # cells [limit, row_stride)


def test_model_signed_scores_and_the_self_form():
    rng = np.random.default_rng(7)
    scores = rng.integers(-9, 10, size=(6, 6)).astype(np.int64)
    for bound in (-20, -3, 0, 4, 20):
        for limit in (0, 1, 2, 6):
            got = model_within(scores.view(np.uint64), bound, True, limit, 4, 3, self_search=True)
            want = cases.expected_within(scores, bound, True, limit, self_search=True, dtype=np.int64)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2].view(np.int64), want[2])
    assert (cases.expected_within(scores, -20, True, 6, self_search=True)[0] == 5).all()  # never the own column
    assert not cases.expected_within(np.abs(scores).astype(np.uint64), -1, False, 3)[0].any()  # a negative bound on distances: no hits

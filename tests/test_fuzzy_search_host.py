"""Fuzzy search (`szs_rocm_fuzzy_search*`, `_Engine.fuzzy_search`, `szs_rocm_fuzzy_search_probe`): what is checked and planned
before a GPU is touched - runs anywhere."""
import ctypes

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi

from host_fakes import _fake_engine, _no_gpu_engine

FUZZY_SEARCH_SYMBOLS = ("szs_rocm_fuzzy_search", "szs_rocm_fuzzy_search_u32tape", "szs_rocm_fuzzy_search_u64tape")
UNTOUCHED = 0x5A5A5A5A5A5A5A5A
SCRATCH_CELLS = 16 << 20  # host/fuzzy_search.c: the cells of a scored tile


def test_fuzzy_search_symbols_exported_and_bound():
    for name in FUZZY_SEARCH_SYMBOLS:
        assert name in _abi.SIGNATURES
        function = getattr(_abi.lib, name)
        assert function.restype is ctypes.c_int and len(function.argtypes) == 11
    assert "szs_rocm_fuzzy_search_probe" in _abi.SIGNATURES
    assert ctypes.cast(_abi.lib.szs_rocm_fuzzy_search_probe, ctypes.c_void_p).value
    assert hasattr(szs.LevenshteinDistances, "fuzzy_search")


def _call(name, engine, k, row_stride, indices, distances, starts, ends, count=2):
    data = np.frombuffer(b"abcabd", dtype=np.uint8).copy()
    offsets = np.array([0, 3, 6], dtype=np.uint64 if name.endswith("u64tape") else np.uint32)
    tape = (_abi.U64Tape if name.endswith("u64tape") else _abi.U32Tape)(data.ctypes.data, offsets.ctypes.data, count)
    error = ctypes.c_char_p()
    if name == "szs_rocm_fuzzy_search":  # the sz_sequence_t form: `count` strings behind callbacks
        get_start = _abi.MEMBER_START(lambda handle, i: data.ctypes.data + int(offsets[i]))
        get_length = _abi.MEMBER_LENGTH(lambda handle, i: int(offsets[i + 1] - offsets[i]))
        tape = _abi.Sequence(None, count, get_start, get_length)
    query = ctypes.byref(tape)
    pointer = lambda array: None if array is None else array.ctypes.data
    status = getattr(_abi.lib, name)(engine, None, query, query, k, pointer(indices), pointer(distances), pointer(starts), pointer(ends),
                                     row_stride, ctypes.byref(error))
    return status, error.value


def _outputs(shape=(2, 3)):
    return [np.full(shape, UNTOUCHED, dtype=np.uint64) for _ in range(4)]  # indices, distances, starts, ends


def _untouched(arrays):
    return all((array == UNTOUCHED).all() for array in arrays)


@pytest.mark.parametrize("name", FUZZY_SEARCH_SYMBOLS)
def test_null_blank_and_other_engines_are_refused(name):
    blank = ctypes.create_string_buffer(4096)  # zeroed memory: no engine magic
    others = [_fake_engine(family=0, unit_cost=0), _fake_engine(family=1), _fake_engine(family=2), _fake_engine(family=3)]
    for engine in [None, ctypes.addressof(blank)] + [ctypes.addressof(other) for other in others]:
        out = _outputs()
        status, message = _call(name, engine, 2, 3, *out)
        assert _abi.STATUS_NAMES[status] == "unknown" and message
        assert _untouched(out)
        status, message = _call(name, engine, 2, 3, *out, count=0)  # also with nothing to do
        assert _abi.STATUS_NAMES[status] == "unknown" and message


@pytest.mark.parametrize("name", FUZZY_SEARCH_SYMBOLS)
@pytest.mark.parametrize("k, row_stride", [(0, 4), (1025, 1025), (4, 3), (2, 1)])
def test_dimensions_are_refused_first(name, k, row_stride):
    fake = _fake_engine()
    for engine in (None, ctypes.addressof(fake)):
        out = _outputs((2, max(row_stride, 1)))
        status, _ = _call(name, engine, k, row_stride, *out)
        assert _abi.STATUS_NAMES[status] == "unexpected_dimensions"
        assert _untouched(out)
    status, _ = _call(name, ctypes.addressof(fake), k, row_stride, None, None, None, None)  # before the outputs are looked at
    assert _abi.STATUS_NAMES[status] == "unexpected_dimensions"


@pytest.mark.parametrize("name", FUZZY_SEARCH_SYMBOLS)
def test_zero_queries_succeed_and_missing_outputs_are_refused(name):
    fake = _fake_engine()
    engine = ctypes.addressof(fake)
    out = _outputs()
    status, _ = _call(name, engine, 2, 3, *out, count=0)
    assert status == 0 and _untouched(out)
    status, _ = _call(name, engine, 2, 3, None, None, None, None, count=0)  # zero queries: nothing is looked at
    assert status == 0
    indices, distances, starts, ends = out
    for arrays in ((None, distances, None, ends), (indices, None, None, ends), (indices, distances, starts, None)):
        status, message = _call(name, engine, 2, 3, *arrays)
        assert _abi.STATUS_NAMES[status] == "unknown" and message, arrays
        assert _untouched(out)


@pytest.mark.parametrize("k", [0, 1025, -1, 2.0, "3", None, True])
def test_python_rejects_a_bad_k_before_the_library(k):
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_search(["abc", "abd"], ["abx", "b"], k=k)


def _tuple(matrix, count=3):
    return (matrix,) * count  # refused before anything is written: one matrix may stand for all


@pytest.mark.parametrize("out", [
    _tuple(np.zeros((2, 3), dtype=np.float32)),
    _tuple(np.zeros((2, 4), dtype=np.uint64)),                 # another shape than (rows, k)
    _tuple(np.zeros((3, 3), dtype=np.uint64)),
    _tuple(np.zeros((2, 6), dtype=np.uint64)[:, ::2]),         # rows that are not contiguous
    (np.zeros((2, 3), dtype=np.uint64), np.zeros((2, 3), dtype=np.uint64), np.zeros((2, 5), dtype=np.uint64)[:, :3]),  # two strides
    np.zeros((2, 3), dtype=np.uint64),                         # not a tuple
    _tuple(np.zeros((2, 3), dtype=np.uint64), 2),              # a pair: the ends are missing
    _tuple(np.zeros((2, 3), dtype=np.uint64), 4),              # four without `starts`
    (np.zeros((2, 3), dtype=np.uint64), None, np.zeros((2, 3), dtype=np.uint64)),
    ([[0, 1, 2], [0, 1, 2]],) * 3,                             # neither arrays nor tensors
], ids=["dtype", "shape", "rows", "column-stride", "strides-differ", "single", "pair", "four", "none", "lists"])
def test_python_rejects_a_bad_out_before_the_library(out):
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_search(["abc", "abd"], ["abx", "b"], k=3, out=out)


def test_python_checks_the_four_outputs_of_starts_and_host_torch_tensors_too():
    import torch

    with pytest.raises(ValueError):  # starts=True takes four
        _no_gpu_engine().fuzzy_search(["abc", "abd"], ["abx", "b"], k=3, out=_tuple(np.zeros((2, 3), dtype=np.uint64)), starts=True)
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_search(["abc", "abd"], ["abx"], k=3, out=_tuple(torch.zeros((2, 3), dtype=torch.int32)))
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_search(["abc", "abd"], ["abx"], k=3, out=_tuple(torch.zeros((2, 2), dtype=torch.int64), 4), starts=True)


# ---- the planner probe -------------------------------------------------------------------------------------------------------

SHAPES = [(1, 1, 1), (3, 200, 16), (256, 1024, 16), (64, 2**20, 16), (2**18 + 1, 5000, 1024)]


@pytest.fixture
def knobs():
    yield
    _abi.tuning_set("top_k_tile", None)
    _abi.tuning_set("fuzzy_search_segment", None)


def _check(queries, candidates, k):
    block, tile, segment, workgroups = _abi.fuzzy_search_probe(queries, candidates, k, longest_query=64)
    assert segment % 64 == 0 and segment >= 64
    assert 1 <= block <= queries and 1 <= tile <= candidates and block * tile <= SCRATCH_CELLS
    assert workgroups == min(block, queries) * -(-tile // segment)
    assert workgroups < 2**31  # the grid's x
    return block, tile, segment, workgroups


@pytest.mark.parametrize("queries, candidates, k", SHAPES)
def test_probe_shapes(knobs, queries, candidates, k):
    _check(queries, candidates, k)


def test_probe_spreads_few_rows_over_the_device(knobs):
    block, tile, segment, workgroups = _check(256, 1024, 16)
    assert (block, tile) == (256, 1024) and workgroups > 256  # the dense fuzzy_find call launches one workgroup a row: 256
    block, tile, segment, workgroups = _check(64, 2**20, 16)
    assert block == 64 and workgroups >= 3 * 256 * 4 * 5  # the device's waves of this kernel several times over (four, less the rounding to 64)


@pytest.mark.parametrize("queries, candidates, k", SHAPES)
def test_probe_honours_the_knobs(knobs, queries, candidates, k):
    _abi.tuning_set("top_k_tile", 100)
    block, tile, segment, _ = _check(queries, candidates, k)
    assert tile == min(100, candidates)
    _abi.tuning_set("fuzzy_search_segment", 64)
    assert _check(queries, candidates, k)[2] == 64
    _abi.tuning_set("fuzzy_search_segment", 65)  # not a multiple of 64: rounded up
    assert _check(queries, candidates, k)[2] == 128
    _abi.tuning_set("top_k_tile", None)
    _abi.tuning_set("fuzzy_search_segment", 1 << 20)
    block, tile, segment, workgroups = _check(queries, candidates, k)
    assert segment == 1 << 20 and workgroups == min(block, queries)  # one segment a row


def test_probe_refusals():
    probe = _abi.lib.szs_rocm_fuzzy_search_probe
    assert _abi.STATUS_NAMES[probe(4, 4, 0, 10, None, None, None, None)] == "unexpected_dimensions"
    assert _abi.STATUS_NAMES[probe(4, 4, 1025, 10, None, None, None, None)] == "unexpected_dimensions"
    assert _abi.STATUS_NAMES[probe(4, 4, 4, 257, None, None, None, None)] == "unexpected_dimensions"  # a query the call refuses
    assert probe(4, 4, 4, 256, None, None, None, None) == 0 and probe(0, 0, 1, 0, None, None, None, None) == 0  # no outputs, nothing to do
    assert _abi.fuzzy_search_probe(4, 0, 4)[3] == 0  # no candidates: nothing is launched

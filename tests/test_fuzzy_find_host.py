"""Fuzzy find (`szs_rocm_fuzzy_find*`, `_Engine.fuzzy_find`): what is checked before a GPU is touched - runs anywhere."""
import ctypes

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi

from host_fakes import _fake_engine, _no_gpu_engine

FUZZY_FIND_SYMBOLS = ("szs_rocm_fuzzy_find", "szs_rocm_fuzzy_find_u32tape", "szs_rocm_fuzzy_find_u64tape")
UNTOUCHED = 0x5A5A5A5A5A5A5A5A


def test_fuzzy_find_symbols_exported_and_bound():
    for name in FUZZY_FIND_SYMBOLS:
        assert name in _abi.SIGNATURES
        function = getattr(_abi.lib, name)
        assert function.restype is ctypes.c_int and len(function.argtypes) == 10
    assert hasattr(szs.LevenshteinDistances, "fuzzy_find")


def _call(name, engine, k, row_stride, indices, distances, ends, count=2):
    data = np.frombuffer(b"abcabd", dtype=np.uint8).copy()
    offsets = np.array([0, 3, 6], dtype=np.uint64 if name.endswith("u64tape") else np.uint32)
    tape = (_abi.U64Tape if name.endswith("u64tape") else _abi.U32Tape)(data.ctypes.data, offsets.ctypes.data, count)
    error = ctypes.c_char_p()
    if name == "szs_rocm_fuzzy_find":  # the sz_sequence_t form: `count` strings behind callbacks
        get_start = _abi.MEMBER_START(lambda handle, i: data.ctypes.data + int(offsets[i]))
        get_length = _abi.MEMBER_LENGTH(lambda handle, i: int(offsets[i + 1] - offsets[i]))
        tape = _abi.Sequence(None, count, get_start, get_length)
    query = ctypes.byref(tape)
    pointer = lambda array: None if array is None else array.ctypes.data
    status = getattr(_abi.lib, name)(engine, None, query, query, pointer(indices), k, pointer(distances), pointer(ends), row_stride,
                                     ctypes.byref(error))
    return status, error.value


def _outputs():
    return np.full((2, 3), UNTOUCHED, dtype=np.uint64), np.full((2, 3), UNTOUCHED, dtype=np.uint64)


@pytest.mark.parametrize("name", FUZZY_FIND_SYMBOLS)
def test_null_blank_and_other_engines_are_refused(name):
    blank = ctypes.create_string_buffer(4096)  # zeroed memory: no engine magic
    others = [_fake_engine(family=0, unit_cost=0), _fake_engine(family=1), _fake_engine(family=2), _fake_engine(family=3)]
    for engine in [None, ctypes.addressof(blank)] + [ctypes.addressof(other) for other in others]:
        indices = np.zeros((2, 3), dtype=np.uint64)
        distances, ends = _outputs()
        status, message = _call(name, engine, 2, 3, indices, distances, ends)
        assert _abi.STATUS_NAMES[status] == "unknown" and message
        assert (distances == UNTOUCHED).all() and (ends == UNTOUCHED).all()
        status, message = _call(name, engine, 2, 3, indices, distances, ends, count=0)  # also with nothing to do
        assert _abi.STATUS_NAMES[status] == "unknown" and message


@pytest.mark.parametrize("name", FUZZY_FIND_SYMBOLS)
@pytest.mark.parametrize("k, row_stride", [(0, 4), (4, 3), (2, 1)])
def test_dimensions_are_refused(name, k, row_stride):
    indices = np.zeros((2, max(row_stride, 1)), dtype=np.uint64)
    distances = np.full((2, max(row_stride, 1)), UNTOUCHED, dtype=np.uint64)
    ends = distances.copy()
    for engine in (None, ctypes.addressof(_fake_engine())):
        status, _ = _call(name, engine, k, row_stride, indices, distances, ends)
        assert _abi.STATUS_NAMES[status] == "unexpected_dimensions"
        assert (distances == UNTOUCHED).all() and (ends == UNTOUCHED).all()


@pytest.mark.parametrize("name", FUZZY_FIND_SYMBOLS)
@pytest.mark.parametrize("k", [1, 3])
def test_the_dense_form_needs_k_equal_to_the_count(name, k):
    engine = _fake_engine()
    distances, ends = _outputs()
    status, message = _call(name, ctypes.addressof(engine), k, 3, None, distances, ends)  # two candidates
    assert _abi.STATUS_NAMES[status] == "unexpected_dimensions" and message
    assert (distances == UNTOUCHED).all() and (ends == UNTOUCHED).all()


@pytest.mark.parametrize("name", FUZZY_FIND_SYMBOLS)
def test_zero_queries_succeed_and_null_distances_are_refused(name):
    engine = _fake_engine()
    indices = np.zeros((2, 3), dtype=np.uint64)
    distances, ends = _outputs()
    status, _ = _call(name, ctypes.addressof(engine), 2, 3, indices, distances, ends, count=0)
    assert status == 0 and (distances == UNTOUCHED).all() and (ends == UNTOUCHED).all()
    status, _ = _call(name, ctypes.addressof(engine), 2, 3, None, None, None, count=0)  # zero queries: nothing is looked at
    assert status == 0
    status, message = _call(name, ctypes.addressof(engine), 2, 3, indices, None, ends)
    assert _abi.STATUS_NAMES[status] == "unknown" and message
    assert (ends == UNTOUCHED).all()


@pytest.mark.parametrize("indices", [
    np.zeros((2, 3), dtype=np.uint32),        # 4-byte cells
    np.zeros((2, 3, 1), dtype=np.uint64),     # not a matrix
    np.zeros(6, dtype=np.uint64),
    np.zeros((3, 3), dtype=np.uint64),        # a row too many
    np.zeros((2, 0), dtype=np.uint64),        # k = 0
    np.zeros((2, 6), dtype=np.uint64)[:, ::2],  # rows that are not contiguous
    np.zeros((3, 2), dtype=np.uint64).T,
    [[0, 1, 0], [1, 0, 1]],                   # neither an array nor a tensor
], ids=["dtype", "3d", "1d", "rows", "k0", "column-stride", "transposed", "list"])
def test_python_fuzzy_find_rejects_bad_indices_before_the_library(indices):
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_find(["abc", "abd"], ["abx", "b"], indices)


def test_python_fuzzy_find_needs_indices_for_the_self_form():
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_find(["abc", "abd"], None)


def _pair(matrix):
    return matrix, matrix.copy()


@pytest.mark.parametrize("out", [
    _pair(np.zeros((2, 3), dtype=np.float32)),
    _pair(np.zeros((2, 4), dtype=np.uint64)),                 # another shape
    _pair(np.zeros((2, 5), dtype=np.uint64)[:, :3]),          # another row stride than the indices'
    _pair(np.zeros((2, 6), dtype=np.uint64)[:, ::2]),
    (np.zeros((2, 3), dtype=np.uint64), np.zeros((2, 5), dtype=np.uint64)[:, :3]),  # two outputs, two strides
    np.zeros((2, 3), dtype=np.uint64),                        # not a pair
    (np.zeros((2, 3), dtype=np.uint64), None),
], ids=["dtype", "shape", "row-stride", "column-stride", "strides-differ", "single", "none"])
def test_python_fuzzy_find_rejects_bad_out_before_the_library(out):
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_find(["abc", "abd"], ["abx", "b"], np.zeros((2, 3), dtype=np.uint64), out=out)


def test_python_fuzzy_find_checks_the_dense_out_and_host_torch_tensors_too():
    import torch

    with pytest.raises(ValueError):  # dense: (rows, len(candidates)) = (2, 2)
        _no_gpu_engine().fuzzy_find(["abc", "abd"], ["abx", "b"], out=_pair(np.zeros((2, 3), dtype=np.uint64)))
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_find(["abc", "abd"], ["abx"], torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_find(["abc", "abd"], ["abx"], torch.zeros((2, 3), dtype=torch.int64),
                                    out=(torch.zeros((2, 2), dtype=torch.int64), torch.zeros((2, 2), dtype=torch.int64)))

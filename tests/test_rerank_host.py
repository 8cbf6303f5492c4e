"""Rerank (`szs_rocm_rerank*`, `_Engine.rerank`): what is checked before a GPU is touched - runs anywhere."""
import ctypes

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi

from host_fakes import _fake_engine, _no_gpu_engine

RERANK_SYMBOLS = ("szs_rocm_rerank", "szs_rocm_rerank_u32tape", "szs_rocm_rerank_u64tape")
UNTOUCHED = 0x5A5A5A5A5A5A5A5A


def test_rerank_symbols_exported_and_bound():
    for name in RERANK_SYMBOLS:
        assert name in _abi.SIGNATURES
        function = getattr(_abi.lib, name)
        assert function.restype is ctypes.c_int and len(function.argtypes) == 9
    assert hasattr(szs.LevenshteinDistances, "rerank") and hasattr(szs.SmithWatermanScores, "rerank")


def _call(name, engine, k, row_stride, indices, scores, count=2):
    data = np.frombuffer(b"abcabd", dtype=np.uint8).copy()
    offsets = np.array([0, 3, 6], dtype=np.uint64 if name.endswith("u64tape") else np.uint32)
    tape = (_abi.U64Tape if name.endswith("u64tape") else _abi.U32Tape)(data.ctypes.data, offsets.ctypes.data, count)
    error = ctypes.c_char_p()
    if name == "szs_rocm_rerank":  # the sz_sequence_t form: `count` strings behind callbacks
        get_start = _abi.MEMBER_START(lambda handle, i: data.ctypes.data + int(offsets[i]))
        get_length = _abi.MEMBER_LENGTH(lambda handle, i: int(offsets[i + 1] - offsets[i]))
        tape = _abi.Sequence(None, count, get_start, get_length)
    query = ctypes.byref(tape)
    status = getattr(_abi.lib, name)(engine, None, query, query, None if indices is None else indices.ctypes.data, k,
                                     None if scores is None else scores.ctypes.data, row_stride, ctypes.byref(error))
    return status, error.value


@pytest.mark.parametrize("name", RERANK_SYMBOLS)
def test_null_and_uninitialised_engines_are_refused(name):
    blank = ctypes.create_string_buffer(4096)  # zeroed memory: no engine magic
    for engine in (None, ctypes.addressof(blank)):
        indices = np.zeros((2, 3), dtype=np.uint64)
        scores = np.full((2, 3), UNTOUCHED, dtype=np.uint64)
        status, message = _call(name, engine, 2, 3, indices, scores)
        assert _abi.STATUS_NAMES[status] == "unknown" and message
        assert (scores == UNTOUCHED).all()


@pytest.mark.parametrize("name", RERANK_SYMBOLS)
@pytest.mark.parametrize("k, row_stride", [(0, 4), (4, 3), (2, 1)])
def test_dimensions_are_refused(name, k, row_stride):
    indices = np.zeros((2, max(row_stride, 1)), dtype=np.uint64)
    scores = np.full((2, max(row_stride, 1)), UNTOUCHED, dtype=np.uint64)
    status, _ = _call(name, None, k, row_stride, indices, scores)
    assert _abi.STATUS_NAMES[status] == "unexpected_dimensions"
    assert (scores == UNTOUCHED).all()


@pytest.mark.parametrize("name", RERANK_SYMBOLS)
def test_zero_queries_succeed_and_null_arrays_are_refused(name):
    engine = _fake_engine()
    indices = np.zeros((2, 3), dtype=np.uint64)
    scores = np.full((2, 3), UNTOUCHED, dtype=np.uint64)
    status, _ = _call(name, ctypes.addressof(engine), 2, 3, indices, scores, count=0)
    assert status == 0 and (scores == UNTOUCHED).all()
    status, _ = _call(name, ctypes.addressof(engine), 2, 3, None, None, count=0)  # zero queries: nothing is looked at
    assert status == 0
    for missing in ("indices", "scores"):
        status, message = _call(name, ctypes.addressof(engine), 2, 3, None if missing == "indices" else indices,
                                None if missing == "scores" else scores)
        assert _abi.STATUS_NAMES[status] == "unknown" and message
        assert (scores == UNTOUCHED).all()


def test_rerank_knob_is_known():
    previous = _abi.tuning_set("rerank", 0)
    try:
        assert _abi._knob_values["rerank"] == "0"
        _abi.tuning_set("SZS_ROCM_RERANK", None)
        assert _abi._knob_values["rerank"] is None
    finally:
        _abi.tuning_set("rerank", previous)


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
def test_python_rerank_rejects_bad_indices_before_the_library(indices):
    with pytest.raises(ValueError):
        _no_gpu_engine().rerank(["abc", "abd"], ["abx", "b"], indices)


@pytest.mark.parametrize("out", [
    np.zeros((2, 3), dtype=np.float32),
    np.zeros((2, 4), dtype=np.uint64),                # another shape
    np.zeros((2, 5), dtype=np.uint64)[:, :3],         # another row stride than the indices'
    np.zeros((2, 6), dtype=np.uint64)[:, ::2],
], ids=["dtype", "shape", "row-stride", "column-stride"])
def test_python_rerank_rejects_bad_out_before_the_library(out):
    with pytest.raises(ValueError):
        _no_gpu_engine().rerank(["abc", "abd"], ["abx", "b"], np.zeros((2, 3), dtype=np.uint64), out=out)


def test_python_rerank_checks_host_torch_tensors_too():
    import torch

    with pytest.raises(ValueError):
        _no_gpu_engine().rerank(["abc", "abd"], ["abx"], torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(ValueError):
        _no_gpu_engine().rerank(["abc", "abd"], ["abx"], torch.zeros((2, 3), dtype=torch.int64), out=torch.zeros((2, 2), dtype=torch.int64))

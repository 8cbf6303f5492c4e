"""Top-k search (`szs_rocm_top_k*`, `_Engine.top_k`): what is checked before a GPU is touched - runs anywhere."""
import ctypes

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi

TOP_K_SYMBOLS = ("szs_rocm_top_k", "szs_rocm_top_k_u32tape", "szs_rocm_top_k_u64tape")
UNTOUCHED = 0x5A5A5A5A5A5A5A5A


def test_top_k_symbols_exported_and_bound():
    for name in TOP_K_SYMBOLS:
        assert name in _abi.SIGNATURES
        function = getattr(_abi.lib, name)
        assert function.restype is ctypes.c_int and len(function.argtypes) == 9


def _call(name, engine, k, row_stride, indices, scores):
    data = np.frombuffer(b"abcabd", dtype=np.uint8).copy()
    offsets = np.array([0, 3, 6], dtype=np.uint64 if name.endswith("u64tape") else np.uint32)
    tape = (_abi.U64Tape if name.endswith("u64tape") else _abi.U32Tape)(data.ctypes.data, offsets.ctypes.data, 2)
    error = ctypes.c_char_p()
    if name == "szs_rocm_top_k":
        query = None  # the engine is refused before the queries are read
    else:
        query = ctypes.byref(tape)
    status = getattr(_abi.lib, name)(engine, None, query, query, k, indices.ctypes.data,
                                     None if scores is None else scores.ctypes.data, row_stride, ctypes.byref(error))
    return status, error.value


@pytest.mark.parametrize("name", TOP_K_SYMBOLS)
def test_null_and_uninitialised_engines_are_refused(name):
    blank = ctypes.create_string_buffer(4096)  # zeroed memory: no engine magic
    for engine in (None, ctypes.addressof(blank)):
        indices = np.full((2, 3), UNTOUCHED, dtype=np.uint64)
        scores = np.full((2, 3), UNTOUCHED, dtype=np.uint64)
        status, message = _call(name, engine, 2, 3, indices, scores)
        assert status != 0 and message
        assert (indices == UNTOUCHED).all() and (scores == UNTOUCHED).all()


@pytest.mark.parametrize("name", TOP_K_SYMBOLS)
@pytest.mark.parametrize("k, row_stride", [(0, 4), (1025, 2048), (4, 3), (2, 1)])
def test_dimensions_are_refused(name, k, row_stride):
    indices = np.full((2, max(row_stride, 1)), UNTOUCHED, dtype=np.uint64)
    status, _ = _call(name, None, k, row_stride, indices, None)
    assert _abi.STATUS_NAMES[status] == "unexpected_dimensions"
    assert (indices == UNTOUCHED).all()


@pytest.mark.parametrize("k", [0, -1, 1025, 2.0, 2.5, "3", None, True])
def test_python_top_k_rejects_bad_k_before_the_library(k):
    engine = object.__new__(szs.LevenshteinDistances)  # no handle, no GPU: `k` must be refused before either is needed
    with pytest.raises(ValueError):
        engine.top_k(["abc", "abd"], ["abx"], k=k)


def test_top_k_tile_knob_is_known():
    previous = _abi.tuning_set("top_k_tile", 3)
    try:
        assert _abi._knob_values["top_k_tile"] == "3"
    finally:
        _abi.tuning_set("top_k_tile", previous)

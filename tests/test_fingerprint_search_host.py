"""Fingerprint search (`szs_rocm_fingerprint_matches`, `szs_rocm_fingerprint_top_k`, `Fingerprints.matches` / `.top_k`): what is
checked before a GPU is touched - runs anywhere."""
import ctypes

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi

UNTOUCHED = 0x5A5A5A5A5A5A5A5A
UNTOUCHED_32 = 0x5A5A5A5A
NDIM = 64
FINGERPRINTS_MAGIC, SIMILARITY_MAGIC = 0x535A5346, 0x535A5345  # host/szs_internal.h


def _handle(magic, dimensions=0):
    """Zeroed memory that carries an engine's first two words and nothing else: the checks under test read no further, and every
    one of them fails before a device is looked for."""
    blank = ctypes.create_string_buffer(8192)
    ctypes.memmove(blank, np.array([magic, dimensions], dtype=np.uint32).ctypes.data, 8)
    return blank


def _hashes(rows=2):
    return np.arange(rows * NDIM, dtype=np.uint32).reshape(rows, NDIM)


def _matches(engine, stride=NDIM * 4, candidate_stride=NDIM * 4, counts_stride=8):
    queries, candidates = _hashes(), _hashes()
    counts = np.full((2, 2), UNTOUCHED_32, dtype=np.uint32)
    error = ctypes.c_char_p()
    status = _abi.lib.szs_rocm_fingerprint_matches(engine, None, queries.ctypes.data, stride, 2, candidates.ctypes.data, candidate_stride, 2,
                                                   counts.ctypes.data, counts_stride, ctypes.byref(error))
    return status, error.value, counts


def _top_k(engine, k=2, row_stride=3, stride=NDIM * 4, candidate_stride=NDIM * 4):
    queries, candidates = _hashes(), _hashes()
    indices = np.full((2, max(row_stride, 1)), UNTOUCHED, dtype=np.uint64)
    matches = np.full((2, max(row_stride, 1)), UNTOUCHED, dtype=np.uint64)
    error = ctypes.c_char_p()
    status = _abi.lib.szs_rocm_fingerprint_top_k(engine, None, queries.ctypes.data, stride, 2, candidates.ctypes.data, candidate_stride, 2, k,
                                                 indices.ctypes.data, matches.ctypes.data, row_stride, ctypes.byref(error))
    return status, error.value, indices, matches


def test_symbols_exported_and_bound():
    for name, arity in (("szs_rocm_fingerprint_matches", 11), ("szs_rocm_fingerprint_top_k", 13)):
        assert name in _abi.SIGNATURES
        function = getattr(_abi.lib, name)
        assert function.restype is ctypes.c_int and len(function.argtypes) == arity


@pytest.mark.parametrize("engine", ["null", "zeroed", "similarity"])
def test_other_handles_are_refused(engine):
    keep = {"null": None, "zeroed": _handle(0), "similarity": _handle(SIMILARITY_MAGIC, NDIM)}[engine]
    handle = None if keep is None else ctypes.addressof(keep)
    status, message, counts = _matches(handle)
    assert status != 0 and message
    assert (counts == UNTOUCHED_32).all()
    status, message, indices, matches = _top_k(handle)
    assert status != 0 and message
    assert (indices == UNTOUCHED).all() and (matches == UNTOUCHED).all()


@pytest.mark.parametrize("k, row_stride", [(0, 4), (1025, 2048), (4, 3), (2, 1)])
def test_k_and_row_stride_are_refused(k, row_stride):
    keep = _handle(FINGERPRINTS_MAGIC, NDIM)
    for handle in (None, ctypes.addressof(keep)):
        status, _, indices, matches = _top_k(handle, k=k, row_stride=row_stride)
        assert _abi.STATUS_NAMES[status] == "unexpected_dimensions"
        assert (indices == UNTOUCHED).all() and (matches == UNTOUCHED).all()


@pytest.mark.parametrize("strides", [(NDIM * 4 - 4, NDIM * 4), (NDIM * 4, NDIM * 4 - 4), (NDIM * 4 + 2, NDIM * 4), (NDIM * 4, NDIM * 4 + 1),
                                     (0, NDIM * 4)])
def test_hash_strides_are_refused(strides):
    keep = _handle(FINGERPRINTS_MAGIC, NDIM)
    status, _, counts = _matches(ctypes.addressof(keep), stride=strides[0], candidate_stride=strides[1])
    assert _abi.STATUS_NAMES[status] == "unexpected_dimensions"
    assert (counts == UNTOUCHED_32).all()
    status, _, indices, matches = _top_k(ctypes.addressof(keep), stride=strides[0], candidate_stride=strides[1])
    assert _abi.STATUS_NAMES[status] == "unexpected_dimensions"
    assert (indices == UNTOUCHED).all() and (matches == UNTOUCHED).all()


@pytest.mark.parametrize("counts_stride", [4, 6])
def test_counts_stride_is_refused(counts_stride):
    keep = _handle(FINGERPRINTS_MAGIC, NDIM)
    status, _, counts = _matches(ctypes.addressof(keep), counts_stride=counts_stride)
    assert _abi.STATUS_NAMES[status] == "unexpected_dimensions"
    assert (counts == UNTOUCHED_32).all()


def _python_engine():
    engine = object.__new__(szs.Fingerprints)  # no handle, no GPU: the arguments must be refused before either is needed
    engine.ndim = NDIM
    return engine


@pytest.mark.parametrize("k", [0, -1, 1025, 2.0, 2.5, "3", None, True])
def test_python_top_k_rejects_bad_k_before_the_library(k):
    with pytest.raises(ValueError):
        _python_engine().top_k(_hashes(), _hashes(), k=k)


@pytest.mark.parametrize("call", ["matches", "top_k"])
@pytest.mark.parametrize("side", ["queries", "candidates"])
@pytest.mark.parametrize("flaw", ["dtype", "signed", "second_dimension", "one_dimension", "strided_columns", "list", "torch_dtype",
                                  "torch_strided"])
def test_python_rejects_bad_hash_matrices_before_the_library(call, side, flaw):
    import torch

    bad = {
        "dtype": lambda: _hashes().astype(np.uint64),
        "signed": lambda: _hashes().astype(np.int32),
        "second_dimension": lambda: np.zeros((2, NDIM + 1), dtype=np.uint32),
        "one_dimension": lambda: np.zeros(NDIM, dtype=np.uint32),
        "strided_columns": lambda: np.zeros((2, 2 * NDIM), dtype=np.uint32)[:, ::2],
        "list": lambda: [[0] * NDIM],
        "torch_dtype": lambda: torch.zeros((2, NDIM), dtype=torch.int64),
        "torch_strided": lambda: torch.zeros((2, 2 * NDIM), dtype=torch.int32)[:, ::2],
    }[flaw]()
    arguments = (bad, _hashes()) if side == "queries" else (_hashes(), bad)
    engine = _python_engine()
    with pytest.raises(ValueError):
        engine.matches(*arguments) if call == "matches" else engine.top_k(*arguments, k=1)


def test_python_never_passes_an_empty_matrix_as_null():
    """NULL candidates mean self-search to the library, and torch gives an empty tensor the pointer 0."""
    import torch

    engine = _python_engine()
    for empty in (np.zeros((0, NDIM), dtype=np.uint32), torch.empty((0, NDIM), dtype=torch.int32)):
        pointer, stride, rows, gpu_index = engine._hashes(empty, "candidate_hashes")
        assert pointer and stride == NDIM * 4 and rows == 0 and gpu_index is None


@pytest.mark.parametrize("flaw", ["float32", "float32_torch", "uint64", "shape", "list"])
def test_python_matches_rejects_bad_out_before_the_library(flaw):
    import types

    import torch

    out = {
        "float32": lambda: np.zeros((2, 2), dtype=np.float32),
        "float32_torch": lambda: torch.zeros((2, 2), dtype=torch.float32),
        "uint64": lambda: np.zeros((2, 2), dtype=np.uint64),
        "shape": lambda: np.zeros((2, 3), dtype=np.uint32),
        "list": lambda: [[0, 0], [0, 0]],
    }[flaw]()
    scope = types.SimpleNamespace(gpu_device=0, handle=None)  # never reached
    with pytest.raises(ValueError):
        _python_engine().matches(_hashes(), _hashes(), device=scope, out=out)


def test_python_rejects_tensors_of_another_gpu():
    """A pointer into another GPU's memory means nothing on the scope's: refused before torch or the library is asked."""
    import types

    def tensor_on(index):  # what the check looks at of a device tensor
        return types.SimpleNamespace(is_cuda=True, device=types.SimpleNamespace(index=index))

    with pytest.raises(ValueError):
        szs._on_call_gpu((("query_hashes", tensor_on(0)), ("candidate_hashes", tensor_on(1))), 0)
    with pytest.raises(ValueError):
        szs._on_call_gpu((("query_hashes", tensor_on(0)), ("candidate_hashes", None)), 1)
    szs._on_call_gpu((("query_hashes", _hashes()), ("candidate_hashes", None)), 0)  # host memory on both sides: nothing to check or drain

"""Fuzzy find with spans (`szs_rocm_fuzzy_find_spans*`, `_Engine.fuzzy_find(..., starts=True)`): what is checked before a GPU is
touched - runs anywhere.  Every refusal is `szs_rocm_fuzzy_find*`'s.  What needs something that passes for an engine - another
family or other costs, the dimensions and the dense form on a unit-cost engine, each of the three outputs NULL, zero queries - is
driven from C against the real `szs_engine_s` (tests/native/fuzzy_find_spans_args_probe.c, built and run below); the calls from
Python here pass no engine or blank memory.  (A query above 256 bytes is refused once the device is bound and the lengths are read:
tests/test_gpu_fuzzy_spans.py has it.)"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi

from host_fakes import _no_gpu_engine

SPANS_SYMBOLS = ("szs_rocm_fuzzy_find_spans", "szs_rocm_fuzzy_find_spans_u32tape", "szs_rocm_fuzzy_find_spans_u64tape")
UNTOUCHED = 0x5A5A5A5A5A5A5A5A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spans_symbols_exported_and_bound():
    for name in SPANS_SYMBOLS:
        assert name in _abi.SIGNATURES
        function = getattr(_abi.lib, name)
        assert function.restype is ctypes.c_int and len(function.argtypes) == 11
    assert "starts" in szs.LevenshteinDistances.fuzzy_find.__code__.co_varnames


def _call(name, engine, k, row_stride, indices, distances, starts, ends, count=2, plain=False):
    """One call of a spans entry - or, `plain`, of its `szs_rocm_fuzzy_find*` twin, which has no `starts`."""
    data = np.frombuffer(b"abcabd", dtype=np.uint8).copy()
    offsets = np.array([0, 3, 6], dtype=np.uint64 if name.endswith("u64tape") else np.uint32)
    tape = (_abi.U64Tape if name.endswith("u64tape") else _abi.U32Tape)(data.ctypes.data, offsets.ctypes.data, count)
    error = ctypes.c_char_p()
    if name == "szs_rocm_fuzzy_find_spans":  # the sz_sequence_t form: `count` strings behind callbacks
        get_start = _abi.MEMBER_START(lambda handle, i: data.ctypes.data + int(offsets[i]))
        get_length = _abi.MEMBER_LENGTH(lambda handle, i: int(offsets[i + 1] - offsets[i]))
        tape = _abi.Sequence(None, count, get_start, get_length)
    query = ctypes.byref(tape)
    pointer = lambda array: None if array is None else array.ctypes.data
    if plain:
        status = getattr(_abi.lib, name.replace("_spans", ""))(engine, None, query, query, pointer(indices), k, pointer(distances),
                                                                pointer(ends), row_stride, ctypes.byref(error))
    else:
        status = getattr(_abi.lib, name)(engine, None, query, query, pointer(indices), k, pointer(distances), pointer(starts), pointer(ends),
                                         row_stride, ctypes.byref(error))
    return status, error.value


def _outputs(shape=(2, 3)):
    return tuple(np.full(shape, UNTOUCHED, dtype=np.uint64) for _ in range(3))


def _untouched(*arrays):
    return all((array == UNTOUCHED).all() for array in arrays)


@pytest.mark.parametrize("name", SPANS_SYMBOLS)
def test_null_and_blank_engines_are_refused(name):
    blank = ctypes.create_string_buffer(4096)  # zeroed memory: no engine magic
    for engine in (None, ctypes.addressof(blank)):
        indices = np.zeros((2, 3), dtype=np.uint64)
        distances, starts, ends = _outputs()
        for count in (2, 0):  # also with nothing to do
            status, message = _call(name, engine, 2, 3, indices, distances, starts, ends, count=count)
            assert _abi.STATUS_NAMES[status] == "unknown" and message
            assert _call(name, engine, 2, 3, indices, distances, None, ends, count=count, plain=True)[0] == status
        assert _untouched(distances, starts, ends)


@pytest.mark.parametrize("name", SPANS_SYMBOLS)
@pytest.mark.parametrize("k, row_stride", [(0, 4), (4, 3), (2, 1)])
def test_dimensions_are_refused(name, k, row_stride):
    indices = np.zeros((2, max(row_stride, 1)), dtype=np.uint64)
    distances, starts, ends = _outputs((2, max(row_stride, 1)))
    for engine in (None, ctypes.addressof(ctypes.create_string_buffer(4096))):  # the dimensions come first, whatever the engine
        status, _ = _call(name, engine, k, row_stride, indices, distances, starts, ends)
        assert _abi.STATUS_NAMES[status] == "unexpected_dimensions"
        assert _call(name, engine, k, row_stride, indices, distances, None, ends, plain=True)[0] == status
        assert _untouched(distances, starts, ends)


def _triple(matrix):
    return matrix, matrix.copy(), matrix.copy()


@pytest.mark.parametrize("out", [
    (np.zeros((2, 3), dtype=np.uint64), np.zeros((2, 3), dtype=np.uint64)),  # a pair: what the call without starts takes
    np.zeros((2, 3), dtype=np.uint64),                                       # not a tuple at all
    _triple(np.zeros((2, 3), dtype=np.float32)),
    _triple(np.zeros((2, 4), dtype=np.uint64)),                              # another shape
    _triple(np.zeros((2, 5), dtype=np.uint64)[:, :3]),                       # another row stride than the indices'
    (np.zeros((2, 3), dtype=np.uint64), np.zeros((2, 5), dtype=np.uint64)[:, :3], np.zeros((2, 3), dtype=np.uint64)),  # starts: a stride of its own
    (np.zeros((2, 3), dtype=np.uint64), None, np.zeros((2, 3), dtype=np.uint64)),
], ids=["pair", "single", "dtype", "shape", "row-stride", "strides-differ", "none"])
def test_python_rejects_bad_out_with_starts_before_the_library(out):
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_find(["abc", "abd"], ["abx", "b"], np.zeros((2, 3), dtype=np.uint64), out=out, starts=True)


def test_python_still_rejects_a_triple_without_starts():
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_find(["abc", "abd"], ["abx", "b"], np.zeros((2, 3), dtype=np.uint64), out=_triple(np.zeros((2, 3), dtype=np.uint64)))


def test_the_c_probe_of_the_argument_paths(tmp_path):
    """tests/native/fuzzy_find_spans_args_probe.c: the same refusals from a C program against the header's prototypes."""
    library = os.path.dirname(_abi.LIBRARY_PATH)
    binary = str(tmp_path / "fuzzy_find_spans_args_probe")
    subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "native", "fuzzy_find_spans_args_probe.c"), "-o", binary, "-L" + library,
                    "-lstringzillas_rocm_shared", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + library, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    ran = subprocess.run([binary], capture_output=True, text=True)
    assert ran.returncode == 0 and "fuzzy_find_spans_args_probe: ok" in ran.stdout, ran.stderr

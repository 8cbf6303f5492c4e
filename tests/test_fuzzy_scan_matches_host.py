"""Fuzzy scan matches (`szs_rocm_fuzzy_scan_matches*`, `_Engine.fuzzy_scan_matches`): what is checked before a GPU is touched - runs
anywhere.  The engine is memory that passes for one up to the point where a GPU would be needed, as in tests/test_fuzzy_scan_host.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi

from host_fakes import _fake_engine, _no_gpu_engine

NAMES = ("szs_rocm_fuzzy_scan_matches", "szs_rocm_fuzzy_scan_matches_u32tape", "szs_rocm_fuzzy_scan_matches_u64tape")
UNTOUCHED = 0x5A5A5A5A5A5A5A5A
LIMIT = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_three_symbols_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "stringzillas", "stringzillas_rocm.h")) as header:
        declared = re.findall(r"SZ_API_RUNTIME\s+[\w\s\*]+?\b(szs?_\w+)\s*\(", header.read())
    for name in NAMES:
        assert name in declared and name in _abi.SIGNATURES
        function = getattr(_abi.lib, name)  # AttributeError: not exported
        assert function.restype is ctypes.c_int and len(function.argtypes) == 11
        assert ctypes.cast(function, ctypes.c_void_p).value
    assert hasattr(szs.LevenshteinDistances, "fuzzy_scan_matches")


def test_the_library_exports_nothing_else_new():
    """The dynamic symbols that speak of matches in a scan are the three entries: no kernel stub, no helper."""
    listed = subprocess.run(["nm", "-D", "--defined-only", _abi.LIBRARY_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in listed.splitlines() if line.strip()}
    assert {name for name in exported if "matches" in name and "fuzzy" in name} == set(NAMES)
    assert "fuzzy_scan_cut" not in exported and not any(name.startswith("szs_hip_") or name.startswith("szs_engine_") for name in exported)


def _call(name, engine, text, text_length, max_distance, limit, counts, distances, ends, count=2, null_queries=False):
    data = np.frombuffer(b"abcabd", dtype=np.uint8).copy()
    offsets = np.array([0, 3, 6], dtype=np.uint64 if name.endswith("u64tape") else np.uint32)
    tape = (_abi.U64Tape if name.endswith("u64tape") else _abi.U32Tape)(data.ctypes.data, offsets.ctypes.data, count)
    error = ctypes.c_char_p()
    if not name.endswith("tape"):  # the sz_sequence_t form: `count` strings behind callbacks
        get_start = _abi.MEMBER_START(lambda handle, i: data.ctypes.data + int(offsets[i]))
        get_length = _abi.MEMBER_LENGTH(lambda handle, i: int(offsets[i + 1] - offsets[i]))
        tape = _abi.Sequence(None, count, get_start, get_length)
    pointer = lambda array: None if array is None else array.ctypes.data
    status = getattr(_abi.lib, name)(engine, None, None if null_queries else ctypes.byref(tape), text, text_length, max_distance, limit,
                                     pointer(counts), pointer(distances), pointer(ends), ctypes.byref(error))
    return _abi.STATUS_NAMES[status], error.value


def _outputs():
    return [np.full(2, UNTOUCHED, dtype=np.uint64)] + [np.full((2, LIMIT), UNTOUCHED, dtype=np.uint64) for _ in range(2)]


def _untouched(arrays):
    return all((array == UNTOUCHED).all() for array in arrays)


@pytest.mark.parametrize("name", NAMES)
def test_a_text_of_4_gib_is_refused_first(name):
    fake = _fake_engine()
    out = _outputs()
    for engine in (None, ctypes.addressof(fake)):  # before the limit and the engine are looked at, with a NULL text and no GPU
        for length in (2**32, 2**40):
            for limit in (LIMIT, 2**24 + 1):
                status, message = _call(name, engine, None, length, 1, limit, *out)
                assert status == "unexpected_dimensions" and b"4 GiB" in message
    status, _ = _call(name, ctypes.addressof(fake), None, 2**32, 1, LIMIT, None, None, None, count=0)  # before the empty batch, too
    assert status == "unexpected_dimensions" and _untouched(out)


@pytest.mark.parametrize("name", NAMES)
def test_a_limit_above_2_to_the_24_is_refused_second(name):
    fake = _fake_engine()
    text = ctypes.create_string_buffer(b"xxabcxx")
    out = _outputs()
    for engine in (None, ctypes.addressof(fake)):  # before the engine
        for limit in (2**24 + 1, 2**40, 2**64 - 1):
            status, message = _call(name, engine, ctypes.addressof(text), 7, 1, limit, *out)
            assert status == "unexpected_dimensions" and b"2^24" in message
            status, _ = _call(name, engine, ctypes.addressof(text), 7, 1, limit, None, None, None, count=0)
            assert status == "unexpected_dimensions"
    status, message = _call(name, None, ctypes.addressof(text), 7, 1, 2**24, *out)  # 2^24 itself passes: the engine is next
    assert status == "unknown" and b"engine" in message and _untouched(out)


@pytest.mark.parametrize("name", NAMES)
def test_null_blank_and_other_engines_are_refused(name):
    blank = ctypes.create_string_buffer(4096)  # zeroed memory: no engine magic
    others = [_fake_engine(family=0, unit_cost=0), _fake_engine(family=1), _fake_engine(family=2), _fake_engine(family=3)]
    text = ctypes.create_string_buffer(b"xxabcxx")
    for engine in [None, ctypes.addressof(blank)] + [ctypes.addressof(other) for other in others]:
        out = _outputs()
        for limit in (LIMIT, 0):
            status, message = _call(name, engine, ctypes.addressof(text), 7, 1, limit, *out)
            assert status == "unknown" and b"engine" in message
            status, message = _call(name, engine, ctypes.addressof(text), 7, 1, limit, *out, count=0)  # also with nothing to do
            assert status == "unknown" and b"engine" in message
            status, message = _call(name, engine, ctypes.addressof(text), 7, 1, limit, *out, null_queries=True)  # before the queries
            assert status == "unknown" and b"engine" in message
        assert _untouched(out)


@pytest.mark.parametrize("name", NAMES)
def test_the_order_behind_the_engine(name):
    fake = _fake_engine()
    engine = ctypes.addressof(fake)
    out = _outputs()
    counts, distances, ends = out
    status, message = _call(name, engine, None, 7, 1, LIMIT, None, None, None, null_queries=True)
    assert status == "unknown" and b"Queries" in message
    status, _ = _call(name, engine, None, 7, 1, LIMIT, None, None, None, count=0)  # zero queries: success, every pointer NULL
    assert status == "success"
    status, _ = _call(name, engine, None, 7, 1, LIMIT, *out, count=0)
    assert status == "success" and _untouched(out)
    for limit in (LIMIT, 0):  # the counts come before the matrices and the text
        status, message = _call(name, engine, None, 7, 1, limit, None, distances, ends)
        assert status == "unknown" and b"Counts" in message
    for arrays in ((counts, None, ends), (counts, distances, None), (counts, None, None)):  # the matrices come before the text
        status, message = _call(name, engine, None, 7, 1, LIMIT, *arrays)
        assert status == "unknown" and b"Distances and ends" in message
    status, message = _call(name, engine, None, 7, 1, LIMIT, *out)  # a NULL text of 7 bytes: refused before a GPU is needed
    assert status == "unknown" and b"Text" in message
    assert _untouched(out)


@pytest.mark.parametrize("name", NAMES)
def test_the_counting_form_takes_null_matrices_and_reaches_the_text_check(name):
    fake = _fake_engine()
    counts = np.full(2, UNTOUCHED, dtype=np.uint64)
    for max_distance in (0, 1, 2**64 - 1):  # any bound is taken
        status, message = _call(name, ctypes.addressof(fake), None, 7, max_distance, 0, counts, None, None)
        assert status == "unknown" and b"Text" in message
    assert _untouched([counts])


# ---- the Python wrapper ------------------------------------------------------------------------------------------------------

def _good():
    return np.zeros(2, dtype=np.uint64), np.zeros((2, LIMIT), dtype=np.uint64), np.zeros((2, LIMIT), dtype=np.uint64)


@pytest.mark.parametrize("out", [
    (np.zeros(2, dtype=np.float32),) + _good()[1:],                                   # counts of 4-byte cells
    (np.zeros(3, dtype=np.uint64),) + _good()[1:],                                    # another length than the queries
    (np.zeros((2, 1), dtype=np.uint64),) + _good()[1:],                               # counts that are no vector
    _good()[:1] + (np.zeros((2, LIMIT + 1), dtype=np.uint64),) + _good()[2:],         # another width than the limit
    _good()[:2] + (np.zeros((3, LIMIT), dtype=np.uint64),),                           # another height than the queries
    _good()[:2] + (np.zeros((2, 2 * LIMIT), dtype=np.uint64)[:, ::2],),               # not contiguous
    _good()[:2] + (np.zeros((2, LIMIT), dtype=np.uint32),),                           # 4-byte cells
    _good()[:2] + (np.zeros(2 * LIMIT, dtype=np.uint64),),                            # a matrix that is a vector
    _good()[0],                                                                       # not a triple
    _good()[:2],
    _good() + _good()[:1],
    _good()[:2] + (None,),
    ([0, 0], [[0] * LIMIT] * 2, [[0] * LIMIT] * 2),                                   # neither arrays nor tensors
], ids=["dtype", "length", "2d-counts", "width", "height", "stride", "cells", "1d-matrix", "single", "pair", "four", "none", "lists"])
def test_python_rejects_a_bad_out_before_the_library(out):
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_scan_matches(["abc", "abd"], b"xxabcxx", 1, limit=LIMIT, out=out)


def test_python_checks_the_shape_against_the_limit_and_torch_tensors_too():
    import torch

    with pytest.raises(ValueError):  # limit=0 takes matrices of shape (rows, 0)
        _no_gpu_engine().fuzzy_scan_matches(["abc", "abd"], b"xxabcxx", 1, limit=0, out=_good())
    with pytest.raises(ValueError):  # the default limit is 64
        _no_gpu_engine().fuzzy_scan_matches(["abc", "abd"], b"xxabcxx", 1, out=_good())
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_scan_matches(["abc", "abd"], b"xxabcxx", 1, limit=LIMIT,
                                            out=(torch.zeros(2, dtype=torch.int32),) + tuple(torch.zeros((2, LIMIT), dtype=torch.int64) for _ in range(2)))
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_scan_matches(["abc", "abd"], b"xxabcxx", 1, limit=LIMIT,
                                            out=(torch.zeros(2, dtype=torch.int64), torch.zeros((2, LIMIT), dtype=torch.int64),
                                                 torch.zeros((LIMIT, 2), dtype=torch.int64).t()))


@pytest.mark.parametrize("max_distance, limit", [(-1, LIMIT), (1, -1), (1.0, LIMIT), (1, 2.0), (None, LIMIT), (1, None), (True, LIMIT),
                                                 (1, True), (2**64, LIMIT), (1, 2**24 + 1), ("1", LIMIT)],
                         ids=["negative-distance", "negative-limit", "float-distance", "float-limit", "no-distance", "no-limit",
                              "bool-distance", "bool-limit", "distance-beyond-size_t", "limit-beyond-2^24", "str"])
def test_python_rejects_a_bad_bound_or_limit_before_the_library(max_distance, limit):
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_scan_matches(["abc", "abd"], b"xxabcxx", max_distance, limit=limit)


@pytest.mark.parametrize("text", ["xxabcxx", ["xxabcxx"], None, 7, np.zeros(7, dtype=np.int32), np.zeros((7, 1), dtype=np.uint8),
                                  np.zeros(14, dtype=np.uint8)[::2]],
                         ids=["str", "list", "none", "int", "dtype", "2d", "stride"])
def test_python_rejects_a_text_that_is_not_bytes_before_the_library(text):
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_scan_matches(["abc", "abd"], text, 1)


def test_python_rejects_a_torch_text_that_is_not_a_byte_vector():
    import torch

    for text in (torch.zeros(7, dtype=torch.int32), torch.zeros((7, 1), dtype=torch.uint8), torch.zeros(14, dtype=torch.uint8)[::2]):
        with pytest.raises(ValueError):
            _no_gpu_engine().fuzzy_scan_matches(["abc", "abd"], text, 1)


def test_the_c_probe_of_the_argument_paths(tmp_path):
    """tests/native/fuzzy_scan_matches_args_probe.c: the same refusals, in their order, from a C program against the header's prototypes."""
    library = os.path.dirname(_abi.LIBRARY_PATH)
    binary = str(tmp_path / "fuzzy_scan_matches_args_probe")
    subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "native", "fuzzy_scan_matches_args_probe.c"), "-o", binary, "-L" + library,
                    "-lstringzillas_rocm_shared", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + library, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    ran = subprocess.run([binary], capture_output=True, text=True)
    assert ran.returncode == 0 and "fuzzy_scan_matches_args_probe: ok" in ran.stdout, ran.stderr

"""Alignments (`szs_rocm_alignments*`, `_Engine.align`): what is checked before a GPU is touched - runs anywhere.  Every refusal is
`szs_rocm_fuzzy_find*`'s.  What needs something that passes for an engine - another family or other costs, the dimensions and the
dense form on a unit-cost engine, each required output NULL, one of `starts` / `ends` alone, zero queries - is driven from C against
the real `szs_engine_s` (tests/native/alignments_args_probe.c, built and run below); the calls from Python here pass no engine or
blank memory.  (A query above 256 bytes and a span above 512 are refused once the device is bound: tests/test_gpu_alignments.py.)"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi

from host_fakes import _no_gpu_engine

ALIGNMENTS_SYMBOLS = ("szs_rocm_alignments", "szs_rocm_alignments_u32tape", "szs_rocm_alignments_u64tape")
UNTOUCHED = 0x5A5A5A5A5A5A5A5A
CAPACITY = 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_alignments_symbols_exported_and_bound():
    for name in ALIGNMENTS_SYMBOLS:
        assert name in _abi.SIGNATURES
        function = getattr(_abi.lib, name)
        assert function.restype is ctypes.c_int and len(function.argtypes) == 14
    assert "capacity" in szs.LevenshteinDistances.align.__code__.co_varnames
    assert _abi._KNOBS["align_trace_kib"] == "SZS_ROCM_ALIGN_TRACE_KIB"


def test_the_knob_is_the_librarys():
    previous = _abi.tuning_set("align_trace_kib", 512)
    try:
        assert _abi.tuning_set("SZS_ROCM_ALIGN_TRACE_KIB", 0) == "512"
    finally:
        _abi.tuning_set("align_trace_kib", previous)


def _call(name, engine, k, row_stride, indices, starts, ends, distances, lengths, ops, capacity=CAPACITY, count=2):
    data = np.frombuffer(b"abcabd", dtype=np.uint8).copy()
    offsets = np.array([0, 3, 6], dtype=np.uint64 if name.endswith("u64tape") else np.uint32)
    tape = (_abi.U64Tape if name.endswith("u64tape") else _abi.U32Tape)(data.ctypes.data, offsets.ctypes.data, count)
    error = ctypes.c_char_p()
    if name == "szs_rocm_alignments":  # the sz_sequence_t form: `count` strings behind callbacks
        get_start = _abi.MEMBER_START(lambda handle, i: data.ctypes.data + int(offsets[i]))
        get_length = _abi.MEMBER_LENGTH(lambda handle, i: int(offsets[i + 1] - offsets[i]))
        tape = _abi.Sequence(None, count, get_start, get_length)
    query = ctypes.byref(tape)
    pointer = lambda array: None if array is None else array.ctypes.data
    status = getattr(_abi.lib, name)(engine, None, query, query, pointer(indices), k, pointer(starts), pointer(ends), pointer(distances),
                                     pointer(lengths), pointer(ops), capacity, row_stride, ctypes.byref(error))
    return status, error.value


def _outputs(shape=(2, 3)):
    return (np.full(shape, UNTOUCHED, dtype=np.uint64), np.full(shape, UNTOUCHED, dtype=np.uint64),
            np.full(shape + (CAPACITY,), 0x5A, dtype=np.uint8))


def _untouched(distances, lengths, ops):
    return (distances == UNTOUCHED).all() and (lengths == UNTOUCHED).all() and (ops == 0x5A).all()


@pytest.mark.parametrize("name", ALIGNMENTS_SYMBOLS)
def test_null_and_blank_engines_are_refused(name):
    blank = ctypes.create_string_buffer(4096)  # zeroed memory: no engine magic
    for engine in (None, ctypes.addressof(blank)):
        indices, spans = np.zeros((2, 3), dtype=np.uint64), np.zeros((2, 3), dtype=np.uint64)
        outputs = _outputs()
        for count in (2, 0):  # also with nothing to do
            for starts, ends in ((spans, spans), (None, None)):
                status, message = _call(name, engine, 2, 3, indices, starts, ends, *outputs, count=count)
                assert _abi.STATUS_NAMES[status] == "unknown" and message
        assert _untouched(*outputs)


@pytest.mark.parametrize("name", ALIGNMENTS_SYMBOLS)
@pytest.mark.parametrize("k, row_stride", [(0, 4), (4, 3), (2, 1)])
def test_dimensions_are_refused(name, k, row_stride):
    indices = np.zeros((2, max(row_stride, 1)), dtype=np.uint64)
    outputs = _outputs((2, max(row_stride, 1)))
    for engine in (None, ctypes.addressof(ctypes.create_string_buffer(4096))):  # the dimensions come first, whatever the engine
        status, _ = _call(name, engine, k, row_stride, indices, None, None, *outputs)
        assert _abi.STATUS_NAMES[status] == "unexpected_dimensions"
        assert _untouched(*outputs)


def _cells(shape=(2, 3), dtype=np.uint64):
    return np.zeros(shape, dtype=dtype)


def _ops(shape=(2, 3, CAPACITY), dtype=np.uint8):
    return np.zeros(shape, dtype=dtype)


@pytest.mark.parametrize("out", [
    (_cells(), _cells()),                                  # a pair: what fuzzy_find takes
    _cells(),                                              # not a tuple at all
    (_cells(dtype=np.float32), _cells(), _ops()),
    (_cells((2, 4)), _cells((2, 4)), _ops((2, 4, CAPACITY))),  # another shape than the indices'
    (_cells((2, 5))[:, :3], _cells((2, 5))[:, :3], _ops((2, 5, CAPACITY))[:, :3]),  # another row stride than the indices'
    (_cells(), _cells((2, 5))[:, :3], _ops()),             # lengths: a stride of its own
    (_cells(), None, _ops()),
    (None, _cells(), _ops()),
    (_cells(), _cells(), _ops(dtype=np.uint16)),
    (_cells(), _cells(), _ops((2, 3, CAPACITY + 1))),      # not the capacity the call names
    (_cells(), _cells(), _ops((2, 3))),
    (_cells(), _cells(), _ops((2, 3, 2 * CAPACITY))[:, :, ::2]),  # not contiguous in its last dimension
    (_cells(), _cells(), _ops((2, 4, CAPACITY))[:, :3]),   # a row stride of its own
    (_cells(), _cells(), None),                            # no ops, but a capacity
], ids=["pair", "single", "dtype", "shape", "row-stride", "strides-differ", "no-lengths", "no-distances", "ops-dtype", "ops-capacity",
        "ops-rank", "ops-strided", "ops-row-stride", "ops-none"])
def test_python_rejects_bad_out_before_the_library(out):
    with pytest.raises(ValueError):
        _no_gpu_engine().align(["abc", "abd"], ["abx", "b"], np.zeros((2, 3), dtype=np.uint64), capacity=CAPACITY, out=out)


def test_python_rejects_one_of_starts_and_ends_alone():
    spans = np.zeros((2, 3), dtype=np.uint64)
    for starts, ends in ((spans, None), (None, spans)):
        with pytest.raises(ValueError):
            _no_gpu_engine().align(["abc", "abd"], ["abx", "b"], np.zeros((2, 3), dtype=np.uint64), starts=starts, ends=ends)
    with pytest.raises(ValueError):  # ... and spans of another shape or stride than the indices'
        _no_gpu_engine().align(["abc", "abd"], ["abx", "b"], np.zeros((2, 3), dtype=np.uint64), starts=np.zeros((2, 4), dtype=np.uint64),
                               ends=np.zeros((2, 4), dtype=np.uint64))
    with pytest.raises(ValueError):
        _no_gpu_engine().align(["abc", "abd"], ["abx", "b"], np.zeros((2, 3), dtype=np.uint64), starts=np.zeros((2, 5), dtype=np.uint64)[:, :3],
                               ends=np.zeros((2, 5), dtype=np.uint64)[:, :3])


def test_python_rejects_bad_capacities_and_missing_candidates():
    for capacity in (-1, 1.5, True):
        with pytest.raises(ValueError):
            _no_gpu_engine().align(["abc"], ["abx"], capacity=capacity)
    with pytest.raises(ValueError):
        _no_gpu_engine().align(["abc"], None)  # the self form needs indices
    with pytest.raises(ValueError):
        _no_gpu_engine().align(["abc"], [])    # the dense form needs a candidate


def test_the_c_probe_of_the_argument_paths(tmp_path):
    """tests/native/alignments_args_probe.c: the same refusals from a C program against the header's prototypes."""
    library = os.path.dirname(_abi.LIBRARY_PATH)
    binary = str(tmp_path / "alignments_args_probe")
    subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "native", "alignments_args_probe.c"), "-o", binary, "-L" + library,
                    "-lstringzillas_rocm_shared", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + library, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    ran = subprocess.run([binary], capture_output=True, text=True)
    assert ran.returncode == 0 and "alignments_args_probe: ok" in ran.stdout, ran.stderr

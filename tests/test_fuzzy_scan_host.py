"""Fuzzy scan (`szs_rocm_fuzzy_scan*`, `_Engine.fuzzy_scan`, `szs_rocm_fuzzy_scan_probe`): what is checked and planned before a GPU
is touched - runs anywhere."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi

from host_fakes import _fake_engine, _no_gpu_engine

PLAIN = ("szs_rocm_fuzzy_scan", "szs_rocm_fuzzy_scan_u32tape", "szs_rocm_fuzzy_scan_u64tape")
SPANS = ("szs_rocm_fuzzy_scan_spans", "szs_rocm_fuzzy_scan_spans_u32tape", "szs_rocm_fuzzy_scan_spans_u64tape")
UNTOUCHED = 0x5A5A5A5A5A5A5A5A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_seven_symbols_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "stringzillas", "stringzillas_rocm.h")) as header:
        declared = re.findall(r"SZ_API_RUNTIME\s+[\w\s\*]+?\b(szs?_\w+)\s*\(", header.read())
    for name, arguments in [(name, 8) for name in PLAIN] + [(name, 9) for name in SPANS] + [("szs_rocm_fuzzy_scan_probe", 7)]:
        assert name in declared and name in _abi.SIGNATURES
        function = getattr(_abi.lib, name)  # AttributeError: not exported
        assert function.restype is ctypes.c_int and len(function.argtypes) == arguments
        assert ctypes.cast(function, ctypes.c_void_p).value
    assert hasattr(szs.LevenshteinDistances, "fuzzy_scan") and callable(_abi.fuzzy_scan_probe)


def _call(name, engine, text, text_length, distances, starts, ends, count=2, null_queries=False):
    data = np.frombuffer(b"abcabd", dtype=np.uint8).copy()
    offsets = np.array([0, 3, 6], dtype=np.uint64 if name.endswith("u64tape") else np.uint32)
    tape = (_abi.U64Tape if name.endswith("u64tape") else _abi.U32Tape)(data.ctypes.data, offsets.ctypes.data, count)
    error = ctypes.c_char_p()
    if not name.endswith("tape"):  # the sz_sequence_t form: `count` strings behind callbacks
        get_start = _abi.MEMBER_START(lambda handle, i: data.ctypes.data + int(offsets[i]))
        get_length = _abi.MEMBER_LENGTH(lambda handle, i: int(offsets[i + 1] - offsets[i]))
        tape = _abi.Sequence(None, count, get_start, get_length)
    pointer = lambda array: None if array is None else array.ctypes.data
    outputs = (pointer(distances), pointer(starts), pointer(ends)) if "spans" in name else (pointer(distances), pointer(ends))
    status = getattr(_abi.lib, name)(engine, None, None if null_queries else ctypes.byref(tape), text, text_length, *outputs, ctypes.byref(error))
    return status, error.value


def _outputs():
    return [np.full(2, UNTOUCHED, dtype=np.uint64) for _ in range(3)]  # distances, starts, ends


def _untouched(arrays):
    return all((array == UNTOUCHED).all() for array in arrays)


@pytest.mark.parametrize("name", PLAIN + SPANS)
def test_a_text_of_4_gib_is_refused_first(name):
    fake = _fake_engine()
    for engine in (None, ctypes.addressof(fake)):  # before the engine is looked at, with a NULL text and no GPU
        out = _outputs()
        for length in (2**32, 2**40):
            status, message = _call(name, engine, None, length, *out)
            assert _abi.STATUS_NAMES[status] == "unexpected_dimensions" and message
        assert _untouched(out)
    status, _ = _call(name, ctypes.addressof(fake), None, 2**32, None, None, None, count=0)  # before the empty batch, too
    assert _abi.STATUS_NAMES[status] == "unexpected_dimensions"


@pytest.mark.parametrize("name", PLAIN + SPANS)
def test_null_blank_and_other_engines_are_refused(name):
    blank = ctypes.create_string_buffer(4096)  # zeroed memory: no engine magic
    others = [_fake_engine(family=0, unit_cost=0), _fake_engine(family=1), _fake_engine(family=2), _fake_engine(family=3)]
    text = ctypes.create_string_buffer(b"xxabcxx")
    for engine in [None, ctypes.addressof(blank)] + [ctypes.addressof(other) for other in others]:
        out = _outputs()
        status, message = _call(name, engine, ctypes.addressof(text), 7, *out)
        assert _abi.STATUS_NAMES[status] == "unknown" and message
        assert _untouched(out)
        status, message = _call(name, engine, ctypes.addressof(text), 7, *out, count=0)  # also with nothing to do
        assert _abi.STATUS_NAMES[status] == "unknown" and message
        status, message = _call(name, engine, ctypes.addressof(text), 7, *out, null_queries=True)  # the engine comes before the queries
        assert _abi.STATUS_NAMES[status] == "unknown" and b"engine" in message


@pytest.mark.parametrize("name", PLAIN + SPANS)
def test_the_order_behind_the_engine(name):
    fake = _fake_engine()
    engine = ctypes.addressof(fake)
    out = _outputs()
    distances, starts, ends = out
    status, message = _call(name, engine, None, 7, None, None, None, null_queries=True)
    assert _abi.STATUS_NAMES[status] == "unknown" and b"Queries" in message
    status, _ = _call(name, engine, None, 7, None, None, None, count=0)  # zero queries: success, every pointer NULL, nothing looked at
    assert status == 0
    status, _ = _call(name, engine, None, 7, *out, count=0)
    assert status == 0 and _untouched(out)
    status, message = _call(name, engine, None, 7, None, starts, ends)  # the outputs come before the text
    assert _abi.STATUS_NAMES[status] == "unknown" and b"Distances" in message
    if "spans" in name:
        for arrays in ((distances, None, ends), (distances, starts, None)):
            status, message = _call(name, engine, None, 7, *arrays)
            assert _abi.STATUS_NAMES[status] == "unknown" and b"Starts and ends" in message
    status, message = _call(name, engine, None, 7, *out)  # a NULL text of 7 bytes: refused before a GPU is needed
    assert _abi.STATUS_NAMES[status] == "unknown" and b"Text" in message
    assert _untouched(out)


# ---- the probe ---------------------------------------------------------------------------------------------------------------

@pytest.fixture
def piece_knob():
    yield
    _abi.tuning_set("fuzzy_scan_piece", None)


def test_probe_shapes(piece_knob):
    assert _abi.fuzzy_scan_probe(1, 64, 1 << 20)[:3] == (4096, 256, 4)  # the least piece: 256 pieces, 4 chunks of 64
    # 256 rows: 80 chunks a row fill the device four times; P = ceil(64 MiB / (64 x 80)) = 13108, rounded up to 13120
    piece, pieces, workgroups, walked = _abi.fuzzy_scan_probe(256, 64, 64 << 20)
    chunks = -(-20480 // 256)
    wanted = -(-(64 << 20) // (64 * chunks))
    assert piece == -(-wanted // 64) * 64 == 13120 and pieces == -(-(64 << 20) // piece)
    assert workgroups == 256 * -(-pieces // 64) == 256 * chunks
    assert walked == (64 << 20) + (pieces - 1) * 128
    assert _abi.fuzzy_scan_probe(5, 256, 0) == (4096, 0, 0, 0)  # an empty text: no pieces, no workgroups
    assert _abi.fuzzy_scan_probe(0, 0, 1 << 20)[2] == 0        # no queries: nothing is launched
    # 2^20 rows and more are one block of 2^20: one chunk a row
    assert _abi.fuzzy_scan_probe(3 << 20, 16, 1 << 30)[2] == (1 << 20) * -(-_abi.fuzzy_scan_probe(3 << 20, 16, 1 << 30)[1] // 64)


def test_probe_honours_the_knob(piece_knob):
    for value, piece in ((64, 64), (65, 128), (1, 64), (8192, 8192)):
        _abi.tuning_set("fuzzy_scan_piece", value)
        got, pieces, workgroups, _ = _abi.fuzzy_scan_probe(3, 40, 5000)
        assert got == piece and pieces == -(-5000 // piece) and workgroups == 3 * -(-pieces // 64)
    _abi.tuning_set("SZS_ROCM_FUZZY_SCAN_PIECE", 64)  # the environment spelling names the same knob
    assert _abi.fuzzy_scan_probe(3, 40, 5000)[:2] == (64, 79)
    # rows x chunks stays below 2^31: the block shrinks
    piece, pieces, workgroups, _ = _abi.fuzzy_scan_probe(1 << 20, 8, (1 << 32) - 1)
    assert (piece, pieces) == (64, 1 << 26) and workgroups < 2**31 and workgroups % (1 << 20) == 0
    _abi.tuning_set("fuzzy_scan_piece", None)
    assert _abi.fuzzy_scan_probe(3, 40, 5000)[:2] == (4096, 2)


def test_probe_refusals():
    probe = _abi.lib.szs_rocm_fuzzy_scan_probe
    assert _abi.STATUS_NAMES[probe(4, 257, 100, None, None, None, None)] == "unexpected_dimensions"  # a query the call refuses
    assert _abi.STATUS_NAMES[probe(4, 10, 2**32, None, None, None, None)] == "unexpected_dimensions"
    assert probe(4, 256, 2**32 - 1, None, None, None, None) == 0 and probe(0, 0, 0, None, None, None, None) == 0  # no outputs, nothing to do


# ---- the Python wrapper ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("out", [
    (np.zeros(2, dtype=np.float32),) * 2,
    (np.zeros(3, dtype=np.uint64),) * 2,                              # another length than the queries
    (np.zeros((2, 1), dtype=np.uint64),) * 2,                         # not a vector
    (np.zeros(4, dtype=np.uint64)[::2],) * 2,                         # not contiguous
    np.zeros(2, dtype=np.uint64),                                     # not a pair
    (np.zeros(2, dtype=np.uint64),) * 3,                              # a triple without `starts`
    (np.zeros(2, dtype=np.uint64), None),
    ([0, 0], [0, 0]),                                                 # neither arrays nor tensors
], ids=["dtype", "length", "2d", "stride", "single", "triple", "none", "lists"])
def test_python_rejects_a_bad_out_before_the_library(out):
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_scan(["abc", "abd"], b"xxabcxx", out=out)


def test_python_checks_the_triple_of_starts_and_host_torch_tensors_too():
    import torch

    with pytest.raises(ValueError):  # starts=True takes three
        _no_gpu_engine().fuzzy_scan(["abc", "abd"], b"xxabcxx", out=(np.zeros(2, dtype=np.uint64),) * 2, starts=True)
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_scan(["abc", "abd"], b"xxabcxx", out=(torch.zeros(2, dtype=torch.int32),) * 2)
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_scan(["abc", "abd"], b"xxabcxx", out=(torch.zeros(3, dtype=torch.int64),) * 3, starts=True)


@pytest.mark.parametrize("text", ["xxabcxx", ["xxabcxx"], None, 7, np.zeros(7, dtype=np.int32), np.zeros((7, 1), dtype=np.uint8),
                                  np.zeros(14, dtype=np.uint8)[::2]],
                         ids=["str", "list", "none", "int", "dtype", "2d", "stride"])
def test_python_rejects_a_text_that_is_not_bytes_before_the_library(text):
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_scan(["abc", "abd"], text)


def test_python_rejects_a_torch_text_that_is_not_a_byte_vector():
    import torch

    for text in (torch.zeros(7, dtype=torch.int32), torch.zeros((7, 1), dtype=torch.uint8), torch.zeros(14, dtype=torch.uint8)[::2]):
        with pytest.raises(ValueError):
            _no_gpu_engine().fuzzy_scan(["abc", "abd"], text)


def test_the_c_probe_of_the_argument_paths(tmp_path):
    """tests/native/fuzzy_scan_args_probe.c: the same refusals, in their order, from a C program against the header's prototypes."""
    library = os.path.dirname(_abi.LIBRARY_PATH)
    binary = str(tmp_path / "fuzzy_scan_args_probe")
    subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "native", "fuzzy_scan_args_probe.c"), "-o", binary, "-L" + library,
                    "-lstringzillas_rocm_shared", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + library, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    ran = subprocess.run([binary], capture_output=True, text=True)
    assert ran.returncode == 0 and "fuzzy_scan_args_probe: ok" in ran.stdout, ran.stderr

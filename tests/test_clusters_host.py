"""`clusters` before a GPU is touched (`szs_rocm_clusters*`, `szs_rocm_fingerprint_clusters`, `szs_rocm_clusters_probe`; DESIGN.md
section 4.16): the symbols, what the probe says a call would score, and the refusals that need no device - runs anywhere."""
import ctypes

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi

from host_fakes import _EngineHead, _fake_engine, _no_gpu_engine

import clusters_cases as cases

SYMBOLS = ("szs_rocm_clusters", "szs_rocm_clusters_u32tape", "szs_rocm_clusters_u64tape")
UNTOUCHED = cases.UNTOUCHED


def test_symbols_exported_and_bound():
    for name in SYMBOLS:
        function = getattr(_abi.lib, name)
        assert name in _abi.SIGNATURES and function.restype is ctypes.c_int and len(function.argtypes) == 7
        assert function.argtypes[3] is ctypes.c_ssize_t  # the bound is signed
    assert len(_abi.lib.szs_rocm_fingerprint_clusters.argtypes) == 9 and len(_abi.lib.szs_rocm_clusters_probe.argtypes) == 6
    assert hasattr(szs.LevenshteinDistances, "clusters") and hasattr(szs.SmithWatermanScores, "clusters") and hasattr(szs.Fingerprints, "clusters")


# ---- the probe ------------------------------------------------------------------------------------------------------------------------


@pytest.fixture
def tile_knob():
    previous = _abi._knob_values["top_k_tile"]
    yield lambda value: _abi.tuning_set("top_k_tile", value)
    _abi.tuning_set("top_k_tile", previous)


def _triangle(count, block, tile):
    """(tiles, pairs): per block of rows, the columns from the block's first string on."""
    starts = range(0, count, block)
    return sum(-(-(count - q0) // tile) for q0 in starts), sum(min(block, count - q0) * (count - q0) for q0 in starts)


@pytest.mark.parametrize("count", [1, 2, 300, 4096, 4097, 16384, 100000, 10**6])
def test_probe_counts_the_triangle_and_the_square(count):
    block, tile, tiles, pairs = _abi.clusters_probe(count, True)
    assert (block, tile) == _abi.within_probe(count, count, 0)[:2]  # within's self-form cut
    assert (tiles, pairs) == _triangle(count, block, tile)
    assert count * (count + 1) // 2 <= pairs  # every pair i <= j ...
    assert pairs < count * count if count > block else pairs == count * count  # ... and below the square once there are two blocks
    assert _abi.clusters_probe(count, False) == (block, tile, -(-count // block) * -(-count // tile), count * count)
    if count > block:  # several blocks: the triangle approaches half of the square
        assert pairs <= count * count // 2 + block * count


def test_probe_tile_knob_changes_tiles_not_pairs(tile_knob):
    block, tile, tiles, pairs = _abi.clusters_probe(300, True)
    assert (block, tile, tiles, pairs) == (300, 300, 1, 300 * 300)  # one block: its own square is all there is
    for knob in (1, 7, 64, 65):
        tile_knob(knob)
        assert _abi.clusters_probe(300, True) == (300, knob, -(-300 // knob), pairs)
        assert _abi.clusters_probe(300, False) == (300, knob, -(-300 // knob), 300 * 300)
    tile_knob(4096)
    big = _abi.clusters_probe(100000, True)
    tile_knob(1000)
    small = _abi.clusters_probe(100000, True)
    assert small[0] == big[0] and small[3] == big[3] and small[2] > big[2]


def test_probe_edges():
    assert _abi.clusters_probe(0, True) == (1, 1, 0, 0) and _abi.clusters_probe(0, False) == (1, 1, 0, 0)
    assert _abi.clusters_probe(2**32 - 1, True)[3] < (2**32 - 1) ** 2 == _abi.clusters_probe(2**32 - 1, False)[3]
    for symmetric in (True, False):
        with pytest.raises(szs.StringZillasError) as refused:
            _abi.clusters_probe(2**32, symmetric)
        assert refused.value.status_name == "unexpected_dimensions"
    assert _abi.lib.szs_rocm_clusters_probe(300, 1, None, None, None, None) == 0  # the outputs are optional


# ---- the refusals, in order, on memory that passes for an engine ---------------------------------------------------------------------


def _call(name, engine, labels, count_word, count=2, strings=True):
    """One C call over `count` strings; `labels` None for NULL; -> (status name, message)."""
    data = np.frombuffer(b"abcabd", dtype=np.uint8).copy()
    offsets = np.array([0, 3, 6], dtype=np.uint64 if name.endswith("u64tape") else np.uint32)
    tape = (_abi.U64Tape if name.endswith("u64tape") else _abi.U32Tape)(data.ctypes.data, offsets.ctypes.data, count)
    if not name.endswith("tape"):  # the sz_sequence_t form: `count` strings behind callbacks
        get_start = _abi.MEMBER_START(lambda handle, i: data.ctypes.data + int(offsets[i]))
        get_length = _abi.MEMBER_LENGTH(lambda handle, i: int(offsets[i + 1] - offsets[i]))
        tape = _abi.Sequence(None, count, get_start, get_length)
    error = ctypes.c_char_p()
    status = getattr(_abi.lib, name)(engine, None, ctypes.byref(tape) if strings else None, 1, None if labels is None else labels.ctypes.data,
                                     None if count_word is None else count_word.ctypes.data, ctypes.byref(error))
    return _abi.STATUS_NAMES[status], error.value


@pytest.mark.parametrize("name", SYMBOLS)
def test_refusals_come_in_order_and_write_nothing(name):
    good, blank = _fake_engine(), ctypes.create_string_buffer(4096)
    labels, word = np.full(2, UNTOUCHED, np.uint64), np.full(1, UNTOUCHED, np.uint64)
    intact = lambda: (labels == UNTOUCHED).all() and (word == UNTOUCHED).all()
    # 1. the count - before the engine is looked at (no string is: the tape only says how many there are)
    for engine in (None, ctypes.addressof(blank), ctypes.addressof(good)):
        status, message = _call(name, engine, labels, word, count=2**32)
        assert status == "unexpected_dimensions" and b"2^32" in message and intact()
    # 2. the engine - before the strings, also with nothing to do
    for engine in (None, ctypes.addressof(blank)):
        for count, strings in ((2, True), (0, True), (2, False)):
            status, message = _call(name, engine, labels, word, count=count, strings=strings)
            assert status == "unknown" and b"ngine" in message and intact()
    fingerprints = ctypes.create_string_buffer(4096)  # ... nor is a family beyond the four an engine of this call
    head = _EngineHead.from_buffer(fingerprints)
    head.magic, head.family = 0x535A5345, 4
    assert _call(name, ctypes.addressof(fingerprints), labels, word)[0] == "unknown" and intact()
    # 3. NULL strings
    status, message = _call(name, ctypes.addressof(good), labels, word, strings=False)
    assert status == "unknown" and b"trings" in message and intact()
    # ... zero strings succeed: nothing is written but the count of clusters, 0 - and that only where there is a word for it
    assert _call(name, ctypes.addressof(good), labels, word, count=0)[0] == "success"
    assert (labels == UNTOUCHED).all() and word[0] == 0
    word[0] = UNTOUCHED
    assert _call(name, ctypes.addressof(good), None, None, count=0)[0] == "success"
    # 4. NULL labels, for every family the call takes
    for family in (0, 1, 2, 3):
        engine = _fake_engine(family)  # (held: the address must not outlive the buffer)
        status, message = _call(name, ctypes.addressof(engine), None, word)
        assert status == "unknown" and b"abels" in message and intact()


def test_fingerprint_refusals():
    labels, word = np.full(2, UNTOUCHED, np.uint64), np.full(1, UNTOUCHED, np.uint64)
    hashes = np.zeros((2, 4), np.uint32)
    error = ctypes.c_char_p()

    def call(engine, stride, count, hashes_pointer=hashes.ctypes.data, labels_pointer=labels.ctypes.data):
        status = _abi.lib.szs_rocm_fingerprint_clusters(engine, None, hashes_pointer, stride, count, 1, labels_pointer, word.ctypes.data,
                                                        ctypes.byref(error))
        return _abi.STATUS_NAMES[status]

    blank = ctypes.create_string_buffer(4096)
    assert call(None, 16, 2**32) == "unexpected_dimensions"  # the count first
    assert call(None, 18, 2) == "unexpected_dimensions"  # then the stride: a multiple of 4
    assert call(None, 16, 2) == "unknown" and call(ctypes.addressof(blank), 16, 2) == "unknown"  # then the engine
    similarity = _fake_engine()
    assert call(ctypes.addressof(similarity), 16, 2) == "unknown"  # a similarity engine is no fingerprints engine
    assert (labels == UNTOUCHED).all() and (word == UNTOUCHED).all()


@pytest.mark.parametrize("bound", [None, 1.5, True, 2**63, -2**63 - 1, "1"])
def test_python_clusters_rejects_a_bad_bound_before_the_library(bound):
    with pytest.raises(ValueError):
        _no_gpu_engine().clusters(["abc", "abd"], bound)


@pytest.mark.parametrize("min_matches", [None, 1.5, True, -1, 2**64])
def test_python_fingerprint_clusters_rejects_bad_min_matches_before_the_library(min_matches):
    with pytest.raises(ValueError):
        object.__new__(szs.Fingerprints).clusters(np.zeros((2, 4), np.uint32), min_matches)

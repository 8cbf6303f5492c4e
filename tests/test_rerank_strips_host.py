"""The routing of rerank rows on bare lengths (`szs_rocm_rerank_probe`, host/rerank.c): which rows the short kernel, the strips kernel
and the row route take, the strip shapes, the parked scratch.  Pure host code: no GPU."""
import ctypes

import numpy as np
import pytest

from stringzilla_amd import _abi

LENGTHS = [0, 256, 257, 300, 512, 513, 2048, 2049, 65536, 65537]
BUDGET = 256 << 20


@pytest.fixture
def rerank_knob():
    previous = _abi._knob_values["rerank"]
    yield lambda value: _abi.tuning_set("rerank", value)
    _abi.tuning_set("rerank", previous)


def test_the_probe_is_exported():
    assert "szs_rocm_rerank_probe" in _abi.SIGNATURES
    assert ctypes.cast(_abi.lib.szs_rocm_rerank_probe, ctypes.c_void_p).value


def test_routes_and_strip_shapes():
    routes, strips, strip_words, scratch = _abi.rerank_probe(LENGTHS, k=16, longest_candidate=3000)
    assert routes.tolist() == [1, 1, 2, 2, 2, 2, 2, 2, 2, 0]
    shape = {length: (int(s), int(w)) for length, s, w in zip(LENGTHS, strips, strip_words)}
    assert shape[257] == (2, 5) and shape[300] == (2, 5) and shape[512] == (2, 8) and shape[513] == (3, 6)
    assert shape[2048] == (8, 8) and shape[2049] == (9, 8)
    assert shape[65536] == (256, 8) and shape[65537] == (0, 0)
    assert shape[0] == (1, 1) and shape[256] == (1, 8)  # the short kernel: one bit-vector of the query's own width
    assert 0 < scratch <= BUDGET


def test_the_rule_for_every_word_count():
    lengths = np.arange(257, 65537, 31, dtype=np.uint32)
    routes, strips, strip_words, _ = _abi.rerank_probe(lengths, k=1, longest_candidate=10)
    words = (lengths.astype(np.int64) + 31) // 32
    want_strips = (words + 7) // 8
    assert (routes == 2).all() and np.array_equal(strips, want_strips)
    assert np.array_equal(strip_words, (words + want_strips - 1) // want_strips)
    assert strip_words.max() == 8 and strip_words.min() >= 5  # as few strips as 8 words allow: never a nearly empty one


def test_other_engines_take_the_row_route():
    for unit_cost, runes in ((True, True), (False, False), (False, True)):
        routes, strips, strip_words, scratch = _abi.rerank_probe(LENGTHS, 16, 3000, unit_cost=unit_cost, runes=runes)
        assert not routes.any() and not strips.any() and not strip_words.any() and scratch == 0


def test_the_knob_picks_the_routes(rerank_knob):
    rerank_knob(1)
    routes, _, _, scratch = _abi.rerank_probe(LENGTHS, 16, 3000)
    assert routes.tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0] and scratch == 0
    rerank_knob(0)
    routes, _, _, scratch = _abi.rerank_probe(LENGTHS, 16, 3000)
    assert not routes.any() and scratch == 0
    rerank_knob(None)
    assert _abi.rerank_probe(LENGTHS, 16, 3000)[0].tolist() == [1, 1, 2, 2, 2, 2, 2, 2, 2, 0]


def test_the_knob_accepts_one_and_restores():
    before = _abi._knob_values["rerank"]
    assert _abi.tuning_set("rerank", 1) == before
    assert _abi.tuning_set("SZS_ROCM_RERANK", before) == "1"
    assert _abi._knob_values["rerank"] == before


@pytest.mark.parametrize("k", [1, 16, 17, 33, 200])
def test_the_parked_scratch_stays_in_budget(k):
    many = np.full(100_000, 1000, dtype=np.uint32)
    sizes = []
    for longest_candidate in (0, 1, 16, 17, 3000, 1 << 20, 1 << 24):
        routes, _, _, scratch = _abi.rerank_probe(many, k, longest_candidate)
        assert (routes == 2).all() and 0 < scratch <= BUDGET, (longest_candidate, scratch)
        dwords = max(1, -(-longest_candidate // 16))
        assert scratch % (dwords * 64 * 4) == 0  # whole workgroups of [dword = 16 columns][64 lanes]
        sizes.append(scratch)
    assert sizes[1] == sizes[0] and sizes[-1] == BUDGET  # 2^24 bytes: the one workgroup the budget holds
    # one row: one workgroup's array
    assert _abi.rerank_probe([1000], k, 3000)[3] == 188 * 64 * 4
    # a candidate no single workgroup's array holds within the budget: the strips route is not taken
    routes, _, _, scratch = _abi.rerank_probe([100, 1000], k, (1 << 24) + 1)
    assert routes.tolist() == [1, 0] and scratch == 0


def test_bad_arguments():
    assert _abi.lib.szs_rocm_rerank_probe(1, 0, None, 0, 0, 10, None, None, None, None) == -15  # k = 0
    assert _abi.lib.szs_rocm_rerank_probe(1, 0, None, 0, 1, 10, None, None, None, None) == 0    # no queries, no outputs

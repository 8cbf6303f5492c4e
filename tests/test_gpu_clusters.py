"""Clusters on the GPU (`szs_rocm_clusters*`, `szs_rocm_fingerprint_clusters`, `_Engine.clusters`, `Fingerprints.clusters`; DESIGN.md
section 4.16) against a host union-find over the oracle's full self-matrix (tests/clusters_cases.py): one label per string, the smallest
index of its component, and the number of components - the same bytes under every tile size.

One thing the default cut decides: up to 4096 strings are ONE block of rows (`szs_rocm_clusters_probe`), whose tiles start at string 0
whatever the tile size - the triangle then saves nothing, and no tile starts off a multiple of the tile.  So beside the 300-string case
there is one of 4100 strings: its second block starts at row 4096, its tiles there under `top_k_tile` 1000 at 4096, 5096 - and only at
that size can a symmetric call report fewer pairs than the square."""
import ctypes
import functools
import random

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi, matrices

import clusters_cases as cases
from test_gpu_within import _family, _rand, _strings

pytestmark = pytest.mark.gpu

UNTOUCHED = cases.UNTOUCHED
FAMILIES = ["levenshtein", "levenshtein_affine", "levenshtein_utf8", "needleman_wunsch", "smith_waterman"]
PLANTED = ("levenshtein", "levenshtein_affine", "levenshtein_utf8")  # seed 1 below: checked on the CPU against the oracle


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return szs.DeviceScope(gpu_device=0)


@pytest.fixture
def tile_knob():
    previous = _abi._knob_values["top_k_tile"]
    yield lambda value: _abi.tuning_set("top_k_tile", value)
    _abi.tuning_set("top_k_tile", previous)


def _edited(rng, text, alphabet):
    """`text` - a list of symbols - with 0 to 2 random edits."""
    text = list(text)
    for _ in range(rng.randint(0, 2)):
        kind, at = rng.choice("sid"), rng.randrange(len(text) + 1)
        if kind == "i":
            text.insert(at, rng.choice(alphabet))
        elif text and kind == "s":
            text[min(at, len(text) - 1)] = rng.choice(alphabet)
        elif len(text) > 1:
            del text[min(at, len(text) - 1)]
    return text


@functools.lru_cache(maxsize=None)
def family_strings(family):
    """The 150 candidates of tests/test_gpu_within.py's family; for the Levenshtein families a third of them replaced by copies of others
    with 0 to 2 random edits, so that small bounds give components of several sizes."""
    alphabet = {"levenshtein": b"ACGT", "levenshtein_affine": b"abcdef", "levenshtein_utf8": None, "needleman_wunsch": b"ARNDCQEGHILKMFPSTWYV",
                "smith_waterman": b"ACGT"}[family]
    strings = list(_strings(family, alphabet)[1])
    if family in PLANTED:
        rng = random.Random(1)
        for at in rng.sample(range(len(strings)), len(strings) // 3):
            source = strings[rng.randrange(len(strings))]
            if alphabet is None:
                strings[at] = "".join(_edited(rng, source.decode(), ["a", "b", "é", "ж", "中", "😀", "ß"])).encode()
            else:
                strings[at] = bytes(_edited(rng, source, alphabet))
    return tuple(strings)


def family_bounds(signed, descending):
    """The quantiles 0.02 / 0.25 / 0.5 of the full self-matrix and both its ends; where hits are the HIGH scores also the mirrored
    quantiles - the bounds with few hits - and on distance engines two negative bounds."""
    quantiles = (0.02, 0.25, 0.5) + ((0.98, 0.995, 0.999) if descending else ())
    bounds = {int(np.quantile(signed, q, method="nearest")) for q in quantiles} | {int(signed.min()), int(signed.max())}
    return sorted(bounds) if descending else [-5, -1] + sorted(bounds)


def _check(got, want_labels, note):
    labels, count = got
    assert isinstance(count, int) and labels.dtype == np.uint64 and labels.shape == want_labels.shape, note
    assert np.array_equal(labels, want_labels), (note, np.flatnonzero(labels != want_labels)[:8])
    assert count == int((want_labels == np.arange(len(want_labels), dtype=np.uint64)).sum()), note
    assert np.array_equal(labels[labels.astype(np.int64)], labels), note


@pytest.mark.parametrize("family", FAMILIES)
def test_families(gpu, oracle, family):
    engine, score, descending, _ = _family(family, gpu)
    strings = list(family_strings(family))
    n = len(strings)
    full = score(oracle, strings, strings)
    seen, largest = set(), 0
    for bound in family_bounds(full.astype(np.int64), descending):
        hits = cases.hits_of(full, bound, descending, self_search=True)
        assert np.array_equal(hits, hits.T), (family, bound)  # what licenses the triangle for these engines
        want = cases.expected_labels(hits)
        got = engine.clusters(strings, bound, device=gpu)
        _check(got, want, (family, bound))
        seen.add("alone" if got[1] == n else "one" if got[1] == 1 else "between")
        largest = max(largest, int(np.bincount(want.astype(np.int64)).max()) if 1 < got[1] < n else 0)
        if not descending and bound < 0:
            assert got[1] == n and engine.last_call_profile().pairs == 0, (family, bound)  # nothing is scored
    assert seen == {"alone", "one", "between"} and largest >= 3, (family, seen, largest)


def _levenshtein_case(count, seed):
    rng = random.Random(seed)
    strings = _rand(rng, count, 4, 14, b"ACGT")
    for at in rng.sample(range(count), count // 3):
        strings[at] = bytes(_edited(rng, strings[rng.randrange(count)], b"ACGT"))
    return strings


@pytest.mark.parametrize("count", [150, 300])
def test_tiling_changes_no_byte(gpu, oracle, tile_knob, count):
    strings = _levenshtein_case(count, count)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    full = oracle.levenshtein(strings, strings)
    for bound in (0, 1, 2):
        want = cases.labels_of_matrix(full, bound, False)
        outputs = {}
        for tile in (None, 64, 1):
            tile_knob(tile)
            block, planned, tiles, pairs = _abi.clusters_probe(count, True)
            assert (block, planned, pairs) == (count, tile or count, count * count)
            outputs[tile] = engine.clusters(strings, bound, device=gpu)
            _check(outputs[tile], want, (count, bound, tile))
            profile = engine.last_call_profile()
            assert profile.pairs == pairs and profile.launches >= 2 * tiles + 2  # per tile the scoring and the union; begin and finish
        assert all(got[0].tobytes() == outputs[None][0].tobytes() and got[1] == outputs[None][1] for got in outputs.values())
    assert 1 < outputs[None][1] < count


@functools.lru_cache(maxsize=None)
def _two_blocks():
    """4100 short strings - one more block of rows than 4096 - with planted near-copies: few hits, components of several sizes."""
    rng = random.Random(41)
    strings = _rand(rng, 4100, 5, 8, b"ARNDCQEGHILKMFPSTWYV")
    for at in rng.sample(range(4100), 600):
        strings[at] = bytes(_edited(rng, strings[rng.randrange(4100)], b"ARNDCQEGHILKMFPSTWYV"))
    strings[4099] = strings[7]  # an edge from the second block of rows back into the first
    return tuple(strings)


def test_two_blocks_score_the_triangle(gpu, oracle, tile_knob):
    strings = list(_two_blocks())
    n = len(strings)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    want = cases.labels_of_matrix(oracle.levenshtein(strings, strings), 1, False)
    assert want[4099] == want[7] and 1 < len(set(want.tolist())) < n
    outputs = []
    for tile in (None, 1000):  # 1000: the tiles of the second block start at 4096 - no multiple of the tile - and at 5096
        tile_knob(tile)
        block, planned, tiles, pairs = _abi.clusters_probe(n, True)
        assert block == 4096 and pairs == 4096 * n + 4 * 4 < n * n
        outputs.append(engine.clusters(strings, 1, device=gpu))
        _check(outputs[-1], want, tile)
        assert engine.last_call_profile().pairs == pairs
    assert outputs[0][0].tobytes() == outputs[1][0].tobytes()


def test_chain(gpu, tile_knob):
    strings = [b"A" * i for i in range(299, -1, -1)]  # distances |i - j|: one path, in descending order of length
    engine = szs.LevenshteinDistances(capabilities=gpu)
    tile_knob(64)  # the path crosses every tile edge, and roots are hooked from many workgroups
    labels, count = engine.clusters(strings, 1, device=gpu)
    assert count == 1 and not labels.any()
    labels, count = engine.clusters(strings, 0, device=gpu)
    assert count == 300 and np.array_equal(labels, np.arange(300, dtype=np.uint64))
    labels, count = engine.clusters(strings[::2], 1, device=gpu)  # every second one: no two within 1
    assert count == 150 and np.array_equal(labels, np.arange(150, dtype=np.uint64))


def test_contention(gpu):
    strings = [b"SAMEBYTE"] * 513  # about 131 thousand hits, all of which meet at root 0
    engine = szs.LevenshteinDistances(capabilities=gpu)
    labels, count = engine.clusters(strings, 0, device=gpu)
    assert count == 1 and labels.shape == (513,) and not labels.any()
    strings[256] = b"another!"
    labels, count = engine.clusters(strings, 3, device=gpu)  # eight substitutions away
    assert count == 2 and labels[256] == 256 and not np.delete(labels, 256).any()


def _asymmetric_table():
    """BLOSUM62 with ONE entry changed: cost(query A, candidate R) = +6, cost(query R, candidate A) stays -1."""
    byte_to_class, costs = matrices.blosum62()
    costs = costs.copy()
    a, r = int(byte_to_class[ord("A")]), int(byte_to_class[ord("R")])
    assert costs[a, r] == costs[r, a]
    costs[a, r] = 6
    return byte_to_class, costs


def test_asymmetric_table_scores_the_square(gpu, oracle):
    table = _asymmetric_table()
    rng = random.Random(17)
    # pairs (i < j) of an R-rich string BEFORE an A-rich one of the same length: only the later string, as the query, scores high
    strings = []
    for _ in range(20):
        length = rng.randint(4, 9)
        strings += [b"R" * length, bytes(rng.choice(b"NDCQ") for _ in range(length)), b"A" * length]
    n = len(strings)
    engine = szs.NeedlemanWunschScores(*table, open=-4, extend=-4, capabilities=gpu)
    full = oracle.needleman_wunsch(strings, strings, *table, -4, -4)
    bound = 20
    hits = cases.hits_of(full, bound, True, self_search=True)
    assert (hits & ~hits.T).any() and (np.tril(hits, -1) & ~np.triu(hits, 1).T).any()  # hit(j, i) alone, with j the LARGER index
    want = cases.expected_labels(hits)
    assert not np.array_equal(want, cases.expected_labels(np.triu(hits)))  # what the triangle - rows i as queries of columns j > i - would give
    _check(engine.clusters(strings, bound, device=gpu), want, "asymmetric")
    assert engine.last_call_profile().pairs == n * n

    # the saving only shows with a second block of rows: the square for this table, the triangle for a symmetric engine of the same n
    many = list(_two_blocks())
    many[10], many[4098] = b"RRRRRR", b"AAAAAA"  # the only hit of this pair has the LAST block's string as its query
    full = oracle.needleman_wunsch(many, many, *table, -4, -4)
    bound = 30
    hits = cases.hits_of(full, bound, True, self_search=True)
    assert hits[4098, 10] and not hits[10, 4098] and hits.sum() < 20000
    want = cases.expected_labels(hits)
    assert want[4098] == 10
    _check(engine.clusters(many, bound, device=gpu), want, "asymmetric, two blocks")
    assert engine.last_call_profile().pairs == len(many) ** 2
    symmetric = szs.LevenshteinDistances(capabilities=gpu)
    symmetric.clusters(many, 0, device=gpu)
    assert symmetric.last_call_profile().pairs < len(many) ** 2
    blosum = szs.NeedlemanWunschScores(*matrices.blosum62(), open=-4, extend=-4, capabilities=gpu)  # a symmetric table: the triangle
    blosum.clusters(many, 60, device=gpu)
    assert blosum.last_call_profile().pairs == symmetric.last_call_profile().pairs


# ---- fingerprints ---------------------------------------------------------------------------------------------------------------------


def _planted_hashes(rows, dimensions, seed):
    rng = np.random.default_rng(seed)
    hashes = rng.integers(0, 2**32, size=(rows, dimensions), dtype=np.uint64).astype(np.uint32)
    planted = rng.choice(rows, size=rows // 3, replace=False)
    for at in planted:  # groups: a copy of another row with d of its dimensions redrawn; the first an exact copy, d = 0
        source, redrawn = int(rng.integers(0, rows)), 0 if at == planted[0] else int(rng.integers(0, dimensions + 1))
        source = source if source != at else (source + 1) % rows
        hashes[at] = hashes[source]
        where = rng.choice(dimensions, size=redrawn, replace=False)
        hashes[at, where] = rng.integers(0, 2**32, size=redrawn, dtype=np.uint64).astype(np.uint32)
    return hashes


def _fingerprint_labels(hashes, min_matches):
    return cases.expected_labels((hashes[:, None, :] == hashes[None, :, :]).sum(-1) >= min_matches)


def test_fingerprints(gpu):
    import torch

    hashes = _planted_hashes(200, 64, 5)
    engine = szs.Fingerprints(64, capabilities=gpu)
    wide = torch.zeros((200, 80), dtype=torch.int32, device="cuda")  # a row stride wider than 4 x dimensions
    wide[:, :64] = torch.from_numpy(hashes.view(np.int32)).cuda()
    counts = {}
    for min_matches in (0, 1, 32, 64, 65):
        want = _fingerprint_labels(hashes, min_matches)
        staged = engine.clusters(hashes, min_matches, device=gpu)  # from a host array: staged
        _check(staged, want, ("host", min_matches))
        direct = engine.clusters(wide[:, :64], min_matches, device=gpu)
        _check(direct, want, ("device", min_matches))
        counts[min_matches] = staged[1]
    assert counts[0] == 1 and counts[65] == 200 and 1 < counts[32] < 200 and counts[32] <= counts[64] < 200


def test_fingerprint_edges(gpu, tile_knob):
    one = szs.Fingerprints(1, capabilities=gpu)
    column = np.array([[7], [9], [7], [3], [9], [7]], dtype=np.uint32)
    _check(one.clusters(column, 1, device=gpu), np.array([0, 1, 0, 3, 1, 0], dtype=np.uint64), "one dimension")
    _check(one.clusters(column, 0, device=gpu), np.zeros(6, dtype=np.uint64), "one dimension, every pair")
    _check(one.clusters(column[:1], 1, device=gpu), np.zeros(1, dtype=np.uint64), "one row")
    labels, count = one.clusters(column[:0], 1, device=gpu)
    assert labels.shape == (0,) and count == 0
    hashes = _planted_hashes(200, 64, 6)
    engine = szs.Fingerprints(64, capabilities=gpu)
    want = _fingerprint_labels(hashes, 40)
    for tile in (64, 7):  # several tiles, each staged behind the launch that still reads the one before
        tile_knob(tile)
        _check(engine.clusters(hashes, 40, device=gpu), want, tile)


# ---- outputs and inputs ---------------------------------------------------------------------------------------------------------------


def test_outputs(gpu, oracle):
    import torch

    strings = _levenshtein_case(150, 150)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    want = cases.labels_of_matrix(oracle.levenshtein(strings, strings), 1, False)
    clusters = int((want == np.arange(150, dtype=np.uint64)).sum())
    for where in ("numpy", "pinned", "device"):
        out = np.full(150, UNTOUCHED, dtype=np.uint64)
        if where != "numpy":
            out = torch.from_numpy(out.view(np.int64))
            out = out.cuda() if where == "device" else out.pin_memory()
        labels, count = engine.clusters(strings, 1, device=gpu, out=out)
        assert labels is out and count == clusters
        got = out if where == "numpy" else out.cpu().numpy().view(np.uint64)
        assert np.array_equal(got, want), where
    _check(engine.clusters(szs.Strs(strings, wide_offsets=True), 1, device=gpu), want, "a u64 tape")

    tape = szs.Strs(strings)._tape(0)
    labels, error = np.full(150, UNTOUCHED, dtype=np.uint64), ctypes.c_char_p()
    status = _abi.lib.szs_rocm_clusters_u32tape(engine.handle, gpu.handle, ctypes.byref(tape), 1, labels.ctypes.data, None, ctypes.byref(error))
    assert status == 0 and np.array_equal(labels, want)  # `clusters_count` NULL

    labels, count = engine.clusters([], 1, device=gpu)
    assert labels.shape == (0,) and labels.dtype == np.uint64 and count == 0
    _check(engine.clusters([b"alone"], 1, device=gpu), np.zeros(1, dtype=np.uint64), "one string")

    with pytest.raises(ValueError):
        engine.clusters(strings, 1, device=gpu, out=np.zeros(149, np.uint64))
    with pytest.raises(ValueError):
        engine.clusters(strings, 1, device=gpu, out=np.zeros(150, np.uint32))


def test_a_refused_call_writes_nothing(gpu):
    tape = szs.Strs([b"abc", b"abd"])._tape(0)
    labels, word, error = np.full(2, UNTOUCHED, dtype=np.uint64), np.full(1, UNTOUCHED, dtype=np.uint64), ctypes.c_char_p()
    fingerprints = szs.Fingerprints(64, capabilities=gpu)
    status = _abi.lib.szs_rocm_clusters_u32tape(fingerprints.handle, gpu.handle, ctypes.byref(tape), 1, labels.ctypes.data, word.ctypes.data,
                                                ctypes.byref(error))
    assert _abi.STATUS_NAMES[status] == "unknown" and (labels == UNTOUCHED).all() and (word == UNTOUCHED).all()
    engine = szs.LevenshteinDistances(capabilities=gpu)
    hashes = np.zeros((2, 64), dtype=np.uint32)
    status = _abi.lib.szs_rocm_fingerprint_clusters(engine.handle, gpu.handle, hashes.ctypes.data, 256, 2, 1, labels.ctypes.data, word.ctypes.data,
                                                    ctypes.byref(error))
    assert _abi.STATUS_NAMES[status] == "unknown" and (labels == UNTOUCHED).all() and (word == UNTOUCHED).all()
    assert engine.clusters([b"abc", b"abd"], 1, device=gpu)[1] == 1  # the engine goes on


def test_same_bytes_every_time(gpu, tile_knob):
    strings = _levenshtein_case(700, 7)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    runs = []
    for tile in (None, 100):
        tile_knob(tile)
        runs += [engine.clusters(strings, 1, device=gpu) for _ in range(3)]
    assert 1 < runs[0][1] < 700
    assert all(labels.tobytes() == runs[0][0].tobytes() and count == runs[0][1] for labels, count in runs)

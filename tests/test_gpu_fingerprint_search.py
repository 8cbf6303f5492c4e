"""Fingerprint search on the GPU (`szs_rocm_fingerprint_matches`, `szs_rocm_fingerprint_top_k`, `Fingerprints.matches` / `.top_k`)
against NumPy over the same hash arrays.  Counts are exact integers: every comparison is `np.array_equal`."""
import ctypes
import random

import numpy as np
import pytest

import stringzilla_amd as szs
from stringzilla_amd import _abi

pytestmark = pytest.mark.gpu

EMPTY = np.uint64(2**64 - 1)
UNTOUCHED = 0x5A5A5A5A5A5A5A5A
UNTOUCHED_32 = 0x5A5A5A5A


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


_engines = {}


def _engine(ndim, gpu):
    if ndim not in _engines:
        _engines[ndim] = szs.Fingerprints(ndim, capabilities=gpu)
    return _engines[ndim]


def _draw(rng, rows, ndim, values=4):
    """Hashes from a small value set: counts vary and ties abound.  The largest value stands in for 0xFFFFFFFF."""
    matrix = rng.integers(0, values, size=(rows, ndim), dtype=np.uint32)
    matrix[matrix == values - 1] = 0xFFFFFFFF
    return matrix


def expected_matches(a, b):
    counts = np.zeros((a.shape[0], b.shape[0]), dtype=np.uint32)
    for q in range(a.shape[0]):
        counts[q] = (a[q][None, :] == b).sum(axis=1)
    return counts


def expected_top_k(matrix, k, self_search=False):
    """First k of a stable descending sort of each row (ties: lower index), the own index skipped in self-search, short rows completed."""
    rows = matrix.shape[0]
    indices = np.full((rows, k), EMPTY, dtype=np.uint64)
    scores = np.zeros((rows, k), dtype=np.uint64)
    for q in range(rows):
        row = matrix[q]
        order = np.argsort(-row.astype(np.int64), kind="stable")
        if self_search:
            order = order[order != q]
        order = order[:k]
        indices[q, :len(order)] = order
        scores[q, :len(order)] = row[order]
    return indices, scores


def _padded(matrix, extra, canary):
    """The same rows inside a wider matrix whose padding holds `canary`; returns (view of the rows, the whole matrix)."""
    whole = np.full((matrix.shape[0], matrix.shape[1] + extra), canary, dtype=matrix.dtype)
    whole[:, :matrix.shape[1]] = matrix
    return whole[:, :matrix.shape[1]], whole


# ---- matches -------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shape", [(1, 1), (3, 257), (130, 65)])
@pytest.mark.parametrize("ndim", [1, 7, 64, 100, 1024])
def test_matches_host_and_device(gpu, ndim, shape):
    import torch

    rng = np.random.default_rng(ndim * 1000 + shape[1])
    engine = _engine(ndim, gpu)
    a, b = _draw(rng, shape[0], ndim), _draw(rng, shape[1], ndim)
    want = expected_matches(a, b)

    got = engine.matches(a, b, device=gpu)
    assert got.dtype == np.uint32 and got.shape == shape
    assert np.array_equal(got, want)

    # padded strides on both inputs and on the output, in host memory: the padding stays as it was
    (a_rows, a_whole), (b_rows, b_whole) = _padded(a, 3, 0xDEADBEEF), _padded(b, 5, 0xDEADBEEF)
    out_rows, out_whole = _padded(np.zeros(shape, dtype=np.uint32), 2, UNTOUCHED_32)
    assert engine.matches(a_rows, b_rows, device=gpu, out=out_rows) is out_rows
    assert np.array_equal(out_rows, want)
    assert (out_whole[:, shape[1]:] == UNTOUCHED_32).all()
    assert (a_whole[:, ndim:] == 0xDEADBEEF).all() and (b_whole[:, ndim:] == 0xDEADBEEF).all()

    # torch GPU memory in and out, dense and padded
    a_gpu, b_gpu = torch.from_numpy(a.view(np.int32)).cuda(), torch.from_numpy(b.view(np.int32)).cuda()
    out_gpu = torch.full(shape, 77, dtype=torch.int32, device="cuda")
    engine.matches(a_gpu, b_gpu, device=gpu, out=out_gpu)
    assert np.array_equal(out_gpu.cpu().numpy().view(np.uint32), want)
    a_wide = torch.from_numpy(a_whole.view(np.int32)).cuda()
    b_wide = torch.from_numpy(b_whole.view(np.int32)).cuda()
    out_wide = torch.full((shape[0], shape[1] + 4), 77, dtype=torch.int32, device="cuda")
    engine.matches(a_wide[:, :ndim], b_wide[:, :ndim], device=gpu, out=out_wide[:, :shape[1]])
    assert np.array_equal(out_wide[:, :shape[1]].cpu().numpy().view(np.uint32), want)
    assert (out_wide[:, shape[1]:] == 77).all()
    assert np.array_equal(a_wide.cpu().numpy().view(np.uint32), a_whole) and np.array_equal(b_wide.cpu().numpy().view(np.uint32), b_whole)

    # mixed: queries on the GPU, candidates on the host, and the reverse
    assert np.array_equal(engine.matches(a_gpu, b, device=gpu), want)
    assert np.array_equal(engine.matches(a, b_gpu, device=gpu), want)


@pytest.mark.parametrize("ndim", [7, 64])
def test_matches_self(gpu, ndim):
    rng = np.random.default_rng(ndim)
    engine = _engine(ndim, gpu)
    a = _draw(rng, 70, ndim)
    a[5] = a[60]
    both = engine.matches(a, a, device=gpu)
    alone = engine.matches(a, None, device=gpu)
    assert np.array_equal(alone, both) and np.array_equal(alone, expected_matches(a, a))
    assert (np.diag(alone) == ndim).all() and alone[5, 60] == ndim


def test_matches_unaligned_rows(gpu):
    """Rows that start on 4-byte but not on 16-byte boundaries."""
    rng = np.random.default_rng(99)
    engine = _engine(64, gpu)
    a, b = _draw(rng, 9, 64), _draw(rng, 33, 64)
    (a_rows, _), (b_rows, _) = _padded(a, 1, 0), _padded(b, 3, 0)
    assert np.array_equal(engine.matches(a_rows, b_rows, device=gpu), expected_matches(a, b))
    import torch

    a_gpu, b_gpu = torch.from_numpy(a_rows.base.view(np.int32)).cuda(), torch.from_numpy(b_rows.base.view(np.int32)).cuda()
    assert np.array_equal(engine.matches(a_gpu[:, :64], b_gpu[:, :64], device=gpu), expected_matches(a, b))


def _empties():
    """Zero fingerprints as NumPy and as torch on the host and the GPU (torch gives the latter two the pointer 0)."""
    import torch

    return (np.zeros((0, 64), dtype=np.uint32), torch.empty((0, 64), dtype=torch.int32),
            torch.empty((0, 64), dtype=torch.int32, device="cuda"))


def test_matches_empty_sides(gpu):
    import torch

    engine = _engine(64, gpu)
    a = _draw(np.random.default_rng(1), 3, 64)
    for empty in _empties():
        assert engine.matches(a, empty, device=gpu).shape == (3, 0)
        assert engine.matches(empty, a, device=gpu).shape == (0, 3)
        assert engine.matches(empty, empty, device=gpu).shape == (0, 0)
        assert engine.matches(empty, None, device=gpu).shape == (0, 0)
        out = torch.empty((3, 0), dtype=torch.int32, device="cuda")
        assert engine.matches(a, empty, device=gpu, out=out) is out


def test_matches_blocks_and_tiles_into_host_memory(gpu):
    """Counts the device cannot write go through a scratch tile of at most 4096 queries x 8192 candidates (32 M cells / 4096):
    4100 x 8200 takes two blocks and two tiles, so the copy-out lands at non-zero row and column offsets and the tile is reused."""
    rng = np.random.default_rng(21)
    engine = _engine(1, gpu)
    a, b = _draw(rng, 4100, 1), _draw(rng, 8200, 1)
    want = (a == b.T).astype(np.uint32)
    out_rows, out_whole = _padded(np.zeros((4100, 8200), dtype=np.uint32), 3, UNTOUCHED_32)
    engine.matches(a, b, device=gpu, out=out_rows)
    assert np.array_equal(out_rows, want) and (out_whole[:, 8200:] == UNTOUCHED_32).all()
    narrow = np.full((4100, 3), UNTOUCHED_32, dtype=np.uint32)  # more than 4096 queries, one tile
    engine.matches(a, b[:3], device=gpu, out=narrow)
    assert np.array_equal(narrow, want[:, :3])


def test_matches_blocks_and_tiles_into_device_memory(gpu):
    """Hashes staged from host memory come 256 MiB at a time, 65,536 rows at 1024 dimensions: 65,540 rows on either side take a
    second block / tile, which a kernel writes straight into the caller's device matrix at its row / column offset."""
    import torch

    rng = np.random.default_rng(22)
    engine = _engine(1024, gpu)
    big, small = _draw(rng, 65_540, 1024), _draw(rng, 2, 1024)
    want = expected_matches(small, big)
    tall = torch.full((65_540, 3), 77, dtype=torch.int32, device="cuda")
    engine.matches(big, small, device=gpu, out=tall[:, :2])
    assert np.array_equal(tall[:, :2].cpu().numpy().view(np.uint32), want.T) and (tall[:, 2] == 77).all()
    wide = torch.full((2, 65_543), 77, dtype=torch.int32, device="cuda")
    engine.matches(small, big, device=gpu, out=wide[:, :65_540])
    assert np.array_equal(wide[:, :65_540].cpu().numpy().view(np.uint32), want) and (wide[:, 65_540:] == 77).all()


# ---- top_k ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("ndim", [7, 64, 100])
def test_top_k_sizes(gpu, ndim):
    rng = np.random.default_rng(ndim + 1)
    engine = _engine(ndim, gpu)
    a, b = _draw(rng, 23, ndim), _draw(rng, 41, ndim)
    full = expected_matches(a, b)
    for k in (1, 7, 41, 44, 1024):
        indices, matches = engine.top_k(a, b, k=k, device=gpu)
        want_indices, want_matches = expected_top_k(full, k)
        assert indices.dtype == np.uint64 and matches.dtype == np.uint64 and indices.shape == (23, k)
        assert np.array_equal(indices, want_indices), k
        assert np.array_equal(matches, want_matches), k


def test_top_k_self_search_with_duplicates(gpu):
    rng = np.random.default_rng(5)
    engine = _engine(64, gpu)
    a = _draw(rng, 17, 64)
    a[3] = a[9] = a[11]  # duplicates at other indices still count
    full = expected_matches(a, a)
    for k in (4, 16, 19):
        indices, matches = engine.top_k(a, None, k=k, device=gpu)
        want_indices, want_matches = expected_top_k(full, k, self_search=True)
        assert np.array_equal(indices, want_indices) and np.array_equal(matches, want_matches), k
    indices, matches = engine.top_k(a, None, k=2, device=gpu)
    assert indices[3, 0] == 9 and indices[9, 0] == 3 and indices[11, 0] == 3 and matches[3, 0] == 64
    single_indices, single_matches = engine.top_k(a[:1], None, k=3, device=gpu)
    assert (single_indices == EMPTY).all() and (single_matches == 0).all()


def test_top_k_empty_sides(gpu):
    engine = _engine(64, gpu)
    a = _draw(np.random.default_rng(2), 2, 64)
    a[1] = a[0]  # a self-search would find these
    for empty in _empties():
        indices, matches = engine.top_k(a, empty, k=3, device=gpu)
        assert (indices == EMPTY).all() and (matches == 0).all() and indices.shape == (2, 3)
        indices, matches = engine.top_k(empty, a, k=2, device=gpu)
        assert indices.shape == (0, 2) and matches.shape == (0, 2)
        indices, matches = engine.top_k(empty, None, k=2, device=gpu)
        assert indices.shape == (0, 2) and matches.shape == (0, 2)


def test_top_k_output_placement(gpu):
    import torch

    rng = np.random.default_rng(9)
    engine = _engine(100, gpu)
    a, b = _draw(rng, 7, 100), _draw(rng, 30, 100)
    want = expected_top_k(expected_matches(a, b), 5)

    # numpy outputs, row stride beyond k: the padding stays as it was
    wide_indices = np.full((7, 9), UNTOUCHED, dtype=np.uint64)
    wide_matches = np.full((7, 9), UNTOUCHED, dtype=np.uint64)
    engine.top_k(a, b, k=5, device=gpu, out=(wide_indices[:, :5], wide_matches[:, :5]))
    assert np.array_equal(wide_indices[:, :5], want[0]) and np.array_equal(wide_matches[:, :5], want[1])
    assert (wide_indices[:, 5:] == UNTOUCHED).all() and (wide_matches[:, 5:] == UNTOUCHED).all()

    # device torch outputs, and the same with a row stride beyond k
    device_indices = torch.zeros((7, 5), dtype=torch.int64, device="cuda")
    device_matches = torch.zeros((7, 5), dtype=torch.int64, device="cuda")
    engine.top_k(a, b, k=5, device=gpu, out=(device_indices, device_matches))
    assert np.array_equal(device_indices.cpu().numpy().view(np.uint64), want[0])
    assert np.array_equal(device_matches.cpu().numpy().view(np.uint64), want[1])
    padded = torch.full((2, 7, 8), 77, dtype=torch.int64, device="cuda")
    engine.top_k(a, b, k=5, device=gpu, out=(padded[0, :, :5], padded[1, :, :5]))
    assert np.array_equal(padded[0, :, :5].cpu().numpy().view(np.uint64), want[0])
    assert np.array_equal(padded[1, :, :5].cpu().numpy().view(np.uint64), want[1])
    assert (padded[:, :, 5:] == 77).all()

    # matches NULL: indices only
    indices_only = np.full((7, 6), UNTOUCHED, dtype=np.uint64)
    engine.top_k(a, b, k=5, device=gpu, out=(indices_only[:, :5], None))
    assert np.array_equal(indices_only[:, :5], want[0]) and (indices_only[:, 5] == UNTOUCHED).all()


def test_top_k_ties_are_independent_of_tiling(gpu, tile_knob):
    import torch

    rng = np.random.default_rng(11)
    engine = _engine(7, gpu)
    a, b = _draw(rng, 9, 7, values=2), _draw(rng, 150, 7, values=2)
    b[20:60] = b[20]  # a long run of ties that tiles of 3 cut in many places
    full = expected_matches(a, b)
    b_gpu = torch.from_numpy(b.view(np.int32)).cuda()
    for tile in (3, 64, None):
        tile_knob(tile)
        for k in (5, 33):
            want = expected_top_k(full, k)
            for candidates in (b, b_gpu):  # staged from host memory tile by tile, and read in place
                indices, matches = engine.top_k(a, candidates, k=k, device=gpu)
                assert np.array_equal(indices, want[0]) and np.array_equal(matches, want[1]), (tile, k)
        want = expected_top_k(expected_matches(b, b), 6, self_search=True)
        indices, matches = engine.top_k(b, None, k=6, device=gpu)
        assert np.array_equal(indices, want[0]) and np.array_equal(matches, want[1]), tile


def test_top_k_automatic_tiling_segments_and_tiles(gpu):
    """8 x 40,000 at the automatic sizes: several row segments per tile; 600 x 40,000: two tiles (16 M cells / 600 rows = 27,962)."""
    import torch

    rng = np.random.default_rng(3)
    engine = _engine(64, gpu)
    b = _draw(rng, 40_000, 64, values=2)
    b_gpu = torch.from_numpy(b.view(np.int32)).cuda()
    for rows in (8, 600):
        a = _draw(rng, rows, 64, values=2)
        want = expected_top_k(expected_matches(a, b), 10)
        from_host = engine.top_k(a, b, k=10, device=gpu)
        from_device = engine.top_k(torch.from_numpy(a.view(np.int32)).cuda(), b_gpu, k=10, device=gpu)
        assert np.array_equal(from_host[0], want[0]) and np.array_equal(from_host[1], want[1]), rows
        assert np.array_equal(from_device[0], from_host[0]) and np.array_equal(from_device[1], from_host[1]), rows


def test_top_k_self_search_in_two_blocks_of_queries(gpu):
    """4,200 fingerprints against themselves: with 4,096 or more candidates a block is 16 M cells / 4096 = 4,096 queries, so a second
    block of 104 begins at query 4,096 - the row that both its self-exclusion and its rows of the host outputs (staged) start from."""
    rng = np.random.default_rng(31)
    engine = _engine(1, gpu)
    a = _draw(rng, 4200, 1)  # one dimension of four values: every count is 0 or 1, a quarter of each row ties at the top
    a[4100], a[4150], a[10], a[4199] = 7, 7, 9, 9  # twins no other row equals: without its own column each finds the other first
    want = expected_top_k(expected_matches(a, a), 5, self_search=True)
    wide_indices = np.full((4200, 6), UNTOUCHED, dtype=np.uint64)
    wide_matches = np.full((4200, 6), UNTOUCHED, dtype=np.uint64)
    engine.top_k(a, None, k=5, device=gpu, out=(wide_indices[:, :5], wide_matches[:, :5]))
    assert np.array_equal(wide_indices[:, :5], want[0]) and np.array_equal(wide_matches[:, :5], want[1])
    assert (wide_indices[:, 5] == UNTOUCHED).all() and (wide_matches[:, 5] == UNTOUCHED).all()
    assert not (wide_indices[:, :5] == np.arange(4200, dtype=np.uint64)[:, None]).any()  # never the own index, in either block
    assert wide_indices[[4100, 4150, 10, 4199], :2].tolist() == [[4150, 0], [4100, 0], [4199, 0], [10, 0]]


def test_other_handles_are_refused_on_the_gpu(gpu):
    similarity = szs.LevenshteinDistances(capabilities=gpu)
    a = _draw(np.random.default_rng(4), 2, 64)
    counts = np.full((2, 2), UNTOUCHED_32, dtype=np.uint32)
    indices = np.full((2, 2), UNTOUCHED, dtype=np.uint64)
    error = ctypes.c_char_p()
    status = _abi.lib.szs_rocm_fingerprint_matches(similarity.handle, gpu.handle, a.ctypes.data, 256, 2, a.ctypes.data, 256, 2,
                                                   counts.ctypes.data, 8, ctypes.byref(error))
    assert status != 0 and error.value and (counts == UNTOUCHED_32).all()
    status = _abi.lib.szs_rocm_fingerprint_top_k(similarity.handle, gpu.handle, a.ctypes.data, 256, 2, a.ctypes.data, 256, 2, 2,
                                                 indices.ctypes.data, None, 2, ctypes.byref(error))
    assert status != 0 and error.value and (indices == UNTOUCHED).all()


# ---- end to end ----------------------------------------------------------------------------------------------------------------


def _documents():
    rng = random.Random(17)
    letters = "abcdefghijklmnopqrstuvwxyz      "
    documents = ["".join(rng.choice(letters) for _ in range(rng.randint(80, 400))).encode() for _ in range(200)]
    copies = {150: 12, 151: 12, 199: 77, 42: 3}  # index -> the document it repeats
    for index, source in copies.items():
        documents[index] = documents[source]
    return documents, copies


def test_near_duplicates_end_to_end(gpu):
    documents, copies = _documents()
    engine = szs.Fingerprints(ndim=256, capabilities=gpu)
    hashes, _ = engine(documents, device=gpu)
    indices, matches = engine.top_k(hashes, k=4, device=gpu)
    groups = {}
    for index, source in copies.items():
        groups.setdefault(source, {source}).add(index)
    for members in groups.values():
        for member in members:
            first = min(members - {member})
            assert indices[member, 0] == first and matches[member, 0] == 256, member
    want = expected_top_k(expected_matches(hashes, hashes), 4, self_search=True)
    assert np.array_equal(indices, want[0]) and np.array_equal(matches, want[1])
    # the Jaccard estimate is the caller's division
    assert (matches / engine.ndim <= 1.0).all()


def test_hashing_is_unchanged_by_searches(gpu):
    import torch

    documents, _ = _documents()
    engine = szs.Fingerprints(ndim=128, capabilities=gpu)
    hashes_before, counts_before = engine(documents, device=gpu)
    engine.matches(hashes_before, device=gpu)
    engine.top_k(hashes_before, k=3, device=gpu)
    engine.top_k(torch.from_numpy(hashes_before.view(np.int32)).cuda(), hashes_before, k=3, device=gpu)
    hashes_after, counts_after = engine(documents, device=gpu)
    assert np.array_equal(hashes_after, hashes_before) and np.array_equal(counts_after, counts_before)
    fresh = szs.Fingerprints(ndim=128, capabilities=gpu)
    fresh_hashes, fresh_counts = fresh(documents, device=gpu)
    assert np.array_equal(fresh_hashes, hashes_before) and np.array_equal(fresh_counts, counts_before)

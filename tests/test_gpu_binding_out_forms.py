"""Every method of the Python binding that sits on the shared argument helpers, on the GPU, in every form its arguments take: `out`
None, NumPy arrays, host tensors, device tensors and - where the C entry takes a row stride - matrices cut from wider ones whose padding
must survive; then both offset widths mixed, inputs already on the device, a single query and `limit=0`.  Three queries, five
candidates, k = 2, limit = 3: the point is the plumbing, the kernels have their own tests.  Expected values come from the plain models
the suite already has (tests/within_cases.py, tests/alignment_cases.py, tests/clusters_cases.py, the fuzzy-scan models)."""
import functools

import numpy as np
import pytest
import torch

import stringzilla_amd as szs

import alignment_cases
import clusters_cases
import within_cases as cases
from test_fuzzy_scan_matches_model import hits_of as scan_hits_of, last_row
from test_fuzzy_scan_occurrences_model import occurrences_of

pytestmark = pytest.mark.gpu

EMPTY, SENTINEL = 2**64 - 1, cases.UNTOUCHED
QUERIES, CANDIDATES = (b"abc", b"abd", b""), (b"abc", b"xabdx", b"b", b"", b"aabbccdd")
TEXT = b"xxabcxxabdxxaxbxcxxabxxxxbdxxabcabdxxxxx"
K, LIMIT, BOUND, NDIM, PADDING = 2, 3, 1, 8, 3
CAPACITY = max(map(len, QUERIES)) + max(map(len, CANDIDATES))  # what `align` picks when nobody says
FORMS = ("none", "numpy", "host-tensor", "device-tensor", "padded-numpy", "padded-device-tensor")


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return szs.DeviceScope(gpu_device=0)


@pytest.fixture(scope="module")
def engines(gpu):
    return szs.LevenshteinDistances(capabilities=gpu), szs.Fingerprints(NDIM, capabilities=gpu)


# ---- the models ---------------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _lev(a, b):
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        diagonal, row[0] = row[0], i
        for j, y in enumerate(b, 1):
            diagonal, row[j] = row[j], min(diagonal + (x != y), row[j] + 1, row[j - 1] + 1)
    return row[-1]


def _matrix(queries, candidates):
    return np.array([[_lev(q, c) for c in candidates] for q in queries], dtype=np.uint64).reshape(len(queries), len(candidates))


def _best(matrix, k):
    """The k smallest cells a row, ties to the lower column -> (indices, cells); missing slots (2^64 - 1, 0)."""
    rows, columns = matrix.shape
    indices, cells = np.full((rows, k), EMPTY, np.uint64), np.zeros((rows, k), np.uint64)
    for q in range(rows):
        order = sorted(range(columns), key=lambda c: (int(matrix[q, c]), c))[:k]
        indices[q, :len(order)], cells[q, :len(order)] = order, matrix[q, order]
    return indices, cells


def _listed(matrix, indices):
    return np.array([[matrix[q, int(c)] for c in row] for q, row in enumerate(indices)], dtype=np.uint64).reshape(indices.shape)


def _scripts(queries, candidates, indices, capacity):
    distances, lengths = np.zeros(indices.shape, np.uint64), np.zeros(indices.shape, np.uint64)
    ops = np.zeros(indices.shape + (capacity,), np.uint8)
    for q, row in enumerate(indices):
        for r, c in enumerate(row):
            distances[q, r], script = alignment_cases.canonical_script(queries[q], candidates[int(c)])
            lengths[q, r], ops[q, r, :len(script)] = len(script), np.frombuffer(script, np.uint8)
    return distances, lengths, ops


def _start_of(query, text, end, distance):
    return next(start for start in range(end, -1, -1) if _lev(query, text[start:end]) == distance)  # the shortest such match


def _columns(queries, text, found, limit, starts):
    """(counts, distances[, starts], ends) of the (end, distance) lists `found` holds per query; the slots behind hold 2^64 - 1."""
    counts = np.array([len(hits) for hits in found], np.uint64)
    distances, begins, ends = (np.full((len(queries), limit), EMPTY, np.uint64) for _ in range(3))
    for q, hits in enumerate(found):
        for slot, (end, distance) in enumerate(hits[:limit]):
            distances[q, slot], ends[q, slot], begins[q, slot] = distance, end, _start_of(queries[q], text, end, distance)
    return (counts, distances, begins, ends) if starts else (counts, distances, ends)


# ---- the methods: name -> (call(out), the members of `out` as (kind, columns), what it must return, the rows of `out`) ----------------
# kinds: "vector" (rows,), "matrix" (rows, columns) with a row stride, "dense" the same without one, "ops" (rows, K, CAPACITY) bytes,
# "counts32" (rows, columns) 4-byte cells with a row stride of their own


def _methods(engines, queries, candidates, limit, side=lambda strings, which: szs.Strs(strings), pad=0):
    """`side` makes what is passed for a list of strings; `pad`: the indices a call TAKES are cut from a matrix `pad` cells wider."""
    engine, rows, text = engines[0], len(queries), TEXT
    Q, C = side(queries, "queries"), side(candidates, "candidates")
    matrix, dense = _matrix(queries, candidates), cases.dense(list(queries), list(candidates))
    top = _best(matrix, K)
    indices = np.full((rows, K + pad), SENTINEL, np.uint64)[:, :K]
    indices[:] = top[0]
    found = _best(dense[0], K)[0]
    scan = [cases.spans(q, [text]) for q in queries]
    scan = tuple(np.array([int(triple[part][0]) for triple in scan], np.uint64) for part in range(3))
    fuzzy = cases.expected_fuzzy_within(dense, BOUND, limit)

    def matrices(count, columns=K, counts=False):
        return (("vector", 0),) * counts + (("matrix", columns),) * count

    methods = {
        "top_k": (lambda out: engine.top_k(Q, C, k=K, out=out), matrices(2), top),
        "rerank": (lambda out: engine.rerank(Q, C, indices, out=out), ("matrix", K), (top[1],)),
        "fuzzy_find": (lambda out: engine.fuzzy_find(Q, C, indices, out=out), matrices(2), (_listed(dense[0], indices), _listed(dense[2], indices))),
        "fuzzy_find-starts": (lambda out: engine.fuzzy_find(Q, C, indices, out=out, starts=True), matrices(3),
                              tuple(_listed(part, indices) for part in dense)),
        "align": (lambda out: engine.align(Q, C, indices, out=out), matrices(2) + (("ops", K),), _scripts(queries, candidates, indices, CAPACITY)),
        "fuzzy_search": (lambda out: engine.fuzzy_search(Q, C, k=K, out=out), matrices(3), (found, _listed(dense[0], found), _listed(dense[2], found))),
        "fuzzy_search-starts": (lambda out: engine.fuzzy_search(Q, C, k=K, out=out, starts=True), matrices(4),
                                (found,) + tuple(_listed(part, found) for part in dense)),
        "within": (lambda out: engine.within(Q, C, bound=BOUND, limit=limit, out=out), matrices(2, limit, counts=True),
                   cases.expected_within(matrix, BOUND, False, limit)),
        "fuzzy_search_within": (lambda out: engine.fuzzy_search_within(Q, C, max_distance=BOUND, limit=limit, out=out),
                                matrices(3, limit, counts=True), fuzzy[:3] + fuzzy[4:]),
        "fuzzy_search_within-starts": (lambda out: engine.fuzzy_search_within(Q, C, max_distance=BOUND, limit=limit, out=out, starts=True),
                                       matrices(4, limit, counts=True), fuzzy),
        "clusters": (lambda out: engine.clusters(C, BOUND, out=out), ("vector", 0),
                     (clusters_cases.labels_of_matrix(_matrix(candidates, candidates), BOUND, False),)),
        "fuzzy_scan": (lambda out: engine.fuzzy_scan(Q, text, out=out), (("vector", 0),) * 2, (scan[0], scan[2])),
        "fuzzy_scan-starts": (lambda out: engine.fuzzy_scan(Q, text, out=out, starts=True), (("vector", 0),) * 3, scan),
        "fuzzy_scan_matches": (lambda out: engine.fuzzy_scan_matches(Q, text, BOUND, limit=limit, out=out),
                               (("vector", 0),) + (("dense", limit),) * 2,
                               _columns(queries, text, [scan_hits_of(q, text, BOUND) for q in queries], limit, False)),
        "fuzzy_scan_occurrences": (lambda out: engine.fuzzy_scan_occurrences(Q, text, BOUND, limit=limit, out=out),
                                   (("vector", 0),) + (("dense", limit),) * 3,
                                   _columns(queries, text, [occurrences_of(last_row(q, text), BOUND) for q in queries], limit, True)),
        "fuzzy_scan_occurrences-no-starts": (lambda out: engine.fuzzy_scan_occurrences(Q, text, BOUND, limit=limit, out=out, starts=False),
                                             (("vector", 0),) + (("dense", limit),) * 2,
                                             _columns(queries, text, [occurrences_of(last_row(q, text), BOUND) for q in queries], limit, False)),
    }
    return {name: method + (len(candidates) if name == "clusters" else rows,) for name, method in methods.items()}


TAKES_STRIDE = ("top_k", "rerank", "fuzzy_find", "fuzzy_find-starts", "align", "fuzzy_search", "fuzzy_search-starts", "within",
                "fuzzy_search_within", "fuzzy_search_within-starts", "Fingerprints.matches", "Fingerprints.top_k")
TAKES_INDICES = ("rerank", "fuzzy_find", "fuzzy_find-starts", "align")
BOUNDED = ("within", "fuzzy_search_within", "fuzzy_search_within-starts", "fuzzy_scan_matches", "fuzzy_scan_occurrences",
           "fuzzy_scan_occurrences-no-starts")
NAMES = ("top_k", "rerank", "fuzzy_find", "fuzzy_find-starts", "align", "fuzzy_search", "fuzzy_search-starts", "within",
         "fuzzy_search_within", "fuzzy_search_within-starts", "clusters", "fuzzy_scan", "fuzzy_scan-starts", "fuzzy_scan_matches",
         "fuzzy_scan_occurrences", "fuzzy_scan_occurrences-no-starts")
FINGERPRINT_NAMES = ("Fingerprints.matches", "Fingerprints.top_k", "Fingerprints.clusters")


@pytest.fixture(scope="module")
def hashes():
    """Hash matrices of three queries and five candidates over so few values that rows share dimensions; 0xFFFFFFFF (the hash of a text
    shorter than the window) among them."""
    rng = np.random.default_rng(8)
    queries, candidates = (rng.integers(0, 3, size=(count, NDIM)).astype(np.uint32) for count in (3, 5))
    queries[0, :2] = candidates[1, :2] = 0xFFFFFFFF
    return queries, candidates


def _fingerprint_methods(engines, query_hashes, candidate_hashes, side=lambda matrix: matrix):
    fingerprints = engines[1]
    equal = (query_hashes[:, None, :] == candidate_hashes[None, :, :]).sum(axis=2).astype(np.uint64).reshape(len(query_hashes), len(candidate_hashes))
    among = (candidate_hashes[:, None, :] == candidate_hashes[None, :, :]).sum(axis=2)
    most = _best(np.uint64(NDIM) - equal, K)
    Q, C = side(query_hashes), side(candidate_hashes)
    methods = {
        "Fingerprints.matches": (lambda out: fingerprints.matches(Q, C, out=out), ("counts32", len(candidate_hashes)), (equal.astype(np.uint32),)),
        "Fingerprints.top_k": (lambda out: fingerprints.top_k(Q, C, k=K, out=out), (("matrix", K),) * 2, (most[0], _listed(equal, most[0]))),
        "Fingerprints.clusters": (lambda out: fingerprints.clusters(C, NDIM // 2 + 1, out=out), ("vector", 0),
                                  (clusters_cases.expected_labels((among >= NDIM // 2 + 1) & ~np.eye(len(among), dtype=bool)),)),
    }
    return {name: method + (len(candidate_hashes if name.endswith("clusters") else query_hashes),) for name, method in methods.items()}


# ---- `out` in every form ------------------------------------------------------------------------------------------------------------------


def _make_out(members, rows, form):
    """-> (`out`, [(the member, what it was cut from or None)])"""
    single = isinstance(members[0], str)
    made = []
    for kind, columns in [members] if single else members:
        shape = {"vector": (rows,), "ops": (rows, K, CAPACITY)}.get(kind, (rows, columns))
        dtype = {"ops": np.uint8, "counts32": np.uint32}.get(kind, np.uint64)
        padded = form.startswith("padded") and kind in ("matrix", "ops", "counts32")
        whole = np.full(shape[:1] + (shape[1] + PADDING,) + shape[2:] if padded else shape, SENTINEL & (2**(8 * np.dtype(dtype).itemsize) - 1), dtype)
        if form.endswith("tensor"):
            whole = torch.from_numpy(whole.view({1: np.uint8, 4: np.int32, 8: np.int64}[whole.itemsize]))
            whole = whole.cuda() if "device" in form else whole
        made.append((whole[:, :shape[1]] if padded else whole, whole if padded else None))
    return (made[0][0] if single else tuple(member for member, _ in made)), made


def _host(array, like):
    array = array.cpu().numpy() if isinstance(array, torch.Tensor) else np.asarray(array)
    return array.view(like.dtype) if array.dtype.itemsize == like.dtype.itemsize else array


def _check(name, call, members, want, rows, form):
    single = isinstance(members[0], str)
    if form == "none":
        got = call(None)
    else:
        out, made = _make_out(members, rows, form)
        got = call(out)
    if name.endswith("clusters"):  # (labels, count)
        assert got[1] == len(set(want[0].tolist())), (name, form)
        got = got[0]
    if form != "none":
        assert got is out, (name, form)  # a given `out` is what comes back
    got = (got,) if single or name.endswith("clusters") else got
    assert len(got) == len(want), (name, form)
    for position, (g, w) in enumerate(zip(got, want)):
        if g is None and w.size == 0:  # `align` with capacity 0
            continue
        g = _host(g, w)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, form, position, g, w)
    if form.startswith("padded"):
        for member, whole in made:
            if whole is not None:
                beside = _host(whole, np.zeros(0, np.uint8))[:, member.shape[1]:]
                assert beside.size and (beside == beside.dtype.type(SENTINEL & (2**(8 * beside.itemsize) - 1))).all(), (name, form)


def _forms(name):
    return [form for form in FORMS if not form.startswith("padded") or name in TAKES_STRIDE]


@pytest.mark.parametrize("name, form", [(name, form) for name in NAMES for form in _forms(name)])
def test_every_form_of_out(engines, name, form):
    padded = form.startswith("padded") and name in TAKES_INDICES  # the results share the row stride of the indices
    _check(name, *_methods(engines, QUERIES, CANDIDATES, LIMIT, pad=PADDING if padded else 0)[name], form)


@pytest.mark.parametrize("name, form", [(name, form) for name in FINGERPRINT_NAMES for form in _forms(name)])
def test_every_form_of_out_of_the_fingerprint_searches(engines, hashes, name, form):
    _check(name, *_fingerprint_methods(engines, *hashes)[name], form)


def test_padded_indices_without_out_give_dense_results(engines):
    for name in TAKES_INDICES:
        _check(name, *_methods(engines, QUERIES, CANDIDATES, LIMIT, pad=PADDING)[name], "none")


# ---- the inputs in every form -------------------------------------------------------------------------------------------------------------


def _mixed(strings, which):
    return szs.Strs(strings, wide_offsets=which == "queries")


def _mixed_the_other_way(strings, which):
    return szs.Strs(strings, wide_offsets=which == "candidates")


def _on_device(strings, which):
    return szs.Strs(strings).to_device(0)


def _plain_list(strings, which):
    return list(strings)


@pytest.mark.parametrize("side", [_mixed, _mixed_the_other_way, _on_device, _plain_list], ids=lambda side: side.__name__.strip("_"))
@pytest.mark.parametrize("name", NAMES)
def test_every_form_of_the_strings(engines, name, side):
    method = _methods(engines, QUERIES, CANDIDATES, LIMIT, side=side)[name]
    _check(name, *method, "none")
    _check(name, *method, "numpy")


@pytest.mark.parametrize("name", NAMES)
def test_a_single_query(engines, name):
    """One row: its stride says nothing, so a matrix cut from a wider one is as good as any."""
    for form in _forms(name):
        padded = form.startswith("padded") and name in TAKES_INDICES
        _check(name, *_methods(engines, QUERIES[:1], CANDIDATES, LIMIT, pad=PADDING if padded else 0)[name], form)


@pytest.mark.parametrize("name", FINGERPRINT_NAMES)
def test_fingerprint_hashes_in_every_form(engines, hashes, name):
    sides = {"numpy": lambda matrix: matrix, "host-tensor": lambda matrix: torch.from_numpy(matrix.view(np.int32)),
             "device-tensor": lambda matrix: torch.from_numpy(matrix.view(np.int32)).cuda(),
             "padded": lambda matrix: np.concatenate([matrix, matrix], axis=1)[:, :NDIM]}
    for side in sides.values():
        method = _fingerprint_methods(engines, *hashes, side=side)[name]
        _check(name, *method, "none")
        _check(name, *method, "device-tensor")
    if not name.endswith("clusters"):  # a single query
        for form in _forms(name):
            _check(name, *_fingerprint_methods(engines, hashes[0][:1], hashes[1])[name], form)


@pytest.mark.parametrize("name", BOUNDED)
def test_limit_zero_counts_only(engines, name):
    call, members, want, rows = _methods(engines, QUERIES, CANDIDATES, 0)[name]
    assert all(part.shape == (rows, 0) for part in want[1:])
    for form in ("none", "numpy", "device-tensor"):
        _check(name, call, members, want, rows, form)
    if not name.startswith("fuzzy_scan"):  # the matrices may be left out altogether
        counts = np.zeros(len(QUERIES), np.uint64)
        assert call((counts,) + (None,) * (len(members) - 1))[0] is counts and np.array_equal(counts, want[0])


def test_text_in_every_form(engines):
    forms = (bytearray(TEXT), memoryview(TEXT), np.frombuffer(TEXT, np.uint8), torch.from_numpy(np.frombuffer(TEXT, np.uint8).copy()),
             torch.from_numpy(np.frombuffer(TEXT, np.uint8).copy()).cuda())
    engine = engines[0]
    for name in ("fuzzy_scan", "fuzzy_scan_matches", "fuzzy_scan_occurrences"):
        want = _methods(engines, QUERIES, CANDIDATES, LIMIT)[name][2]
        for text in forms:
            got = engine.fuzzy_scan(list(QUERIES), text) if name == "fuzzy_scan" else getattr(engine, name)(list(QUERIES), text, BOUND, limit=LIMIT)
            assert cases.same(got, want), (name, type(text))

"""The argument checks of every method of the Python binding that sits on the shared helpers (`_array_facts`, `_listed_cells`,
`_vector_cells`, `_integer`, `_text_bytes`, ...): one table, every method, every kind of flaw - and the ordering rule from both sides.
A flawed argument is a `ValueError` before the method needs a scope, a handle or a GPU; a well-formed call gets past every check and
fails on the missing scope of an engine that has none, with `AttributeError` and with nothing else.  Runs anywhere.

Before the methods shared their helpers, `top_k`, `clusters`, `Fingerprints.matches`, `Fingerprints.top_k` and `Fingerprints.clusters`
resolved the scope BEFORE they looked at `out`: on an engine without one, every flawed `out` of those five (the cases whose id
starts with one of `SCOPE_CAME_FIRST`) was an accidental `AttributeError` there, as was a list or a 1-tuple as `out` of a `top_k` on
a real engine.  All other cases hold on either side of that change."""
import numpy as np
import pytest
import torch

import stringzilla_amd as szs

from host_fakes import _no_gpu_engine

SCOPE_CAME_FIRST = ("top_k-out", "clusters-out", "Fingerprints.matches-out", "Fingerprints.top_k-out", "Fingerprints.clusters-out")

QUERIES, CANDIDATES, TEXT = ["abc", "abd"], ["abx", "b", "abcd"], b"xxabcxxabdxxaxbxcxxabxxxxbdxxabcabdxxxxx"
ROWS, K, LIMIT, CAPACITY, NDIM = 2, 2, 3, 5, 8
INDICES = np.zeros((ROWS, K), np.uint64)
HASHES, OTHER_HASHES = np.zeros((ROWS, NDIM), np.uint32), np.zeros((3, NDIM), np.uint32)


def _fingerprints():
    engine = object.__new__(szs.Fingerprints)  # no handle, no scope, no GPU
    engine.ndim = NDIM
    return engine


# ---- what an `out` member looks like when it is right, and every way it can be wrong ---------------------------------------------------
# a member is (kind, columns, required): "vector" of ROWS cells, "matrix" (ROWS, columns) with a row stride, "dense" the same without
# one, "ops" the (ROWS, K, CAPACITY) bytes of `align`, "counts32" the (ROWS, columns) 4-byte matrix of `Fingerprints.matches`


def _good(kind, columns):
    if kind == "vector":
        return np.zeros(ROWS, np.uint64)
    if kind == "ops":
        return np.zeros((ROWS, K, CAPACITY), np.uint8)
    return np.zeros((ROWS, columns), np.uint32 if kind == "counts32" else np.uint64)


def _flaws(kind, columns):
    if kind == "vector":
        return {"list": [0] * ROWS, "dtype": np.zeros(ROWS, np.uint32), "torch-dtype": torch.zeros(ROWS, dtype=torch.int32),
                "shape": np.zeros(ROWS + 1, np.uint64), "2d": np.zeros((ROWS, 1), np.uint64), "stride": np.zeros(2 * ROWS, np.uint64)[::2]}
    if kind == "ops":
        return {"list": [[[0] * CAPACITY] * K] * ROWS, "dtype": np.zeros((ROWS, K, CAPACITY), np.uint16),
                "shape": np.zeros((ROWS, K + 1, CAPACITY), np.uint8), "2d": np.zeros((ROWS, K * CAPACITY), np.uint8),
                "inner-stride": np.zeros((ROWS, K, 2 * CAPACITY), np.uint8)[:, :, ::2],
                "slot-stride": np.zeros((ROWS, K, CAPACITY + 3), np.uint8)[:, :, :CAPACITY],
                "row-stride": np.zeros((ROWS, K + 3, CAPACITY), np.uint8)[:, :K]}
    if kind == "counts32":
        return {"list": [[0] * columns] * ROWS, "dtype": np.zeros((ROWS, columns), np.uint64), "float": np.zeros((ROWS, columns), np.float32),
                "torch-dtype": torch.zeros((ROWS, columns), dtype=torch.float32), "shape": np.zeros((ROWS, columns + 1), np.uint32),
                "1d": np.zeros(ROWS * columns, np.uint32), "inner-stride": np.zeros((ROWS, 2 * columns), np.uint32)[:, ::2]}
    return {"list": [[0] * columns] * ROWS, "dtype": np.zeros((ROWS, columns), np.uint32),
            "torch-dtype": torch.zeros((ROWS, columns), dtype=torch.int32), "shape": np.zeros((ROWS, columns + 1), np.uint64),
            "rows": np.zeros((ROWS + 1, columns), np.uint64), "1d": np.zeros(ROWS * columns, np.uint64),
            "inner-stride": np.zeros((ROWS, 2 * columns), np.uint64)[:, ::2],
            "row-stride": np.zeros((ROWS, columns + 3), np.uint64)[:, :columns]}  # another row stride than the other matrices'


# ---- the table: (id, call(**arguments), well-formed arguments, members of `out` or one member, integers, takes a text, takes indices) -


def _engine_call(method, *positional, **fixed):
    return lambda **arguments: getattr(_no_gpu_engine(), method)(*positional, **fixed, **arguments)


def _fingerprints_call(method, *positional):
    return lambda **arguments: getattr(_fingerprints(), method)(*positional, **arguments)


def _text_call(method, **fixed):
    return lambda text=TEXT, **arguments: getattr(_no_gpu_engine(), method)(QUERIES, text, **fixed, **arguments)


def _indices_call(method, **fixed):
    return lambda indices=INDICES, **arguments: getattr(_no_gpu_engine(), method)(QUERIES, CANDIDATES, indices, **fixed, **arguments)


VECTOR, OPTIONAL, DISTANCE, ANY = ("vector", 0, True), False, (0, 2**64 - 1), (-2**63, 2**63 - 1)


def _matrices(count, columns, kind="matrix"):
    return [(kind, columns, True)] * count


TABLE = [
    ("top_k", _engine_call("top_k", QUERIES, CANDIDATES), dict(k=K), [("matrix", K, True), ("matrix", K, OPTIONAL)], dict(k=(1, 1024))),
    ("rerank", _indices_call("rerank"), dict(), ("matrix", K, True), dict()),
    ("fuzzy_find", _indices_call("fuzzy_find"), dict(), _matrices(2, K), dict()),
    ("fuzzy_find-starts", _indices_call("fuzzy_find", starts=True), dict(), _matrices(3, K), dict()),
    ("align", _indices_call("align"), dict(), _matrices(2, K) + [("ops", 0, OPTIONAL)], dict(capacity=(0, None))),
    ("fuzzy_search", _engine_call("fuzzy_search", QUERIES, CANDIDATES), dict(k=K), _matrices(3, K), dict(k=(1, 1024))),
    ("fuzzy_search-starts", _engine_call("fuzzy_search", QUERIES, CANDIDATES, starts=True), dict(k=K), _matrices(4, K), dict(k=(1, 1024))),
    ("within", _engine_call("within", QUERIES, CANDIDATES), dict(bound=1, limit=LIMIT),
     [VECTOR, ("matrix", LIMIT, True), ("matrix", LIMIT, OPTIONAL)], dict(bound=ANY, limit=(0, 65536))),
    ("fuzzy_search_within", _engine_call("fuzzy_search_within", QUERIES, CANDIDATES), dict(max_distance=1, limit=LIMIT),
     [VECTOR] + _matrices(3, LIMIT), dict(max_distance=DISTANCE, limit=(0, 65536))),
    ("fuzzy_search_within-starts", _engine_call("fuzzy_search_within", QUERIES, CANDIDATES, starts=True), dict(max_distance=1, limit=LIMIT),
     [VECTOR] + _matrices(4, LIMIT), dict(max_distance=DISTANCE, limit=(0, 65536))),
    ("clusters", _engine_call("clusters", QUERIES), dict(bound=1), VECTOR, dict(bound=ANY)),
    ("fuzzy_scan", _text_call("fuzzy_scan"), dict(), [VECTOR] * 2, dict()),
    ("fuzzy_scan-starts", _text_call("fuzzy_scan", starts=True), dict(), [VECTOR] * 3, dict()),
    ("fuzzy_scan_matches", _text_call("fuzzy_scan_matches"), dict(max_distance=1, limit=LIMIT), [VECTOR] + _matrices(2, LIMIT, "dense"),
     dict(max_distance=DISTANCE, limit=(0, 2**24))),
    ("fuzzy_scan_occurrences", _text_call("fuzzy_scan_occurrences"), dict(max_distance=1, limit=LIMIT),
     [VECTOR] + _matrices(3, LIMIT, "dense"), dict(max_distance=DISTANCE, limit=(0, 2**24))),
    ("fuzzy_scan_occurrences-no-starts", _text_call("fuzzy_scan_occurrences", starts=False), dict(max_distance=1, limit=LIMIT),
     [VECTOR] + _matrices(2, LIMIT, "dense"), dict(max_distance=DISTANCE, limit=(0, 2**24))),
    ("Fingerprints.matches", _fingerprints_call("matches", HASHES, OTHER_HASHES), dict(), ("counts32", 3, True), dict()),
    ("Fingerprints.top_k", _fingerprints_call("top_k", HASHES, OTHER_HASHES), dict(k=K), [("matrix", K, True), ("matrix", K, OPTIONAL)],
     dict(k=(1, 1024))),
    ("Fingerprints.clusters", _fingerprints_call("clusters", HASHES), dict(min_matches=1), VECTOR, dict(min_matches=DISTANCE)),
]
TAKES_TEXT = {name for name, *_ in TABLE if name.startswith("fuzzy_scan")}
TAKES_INDICES = ("rerank", "fuzzy_find", "fuzzy_find-starts", "align")


def _good_out(members):
    return _good(*members[:2]) if isinstance(members, tuple) else tuple(_good(kind, columns) for kind, columns, _ in members)


def _refused():
    """(id, call, arguments) of every flawed call of the table."""
    for name, call, good, members, integers in TABLE:
        single = isinstance(members, tuple)
        for position, (kind, columns, required) in enumerate([members] if single else members):
            flaws = dict(_flaws(kind, columns))
            if required and not single:
                flaws["none"] = None
            for flaw, member in flaws.items():
                out = list(_good_out([members] if single else members))
                out[position] = member
                yield f"{name}-out{position}-{flaw}", call, dict(good, out=out[0] if single else tuple(out))
        if not single:  # the wrong kind of thing, and the wrong number of members
            outs = {"list": [0] * len(members), "array": _good(*members[-1][:2]), "short": _good_out(members)[:1],
                    "long": _good_out(members) + (_good(*members[-1][:2]), _good(*members[-1][:2]))}
            if name.endswith("top_k"):
                del outs["long"]  # (a `top_k` has always looked at the first two members of whatever it is given)
            for flaw, out in outs.items():
                yield f"{name}-out-{flaw}", call, dict(good, out=out)
        for argument, (low, high) in integers.items():
            values = {"bool": True, "float": 1.5, "whole-float": 2.0, "string": "1", "below": low - 1, "numpy-bool": np.True_}
            if argument != "capacity":  # (`capacity` None is "whatever fits")
                values["none"] = None
            if high is not None:
                values["above"] = high + 1
            for flaw, value in values.items():
                yield f"{name}-{argument}-{flaw}", call, dict(good, **{argument: value})
        if name in TAKES_TEXT:
            texts = {"str": "abc", "list": [97, 98], "none": None, "int8": np.zeros(4, np.int8), "uint16": np.zeros(4, np.uint16),
                     "2d": np.zeros((2, 2), np.uint8), "strided": np.zeros(8, np.uint8)[::2], "torch-int8": torch.zeros(4, dtype=torch.int8),
                     "torch-2d": torch.zeros((2, 2), dtype=torch.uint8), "torch-strided": torch.zeros(8, dtype=torch.uint8)[::2]}
            for flaw, text in texts.items():
                yield f"{name}-text-{flaw}", call, dict(good, text=text)
        if name in TAKES_INDICES:
            for flaw, indices in dict(_flaws("matrix", K), rows=np.zeros((ROWS + 1, K), np.uint64)).items():
                if flaw not in ("row-stride", "shape"):  # (alone, padded or wider indices are fine: the results take their stride and k)
                    yield f"{name}-indices-{flaw}", call, dict(good, indices=indices)


REFUSED = list(_refused())


@pytest.mark.parametrize("call, arguments", [case[1:] for case in REFUSED], ids=[case[0] for case in REFUSED])
def test_flawed_arguments_are_refused_before_a_scope_is_needed(call, arguments):
    with pytest.raises(ValueError):
        call(**arguments)


def _accepted():
    for name, call, good, members, integers in TABLE:
        yield name, call, good
        yield name + "-out", call, dict(good, out=_good_out(members))
        if not isinstance(members, tuple) and not all(required for _, _, required in members):
            yield name + "-out-without-the-optional", call, dict(good, out=tuple(
                _good(kind, columns) if required else None for kind, columns, required in members))
        for argument, (low, high) in integers.items():
            for value in (low, np.int64(max(low, 0))) + (() if high is None else (high,)):
                if argument not in ("limit", "k", "capacity"):  # (those size the `out` the other cases pass)
                    yield f"{name}-out-{argument}-{value!r}", call, dict(good, out=_good_out(members), **{argument: value})
                else:
                    yield f"{name}-{argument}-{value!r}", call, dict(good, **{argument: value})
        if name in TAKES_TEXT:
            for form, text in (("bytearray", bytearray(TEXT)), ("memoryview", memoryview(TEXT)), ("numpy", np.frombuffer(TEXT, np.uint8)),
                               ("torch", torch.zeros(9, dtype=torch.uint8)), ("empty", b"")):
                yield f"{name}-text-{form}", call, dict(good, text=text)
        if name in TAKES_INDICES:
            padded = np.zeros((ROWS, K + 3), np.uint64)[:, :K]
            yield name + "-padded-indices", call, dict(good, indices=padded)
            yield name + "-torch-indices", call, dict(good, indices=torch.zeros((ROWS, K), dtype=torch.int64))


ACCEPTED = list(_accepted())


@pytest.mark.parametrize("call, arguments", [case[1:] for case in ACCEPTED], ids=[case[0] for case in ACCEPTED])
def test_well_formed_arguments_pass_every_check_and_stop_at_the_missing_scope(call, arguments):
    with pytest.raises(AttributeError, match="_scope"):
        call(**arguments)


def test_align_takes_its_capacity_from_out_and_zero_needs_no_ops():
    matrices = lambda: (np.zeros((ROWS, K), np.uint64), np.zeros((ROWS, K), np.uint64))  # noqa: E731
    with pytest.raises(AttributeError, match="_scope"):
        _no_gpu_engine().align(QUERIES, CANDIDATES, INDICES, capacity=0, out=matrices() + (None,))
    with pytest.raises(AttributeError, match="_scope"):
        _no_gpu_engine().align(QUERIES, CANDIDATES, INDICES, capacity=CAPACITY, out=matrices() + (np.zeros((ROWS, K, CAPACITY), np.uint8),))
    with pytest.raises(ValueError):
        _no_gpu_engine().align(QUERIES, CANDIDATES, INDICES, capacity=CAPACITY, out=matrices() + (None,))
    with pytest.raises(ValueError):
        _no_gpu_engine().align(QUERIES, CANDIDATES, INDICES, capacity=CAPACITY + 1, out=matrices() + (np.zeros((ROWS, K, CAPACITY), np.uint8),))
    with pytest.raises(ValueError):
        _no_gpu_engine().align(QUERIES, CANDIDATES, INDICES, starts=INDICES)  # `starts` without `ends`


def test_limit_zero_takes_none_or_empty_matrices():
    counts = np.zeros(ROWS, np.uint64)
    for empty in (None, np.zeros((ROWS, 0), np.uint64)):
        with pytest.raises(AttributeError, match="_scope"):
            _no_gpu_engine().within(QUERIES, CANDIDATES, bound=1, limit=0, out=(counts, empty, empty))
    with pytest.raises(ValueError):
        _no_gpu_engine().within(QUERIES, CANDIDATES, bound=1, limit=0, out=(counts, np.zeros((ROWS, 1), np.uint64), None))
    with pytest.raises(AttributeError, match="_scope"):
        _no_gpu_engine().fuzzy_scan_matches(QUERIES, TEXT, 1, limit=0, out=(counts,) + (np.zeros((ROWS, 0), np.uint64),) * 2)
    with pytest.raises(ValueError):
        _no_gpu_engine().fuzzy_scan_matches(QUERIES, TEXT, 1, limit=0, out=(counts, None, None))

#!/usr/bin/env python3
"""Times fuzzy find with spans (`engine.fuzzy_find(..., starts=True)`, szs_rocm_fuzzy_find_spans*) beside the
plain call on one GPU.  One JSON line per leg; the legs, inputs and seeds are scripts/measure_fuzzy_find.py's.

  listed    (a) 65,536 queries x k = 16 of 16,384 candidates, `std::mt19937_64` U[96, 160] printable ASCII.
  documents (b) 256 patterns of U[16, 64] bytes, dense (`indices=None`), against 1,024 documents of U[1024, 3072] bytes.

Each leg runs once through `fuzzy_find` and once with `starts=True`: one warm-up, then `--repeats` synchronous calls.  Wall time = a
host clock around the call after a device synchronise, the best of them; kernel time = the library's event pair around its launches
(`last_call_profile`) - both launches of the spans call sit inside one pair - the best of the repeats, and the last one's as
measure_fuzzy_find.py reports it.  The line gives the ratio of the two kernel times.  Every leg is verified in the run that times
it: `--checked` of its pairs - distance, start and end - against the plain DP below, the plain call's distances and ends bit-equal
to the spans call's, launches (1 and 2), pairs and cells against the host's sums.  Any mismatch ends the run with a non-zero exit
status.  `--record FILE` appends every line to FILE as well (profiles/rNN/measure_fuzzy_spans.jsonl).
"""
import argparse
import json
import os
import sys
import time

parser = argparse.ArgumentParser()
parser.add_argument("--legs", default="listed,documents")
parser.add_argument("--repeats", type=int, default=5)
parser.add_argument("--many", type=int, default=65536, help="queries of leg (a)")
parser.add_argument("--corpus", type=int, default=16384, help="candidates of leg (a)")
parser.add_argument("--k", type=int, default=16)
parser.add_argument("--patterns", type=int, default=256, help="queries of leg (b)")
parser.add_argument("--documents", type=int, default=1024, help="candidates of leg (b)")
parser.add_argument("--checked", type=int, default=512, help="pairs of each leg verified against the DP")
parser.add_argument("--record", default=None, help="a file every JSON line is appended to")
args = parser.parse_args()
legs = args.legs.split(",")
if not set(legs) <= {"listed", "documents"} or min(args.repeats, args.many, args.corpus, args.k, args.patterns, args.documents, args.checked) < 1:
    parser.error("--legs takes listed, documents; the counts must be at least 1")

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import stringzilla_amd as szs
from stringzilla_amd import workloads

K = args.k


def last_rows(pattern, texts, lengths, free_start):
    """The last row of the unit-cost DP of `pattern` against every text, column by column: yields (j, D[m][j] per text)."""
    m, rows = len(pattern), np.arange(len(pattern) + 1)
    padded = np.zeros((len(texts), max(int(lengths.max()), 1)), np.uint8)
    for at, text in enumerate(texts):
        padded[at, :len(text)] = np.frombuffer(text, np.uint8)
    column = np.tile(rows, (len(texts), 1))
    for j in range(1, int(lengths.max()) + 1):
        step = np.full_like(column, 0 if free_start else j)
        step[:, 1:] = np.minimum(column[:, :-1] + (pattern[None, :] != padded[:, j - 1, None]), column[:, 1:] + 1)
        column = np.minimum.accumulate(step - rows, axis=1) + rows
        yield j, column[:, m]


def spans(query, texts):
    """(distances, starts, ends) of `query` inside every text: the semi-global DP (D[0][j] = 0), then the global DP of the reversed
    query over c[:end] reversed - start = end - the smallest t whose lev(q, c[end - t : end]) is the distance."""
    m, pattern = len(query), np.frombuffer(query, np.uint8)
    lengths = np.array([len(text) for text in texts], dtype=np.int64)
    best, end = np.full(len(texts), m, np.int64), np.zeros(len(texts), np.int64)
    for j, last in last_rows(pattern, texts, lengths, True):
        better = (j <= lengths) & (last < best)
        best[better], end[better] = last[better], j
    heads = [text[:int(e)][::-1] for text, e in zip(texts, end)]
    least, back = np.full(len(texts), m, np.int64), np.zeros(len(texts), np.int64)
    for t, last in last_rows(pattern[::-1], heads, end, False):
        better = (t <= end) & (last < least)
        least[better], back[better] = last[better], t
    return best, end - back, end


def timed(run, repeats):
    """(best wall, median wall, best kernel, last kernel) in seconds / milliseconds of `repeats` calls after one warm-up."""
    run()  # warm-up: allocations, code objects
    walls, kernels = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        started = time.perf_counter()
        run()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - started)
        kernels.append(engine.last_call_profile().kernel_milliseconds)
    return min(walls), float(np.median(walls)), min(kernels), kernels[-1]


def tape(seed, count, shortest, longest):
    return workloads.mt19937_64_tape(seed, count, shortest, longest, workloads.ASCII_PRINTABLE).to_device(0)


def emit(line):
    print(json.dumps(line), flush=True)
    if args.record:
        os.makedirs(os.path.dirname(os.path.abspath(args.record)), exist_ok=True)
        with open(args.record, "a") as record:
            record.write(json.dumps(line) + "\n")


def against_the_dp(queries, candidates, rows, picks, got):
    """Rows `rows` of a call, slot by slot against the DP: picks[r] lists the candidates of row rows[r]; got = (distances, starts, ends)."""
    for at, row in enumerate(rows):
        want = spans(queries[int(row)], [candidates[int(index)] for index in picks[at]])
        if not all(np.array_equal(got[part][at], want[part]) for part in range(3)):
            return False
    return True


def measure(leg, queries, candidates, indices, host_indices, shape, forward_cells, rows, picks, extra):
    """Times the two calls on one set of inputs, verifies them, emits the line; the names of what did not hold."""
    out = torch.zeros((3,) + shape, dtype=torch.int64, device="cuda")
    plain_out = torch.zeros((2,) + shape, dtype=torch.int64, device="cuda")
    runs, failed = {}, []
    for name, run in (("fuzzy_find", lambda: engine.fuzzy_find(queries, candidates, indices, device=gpu, out=(plain_out[0], plain_out[1]))),
                      ("spans", lambda: engine.fuzzy_find(queries, candidates, indices, device=gpu, out=(out[0], out[1], out[2]), starts=True)),
                      ("fuzzy_find again", lambda: engine.fuzzy_find(queries, candidates, indices, device=gpu, out=(plain_out[0], plain_out[1])))):
        best, median, kernel, kernel_last = timed(run, args.repeats)
        profile = engine.last_call_profile()
        runs[name] = {"wall_ms": round(best * 1e3, 3), "median_ms": round(median * 1e3, 3), "kernel_ms": round(kernel, 4),
                      "kernel_ms_last": round(kernel_last, 4), "launches": int(profile.launches), "pairs": int(profile.pairs),
                      "cells": int(profile.cells)}
    distances, starts, ends = (matrix.cpu().numpy() for matrix in out)
    lengths = queries.lengths().astype(np.int64)[:, None]
    reverse_cells = int((lengths * np.minimum(ends, lengths + distances)).sum())
    pairs = shape[0] * shape[1]
    checks = {
        "spans == DP (distance, start, end)": against_the_dp(queries, candidates, rows, picks, tuple(
            matrix[rows[:, None], picks] if host_indices is None else matrix[rows] for matrix in (distances, starts, ends))),
        "fuzzy_find's distances and ends == the spans call's": bool(
            np.array_equal(plain_out[0].cpu().numpy(), distances) and np.array_equal(plain_out[1].cpu().numpy(), ends)),
        "start <= end and end - start <= m + d": bool((starts <= ends).all() and (ends - starts <= lengths + distances).all()),
        "launches 1 and 2": runs["fuzzy_find"]["launches"] == 1 and runs["fuzzy_find again"]["launches"] == 1 and runs["spans"]["launches"] == 2,
        "pairs == the host's": all(run["pairs"] == pairs for run in runs.values()),
        "cells == the host's": runs["fuzzy_find"]["cells"] == forward_cells and runs["spans"]["cells"] == forward_cells + reverse_cells,
    }
    plain = min(runs["fuzzy_find"], runs["fuzzy_find again"], key=lambda run: run["kernel_ms"])
    emit({"leg": leg, **extra, "pairs": pairs, "forward_cells": forward_cells, "reverse_cells": reverse_cells, **runs,
          "spans_over_fuzzy_find_kernel": round(runs["spans"]["kernel_ms"] / plain["kernel_ms"], 3) if plain["kernel_ms"] else None,
          "columns_predicted_ratio": round(1 + reverse_cells / forward_cells, 3) if forward_cells else None,
          "verified_pairs_against_dp": int(picks.size), "verified": all(checks.values())})
    return [f"{leg[:3]} {name}" for name, held in checks.items() if not held]


gpu = szs.DeviceScope(gpu_device=0)
engine = szs.LevenshteinDistances(capabilities=gpu)
mismatches = []  # the run then fails, so no figure is recorded beside a wrong result

if "listed" in legs:
    queries, candidates = tape(2002, args.many, 96, 160), tape(2001, args.corpus, 96, 160)
    host_indices = np.random.default_rng(17).integers(0, args.corpus, size=(args.many, K), dtype=np.uint64)
    indices = torch.from_numpy(host_indices.view(np.int64)).cuda()
    cells = int((queries.lengths()[:, None] * candidates.lengths()[host_indices.astype(np.int64)]).sum())
    rows = np.random.default_rng(18).choice(args.many, size=max(1, min(args.many, args.checked // K)), replace=False)
    mismatches += measure("(a) listed: rerank's leg (d) inputs through fuzzy_find and with starts", queries, candidates, indices, host_indices,
                          (args.many, K), cells, rows, host_indices[rows], {"k": K, "queries": args.many, "corpus": args.corpus})

if "documents" in legs:
    patterns, documents = tape(2005, args.patterns, 16, 64), tape(2004, args.documents, 1024, 3072)
    cells = int(patterns.lengths().sum()) * int(documents.lengths().sum())
    rng = np.random.default_rng(19)
    rows = rng.choice(args.patterns, size=max(1, min(args.patterns, args.checked // 64)), replace=False)
    picks = np.stack([rng.choice(args.documents, size=min(64, args.documents), replace=False) for _ in rows])
    mismatches += measure("(b) documents: every pattern in every document, dense, and with starts", patterns, documents, None, None,
                          (args.patterns, args.documents), cells, rows, picks, {"patterns": args.patterns, "documents": args.documents})

if mismatches:
    sys.exit("results differ: " + ", ".join(mismatches))

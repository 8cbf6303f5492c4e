#!/usr/bin/env python3
"""Times fuzzy find (`engine.fuzzy_find`, szs_rocm_fuzzy_find*) on one GPU.  One JSON line per leg.

  listed    (a) rerank's leg (d) inputs - 65,536 queries x k = 16 of 16,384 candidates, `std::mt19937_64` U[96, 160] printable ASCII -
                through fuzzy_find and, in the same run, through rerank on its kernel route.  The two kernels walk the same columns,
                so rerank's kernel time (the library's event pair) is the yardstick: the line reports the ratio.
  documents (b) what the call is for: 256 patterns of U[16, 64] bytes, dense (`indices=None`), against 1,024 documents of
                U[1024, 3072] bytes: wall time, kernel time, TCUPS.

Wall time = a host clock around the synchronous call after a device synchronise; the best of `--repeats` calls after one warm-up;
kernel time = the library's event pair around its launch (`last_call_profile`).  Every leg is verified in the run that times it:
a sample of its pairs against the plain semi-global DP below, every pair of (a) against `distance <= min(len(query), rerank's score)`
and `end <= len(candidate)`, and the profile's cells against the host's sum of m x n.  Any mismatch ends the run with a non-zero exit
status.  `--record FILE` appends every line to FILE as well (profiles/rNN/measure_fuzzy_find.jsonl).
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
from stringzilla_amd import _abi, workloads

K = args.k


def semi_global(query, texts):
    """(distances, ends) of `query` inside every text: D[0][j] = 0, D[i][0] = i, unit costs; the smallest j of the minimum of row m."""
    m, pattern, rows = len(query), np.frombuffer(query, np.uint8), np.arange(len(query) + 1)
    lengths = np.array([len(text) for text in texts])
    padded = np.zeros((len(texts), max(int(lengths.max()), 1)), np.uint8)
    for at, text in enumerate(texts):
        padded[at, :len(text)] = np.frombuffer(text, np.uint8)
    column = np.tile(rows, (len(texts), 1))
    best, end = column[:, m].copy(), np.zeros(len(texts), np.int64)
    for j in range(1, int(lengths.max()) + 1):
        step = np.zeros_like(column)
        step[:, 1:] = np.minimum(column[:, :-1] + (pattern[None, :] != padded[:, j - 1, None]), column[:, 1:] + 1)
        column = np.minimum.accumulate(step - rows, axis=1) + rows
        better = (j <= lengths) & (column[:, m] < best)
        best[better], end[better] = column[better, m], j
    return best, end


def timed(run, repeats):
    run()  # warm-up: allocations, code objects
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        started = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - started)
    return min(times), float(np.median(times))


def tape(seed, count, shortest, longest):
    return workloads.mt19937_64_tape(seed, count, shortest, longest, workloads.ASCII_PRINTABLE).to_device(0)


def emit(line):
    print(json.dumps(line), flush=True)
    if args.record:
        os.makedirs(os.path.dirname(os.path.abspath(args.record)), exist_ok=True)
        with open(args.record, "a") as record:
            record.write(json.dumps(line) + "\n")


def against_the_dp(queries, candidates, rows, picks, distances, ends):
    """Rows `rows` of a call, slot by slot against the DP: picks[r] lists the candidates of row rows[r]."""
    for at, row in enumerate(rows):
        want = semi_global(queries[int(row)], [candidates[int(index)] for index in picks[at]])
        if not (np.array_equal(distances[at], want[0]) and np.array_equal(ends[at], want[1])):
            return False
    return True


gpu = szs.DeviceScope(gpu_device=0)
engine = szs.LevenshteinDistances(capabilities=gpu)
mismatches = []  # the run then fails, so no figure is recorded beside a wrong result

if "listed" in legs:
    queries, candidates = tape(2002, args.many, 96, 160), tape(2001, args.corpus, 96, 160)
    host_indices = np.random.default_rng(17).integers(0, args.corpus, size=(args.many, K), dtype=np.uint64)
    indices = torch.from_numpy(host_indices.view(np.int64)).cuda()
    cells = int((queries.lengths()[:, None] * candidates.lengths()[host_indices.astype(np.int64)]).sum())
    out = torch.zeros((2, args.many, K), dtype=torch.int64, device="cuda")
    scores = torch.zeros((args.many, K), dtype=torch.int64, device="cuda")
    runs = {}
    _abi.tuning_set("rerank", None)
    for name, run in (("fuzzy_find", lambda: engine.fuzzy_find(queries, candidates, indices, device=gpu, out=(out[0], out[1]))),
                      ("rerank", lambda: engine.rerank(queries, candidates, indices, device=gpu, out=scores)),
                      ("fuzzy_find again", lambda: engine.fuzzy_find(queries, candidates, indices, device=gpu, out=(out[0], out[1])))):
        best, median = timed(run, args.repeats)
        profile = engine.last_call_profile()
        runs[name] = {"wall_ms": round(best * 1e3, 3), "median_ms": round(median * 1e3, 3), "kernel_ms": round(profile.kernel_milliseconds, 4),
                      "launches": int(profile.launches), "profile_cells_match": bool(profile.cells == cells),
                      "profile_pairs_match": bool(profile.pairs == args.many * K)}
    distances, ends = out[0].cpu().numpy(), out[1].cpu().numpy()
    globally = scores.cpu().numpy()
    bounded = bool((distances <= np.minimum(queries.lengths()[:, None].astype(np.int64), globally)).all()
                   and (ends <= candidates.lengths()[host_indices.astype(np.int64)].astype(np.int64)).all())
    rows = np.random.default_rng(18).choice(args.many, size=max(1, min(args.many, args.checked // K)), replace=False)
    same = against_the_dp(queries, candidates, rows, host_indices[rows], distances[rows], ends[rows])
    fuzzy = min(runs["fuzzy_find"], runs["fuzzy_find again"], key=lambda run: run["kernel_ms"])
    emit({"leg": "(a) listed: rerank's leg (d) inputs through fuzzy_find and through rerank", "k": K, "queries": args.many, "corpus": args.corpus,
          "pairs": args.many * K, "cells": cells, **runs,
          "fuzzy_find_over_rerank_kernel": round(fuzzy["kernel_ms"] / runs["rerank"]["kernel_ms"], 3) if runs["rerank"]["kernel_ms"] else None,
          "fuzzy_find_kernel_tcups": round(cells / (fuzzy["kernel_ms"] * 1e-3) / 1e12, 4) if fuzzy["kernel_ms"] else None,
          "rerank_kernel_tcups": round(cells / (runs["rerank"]["kernel_ms"] * 1e-3) / 1e12, 4) if runs["rerank"]["kernel_ms"] else None,
          "verified_pairs_against_dp": int(len(rows) * K), "verified": bool(same), "within_min_of_m_and_rerank": bounded})
    if not same:
        mismatches.append("(a) fuzzy_find==DP")
    if not bounded:
        mismatches.append("(a) distance<=min(m, rerank), end<=n")
    if not all(run["profile_cells_match"] and run["profile_pairs_match"] for run in runs.values()):
        mismatches.append("(a) profile cells and pairs==the host's")

if "documents" in legs:
    patterns, documents = tape(2005, args.patterns, 16, 64), tape(2004, args.documents, 1024, 3072)
    cells = int(patterns.lengths().sum()) * int(documents.lengths().sum())
    out = torch.zeros((2, args.patterns, args.documents), dtype=torch.int64, device="cuda")
    best, median = timed(lambda: engine.fuzzy_find(patterns, documents, device=gpu, out=(out[0], out[1])), args.repeats)
    profile = engine.last_call_profile()
    distances, ends = out[0].cpu().numpy(), out[1].cpu().numpy()
    rng = np.random.default_rng(19)
    rows = rng.choice(args.patterns, size=max(1, min(args.patterns, args.checked // 64)), replace=False)
    picks = np.stack([rng.choice(args.documents, size=min(64, args.documents), replace=False) for _ in rows])
    same = against_the_dp(patterns, documents, rows, picks, distances[rows[:, None], picks], ends[rows[:, None], picks])
    emit({"leg": "(b) documents: every pattern in every document, dense", "patterns": args.patterns, "documents": args.documents,
          "pairs": args.patterns * args.documents, "cells": cells, "wall_ms": round(best * 1e3, 3), "median_ms": round(median * 1e3, 3),
          "kernel_ms": round(profile.kernel_milliseconds, 4), "launches": int(profile.launches),
          "tcups_by_wall": round(cells / best / 1e12, 4),
          "tcups_by_kernel": round(cells / (profile.kernel_milliseconds * 1e-3) / 1e12, 4) if profile.kernel_milliseconds else None,
          "profile_cells_match": bool(profile.cells == cells), "verified_pairs_against_dp": int(picks.size), "verified": bool(same)})
    if not same:
        mismatches.append("(b) fuzzy_find==DP")
    if profile.cells != cells or profile.pairs != args.patterns * args.documents:
        mismatches.append("(b) profile cells and pairs==the host's")

if mismatches:
    sys.exit("results differ: " + ", ".join(mismatches))

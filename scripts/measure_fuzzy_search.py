#!/usr/bin/env python3
"""Times fuzzy search (`engine.fuzzy_search`, szs_rocm_fuzzy_search*) on one GPU.  One JSON line per leg.

  documents (b') section 4.9 leg (b)'s inputs and seeds - 256 patterns of U[16, 64] bytes in 1,024 documents of U[1024, 3072] bytes -
                 at k = 16, and in the same run the dense `fuzzy_find` call over the same strings: the scoring kernels walk the same
                 columns, so the dense call's kernel time (the library's event pair) is the yardstick; the line reports the ratio.
  corpus    (c)  64 patterns of U[16, 64] bytes in 2^20 documents of U[96, 160] bytes at k = 16: no baseline (the dense call's outputs
                 would be 1 GiB); kernel time, wall time, TCUPS.

Wall time = a host clock around the synchronous call after a device synchronise; the best of `--repeats` calls after one warm-up;
kernel time = the library's event pairs around its scoring launches (`last_call_profile`).  Every leg is verified in the run that
times it.  (b'): the search's rows against a stable sort of the dense call's own matrix - every row, exactly - and 512 pairs of that
matrix against the plain semi-global DP below.  (c): 512 listed pairs (distance and end) against the DP, and 512 sampled
(row, candidate) pairs that the rows do NOT list: none may beat the row's k-th (distance, index).  The profile's pairs and cells are
checked against the host's.  Any mismatch ends the run with a non-zero exit status.  `--record FILE` appends every line to FILE as
well (profiles/rNN/measure_fuzzy_search.jsonl).
"""
import argparse
import json
import os
import sys
import time

parser = argparse.ArgumentParser()
parser.add_argument("--legs", default="documents,corpus")
parser.add_argument("--repeats", type=int, default=5)
parser.add_argument("--k", type=int, default=16)
parser.add_argument("--patterns", type=int, default=256, help="queries of leg (b')")
parser.add_argument("--documents", type=int, default=1024, help="candidates of leg (b')")
parser.add_argument("--few", type=int, default=64, help="queries of leg (c)")
parser.add_argument("--corpus", type=int, default=1 << 20, help="candidates of leg (c)")
parser.add_argument("--checked", type=int, default=512, help="pairs of each kind verified against the DP")
parser.add_argument("--record", default=None, help="a file every JSON line is appended to")
args = parser.parse_args()
legs = args.legs.split(",")
if not set(legs) <= {"documents", "corpus"} or min(args.repeats, args.k, args.patterns, args.documents, args.few, args.corpus, args.checked) < 1:
    parser.error("--legs takes documents, corpus; the counts must be at least 1")
if args.k > min(args.documents, args.corpus):
    parser.error("--k must not exceed the candidates of a leg")

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


def figures(best, median, profile):
    return {"wall_ms": round(best * 1e3, 3), "median_ms": round(median * 1e3, 3), "kernel_ms": round(profile.kernel_milliseconds, 4),
            "launches": int(profile.launches)}


gpu = szs.DeviceScope(gpu_device=0)
engine = szs.LevenshteinDistances(capabilities=gpu)
mismatches = []  # the run then fails, so no figure is recorded beside a wrong result
for knob in ("top_k_tile", "fuzzy_search_segment"):
    _abi.tuning_set(knob, None)

if "documents" in legs:
    patterns, documents = tape(2005, args.patterns, 16, 64), tape(2004, args.documents, 1024, 3072)
    cells = int(patterns.lengths().sum()) * int(documents.lengths().sum())
    found = torch.zeros((3, args.patterns, K), dtype=torch.int64, device="cuda")
    matrix = torch.zeros((2, args.patterns, args.documents), dtype=torch.int64, device="cuda")
    runs = {}
    for name, run in (("fuzzy_search", lambda: engine.fuzzy_search(patterns, documents, k=K, device=gpu, out=tuple(found))),
                      ("dense fuzzy_find", lambda: engine.fuzzy_find(patterns, documents, device=gpu, out=(matrix[0], matrix[1]))),
                      ("fuzzy_search again", lambda: engine.fuzzy_search(patterns, documents, k=K, device=gpu, out=tuple(found)))):
        best, median = timed(run, args.repeats)
        profile = engine.last_call_profile()
        searched = name != "dense fuzzy_find"
        pairs = args.patterns * args.documents + (args.patterns * K if searched else 0)
        runs[name] = {**figures(best, median, profile), "profile_pairs_match": bool(profile.pairs == pairs), "profile_cells": int(profile.cells)}
    indices, distances, ends = (part.cpu().numpy() for part in found)
    winners_cells = int((patterns.lengths()[:, None] * documents.lengths()[indices]).sum())  # the winners pass scores the listed pairs again
    for name, run in runs.items():
        run["profile_cells_match"] = bool(run.pop("profile_cells") == cells + (winners_cells if name != "dense fuzzy_find" else 0))
    dense_distances, dense_ends = matrix[0].cpu().numpy(), matrix[1].cpu().numpy()
    order = np.argsort(dense_distances, axis=1, kind="stable")[:, :K]  # ties to the lower index
    at_rows = np.arange(args.patterns)[:, None]
    selected = bool(np.array_equal(indices, order) and np.array_equal(distances, dense_distances[at_rows, order])
                    and np.array_equal(ends, dense_ends[at_rows, order]))
    rng = np.random.default_rng(19)
    rows = rng.choice(args.patterns, size=max(1, min(args.patterns, args.checked // 64)), replace=False)
    picks = np.stack([rng.choice(args.documents, size=min(64, args.documents), replace=False) for _ in rows])
    same = against_the_dp(patterns, documents, rows, picks, dense_distances[rows[:, None], picks], dense_ends[rows[:, None], picks])
    block, tile, segment, workgroups = _abi.fuzzy_search_probe(args.patterns, args.documents, K)
    search = min(runs["fuzzy_search"], runs["fuzzy_search again"], key=lambda run: run["kernel_ms"])
    dense = runs["dense fuzzy_find"]
    emit({"leg": "(b') documents: the k best documents per pattern, and the dense fuzzy_find call in the same run", "k": K,
          "patterns": args.patterns, "documents": args.documents, "pairs": args.patterns * args.documents, "cells": cells,
          "tile": tile, "segment": segment, "workgroups": workgroups, **runs,
          "search_over_dense_kernel": round(search["kernel_ms"] / dense["kernel_ms"], 3) if dense["kernel_ms"] else None,
          "search_over_dense_wall": round(search["wall_ms"] / dense["wall_ms"], 3) if dense["wall_ms"] else None,
          "search_kernel_tcups": round(cells / (search["kernel_ms"] * 1e-3) / 1e12, 4) if search["kernel_ms"] else None,
          "dense_kernel_tcups": round(cells / (dense["kernel_ms"] * 1e-3) / 1e12, 4) if dense["kernel_ms"] else None,
          "rows_equal_the_sorted_dense_matrix": selected, "verified_pairs_against_dp": int(picks.size), "verified": bool(same)})
    if not selected:
        mismatches.append("(b') fuzzy_search==stable sort of the dense matrix")
    if not same:
        mismatches.append("(b') fuzzy_find==DP")
    if not all(run["profile_cells_match"] and run["profile_pairs_match"] for run in runs.values()):
        mismatches.append("(b') profile cells and pairs==the host's")

if "corpus" in legs:
    patterns, corpus = tape(2007, args.few, 16, 64), tape(2006, args.corpus, 96, 160)
    cells = int(patterns.lengths().sum()) * int(corpus.lengths().sum())
    found = torch.zeros((3, args.few, K), dtype=torch.int64, device="cuda")
    best, median = timed(lambda: engine.fuzzy_search(patterns, corpus, k=K, device=gpu, out=tuple(found)), args.repeats)
    profile = engine.last_call_profile()
    indices, distances, ends = (part.cpu().numpy() for part in found)
    rng = np.random.default_rng(23)
    slots = max(1, min(K, args.checked // args.few))  # 512 listed pairs: the first `slots` of every row
    every = np.arange(args.few)
    listed = against_the_dp(patterns, corpus, every, indices[:, :slots], distances[:, :slots], ends[:, :slots])
    ascending = bool(((distances[:, 1:] > distances[:, :-1]) |
                      ((distances[:, 1:] == distances[:, :-1]) & (indices[:, 1:] > indices[:, :-1]))).all())  # ties: the lower index first
    rows = rng.choice(args.few, size=max(1, min(args.few, args.checked // 64)), replace=False)
    unbeaten = True
    for row in rows:  # candidates the row does not list: none beats its k-th (distance, index)
        others = np.setdiff1d(rng.choice(args.corpus, size=min(64, args.corpus), replace=False), indices[row].astype(np.int64))
        theirs, _ = semi_global(patterns[int(row)], [corpus[int(index)] for index in others])
        last_distance, last_index = int(distances[row, K - 1]), int(indices[row, K - 1])
        unbeaten = unbeaten and bool(((theirs > last_distance) | ((theirs == last_distance) & (others > last_index))).all())
    block, tile, segment, workgroups = _abi.fuzzy_search_probe(args.few, args.corpus, K)
    pairs = args.few * args.corpus + args.few * K
    winners_cells = int((patterns.lengths()[:, None] * corpus.lengths()[indices]).sum())
    emit({"leg": "(c) corpus: the k best documents per pattern, no baseline", "k": K, "patterns": args.few, "documents": args.corpus,
          "pairs": args.few * args.corpus, "cells": cells, "tile": tile, "segment": segment, "workgroups": workgroups,
          **figures(best, median, profile), "tcups_by_wall": round(cells / best / 1e12, 4),
          "tcups_by_kernel": round(cells / (profile.kernel_milliseconds * 1e-3) / 1e12, 4) if profile.kernel_milliseconds else None,
          "profile_pairs_match": bool(profile.pairs == pairs), "profile_cells_match": bool(profile.cells == cells + winners_cells),
          "verified_listed_pairs_against_dp": int(args.few * slots), "verified": bool(listed), "rows_ascend": ascending,
          "verified_unlisted_pairs_against_dp": int(len(rows) * 64), "none_beats_the_kth": bool(unbeaten)})
    if not (listed and ascending and unbeaten):
        mismatches.append("(c) listed pairs==DP, rows ascend, no unlisted candidate beats the k-th")
    if profile.pairs != pairs or profile.cells != cells + winners_cells:
        mismatches.append("(c) profile cells and pairs==the host's")

if mismatches:
    sys.exit("results differ: " + ", ".join(mismatches))

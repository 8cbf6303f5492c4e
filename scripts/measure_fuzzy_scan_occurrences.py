#!/usr/bin/env python3
"""Times fuzzy scan occurrences (`engine.fuzzy_scan_occurrences`, szs_rocm_fuzzy_scan_occurrences*) beside
fuzzy scan matches on one GPU, in ONE process.  One JSON line.

The input is section 4.12's own (scripts/measure_fuzzy_scan_matches.py builds the same bytes): 256 patterns of U[16, 64] bytes in ONE
16 MiB std::mt19937_64 ASCII text with 4096 planted copies under 0 to 3 edits, `max_distance` 2.  Five legs, the best of `--repeats`
calls each after one warm-up:

  matches count       `fuzzy_scan_matches(limit=0)`                      the baseline of the forward legs: its code is section 4.12's
  matches write       `fuzzy_scan_matches(limit=64)`
  occurrences count   `fuzzy_scan_occurrences(limit=0)`
  occurrences write   `fuzzy_scan_occurrences(limit=64, starts=False)`
  occurrences starts  `fuzzy_scan_occurrences(limit=64, starts=True)`

Checked in the same run, and the exit status is non-zero otherwise: every reported (end, distance) is a hit of `fuzzy_scan_matches` for
the same bound with the same distance (both calls again with a `--subset-limit` that holds every hit), the ends ascend, the slots
behind min(count, limit) are all ones, the three forms agree on counts, distances and ends, every start lies within m + distance bytes
of its end, and - for `--sampled` patterns, on the CPU - every reported span is the shortest window ending there at that distance.

Wall time = a host clock around the synchronous call after a device synchronise; kernel time = the library's event pair
(`last_call_profile`).  `--record FILE` appends the line to FILE as well (profiles/rNN/measure_fuzzy_scan_occurrences.jsonl).
"""
import argparse
import json
import os
import sys
import time

parser = argparse.ArgumentParser()
parser.add_argument("--repeats", type=int, default=5)
parser.add_argument("--patterns", type=int, default=256)
parser.add_argument("--text", type=int, default=16 << 20, help="bytes of the text")
parser.add_argument("--planted", type=int, default=4096, help="mutated copies of patterns written into the text")
parser.add_argument("--sampled", type=int, default=8, help="patterns whose spans are verified on the CPU")
parser.add_argument("--subset-limit", type=int, default=1024, help="slots a row of the run that checks the subset property")
parser.add_argument("--record", default=None, help="a file the JSON line is appended to")
args = parser.parse_args()
if min(args.repeats, args.patterns, args.text, args.sampled, args.subset_limit) < 1 or args.planted < 0 or args.text >= 1 << 32:
    parser.error("the counts must be at least 1, a text has less than 4 GiB")

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
import torch

import stringzilla_amd as szs
from stringzilla_amd import _abi, workloads

EMPTY = np.uint64(2**64 - 1)
BOUND, LIMIT = 2, 64


def global_row(query, window):
    """lev(query, window[len(window) - t:]) for t = 0 ... len(window): the bottom row of the global DP of both reversed."""
    backwards = window[::-1]
    column = list(range(len(query) + 1))
    row = [len(query)]
    for t, symbol in enumerate(backwards, 1):
        diagonal, column[0] = column[0], t
        for i, wanted in enumerate(reversed(query), 1):
            diagonal, column[i] = column[i], min(diagonal + (wanted != symbol), column[i] + 1, column[i - 1] + 1)
        row.append(column[-1])
    return row


def timed(run, repeats):
    run()  # warm-up: allocations, code objects
    times, kernels = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        started = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - started)
        kernels.append(engine.last_call_profile().kernel_milliseconds)
    return {"wall_ms": round(min(times) * 1e3, 3), "median_ms": round(float(np.median(times)) * 1e3, 3),
            "kernel_ms": round(min(kernels), 4), "kernel_median_ms": round(float(np.median(kernels)), 4),
            "kernel_worst_ms": round(max(kernels), 4), "launches": int(engine.last_call_profile().launches),
            "cells": int(engine.last_call_profile().cells)}


gpu = szs.DeviceScope(gpu_device=0)
engine = szs.LevenshteinDistances(capabilities=gpu)
_abi.tuning_set("fuzzy_scan_piece", None)

# section 4.12's input, the same bytes: the text and patterns of section 4.11 (a), then the planted copies
n = args.text
host_patterns = workloads.mt19937_64_tape(2105, args.patterns, 16, 64, workloads.ASCII_PRINTABLE)
patterns = host_patterns.to_device(0)
lengths = patterns.lengths()
host_text = workloads.mt19937_64_tape(2104, 1, n, n, workloads.ASCII_PRINTABLE).data[:n].copy()
rng = np.random.default_rng(416)
letters = np.frombuffer(bytes(range(32, 127)), np.uint8)
for _ in range(args.planted):
    copy = bytearray(host_patterns[int(rng.integers(args.patterns))])
    for _ in range(int(rng.integers(0, 4))):
        kind, at = int(rng.integers(3)), int(rng.integers(len(copy)))
        if kind == 0:
            copy[at] = int(rng.choice(letters))
        elif kind == 1 and len(copy) > 1:
            del copy[at]
        else:
            copy.insert(at, int(rng.choice(letters)))
    at = int(rng.integers(0, n - len(copy)))
    host_text[at:at + len(copy)] = np.frombuffer(bytes(copy), np.uint8)
text = torch.from_numpy(host_text).cuda()
sampled = sorted(int(q) for q in rng.choice(args.patterns, size=min(args.sampled, args.patterns), replace=False))
piece, pieces, workgroups, _ = _abi.fuzzy_scan_probe(args.patterns, int(lengths.max()), n)
warm_ups = {int(m): sum(min(p * piece, 2 * int(m)) for p in range(pieces)) for m in set(int(m) for m in lengths)}
walked_matches = sum(int(m) * (n + warm_ups[int(m)]) for m in lengths)
walked_occurrences = sum(int(m) * (n + warm_ups[int(m)] + pieces - 1) for m in lengths)  # one tail column a piece but the last


def matrices(count, limit):
    return tuple(torch.zeros((args.patterns, limit), dtype=torch.int64, device="cuda") for _ in range(count))


def vector():
    return torch.zeros(args.patterns, dtype=torch.int64, device="cuda")


def host(arrays):
    return [array.cpu().numpy().view(np.uint64) for array in arrays]


legs = {}
out_hits_0, out_hits = (vector(),) + matrices(2, 0), (vector(),) + matrices(2, LIMIT)
legs["matches count"] = timed(lambda: engine.fuzzy_scan_matches(patterns, text, BOUND, limit=0, device=gpu, out=out_hits_0), args.repeats)
legs["matches write"] = timed(lambda: engine.fuzzy_scan_matches(patterns, text, BOUND, limit=LIMIT, device=gpu, out=out_hits), args.repeats)
out_0, out_3, out_4 = (vector(),) + matrices(3, 0), (vector(),) + matrices(2, LIMIT), (vector(),) + matrices(3, LIMIT)
legs["occurrences count"] = timed(lambda: engine.fuzzy_scan_occurrences(patterns, text, BOUND, limit=0, device=gpu, out=out_0), args.repeats)
legs["occurrences write"] = timed(
    lambda: engine.fuzzy_scan_occurrences(patterns, text, BOUND, limit=LIMIT, starts=False, device=gpu, out=out_3), args.repeats)
legs["occurrences starts"] = timed(lambda: engine.fuzzy_scan_occurrences(patterns, text, BOUND, limit=LIMIT, device=gpu, out=out_4), args.repeats)

# ---- the checks -----------------------------------------------------------------------------------------------------------------
mismatches = []
counts_0 = host(out_0[:1])[0]
counts_3, distances_3, ends_3 = host(out_3)
counts, distances, starts, ends = host(out_4)
hit_counts = host(out_hits_0[:1])[0]
if not (np.array_equal(counts_0, counts_3) and np.array_equal(counts_0, counts) and np.array_equal(distances_3, distances)
        and np.array_equal(ends_3, ends)):
    mismatches.append("the three forms agree on counts, distances and ends")
if legs["occurrences count"]["cells"] != walked_occurrences or legs["matches count"]["cells"] != walked_matches:
    mismatches.append("profile cells==the walked bytes of one pass")
if not (counts <= hit_counts).all():
    mismatches.append("no more occurrences than hits")

# the subset property, with a capacity that holds every hit of every row
wide = args.subset_limit
all_hits = engine.fuzzy_scan_matches(patterns, text, BOUND, limit=wide, device=gpu)  # (returned arrays are NumPy's)
all_found = engine.fuzzy_scan_occurrences(patterns, text, BOUND, limit=wide, starts=False, device=gpu)
subset = bool(int(all_hits[0].max()) <= wide)  # else the capacity was too small to check anything: a failure, not a pass
for q in range(args.patterns):
    hits = {(int(j), int(d)) for j, d in zip(all_hits[2][q, :int(all_hits[0][q])], all_hits[1][q, :int(all_hits[0][q])])}
    kept = int(all_found[0][q])
    subset = subset and {(int(j), int(d)) for j, d in zip(all_found[2][q, :kept], all_found[1][q, :kept])} <= hits
    subset = subset and bool(np.array_equal(all_found[2][q, :min(kept, LIMIT)], ends[q, :min(kept, LIMIT)]))
if not subset:
    mismatches.append("every occurrence is a hit of fuzzy_scan_matches with the same distance")

shaped = True
for q in range(args.patterns):
    kept, m = int(min(int(counts[q]), LIMIT)), int(lengths[q])
    shaped = shaped and all(bool((matrix[q, kept:] == EMPTY).all()) for matrix in (distances, starts, ends))
    shaped = shaped and bool((np.diff(ends[q, :kept].astype(np.int64)) > 0).all())
    taken = ends[q, :kept].astype(np.int64) - starts[q, :kept].astype(np.int64)
    shaped = shaped and bool((np.abs(taken - m) <= distances[q, :kept].astype(np.int64)).all() and (distances[q, :kept] <= BOUND).all())
if not shaped:
    mismatches.append("ascending ends, empty slots behind them, starts within m + distance of their ends")

spans, spans_checked = True, 0
for q in sampled:
    query = bytes(host_patterns[q])
    for d, s, e in zip(distances[q], starts[q], ends[q]):
        if e == EMPTY:
            break
        window = min(int(e), len(query) + int(d))
        row = global_row(query, bytes(host_text[int(e) - window:int(e)]))
        spans = spans and row[int(e) - int(s)] == int(d) and int(d) not in row[:int(e) - int(s)]
        spans_checked += 1
if not spans:
    mismatches.append("every sampled span is the shortest window ending there at its distance")


def ratio(leg, baseline):
    return round(legs[leg]["kernel_ms"] / legs[baseline]["kernel_ms"], 4) if legs[baseline]["kernel_ms"] else None


line = {"input": {"patterns": args.patterns, "text_bytes": n, "planted": args.planted, "max_distance": BOUND, "limit": LIMIT, "piece": piece,
                  "pieces": pieces, "workgroups": workgroups, "cells": int(lengths.sum()) * n, "walked_cells_one_pass_matches": walked_matches,
                  "walked_cells_one_pass_occurrences": walked_occurrences},
        "legs": legs,
        "occurrences_count_over_matches_count_kernel": ratio("occurrences count", "matches count"),
        "occurrences_write_over_matches_write_kernel": ratio("occurrences write", "matches write"),
        "starts_add_kernel_ms": round(legs["occurrences starts"]["kernel_ms"] - legs["occurrences write"]["kernel_ms"], 4),
        "hits": int(hit_counts.sum()), "occurrences": int(counts.sum()), "rows_with_occurrences": int((counts > 0).sum()),
        "largest_count": int(counts.max()), "rows_above_the_limit": int((counts > LIMIT).sum()),
        "sampled_patterns": sampled, "sampled_spans_checked": spans_checked, "mismatches": mismatches}
print(json.dumps(line), flush=True)
if args.record:
    os.makedirs(os.path.dirname(os.path.abspath(args.record)), exist_ok=True)
    with open(args.record, "a") as record:
        record.write(json.dumps(line) + "\n")
if mismatches:
    sys.exit("results differ: " + ", ".join(mismatches))

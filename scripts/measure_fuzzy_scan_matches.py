#!/usr/bin/env python3
"""Times fuzzy scan matches (`engine.fuzzy_scan_matches`, szs_rocm_fuzzy_scan_matches*) on one GPU.  One JSON
line per leg; run ONE leg per process, each GPU step under its own time limit, chained with `&&` (profiles/r16/README.md has the lines).

  count  (a) section 4.11 (a)'s input - 256 patterns of U[16, 64] bytes in ONE 16 MiB std::mt19937_64 ASCII text - with a few thousand
             mutated copies of the patterns planted, so that hits are rare; `max_distance` 2, `limit` 0: the count and the offsets
             alone.  The counts of 8 sampled patterns are checked against the plain DP on the CPU over the WHOLE text.
  write  (a) the same call with `limit` 64: what the fills and the write pass add.  Every reported (end, distance) of the 8 sampled
             patterns is checked against the DP of the window that ends there, the counts against the `count` leg's rule.
  scan   (a) `fuzzy_scan` on the same input.  Run it with `--package` naming a checkout of the PARENT commit, built in a directory of
             its own: that build is the baseline of the `count` leg, this one is not.
  dense  (b) the same text with `max_distance` 64, `limit` 64: every column is a hit for most patterns, only each row's first chunk
             writes.  No baseline; recorded as measured.  Reported hits of the 8 sampled patterns against the window DP.

Wall time = a host clock around the synchronous call after a device synchronise; the best of `--repeats` calls after one warm-up;
kernel time = the library's event pair (`last_call_profile`).  Any mismatch ends the run with a non-zero exit status.  `--record FILE`
appends every line to FILE as well (profiles/rNN/measure_fuzzy_scan_matches.jsonl).
"""
import argparse
import json
import os
import sys
import time

parser = argparse.ArgumentParser()
parser.add_argument("--legs", default="count")
parser.add_argument("--repeats", type=int, default=5)
parser.add_argument("--patterns", type=int, default=256)
parser.add_argument("--text", type=int, default=16 << 20, help="bytes of the text")
parser.add_argument("--planted", type=int, default=4096, help="mutated copies of patterns written into the text")
parser.add_argument("--sampled", type=int, default=8, help="patterns verified against the plain DP")
parser.add_argument("--package", default=None, help="the root of the checkout whose stringzilla_amd is measured (default: this one)")
parser.add_argument("--record", default=None, help="a file every JSON line is appended to")
args = parser.parse_args()
legs = args.legs.split(",")
if not set(legs) <= {"count", "write", "scan", "dense"} or min(args.repeats, args.patterns, args.text, args.sampled) < 1 or args.planted < 0:
    parser.error("--legs takes count, write, scan, dense; the counts must be at least 1")
if args.text >= 1 << 32:
    parser.error("a text has less than 4 GiB")

root = os.path.abspath(args.package) if args.package else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
import torch

import stringzilla_amd as szs
from stringzilla_amd import _abi, workloads

if os.path.dirname(os.path.dirname(os.path.abspath(szs.__file__))) != root:
    sys.exit(f"stringzilla_amd came from {szs.__file__}, not from {root}")
EMPTY = np.uint64(2**64 - 1)


def last_row(query, text):
    """D[m][j], j = 0 ... n, of the unit-cost DP with a free start in `text` (a uint8 array): row by row over the whole text - the
    insertions along a row are a running minimum of (value - j) - with no window and no bit-vector."""
    n = len(text)
    columns = np.arange(n + 1, dtype=np.int32)
    row = np.zeros(n + 1, dtype=np.int32)
    for i, wanted in enumerate(np.frombuffer(query, np.uint8), 1):
        step = np.empty(n + 1, dtype=np.int32)
        step[0] = i
        np.minimum(row[:-1] + (text != wanted), row[1:] + 1, out=step[1:])
        step -= columns
        np.minimum.accumulate(step, out=step)
        step += columns
        row = step
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
            "launches": int(engine.last_call_profile().launches)}


def emit(line):
    print(json.dumps(line), flush=True)
    if args.record:
        os.makedirs(os.path.dirname(os.path.abspath(args.record)), exist_ok=True)
        with open(args.record, "a") as record:
            record.write(json.dumps(line) + "\n")


gpu = szs.DeviceScope(gpu_device=0)
engine = szs.LevenshteinDistances(capabilities=gpu)
mismatches = []  # the run then fails, so no figure is recorded beside a wrong result
_abi.tuning_set("fuzzy_scan_piece", None)

# the input of every leg, the same bytes in every process: section 4.11 (a)'s text and patterns, then the planted copies
n = args.text
host_patterns = workloads.mt19937_64_tape(2105, args.patterns, 16, 64, workloads.ASCII_PRINTABLE)
patterns = host_patterns.to_device(0)
lengths = patterns.lengths()
host_text = workloads.mt19937_64_tape(2104, 1, n, n, workloads.ASCII_PRINTABLE).data[:n].copy()
rng = np.random.default_rng(416)
letters = np.frombuffer(bytes(range(32, 127)), np.uint8)
for _ in range(args.planted):  # 0 to 3 edits: most copies are within a bound of 2, some are just beyond it
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
walked = sum(int(m) * (n + sum(min(p * piece, 2 * int(m)) for p in range(pieces))) for m in lengths)
shape = {"patterns": args.patterns, "text_bytes": n, "planted": args.planted, "cells": int(lengths.sum()) * n, "piece": piece, "pieces": pieces,
         "workgroups": workgroups, "walked_cells_one_pass": walked}


def windows_hold(counts, distances, ends, bound, limit):
    """Every reported (end, distance) of the sampled patterns against the DP of the window that ends there (a start within 2 m bytes
    attains D[m][j]); the ends ascend; the slots behind min(count, limit) are empty."""
    good = True
    for q in sampled:
        query, kept = host_patterns[q], int(min(int(counts[q]), limit))
        m = len(query)
        good = good and bool((distances[q, kept:] == EMPTY).all() and (ends[q, kept:] == EMPTY).all())
        good = good and bool((np.diff(ends[q, :kept].astype(np.int64)) > 0).all())
        for d, e in zip(distances[q, :kept], ends[q, :kept]):
            first = max(0, int(e) - 3 * m)
            good = good and 1 <= int(e) <= n and int(d) <= bound and int(last_row(query, host_text[first:int(e)])[-1]) == int(d)
    return good


if "count" in legs:
    counted = torch.zeros(args.patterns, dtype=torch.int64, device="cuda")
    empty = torch.zeros((args.patterns, 0), dtype=torch.int64, device="cuda")
    count = timed(lambda: engine.fuzzy_scan_matches(patterns, text, 2, limit=0, device=gpu, out=(counted, empty, empty)), args.repeats)
    cells = int(engine.last_call_profile().cells)
    counts = counted.cpu().numpy().view(np.uint64)
    started = time.perf_counter()
    agree = all(int((last_row(host_patterns[q], host_text)[1:] <= 2).sum()) == int(counts[q]) for q in sampled)
    emit({"leg": "(a) count: max_distance 2, limit 0", **shape, "fuzzy_scan_matches": count, "profile_cells": cells,
          "profile_cells_match": bool(cells == walked), "hits": int(counts.sum()), "rows_with_hits": int((counts > 0).sum()),
          "largest_count": int(counts.max()), "sampled_patterns": sampled, "counts_match_the_whole_text_dp": bool(agree),
          "dp_seconds": round(time.perf_counter() - started, 1),
          "kernel_tcups": round(shape["cells"] / (count["kernel_ms"] * 1e-3) / 1e12, 4) if count["kernel_ms"] else None})
    if not agree:
        mismatches.append("(a) counts==the plain DP over the whole text")
    if cells != walked:
        mismatches.append("(a) profile cells==the walked bytes of one pass")

for leg, bound in (("write", 2), ("dense", 64)):
    if leg not in legs:
        continue
    limit = 64
    out = (torch.zeros(args.patterns, dtype=torch.int64, device="cuda"), torch.zeros((args.patterns, limit), dtype=torch.int64, device="cuda"),
           torch.zeros((args.patterns, limit), dtype=torch.int64, device="cuda"))
    written = timed(lambda: engine.fuzzy_scan_matches(patterns, text, bound, limit=limit, device=gpu, out=out), args.repeats)
    cells = int(engine.last_call_profile().cells)
    counts, distances, ends = (array.cpu().numpy().view(np.uint64) for array in out)
    again = timed(lambda: engine.fuzzy_scan_matches(patterns, text, bound, limit=0, device=gpu, out=(out[0], out[1][:, :0], out[2][:, :0])), args.repeats)
    same_counts = bool(np.array_equal(counts, out[0].cpu().numpy().view(np.uint64)))
    good = windows_hold(counts, distances, ends, bound, limit)
    every_column = int((counts == n).sum())
    emit({"leg": f"({'a' if leg == 'write' else 'b'}) {leg}: max_distance {bound}, limit {limit}", **shape, "fuzzy_scan_matches": written,
          "the same call with limit 0, same process": again,
          "write_adds_kernel_ms": round(written["kernel_ms"] - again["kernel_ms"], 4),
          "write_over_count_kernel": round(written["kernel_ms"] / again["kernel_ms"], 4) if again["kernel_ms"] else None,
          "profile_cells": cells, "cells_over_one_pass": round(cells / walked, 4), "hits": int(counts.sum()),
          "rows_with_hits": int((counts > 0).sum()), "rows_above_the_limit": int((counts > limit).sum()), "rows_with_every_column_a_hit": every_column,
          "sampled_patterns": sampled, "reported_hits_match_their_window_dp": bool(good), "counts_match_the_counting_form": same_counts})
    if not good:
        mismatches.append(f"({leg}) every reported (end, distance) is the DP's in the window that ends there")
    if not same_counts:
        mismatches.append(f"({leg}) the counts of limit 64 and of limit 0 agree")

if "scan" in legs:
    scanned = torch.zeros((2, args.patterns), dtype=torch.int64, device="cuda")
    scan = timed(lambda: engine.fuzzy_scan(patterns, text, device=gpu, out=tuple(scanned)), args.repeats)
    cells = int(engine.last_call_profile().cells)
    distances = scanned[0].cpu().numpy()
    emit({"leg": "(a) scan: fuzzy_scan on the same input", "package": args.package or ".", **shape, "fuzzy_scan": scan, "profile_cells": cells,
          "profile_cells_match": bool(cells == walked), "rows_within_2": int((distances <= 2).sum())})
    if cells != walked:
        mismatches.append("(scan) profile cells==the walked bytes")

if mismatches:
    sys.exit("results differ: " + ", ".join(mismatches))

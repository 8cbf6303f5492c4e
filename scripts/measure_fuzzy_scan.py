#!/usr/bin/env python3
"""Times fuzzy scan (`engine.fuzzy_scan`, szs_rocm_fuzzy_scan*) on one GPU.  One JSON line per leg; run one
leg per process (`--legs text16` / `--legs text256`).

  text16  (a) 256 patterns of U[16, 64] bytes in ONE 16 MiB std::mt19937_64 ASCII text, three ways in the same run:
              `fuzzy_scan`; the one-lane route `fuzzy_find(patterns, [text])`, unchanged code - the baseline; and the workaround a user
              had before: overlapping copies of 4096 + 512 bytes through `fuzzy_search(k=1)`, chunk offsets mapped back on the host.
              All three must agree on every (distance, end).
  text256 (b) 4 patterns in a 256 MiB text, `fuzzy_scan` only; 512 windows of the text - the one that ends at each reported end, and
              sampled ones elsewhere - against the plain DP: the reported (distance, end) is attained, and no window beats it.

Wall time = a host clock around the synchronous call after a device synchronise; the best of `--repeats` calls after one warm-up;
kernel time = the library's event pair (`last_call_profile`): for `fuzzy_scan` the scan, its emit and the memset between the events,
for `fuzzy_find` its one launch, for `fuzzy_search` its scoring launches (not its folds, not its winners pass).  Any mismatch ends the
run with a non-zero exit status.  `--record FILE` appends every line to FILE as well (profiles/rNN/measure_fuzzy_scan.jsonl).
"""
import argparse
import json
import os
import sys
import time

parser = argparse.ArgumentParser()
parser.add_argument("--legs", default="text16")
parser.add_argument("--repeats", type=int, default=5)
parser.add_argument("--baseline-repeats", type=int, default=None, help="calls of the one-lane baseline (default: --repeats)")
parser.add_argument("--patterns", type=int, default=256, help="queries of leg (a)")
parser.add_argument("--text", type=int, default=16 << 20, help="bytes of leg (a)'s text")
parser.add_argument("--few", type=int, default=4, help="queries of leg (b)")
parser.add_argument("--long-text", type=int, default=256 << 20, help="bytes of leg (b)'s text")
parser.add_argument("--checked", type=int, default=512, help="windows of leg (b) verified against the DP")
parser.add_argument("--record", default=None, help="a file every JSON line is appended to")
args = parser.parse_args()
legs = args.legs.split(",")
if not set(legs) <= {"text16", "text256"} or min(args.repeats, args.patterns, args.text, args.few, args.long_text, args.checked) < 1:
    parser.error("--legs takes text16, text256; the counts must be at least 1")
if max(args.text, args.long_text) >= 1 << 32:
    parser.error("a text has less than 4 GiB")

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import stringzilla_amd as szs
from stringzilla_amd import _abi, workloads

CHUNK, OVERLAP = 4096, 512  # the workaround's copies: 4096 own bytes behind 512 = 2 x the longest query's that came before


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


def one_text(seed, n):
    """`n` bytes of std::mt19937_64 printable ASCII: a tape of one string."""
    return workloads.mt19937_64_tape(seed, 1, n, n, workloads.ASCII_PRINTABLE).data[:n]


gpu = szs.DeviceScope(gpu_device=0)
engine = szs.LevenshteinDistances(capabilities=gpu)
mismatches = []  # the run then fails, so no figure is recorded beside a wrong result
for knob in ("top_k_tile", "fuzzy_search_segment", "fuzzy_scan_piece"):
    _abi.tuning_set(knob, None)

if "text16" in legs:
    n = args.text
    patterns = workloads.mt19937_64_tape(2105, args.patterns, 16, 64, workloads.ASCII_PRINTABLE).to_device(0)
    host_text = one_text(2104, n)
    text = torch.from_numpy(host_text).cuda()
    lengths = patterns.lengths()
    piece, pieces, workgroups, _ = _abi.fuzzy_scan_probe(args.patterns, int(lengths.max()), n)

    scanned = torch.zeros((2, args.patterns), dtype=torch.int64, device="cuda")
    scan = timed(lambda: engine.fuzzy_scan(patterns, text, device=gpu, out=tuple(scanned)), args.repeats)
    scan_cells = int(engine.last_call_profile().cells)
    walked = sum(int(m) * (n + sum(min(p * piece, 2 * int(m)) for p in range(pieces))) for m in lengths)

    whole = szs.Strs.from_device(text, torch.tensor([0, n], dtype=torch.int64 if n >= 1 << 31 else torch.int32, device="cuda"))
    if patterns.wide_offsets != whole.wide_offsets:
        sys.exit("the text's tape and the patterns' must share an offset width")
    found = torch.zeros((2, args.patterns, 1), dtype=torch.int64, device="cuda")
    find = timed(lambda: engine.fuzzy_find(patterns, whole, device=gpu, out=tuple(found)), args.baseline_repeats or args.repeats)

    # the workaround: chunk c is text[max(0, c x 4096 - 512) : (c + 1) x 4096]; the lowest chunk that attains the distance owns its end
    begins = np.maximum(np.arange(0, n, CHUNK, dtype=np.int64) - OVERLAP, 0)
    finishes = np.minimum(np.arange(0, n, CHUNK, dtype=np.int64) + CHUNK, n)
    offsets = np.zeros(len(begins) + 1, dtype=np.uint32)
    np.cumsum(finishes - begins, out=offsets[1:])
    gather = np.arange(int(offsets[-1]), dtype=np.int64) + np.repeat(begins - offsets[:-1].astype(np.int64), finishes - begins)
    chunks = szs.Strs.from_tape(host_text[gather], offsets).to_device(0)
    searched = torch.zeros((3, args.patterns, 1), dtype=torch.int64, device="cuda")
    search = timed(lambda: engine.fuzzy_search(patterns, chunks, k=1, device=gpu, out=tuple(searched)), args.repeats)
    chunk_index, chunk_distance, chunk_end = (part[:, 0].cpu().numpy() for part in searched)
    mapped_end = np.where(chunk_end > 0, begins[chunk_index] + chunk_end, 0)

    scan_distance, scan_end = (part.cpu().numpy() for part in scanned)
    find_distance, find_end = (part[:, 0].cpu().numpy() for part in found)
    agree_find = bool(np.array_equal(scan_distance, find_distance) and np.array_equal(scan_end, find_end))
    agree_search = bool(np.array_equal(scan_distance, chunk_distance) and np.array_equal(scan_end, mapped_end))
    cells = int(lengths.sum()) * n
    emit({"leg": "(a) one 16 MiB text: fuzzy_scan, the one-lane fuzzy_find baseline, and overlapping chunks through fuzzy_search(k=1)",
          "patterns": args.patterns, "text_bytes": n, "cells": cells, "piece": piece, "pieces": pieces, "workgroups": workgroups,
          "fuzzy_scan": scan, "fuzzy_find one lane a query": find, "fuzzy_search of chunks": {**search, "chunks": len(begins)},
          "scan_over_find_kernel": round(scan["kernel_ms"] / find["kernel_ms"], 5) if find["kernel_ms"] else None,
          "scan_over_search_kernel": round(scan["kernel_ms"] / search["kernel_ms"], 4) if search["kernel_ms"] else None,
          "scan_over_search_wall": round(scan["wall_ms"] / search["wall_ms"], 4) if search["wall_ms"] else None,
          "scan_kernel_tcups": round(cells / (scan["kernel_ms"] * 1e-3) / 1e12, 4) if scan["kernel_ms"] else None,
          "profile_cells_match": bool(scan_cells == walked), "agrees_with_fuzzy_find": agree_find, "agrees_with_chunks": agree_search})
    if not agree_find:
        mismatches.append("(a) fuzzy_scan==fuzzy_find")
    if not agree_search:
        mismatches.append("(a) fuzzy_scan==chunks through fuzzy_search")
    if scan_cells != walked:
        mismatches.append("(a) profile cells==the walked bytes")

if "text256" in legs:
    n = args.long_text
    patterns = workloads.mt19937_64_tape(2107, args.few, 16, 64, workloads.ASCII_PRINTABLE).to_device(0)
    host_text = one_text(2106, n)
    text = torch.from_numpy(host_text).cuda()
    lengths = patterns.lengths()
    piece, pieces, workgroups, _ = _abi.fuzzy_scan_probe(args.few, int(lengths.max()), n)
    scanned = torch.zeros((2, args.few), dtype=torch.int64, device="cuda")
    scan = timed(lambda: engine.fuzzy_scan(patterns, text, device=gpu, out=tuple(scanned)), args.repeats)
    distances, ends = (part.cpu().numpy() for part in scanned)
    rng = np.random.default_rng(29)
    per_pattern = max(1, args.checked // args.few)
    attained, unbeaten = True, True
    for q in range(args.few):
        query, d, e = patterns[q], int(distances[q]), int(ends[q])
        m = len(query)
        # the window that ends at the reported end: a start within 2 m bytes attains d there, and no earlier exact column does
        first = max(0, e - 2 * m - CHUNK)
        window_d, window_e = semi_global(query, [host_text[first:e].tobytes()])
        attained = attained and (int(window_d[0]), first + int(window_e[0])) == (d, e)
        # sampled windows elsewhere: a DP that starts later sees no less than the true one, so none may beat (d, e)
        starts = rng.integers(0, max(1, n - CHUNK - 2 * m), size=per_pattern - 1)
        their_d, their_e = semi_global(query, [host_text[s:s + CHUNK + 2 * m].tobytes() for s in starts])
        for s, wd, we in zip(starts, their_d, their_e):
            unbeaten = unbeaten and (int(wd), int(s) + int(we)) >= (d, e)
    cells = int(lengths.sum()) * n
    emit({"leg": "(b) one 256 MiB text: fuzzy_scan only", "patterns": args.few, "text_bytes": n, "cells": cells, "piece": piece,
          "pieces": pieces, "workgroups": workgroups, "fuzzy_scan": scan,
          "scan_kernel_tcups": round(cells / (scan["kernel_ms"] * 1e-3) / 1e12, 4) if scan["kernel_ms"] else None,
          "verified_windows_against_dp": int(args.few * per_pattern), "reported_is_attained": bool(attained), "none_beats_it": bool(unbeaten)})
    if not (attained and unbeaten):
        mismatches.append("(b) the reported (distance, end) is attained in its window, and no sampled window beats it")

if mismatches:
    sys.exit("results differ: " + ", ".join(mismatches))

#!/usr/bin/env python3
"""Times alignments (`engine.align`, szs_rocm_alignments*) behind fuzzy find with spans on one GPU.  One JSON
line per leg; the legs, inputs and seeds are scripts/measure_fuzzy_spans.py's.

  listed    (a) 65,536 queries x k = 16 of 16,384 candidates, `std::mt19937_64` U[96, 160] printable ASCII.
  documents (b) 256 patterns of U[16, 64] bytes, dense (`indices=None`), against 1,024 documents of U[1024, 3072] bytes.

Each leg runs `fuzzy_find`, `fuzzy_find(starts=True)` and then `align` on the spans that call returned: one warm-up, then `--repeats`
synchronous calls each.  Kernel time = the library's event pair around its launches (`last_call_profile`), the best of the repeats;
wall time = a host clock around the call after a device synchronise.  The YARDSTICK of `align` is the spans call's reverse pass in
the same run - its kernel time less the plain call's: `align` walks the same columns, stores two dwords a word and column on top, and
then takes about m + t dependent steps per pair.  The line gives that ratio.  Every leg is verified in the run that times it:
`--checked` of its pairs - distance, length and every op with the zeros behind them - against the canonical script of the plain DP
(tests/alignment_cases.py), the distances against fuzzy find's, launches, pairs and cells against the host's sums.  Any mismatch ends
the run with a non-zero exit status.  `--record FILE` appends every line to FILE as well (profiles/rNN/measure_alignments.jsonl).
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]  # the canonical script is the tests': one definition
import numpy as np
import torch

import alignment_cases
import stringzilla_amd as szs
from stringzilla_amd import workloads

K = args.k


def timed(run, repeats):
    """(best wall in seconds, best kernel, last kernel in milliseconds) of `repeats` calls after one warm-up."""
    run()  # warm-up: allocations, code objects
    walls, kernels = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        started = time.perf_counter()
        run()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - started)
        kernels.append(engine.last_call_profile().kernel_milliseconds)
    return min(walls), min(kernels), kernels[-1]


def tape(seed, count, shortest, longest):
    return workloads.mt19937_64_tape(seed, count, shortest, longest, workloads.ASCII_PRINTABLE).to_device(0)


def emit(line):
    print(json.dumps(line), flush=True)
    if args.record:
        os.makedirs(os.path.dirname(os.path.abspath(args.record)), exist_ok=True)
        with open(args.record, "a") as record:
            record.write(json.dumps(line) + "\n")


def against_the_dp(queries, candidates, rows, picks, starts, ends, got, capacity):
    """Rows `rows` of the call against the canonical scripts: picks[r] lists the candidates of row rows[r]; `starts`, `ends` and
    got = (distances, lengths, ops) are those rows' slots."""
    for at, row in enumerate(rows):
        spans = [candidates[int(index)][int(start):int(end)] for index, start, end in zip(picks[at], starts[at], ends[at])]
        distances, lengths, scripts = alignment_cases.canonical_scripts(queries[int(row)], spans)
        ops = np.zeros((len(spans), capacity), np.uint8)
        ops[:, :scripts.shape[1]] = scripts  # the capacity holds every script of these legs
        if not (np.array_equal(got[0][at], distances) and np.array_equal(got[1][at], lengths) and np.array_equal(got[2][at], ops)):
            return False
    return True


def measure(leg, queries, candidates, indices, host_indices, shape, rows, picks, extra):
    """Times the three calls on one set of inputs, verifies `align`, emits the line; the names of what did not hold."""
    spans_out = torch.zeros((3,) + shape, dtype=torch.int64, device="cuda")
    plain_out = torch.zeros((2,) + shape, dtype=torch.int64, device="cuda")
    capacity = int(queries.lengths().max()) + min(512, int(candidates.lengths().max()))
    cells_out = torch.zeros((2,) + shape, dtype=torch.int64, device="cuda")
    ops_out = torch.zeros(shape + (capacity,), dtype=torch.uint8, device="cuda")
    runs = {}
    for name, run in (
            ("fuzzy_find", lambda: engine.fuzzy_find(queries, candidates, indices, device=gpu, out=(plain_out[0], plain_out[1]))),
            ("spans", lambda: engine.fuzzy_find(queries, candidates, indices, device=gpu, out=tuple(spans_out), starts=True)),
            ("align", lambda: engine.align(queries, candidates, indices, starts=spans_out[1], ends=spans_out[2], device=gpu,
                                           out=(cells_out[0], cells_out[1], ops_out)))):
        best, kernel, kernel_last = timed(run, args.repeats)
        profile = engine.last_call_profile()
        runs[name] = {"wall_ms": round(best * 1e3, 3), "kernel_ms": round(kernel, 4), "kernel_ms_last": round(kernel_last, 4),
                      "launches": int(profile.launches), "pairs": int(profile.pairs), "cells": int(profile.cells),
                      "bytes": int(profile.algorithmic_bytes)}
    distances, starts, ends = (matrix.cpu().numpy() for matrix in spans_out)
    lengths = queries.lengths().astype(np.int64)[:, None]
    span_cells = int((lengths * (ends - starts)).sum())
    script_lengths = cells_out[1].cpu().numpy()
    slots = (lambda matrix: matrix[rows[:, None], picks]) if host_indices is None else (lambda matrix: matrix[rows])
    on_device = torch.from_numpy(rows).cuda()
    checked_ops = ops_out[on_device].cpu().numpy()
    if host_indices is None:
        checked_ops = checked_ops[np.arange(len(rows))[:, None], picks]
    pairs = shape[0] * shape[1]
    checks = {
        "align == the canonical script (distance, length, ops)": against_the_dp(
            queries, candidates, rows, picks, slots(starts), slots(ends), (slots(cells_out[0].cpu().numpy()), slots(script_lengths), checked_ops),
            capacity),
        "align's distances == the spans call's": bool(np.array_equal(cells_out[0].cpu().numpy(), distances)),
        "max(m, t) <= L <= m + t": bool((script_lengths >= np.maximum(lengths, ends - starts)).all() and
                                        (script_lengths <= lengths + ends - starts).all()),
        "launches 1, 2 and 1": [runs[name]["launches"] for name in ("fuzzy_find", "spans", "align")] == [1, 2, 1],
        "pairs == the host's": all(run["pairs"] == pairs for run in runs.values()),
        "align's cells == m x t over the spans": runs["align"]["cells"] == span_cells,
    }
    reverse_pass = runs["spans"]["kernel_ms"] - runs["fuzzy_find"]["kernel_ms"]
    trace_bytes = int((np.maximum((lengths + 31) // 32, 1) * (ends - starts)).sum()) * 8  # what the forward halves store, summed over the pairs
    emit({"leg": leg, **extra, "pairs": pairs, "capacity": capacity, "span_cells": span_cells, "ops": int(script_lengths.sum()),
          "trace_bytes_stored": trace_bytes, **runs, "reverse_pass_kernel_ms": round(reverse_pass, 4),
          "align_over_reverse_pass_kernel": round(runs["align"]["kernel_ms"] / reverse_pass, 3) if reverse_pass > 0 else None,
          "align_over_spans_kernel": round(runs["align"]["kernel_ms"] / runs["spans"]["kernel_ms"], 3) if runs["spans"]["kernel_ms"] else None,
          "verified_pairs_against_dp": int(picks.size), "verified": all(checks.values())})
    return [f"{leg[:3]} {name}" for name, held in checks.items() if not held]


gpu = szs.DeviceScope(gpu_device=0)
engine = szs.LevenshteinDistances(capabilities=gpu)
mismatches = []  # the run then fails, so no figure is recorded beside a wrong result

if "listed" in legs:
    queries, candidates = tape(2002, args.many, 96, 160), tape(2001, args.corpus, 96, 160)
    host_indices = np.random.default_rng(17).integers(0, args.corpus, size=(args.many, K), dtype=np.uint64)
    indices = torch.from_numpy(host_indices.view(np.int64)).cuda()
    rows = np.random.default_rng(18).choice(args.many, size=max(1, min(args.many, args.checked // K)), replace=False)
    mismatches += measure("(a) listed: rerank's leg (d) inputs through fuzzy_find with starts, then align", queries, candidates, indices,
                          host_indices, (args.many, K), rows, host_indices[rows], {"k": K, "queries": args.many, "corpus": args.corpus})

if "documents" in legs:
    patterns, documents = tape(2005, args.patterns, 16, 64), tape(2004, args.documents, 1024, 3072)
    rng = np.random.default_rng(19)
    rows = rng.choice(args.patterns, size=max(1, min(args.patterns, args.checked // 64)), replace=False)
    picks = np.stack([rng.choice(args.documents, size=min(64, args.documents), replace=False) for _ in rows])
    mismatches += measure("(b) documents: every pattern in every document, dense, with starts, then align", patterns, documents, None, None,
                          (args.patterns, args.documents), rows, picks, {"patterns": args.patterns, "documents": args.documents})

if mismatches:
    sys.exit("results differ: " + ", ".join(mismatches))

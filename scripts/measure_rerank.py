#!/usr/bin/env python3
"""Times rerank (`engine.rerank`, szs_rocm_rerank*) on one GPU beside what a user had before it.  One JSON line per leg.

  kernel   (a) 1024 queries x k = 16 listed candidates out of 16,384: the kernel route (hip/myers_rerank.hip), one launch
  rows     (b) the same call with the `rerank` knob at 0: one engine call per row
  matrix   (c) the full 1024 x 16,384 matrix call into device memory followed by a gather: what existed before rerank
  million  (d) 65,536 queries x k = 16 (1 M pairs), kernel route: pairs/s, TCUPS and the fraction of the cross-product short
               kernel's 96.3 TCUPS (README.md)
  documents (e) 1024 queries x k = 16 out of 16,384, every string U[1024, 3072] ASCII: the strips route (hip/myers_rerank_strips.hip,
               one launch) beside the `rerank` knob at 1, which sends these rows down the row route as before that kernel existed

Strings are config 2's (`std::mt19937_64`, U[96, 160] printable ASCII); indices are uniform, seeded.  Wall time = a host clock
around the synchronous call after a device synchronise; the best of `--repeats` calls after one warm-up.  (a), (b) and (c) run in one
process and are verified against each other in that run; (d) is verified against the row route on its first 256 rows; a mismatch
ends the run with a non-zero exit status; so do the two runs of (e) when their scores differ.  `--record FILE` appends every line
to FILE as well (profiles/rNN/measure_rerank.jsonl).  Kernel time
of (d): `rocprofv3 --kernel-trace --stats -- python scripts/measure_rerank.py --legs million`, in a run of its own.
"""
import argparse
import json
import os
import sys
import time

parser = argparse.ArgumentParser()
parser.add_argument("--legs", default="kernel,rows,matrix,million,documents")
parser.add_argument("--repeats", type=int, default=5)
parser.add_argument("--queries", type=int, default=1024)
parser.add_argument("--corpus", type=int, default=16384)
parser.add_argument("--many", type=int, default=65536, help="queries of leg (d)")
parser.add_argument("--k", type=int, default=16)
parser.add_argument("--record", default=None, help="a file every JSON line is appended to")
args = parser.parse_args()
legs = args.legs.split(",")
if not set(legs) <= {"kernel", "rows", "matrix", "million", "documents"} or min(args.repeats, args.queries, args.corpus, args.many, args.k) < 1:
    parser.error("--legs takes kernel, rows, matrix, million, documents; the counts must be at least 1")

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import stringzilla_amd as szs
from stringzilla_amd import _abi, workloads

SHORT_KERNEL_TCUPS = 96.3  # the cross-product short kernel on config 2 (README.md)
K = args.k


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


def tape(seed, count, shortest=96, longest=160):
    return workloads.mt19937_64_tape(seed, count, shortest, longest, workloads.ASCII_PRINTABLE).to_device(0)


def emit(line):
    print(json.dumps(line), flush=True)
    if args.record:
        os.makedirs(os.path.dirname(os.path.abspath(args.record)), exist_ok=True)
        with open(args.record, "a") as record:
            record.write(json.dumps(line) + "\n")


def report(leg, best, median, pairs, cells, **more):
    emit({"leg": leg, "k": K, "wall_ms": round(best * 1e3, 3), "median_ms": round(median * 1e3, 3), "pairs": pairs,
          "pairs_per_s": float(f"{pairs / best:.4g}"), "tcups": round(cells / best / 1e12, 4), **more})


def listed_cells(queries, candidates, indices):
    return int((queries.lengths()[:, None] * candidates.lengths()[indices.astype(np.int64)]).sum())


gpu = szs.DeviceScope(gpu_device=0)
engine = szs.LevenshteinDistances(capabilities=gpu)
candidates = tape(2001, args.corpus)
results = {}
mismatches = []  # legs whose results differ: the run then fails, so no figure is recorded beside a wrong result

if set(legs) & {"kernel", "rows", "matrix"}:
    queries = tape(2000, args.queries)
    host_indices = np.random.default_rng(16).integers(0, args.corpus, size=(args.queries, K), dtype=np.uint64)
    indices = torch.from_numpy(host_indices.view(np.int64)).cuda()
    cells = listed_cells(queries, candidates, host_indices)
    for leg in ("kernel", "rows"):
        if leg not in legs:
            continue
        _abi.tuning_set("rerank", None if leg == "kernel" else 0)
        out = torch.zeros((args.queries, K), dtype=torch.int64, device="cuda")
        best, median = timed(lambda: engine.rerank(queries, candidates, indices, device=gpu, out=out), args.repeats)
        profile = engine.last_call_profile()
        results[leg] = out.cpu().numpy()
        report("(a) kernel route" if leg == "kernel" else "(b) rerank=0: one engine call per row", best, median, args.queries * K, cells,
               launches=int(profile.launches), kernel_ms=round(profile.kernel_milliseconds, 4), queries=args.queries, corpus=args.corpus)
    _abi.tuning_set("rerank", None)
    if "matrix" in legs:
        matrix = torch.zeros((args.queries, args.corpus), dtype=torch.int64, device="cuda")

        def full_matrix_then_gather():
            engine(queries, candidates, device=gpu, out=matrix)
            return torch.gather(matrix, 1, indices)

        best, median = timed(full_matrix_then_gather, args.repeats)
        results["matrix"] = full_matrix_then_gather().cpu().numpy()
        report("(c) full matrix into device memory + gather", best, median, args.queries * K, cells, queries=args.queries, corpus=args.corpus,
               cells_scored_over_cells_wanted=round(int(queries.lengths().sum()) * int(candidates.lengths().sum()) / cells, 1))
    names = sorted(results)
    agree = {f"{a}=={b}": bool(np.array_equal(results[a], results[b])) for a in names for b in names if a < b}
    emit({"verified": agree})
    mismatches += [pair for pair, same in agree.items() if not same]

if "million" in legs:
    queries = tape(2002, args.many)
    host_indices = np.random.default_rng(17).integers(0, args.corpus, size=(args.many, K), dtype=np.uint64)
    indices = torch.from_numpy(host_indices.view(np.int64)).cuda()
    out = torch.zeros((args.many, K), dtype=torch.int64, device="cuda")
    best, median = timed(lambda: engine.rerank(queries, candidates, indices, device=gpu, out=out), args.repeats)
    profile = engine.last_call_profile()
    cells = listed_cells(queries, candidates, host_indices)
    checked = min(args.many, 256)
    _abi.tuning_set("rerank", 0)
    by_rows = engine.rerank(queries.select(np.arange(checked)), candidates, host_indices[:checked], device=gpu)
    _abi.tuning_set("rerank", None)
    same = np.array_equal(out[:checked].cpu().numpy().view(np.uint64), by_rows)
    report("(d) kernel route, many rows", best, median, args.many * K, cells, queries=args.many, corpus=args.corpus,
           launches=int(profile.launches), kernel_ms=round(profile.kernel_milliseconds, 4),
           kernel_tcups=round(cells / (profile.kernel_milliseconds * 1e-3) / 1e12, 4) if profile.kernel_milliseconds else None,
           kernel_tcups_over_short_kernel=round(cells / (profile.kernel_milliseconds * 1e-3) / 1e12 / SHORT_KERNEL_TCUPS, 4)
           if profile.kernel_milliseconds else None,
           profile_cells_match=bool(profile.cells == cells), verified_rows=checked, verified=bool(same))
    if not same:
        mismatches.append("(d) kernel route==row route")
    if profile.cells != cells:
        mismatches.append("(d) profile cells==listed cells")

if "documents" in legs:
    queries, documents = tape(2003, args.queries, 1024, 3072), tape(2004, args.corpus, 1024, 3072)
    host_indices = np.random.default_rng(18).integers(0, args.corpus, size=(args.queries, K), dtype=np.uint64)
    indices = torch.from_numpy(host_indices.view(np.int64)).cuda()
    cells = listed_cells(queries, documents, host_indices)
    runs = {}
    for knob in (None, 1):  # automatic: the strips kernel; 1: the short kernel only, these rows as engine calls of their own
        _abi.tuning_set("rerank", knob)
        out = torch.zeros((args.queries, K), dtype=torch.int64, device="cuda")
        best, median = timed(lambda: engine.rerank(queries, documents, indices, device=gpu, out=out), args.repeats)
        profile = engine.last_call_profile()
        runs[knob] = {"wall_ms": round(best * 1e3, 3), "median_ms": round(median * 1e3, 3), "launches": int(profile.launches),
                      "kernel_ms": round(profile.kernel_milliseconds, 4), "profile_cells_match": bool(profile.cells == cells),
                      "scores": out.cpu().numpy()}
    _abi.tuning_set("rerank", None)
    same = bool(np.array_equal(runs[None].pop("scores"), runs[1].pop("scores")))
    strips, rows = runs[None], runs[1]
    emit({"leg": "(e) documents: strips route beside rerank=1", "k": K, "queries": args.queries, "corpus": args.corpus, "pairs": args.queries * K,
          "cells": cells, "strips": strips, "rerank_1": rows, "rerank_1_over_strips_wall": round(rows["wall_ms"] / strips["wall_ms"], 2),
          "strips_pairs_per_s": float(f"{args.queries * K / (strips['wall_ms'] * 1e-3):.4g}"),
          "strips_tcups_by_wall": round(cells / (strips["wall_ms"] * 1e-3) / 1e12, 4),
          "strips_tcups_by_kernel": round(cells / (strips["kernel_ms"] * 1e-3) / 1e12, 4) if strips["kernel_ms"] else None, "verified": same})
    if not same:
        mismatches.append("(e) strips route==rerank=1")
    if not strips["profile_cells_match"]:
        mismatches.append("(e) profile cells==listed cells")

if mismatches:
    sys.exit("results differ: " + ", ".join(mismatches))

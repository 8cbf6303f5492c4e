#!/usr/bin/env python3
"""Times top-k search (`engine.top_k`, szs_rocm_top_k_*) on one GPU and prints one JSON line per measurement.

  config2   config 2's batch (1024 x 1024 ASCII, U[96,160]): top_k with k = 1, 16 and 128 beside the same engine's full-matrix
            call into device memory.  Wall time = a host clock around the synchronous call, after a device synchronise.
  corpus    1024 queries x 2^22 std::mt19937_64 candidates, U[96,160] ASCII, k = 16 (its full matrix would be 32 GiB):
            TCUPS from the cells of the lengths over the wall time of the whole call.

Kernel shares (scoring vs the top_k_* selection kernels) come from a separate `rocprofv3 --kernel-trace --stats` run of this script.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import stringzilla_amd as szs
from stringzilla_amd import workloads

parser = argparse.ArgumentParser()
parser.add_argument("--workloads", default="config2,corpus")
parser.add_argument("--repeats", type=int, default=5)
parser.add_argument("--corpus", type=int, default=1 << 22, help="candidates of the large corpus")
args = parser.parse_args()

gpu = szs.DeviceScope(gpu_device=0)


def timed(run, repeats):
    run()  # warm-up: allocations, code objects
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        started = time.perf_counter()
        run()
        times.append(time.perf_counter() - started)
    return min(times), float(np.median(times))


for name in args.workloads.split(","):
    if name == "config2":
        load = workloads.config(2)
        engine = szs.LevenshteinDistances(**load.costs, capabilities=gpu)
        load.queries.to_device(0), load.candidates.to_device(0)
        rows, columns = len(load.queries), len(load.candidates)
        matrix = torch.empty((rows, columns), dtype=torch.int64, device="cuda")
        best, median = timed(lambda: engine(load.queries, load.candidates, device=gpu, out=matrix), args.repeats)
        full_ms = best * 1e3
        print(json.dumps({"workload": load.name, "call": "full matrix into device memory", "wall_ms": round(full_ms, 4),
                          "median_ms": round(median * 1e3, 4), "cells": load.cells}), flush=True)
        for k in (1, 16, 128):
            indices = torch.empty((rows, k), dtype=torch.int64, device="cuda")
            scores = torch.empty((rows, k), dtype=torch.int64, device="cuda")
            best, median = timed(lambda: engine.top_k(load.queries, load.candidates, k=k, device=gpu, out=(indices, scores)), args.repeats)
            # the same answer as a stable selection over the full matrix
            full = matrix.cpu().numpy().view(np.uint64)
            expected = np.argsort(full, axis=1, kind="stable")[:, :k]
            exact = bool(np.array_equal(indices.cpu().numpy().view(np.uint64), expected))
            print(json.dumps({"workload": load.name, "call": f"top_k k={k}", "wall_ms": round(best * 1e3, 4), "median_ms": round(median * 1e3, 4),
                              "vs_full_matrix": round(best * 1e3 / full_ms, 3), "exact": exact}), flush=True)
    elif name == "corpus":
        ascii_letters = np.arange(32, 127, dtype=np.uint8)
        queries = workloads.mt19937_64_tape(7000, 1024, 96, 160, ascii_letters).to_device(0)
        candidates = workloads.mt19937_64_tape(7001, args.corpus, 96, 160, ascii_letters).to_device(0)
        cells = int(queries.lengths().sum()) * int(candidates.lengths().sum())
        engine = szs.LevenshteinDistances(capabilities=gpu)
        indices = torch.empty((1024, 16), dtype=torch.int64, device="cuda")
        scores = torch.empty((1024, 16), dtype=torch.int64, device="cuda")
        best, median = timed(lambda: engine.top_k(queries, candidates, k=16, device=gpu, out=(indices, scores)), max(1, args.repeats // 2))
        profile = engine.last_call_profile()
        print(json.dumps({"workload": f"1024 x {args.corpus} mt19937_64 U[96,160] ASCII", "call": "top_k k=16", "wall_ms": round(best * 1e3, 2),
                          "median_ms": round(median * 1e3, 2), "cells": cells, "tcups": round(cells / best / 1e12, 2),
                          "scoring_kernel_ms": round(profile.kernel_milliseconds, 2),
                          "scoring_tcups": round(cells / (profile.kernel_milliseconds * 1e-3) / 1e12, 2) if profile.kernel_milliseconds else None,
                          "full_matrix_GiB": round(1024 * args.corpus * 8 / 2**30, 1)}), flush=True)
    else:
        raise SystemExit(f"unknown workload {name!r}")

#!/usr/bin/env python3
"""Times fingerprint search (`Fingerprints.matches` / `.top_k`, szs_rocm_fingerprint_*) on one GPU beside what a user had before it:
a torch broadcast compare.  One JSON line per measurement.

  matches        (a) `matches` of 1024 x 1024 fingerprints at D = 1024 into device memory
  search_device  (b) `top_k`, k = 16, of 1024 queries against 2^20 candidates at D = 1024, candidates in device memory
  search_host    (c) the same with the candidates in plain host memory (staged tile by tile)
  torch_matches  (d) `(a[:, None, :] == b[None]).sum(-1)` on the same GPU, chunked over candidates so that the boolean intermediate
                     stays under 1 GiB
  torch_search   (d) the same over the 2^20 candidates, with `torch.topk` on top

Hashes are drawn uniformly from 16 values, so that counts spread (mean D / 16) and the selection has ties to break.  Wall time = a
host clock around the synchronous call, after a device synchronise; the best of `--repeats` calls after one warm-up.  Without
`--case` every case runs in a child process of its own under its own time limit, and the first failure ends the run.  Kernel shares
(the match kernel vs the top_k_* selection kernels) come from a separate `rocprofv3 --kernel-trace --stats` run of one case.
"""
import argparse
import json
import os
import subprocess
import sys
import time

CASES = {"matches": 120, "torch_matches": 120, "search_device": 240, "search_host": 360, "torch_search": 420}  # seconds each may take

parser = argparse.ArgumentParser()
parser.add_argument("--case", choices=sorted(CASES))
parser.add_argument("--cases", default="matches,torch_matches,search_device,search_host,torch_search")
parser.add_argument("--repeats", type=int, default=5)
parser.add_argument("--corpus", type=int, default=1 << 20, help="candidates of the search cases")
parser.add_argument("--ndim", type=int, default=1024)
parser.add_argument("--queries", type=int, default=1024)
args = parser.parse_args()
if min(args.queries, args.ndim, args.repeats) < 1 or args.corpus < 16:
    parser.error("--queries, --ndim and --repeats must be at least 1, --corpus at least k = 16")

if args.case is None:
    for name in args.cases.split(","):
        command = [sys.executable, os.path.abspath(__file__), "--case", name, "--repeats", str(args.repeats), "--corpus", str(args.corpus),
                   "--ndim", str(args.ndim), "--queries", str(args.queries)]
        try:
            code = subprocess.run(command, timeout=CASES[name]).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{name}: no result within {CASES[name]} s - nothing more is started")
        if code:
            raise SystemExit(f"{name}: exit status {code} - nothing more is started")
    raise SystemExit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import stringzilla_amd as szs

Q, C, D, K = args.queries, args.corpus, args.ndim, 16
VALU_LANE_OPS = 256 * 4 * 32 * 2.4e9  # CUs x SIMDs x lanes per clock x peak clock
LANE_OPS_PER_COMPARE = 2              # v_cmp_eq_u32 + its share of v_cndmask_b32 / v_addc_co_u32


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


def draw(rows, seed):
    generator = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 16, (rows, D), dtype=torch.int32, device="cuda", generator=generator)


def torch_matches(a, b, chunk):
    """What a user wrote before: broadcast compare and sum, a chunk of candidates at a time."""
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.int32, device=a.device)
    for first in range(0, b.shape[0], chunk):
        out[:, first:first + chunk] = (a[:, None, :] == b[None, first:first + chunk]).sum(-1, dtype=torch.int32)
    return out


def report(call, best, median, compares, **more):
    rate = compares / best
    print(json.dumps({"call": call, "queries": Q, "ndim": D, "wall_ms": round(best * 1e3, 3), "median_ms": round(median * 1e3, 3),
                      "compares_per_s": float(f"{rate:.4g}"),
                      "of_valu_issue_ceiling": round(rate * LANE_OPS_PER_COMPARE / VALU_LANE_OPS, 3), **more}), flush=True)


chunk = max(1, ((1 << 30) - 1) // (Q * D))  # the (Q, chunk, D) boolean intermediate stays under 1 GiB
gpu = szs.DeviceScope(gpu_device=0)
engine = szs.Fingerprints(D, capabilities=gpu)
queries = draw(Q, 1)

if args.case in ("matches", "torch_matches"):
    candidates = draw(Q, 2)
    want = torch_matches(queries, candidates, chunk)
    if args.case == "matches":
        out = torch.empty((Q, Q), dtype=torch.int32, device="cuda")
        best, median = timed(lambda: engine.matches(queries, candidates, device=gpu, out=out), args.repeats)
        report("(a) matches into device memory", best, median, Q * Q * D, candidates=Q, exact=bool(torch.equal(out, want)))
    else:
        best, median = timed(lambda: torch_matches(queries, candidates, chunk), args.repeats)
        report("(d) torch broadcast compare + sum", best, median, Q * Q * D, candidates=Q, chunk=chunk)
else:
    candidates = draw(C, 3)
    if args.case == "torch_search":
        best, median = timed(lambda: torch.topk(torch_matches(queries, candidates, chunk), K, dim=1), args.repeats)
        report("(d) torch broadcast compare + sum + topk", best, median, Q * C * D, candidates=C, k=K, chunk=chunk)
    else:
        pool = candidates if args.case == "search_device" else candidates.cpu().numpy().view(np.uint32)
        indices = torch.empty((Q, K), dtype=torch.int64, device="cuda")
        matches = torch.empty((Q, K), dtype=torch.int64, device="cuda")
        best, median = timed(lambda: engine.top_k(queries, pool, k=K, device=gpu, out=(indices, matches)), args.repeats)
        # the same counts as torch's selection over a slice of the queries (its order among ties is not defined: counts only)
        checked = min(Q, 64)
        want = torch.topk(torch_matches(queries[:checked], candidates, chunk * (Q // checked)), K, dim=1).values
        where = "device" if args.case == "search_device" else "plain host"
        report(f"({'b' if args.case == 'search_device' else 'c'}) top_k k={K}, candidates in {where} memory", best, median, Q * C * D,
               candidates=C, k=K, exact_counts=bool(torch.equal(matches[:checked], want.to(torch.int64))),
               corpus_GiB=round(C * D * 4 / 2**30, 2))

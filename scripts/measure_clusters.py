#!/usr/bin/env python3
"""Times `clusters` (`engine.clusters`, `Fingerprints.clusters`) on one GPU beside the cheapest sibling that
sees every edge today, in ONE process: the parent commit has no such call, so the yardstick is the sibling in the same run.  One JSON
line per leg.

  a  `--count` strings of U[96, 160] bytes from std::mt19937_64 (seed 4160), an eighth of them replaced by copies of others with up to
     three substitutions; unit-cost Levenshtein, bound 3 - a few thousand edges: `within(strings, None, bound, limit=0)` beside
     `clusters(strings, bound)`.
  b  the same count, all strings identical, bound 0: every cell is a hit - the worst case for the forest.
  c  `--rows` x 64 random hashes with planted groups, `min_matches` 32: `Fingerprints.top_k(k=1)` in its self form beside
     `Fingerprints.clusters`.

Wall time = a host clock around the synchronous call after a device synchronise; the best of `--repeats` calls after one warm-up.
Every leg is verified in the run that times it: `--checked` sampled labels against a host union-find (tests/clusters_cases.py's rule:
the smallest index of the component) over ALL edges - for (a) the rows of `within` at a limit no row reaches, for (b) every pair, for
(c) the thresholded `matches` matrix, a block of rows at a time.  Any difference ends the run with a non-zero exit status.
`--record FILE` appends every line to FILE (profiles/rNN/measure_clusters.jsonl).
"""
import argparse
import json
import os
import sys
import time

parser = argparse.ArgumentParser()
parser.add_argument("--legs", default="a,b,c")
parser.add_argument("--repeats", type=int, default=5)
parser.add_argument("--count", type=int, default=16384, help="strings of legs a and b")
parser.add_argument("--rows", type=int, default=65536, help="fingerprints of leg c")
parser.add_argument("--checked", type=int, default=512, help="sampled labels verified per leg")
parser.add_argument("--record", default=None, help="a file every JSON line is appended to")
args = parser.parse_args()
legs = args.legs.split(",")
if not set(legs) <= {"a", "b", "c"} or min(args.repeats, args.count, args.rows, args.checked) < 1:
    parser.error("--legs takes a, b, c; the counts must be at least 1")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import stringzilla_amd as szs
from stringzilla_amd import _abi, workloads

BOUND, MIN_MATCHES, LIMIT = 3, 32, 64


def timed(run):
    run()  # warm-up: allocations, code objects
    times = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        started = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - started)
    return {"wall_ms": round(min(times) * 1e3, 3), "median_ms": round(float(np.median(times)) * 1e3, 3)}


def emit(line):
    print(json.dumps(line), flush=True)
    if args.record:
        os.makedirs(os.path.dirname(os.path.abspath(args.record)), exist_ok=True)
        with open(args.record, "a") as record:
            record.write(json.dumps(line) + "\n")


def profiled(engine):
    profile = engine.last_call_profile()
    return {"kernel_ms": round(profile.kernel_milliseconds, 4), "launches": int(profile.launches), "pairs": int(profile.pairs)}


def host_labels(count, first, second):
    """The smallest index of every component of the undirected edges (first[e], second[e])."""
    parent = list(range(count))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in zip(first.tolist(), second.tolist()):
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(count)], dtype=np.uint64)


def verified(name, labels, count, want):
    sample = np.sort(np.random.default_rng(43).choice(len(want), size=min(len(want), args.checked), replace=False))
    same = bool(np.array_equal(labels[sample], want[sample])) and count == int((want == np.arange(len(want), dtype=np.uint64)).sum())
    if not same:
        mismatches.append(f"{name}: sampled labels and the count == the host union-find")
    return {"verified_labels": int(len(sample)), "verified": same}


gpu = szs.DeviceScope(gpu_device=0)
mismatches = []  # the run then fails, so no figure is recorded beside a wrong result
_abi.tuning_set("top_k_tile", None)


def string_leg(name, strings, bound, want_of):
    engine = szs.LevenshteinDistances(capabilities=gpu)
    n = len(strings)
    counts, labels = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
    within = {**timed(lambda: engine.within(strings, None, bound=bound, limit=0, device=gpu, out=(counts, None, None))), **profiled(engine)}
    found = []
    clusters = {**timed(lambda: found.append(engine.clusters(strings, bound, device=gpu, out=labels)[1])), **profiled(engine)}
    got = labels.cpu().numpy().view(np.uint64)
    edges = int(counts.cpu().numpy().view(np.uint64).sum()) // 2
    probe = _abi.clusters_probe(n, True)
    emit({"leg": name, "strings": n, "bound": bound, "within limit=0": within, "clusters": clusters, "edges": edges, "clusters_count": found[-1],
          "block": probe[0], "tile": probe[1], "tiles": probe[2], "pairs_over_the_square": round(clusters["pairs"] / (n * n), 4),
          "clusters_over_within_wall": round(clusters["wall_ms"] / within["wall_ms"], 3),
          "clusters_over_within_kernel": round(clusters["kernel_ms"] / within["kernel_ms"], 3), **verified(name, got, found[-1], want_of(engine))})


if "a" in legs or "b" in legs:
    tape = workloads.mt19937_64_tape(4160, args.count, 96, 160, workloads.ASCII_PRINTABLE)

if "a" in legs:
    rng = np.random.default_rng(4161)
    strings = [bytearray(tape[i]) for i in range(args.count)]
    for at in rng.choice(args.count, size=args.count // 8, replace=False):
        copy = bytearray(strings[int(rng.integers(0, args.count))])
        for _ in range(int(rng.integers(0, 4))):
            copy[int(rng.integers(0, len(copy)))] = int(rng.integers(32, 127))
        strings[int(at)] = copy
    planted = szs.Strs([bytes(s) for s in strings]).to_device(0)

    def want_a(engine):
        counts, indices, _ = engine.within(planted, None, bound=BOUND, limit=LIMIT, device=gpu)
        if int(counts.max(initial=0)) > LIMIT:
            sys.exit("leg a: a row has more neighbours than the verification lists")
        rows, slots = np.nonzero(indices != np.uint64(2**64 - 1))
        return host_labels(args.count, rows, indices[rows, slots].astype(np.int64))

    string_leg("(a) planted near-duplicates among mt19937_64 U[96,160]", planted, BOUND, want_a)

if "b" in legs:
    same = szs.Strs([tape[0]] * args.count).to_device(0)
    string_leg("(b) all strings identical: every cell a hit", same, 0, lambda engine: np.zeros(args.count, dtype=np.uint64))

if "c" in legs:
    rows = args.rows
    rng = np.random.default_rng(4162)
    hashes = rng.integers(0, 2**32, size=(rows, 64), dtype=np.uint64).astype(np.uint32)
    for at in rng.choice(rows, size=rows // 8, replace=False):
        hashes[at] = hashes[int(rng.integers(0, rows))]
        redrawn = rng.choice(64, size=int(rng.integers(0, 48)), replace=False)
        hashes[at, redrawn] = rng.integers(0, 2**32, size=len(redrawn), dtype=np.uint64).astype(np.uint32)
    device_hashes = torch.from_numpy(hashes.view(np.int32)).cuda()
    engine = szs.Fingerprints(64, capabilities=gpu)
    best = torch.zeros((2, rows, 1), dtype=torch.int64, device="cuda")
    labels = torch.zeros(rows, dtype=torch.int64, device="cuda")
    top_k = timed(lambda: engine.top_k(device_hashes, None, k=1, device=gpu, out=(best[0], best[1])))
    found = []
    clusters = timed(lambda: found.append(engine.clusters(device_hashes, MIN_MATCHES, device=gpu, out=labels)[1]))
    first, second = [], []
    for r0 in range(0, rows, 4096):  # every edge, from the thresholded matrix of matches: 4096 rows at a time
        block = torch.empty((min(4096, rows - r0), rows), dtype=torch.int32, device="cuda")
        engine.matches(device_hashes[r0:r0 + 4096], device_hashes, device=gpu, out=block)
        i, j = torch.nonzero(block >= MIN_MATCHES, as_tuple=True)
        first.append((i + r0).cpu().numpy()), second.append(j.cpu().numpy())
    first, second = np.concatenate(first), np.concatenate(second)
    want = host_labels(rows, first[first != second], second[first != second])
    name = "(c) fingerprints: top_k(k=1) in its self form beside clusters"
    probe = _abi.clusters_probe(rows, True)
    emit({"leg": name, "rows": rows, "dimensions": 64, "min_matches": MIN_MATCHES, "top_k k=1": top_k, "clusters": clusters,
          "edges": int((first != second).sum()) // 2, "clusters_count": found[-1], "block": probe[0], "tile": probe[1], "tiles": probe[2],
          "pairs_over_the_square": round(probe[3] / (rows * rows), 4), "clusters_over_top_k_wall": round(clusters["wall_ms"] / top_k["wall_ms"], 3),
          **verified(name, labels.cpu().numpy().view(np.uint64), found[-1], want)})

if mismatches:
    sys.exit("results differ: " + ", ".join(mismatches))

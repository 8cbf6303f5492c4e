#!/usr/bin/env python3
"""Times the bounded searches (`engine.within`, `engine.fuzzy_search_within`) on one GPU beside their sorting
siblings, in ONE process: the parent commit has no such call, so the yardstick is the sibling in the same run.  One JSON line per leg.

  config2  scripts/measure_top_k.py's config 2 batch (1024 x 1024 ASCII, U[96,160]): `top_k(k=16)`, `within(limit=16)` and
           `within(limit=0)`, the bound = the median 16th-best score of a sample of rows.
  corpus   the same script's 1024 queries x 2^22 std::mt19937_64 candidates (seeds 7000 / 7001): the same three calls.
  fuzzy    scripts/measure_fuzzy_search.py leg (c) - 64 patterns of U[16, 64] bytes (seed 2007) in 2^20 documents of U[96, 160] bytes
           (seed 2006): `fuzzy_search(k=16)`, `fuzzy_search_within(max_distance=2, limit=16)` and the same with `limit=0`.

Wall time = a host clock around the synchronous call after a device synchronise; the best of `--repeats` calls after one warm-up.  The
scoring launches of a pair of calls are identical; only the fold differs.  Every leg is verified in the run that times it: up to
`--checked` sampled rows against the numpy expectation (tests/within_cases.py) over the rows of the engine's own matrix call - for
`fuzzy` the dense `fuzzy_find` call - and for `fuzzy` the listed pairs of those rows against the plain semi-global DP as well.  Any
difference ends the run with a non-zero exit status.  `--record FILE` appends every line to FILE (profiles/rNN/measure_within.jsonl).
"""
import argparse
import json
import os
import sys
import time

parser = argparse.ArgumentParser()
parser.add_argument("--legs", default="config2,corpus,fuzzy")
parser.add_argument("--repeats", type=int, default=5)
parser.add_argument("--limit", type=int, default=16)
parser.add_argument("--corpus", type=int, default=1 << 22, help="candidates of leg `corpus`")
parser.add_argument("--few", type=int, default=64, help="queries of leg `fuzzy`")
parser.add_argument("--documents", type=int, default=1 << 20, help="candidates of leg `fuzzy`")
parser.add_argument("--max-distance", type=int, default=2)
parser.add_argument("--checked", type=int, default=512, help="sampled rows verified per leg")
parser.add_argument("--record", default=None, help="a file every JSON line is appended to")
args = parser.parse_args()
legs = args.legs.split(",")
if not set(legs) <= {"config2", "corpus", "fuzzy"} or min(args.repeats, args.limit, args.corpus, args.few, args.documents, args.checked) < 1:
    parser.error("--legs takes config2, corpus, fuzzy; the counts must be at least 1")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import stringzilla_amd as szs
from stringzilla_amd import _abi, workloads

import within_cases as cases

LIMIT = args.limit
CHUNK_CELLS = 1 << 25  # of a verification matrix of the fuzzy leg: 256 MiB of device memory
COLUMNS = 1 << 18  # candidates of a verification matrix of the similarity legs: with 512 rows, 1 GiB


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


def sampled_rows(rows, seed):
    return np.sort(np.random.default_rng(seed).choice(rows, size=min(rows, args.checked), replace=False))


def chunks_of(rows, columns):
    step = max(1, CHUNK_CELLS // max(columns, 1))
    return [rows[at:at + step] for at in range(0, len(rows), step)]


gpu = szs.DeviceScope(gpu_device=0)
mismatches = []  # the run then fails, so no figure is recorded beside a wrong result
for knob in ("top_k_tile", "fuzzy_search_segment"):
    _abi.tuning_set(knob, None)


def similarity_leg(name, engine, queries, candidates):
    rows, columns = len(queries), len(candidates)
    best = torch.zeros((2, rows, LIMIT), dtype=torch.int64, device="cuda")
    counts = torch.zeros(rows, dtype=torch.int64, device="cuda")
    hits = torch.zeros((2, rows, LIMIT), dtype=torch.int64, device="cuda")
    top_k = {**timed(lambda: engine.top_k(queries, candidates, k=LIMIT, device=gpu, out=(best[0], best[1]))), **profiled(engine)}
    kth = best[1, :, LIMIT - 1].cpu().numpy()
    bound = int(np.median(kth[sampled_rows(rows, 29)[:64]]))  # the median k-th best score of a sample of rows
    within = {**timed(lambda: engine.within(queries, candidates, bound=bound, limit=LIMIT, device=gpu, out=(counts, hits[0], hits[1]))),
              **profiled(engine)}
    got = counts.cpu().numpy().view(np.uint64), hits[0].cpu().numpy().view(np.uint64), hits[1].cpu().numpy().view(np.uint64)
    only = torch.zeros(rows, dtype=torch.int64, device="cuda")
    counted = {**timed(lambda: engine.within(queries, candidates, bound=bound, limit=0, device=gpu, out=(only, None, None))), **profiled(engine)}
    same = bool(np.array_equal(only.cpu().numpy().view(np.uint64), got[0]))
    checked = sampled_rows(rows, 31)
    sampled = queries.select(checked).to_device(0)
    want = [np.zeros(len(checked), np.uint64), np.full((len(checked), LIMIT), cases.EMPTY, np.uint64), np.zeros((len(checked), LIMIT), np.uint64)]
    for c0 in range(0, columns, COLUMNS):  # the sampled rows of the engine's own matrix call, 2^18 candidates at a time
        c1 = min(c0 + COLUMNS, columns)
        first, last = int(candidates.offsets[c0]), int(candidates.offsets[c1])
        part = szs.Strs.from_tape(candidates.data[first:last], candidates.offsets[c0:c1 + 1] - candidates.offsets[c0])
        matrix = torch.empty((len(checked), c1 - c0), dtype=torch.int64, device="cuda")
        engine(sampled, part, device=gpu, out=matrix)
        counts_here, indices_here, scores_here = cases.expected_within(matrix.cpu().numpy().view(np.uint64), bound, False, LIMIT)
        for r in range(len(checked)):  # a row's leftmost hits: those of the chunks before, then this chunk's
            held, more = int(min(want[0][r], LIMIT)), int(min(counts_here[r], LIMIT))
            take = min(more, LIMIT - held)
            want[1][r, held:held + take], want[2][r, held:held + take] = indices_here[r, :take] + np.uint64(c0), scores_here[r, :take]
        want[0] += counts_here
    same = same and cases.same([part[checked] for part in got], want)
    emit({"leg": name, "queries": rows, "candidates": columns, "limit": LIMIT, "bound": bound, f"top_k k={LIMIT}": top_k,
          f"within limit={LIMIT}": within, "within limit=0": counted, "within_over_top_k_wall": round(within["wall_ms"] / top_k["wall_ms"], 3),
          "counts_only_over_top_k_wall": round(counted["wall_ms"] / top_k["wall_ms"], 3), "hits": int(got[0].sum()),
          "rows_beyond_the_limit": int((got[0] > LIMIT).sum()), "verified_rows": int(len(checked)), "verified": same})
    if not same:
        mismatches.append(f"{name}: within==numpy over the matrix call's rows")


if "config2" in legs:
    load = workloads.config(2)
    load.queries.to_device(0), load.candidates.to_device(0)
    similarity_leg(load.name, szs.LevenshteinDistances(**load.costs, capabilities=gpu), load.queries, load.candidates)

if "corpus" in legs:
    ascii_letters = np.arange(32, 127, dtype=np.uint8)
    queries = workloads.mt19937_64_tape(7000, 1024, 96, 160, ascii_letters).to_device(0)
    candidates = workloads.mt19937_64_tape(7001, args.corpus, 96, 160, ascii_letters).to_device(0)
    similarity_leg(f"1024 x {args.corpus} mt19937_64 U[96,160] ASCII", szs.LevenshteinDistances(capabilities=gpu), queries, candidates)

if "fuzzy" in legs:
    engine = szs.LevenshteinDistances(capabilities=gpu)
    patterns = workloads.mt19937_64_tape(2007, args.few, 16, 64, workloads.ASCII_PRINTABLE).to_device(0)
    corpus = workloads.mt19937_64_tape(2006, args.documents, 96, 160, workloads.ASCII_PRINTABLE).to_device(0)
    rows, columns, bound = args.few, args.documents, args.max_distance
    found = torch.zeros((3, rows, LIMIT), dtype=torch.int64, device="cuda")
    counts = torch.zeros(rows, dtype=torch.int64, device="cuda")
    hits = torch.zeros((3, rows, LIMIT), dtype=torch.int64, device="cuda")
    search = {**timed(lambda: engine.fuzzy_search(patterns, corpus, k=LIMIT, device=gpu, out=tuple(found))), **profiled(engine)}
    within = {**timed(lambda: engine.fuzzy_search_within(patterns, corpus, max_distance=bound, limit=LIMIT, device=gpu,
                                                         out=(counts,) + tuple(hits))), **profiled(engine)}
    got = [counts.cpu().numpy().view(np.uint64)] + [part.cpu().numpy().view(np.uint64) for part in hits]
    only = torch.zeros(rows, dtype=torch.int64, device="cuda")
    empty = torch.zeros((rows, 0), dtype=torch.int64, device="cuda")
    counted = {**timed(lambda: engine.fuzzy_search_within(patterns, corpus, max_distance=bound, limit=0, device=gpu,
                                                          out=(only, empty, empty, empty))), **profiled(engine)}
    same = bool(np.array_equal(only.cpu().numpy().view(np.uint64), got[0]))
    checked, listed = sampled_rows(rows, 37), True
    for chunk in chunks_of(checked, columns):  # the dense call over the same strings, a chunk of rows at a time
        dense = torch.empty((2, len(chunk), columns), dtype=torch.int64, device="cuda")
        engine.fuzzy_find(patterns.select(chunk), corpus, device=gpu, out=(dense[0], dense[1]))
        distances, ends = dense[0].cpu().numpy().view(np.uint64), dense[1].cpu().numpy().view(np.uint64)
        want = cases.expected_fuzzy_within((distances, ends, ends), bound, LIMIT)  # (no starts asked for: the ends twice)
        same = same and cases.same([part[chunk] for part in got], [want[0], want[1], want[2], want[4]])
        for at, row in enumerate(chunk):  # ... and the listed pairs against the plain DP
            held = [int(index) for index in got[1][row] if index != cases.EMPTY]
            if held:
                best, _, end = cases.spans(patterns[int(row)], [corpus[index] for index in held])
                listed = listed and np.array_equal(best, got[2][row, :len(held)].astype(np.int64)) and np.array_equal(end, got[3][row, :len(held)].astype(np.int64))
    emit({"leg": "(c) corpus: fuzzy_search beside fuzzy_search_within", "patterns": rows, "documents": columns, "limit": LIMIT,
          "max_distance": bound, f"fuzzy_search k={LIMIT}": search, f"fuzzy_search_within limit={LIMIT}": within,
          "fuzzy_search_within limit=0": counted, "within_over_search_wall": round(within["wall_ms"] / search["wall_ms"], 3),
          "counts_only_over_search_wall": round(counted["wall_ms"] / search["wall_ms"], 3), "hits": int(got[0].sum()),
          "rows_beyond_the_limit": int((got[0] > LIMIT).sum()), "verified_rows": int(len(checked)), "verified": bool(same),
          "listed_pairs_equal_the_dp": bool(listed)})
    if not (same and listed):
        mismatches.append("fuzzy: fuzzy_search_within==numpy over the dense call's rows, listed pairs==DP")

if mismatches:
    sys.exit("results differ: " + ", ".join(mismatches))

"""Seeded batches that drive the 16-bit weighted kernels to the ENDS of their value ranges.

Four code paths keep DP cells (or parked rows) in 16 bits under a bound the host computes (host/dispatch.c, `szs_call_decide`):
the team tier in its narrow and wide orders (hip/team_core.hpp: `team_reach_limit`), hip/weighted_packed.hip and the `int16_t`
parking of hip/weighted.hip (both below 32000).  `batch()` builds, for one objective, one gap model and one such limit, strings
whose bound lies ONE length step below the limit - or is the first to reach it - and whose scores come as close to that end of
the range as the arithmetic allows: costs of 127 / -128, runs of one letter, runs of letters that never match, borders that
run all the way down.  It checks from the oracle alone that the batch gets there.

A plain module: no fixtures, no settings.  tests/test_value_ranges_model.py (CPU) and tests/test_gpu_value_ranges.py import it.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

from oracle import binding

FACTOR = 0.9  # of the limit, as tests/test_team_model.py asks of its edge cases
TEAM_LIMITS = {"global": (15000, 32000), "local": (29000, 62000), "distance": (30000, 64000)}  # hip/team_core.hpp: team_reach_limit, (narrow, wide)
PARKED_LIMIT = 32000  # host/dispatch.c: `d->narrow`, which also admits hip/weighted_packed.hip


class Batch(NamedTuple):
    byte_to_class: Optional[np.ndarray]  # None for a distance
    costs: object  # the 32 x 32 class table, or the (match, mismatch, open, extend) of a Levenshtein engine
    gaps: tuple  # (open, extend), signed and ADDED; a distance: (-open, -extend), what the team tier adds
    queries: list
    candidates: Optional[list]  # None: a symmetric call
    bound: int  # what dispatch.c compares with the limit
    expected: np.ndarray  # the oracle's matrix
    objective: str
    affine: bool
    limit: int
    aim: Optional[str]


def class_table(magnitude):
    """Four classes (0: every other byte, costs 0), asymmetric off-diagonals: 127 / 120 against -128 / -127 at 128."""
    byte_to_class = np.zeros(256, np.uint8)
    for index, letter in enumerate(b"ABC"):
        byte_to_class[letter] = index + 1
    top = min(magnitude, 127)
    table = np.zeros((32, 32), np.int8)
    for a in (1, 2, 3):
        for b in (1, 2, 3):
            table[a, b] = (top if a != 2 else top - top // 18) if a == b else (-magnitude if (a, b) in ((1, 2), (3, 1), (2, 3)) else -(magnitude - 1))
    return byte_to_class, table


def bound_of(objective, linear, magnitude, longest_query, longest_candidate):
    """The caller's bound, as `szs_call_decide` forms it (host/dispatch.c:371-401)."""
    if objective == "global":
        return (longest_query + longest_candidate + (1 if linear else 3)) * magnitude
    if objective == "local":
        return (min(longest_query, longest_candidate) + 3) * magnitude
    return (max(longest_query, longest_candidate) + (1 if linear else 3)) * magnitude


def _family(rng, longest):
    """Nine strings of at most `longest` bytes, an odd count so that the last one of a (longest first) list has no partner:
    runs of one letter - the best-scoring one twice, for the low AND the high half of a register -, a near-run whose partner
    in that list is a tenth of its length (the padded rows of the high half run on for most of the matrix), tiny ones, the
    empty string."""
    near = bytearray(b"A" * max(longest - 1, 0))
    for at in rng.integers(0, max(len(near), 1), size=len(near) // 40):
        near[at] = ord("B")
    strings = [b"A" * longest, b"A" * longest, b"B" * longest, b"C" * longest, bytes(near), b"A" * max(longest // 10, min(longest, 1)), b"ABCABCA", b"BABA", b""]
    return [s[:longest] for s in strings]


def _extras(rng, longest, count):
    letters = np.frombuffer(b"ABC", np.uint8)
    half = longest // 2
    fixed = [b"A", b"CC", b"AB" * half, b"A" * half + b"B" + b"A" * max(half - 1, 0), b"B" * min(40, longest)]
    return [s[:longest] for s in fixed] + [letters[rng.integers(0, 3, size=int(rng.integers(0, longest + 1)))].tobytes() for _ in range(count)]


@functools.lru_cache(maxsize=None)
def batch(objective, affine, limit, table=128, costs=(-128, -128), aim="bottom", long_side="queries", at_limit=False, symmetric=False, seed=0):
    """One batch.  `costs`: (open, extend) of a class-table engine over `class_table(table)`, or (match, mismatch, open, extend)
    of a Levenshtein engine.  `aim`: the end of the range the scores must reach - "top" (largest score) or "bottom" (lowest
    score, largest distance) - or None where no input can get within FACTOR of it (say why at the call).  `long_side`: which
    side holds the long strings where the two differ.  `at_limit`: the first length whose bound reaches the limit instead of
    the last one below it.  Cached: the arrays are shared between tests and must not be written to."""
    rng = np.random.default_rng(1000 * seed + limit % 997 + len(objective))
    oracle = binding.oracle()
    if objective == "distance":
        linear = costs[2] == costs[3]
        magnitude = max(abs(c) for c in costs)
    else:
        linear = costs[0] == costs[1]
        byte_to_class, class_costs = class_table(table)
        magnitude = max(int(np.abs(class_costs.astype(np.int64)).max()), abs(costs[0]), abs(costs[1]))
    assert linear != bool(affine), (costs, affine)
    steps = -(-limit // magnitude) - (0 if at_limit else 1)  # (span + border) x magnitude: the last below the limit / the first to reach it
    span = steps - (3 if objective == "local" or not linear else 1)

    if objective == "global":  # span: both longest strings together
        if symmetric:
            longer, shorter = span // 2, span // 2
        elif aim == "bottom":  # -magnitude x (longer side) at best: the other side must stay a twenty-fifth of it
            shorter = max(1, span // 25)
            longer = span - shorter
        else:
            shorter = span // 2
            longer = span - shorter
    elif objective == "local":  # span: the shorter of the two longest strings
        shorter, longer = span, span if symmetric else span + span // 3
    else:  # span: the longer of the two
        shorter, longer = span if symmetric else span - 7, span
    longest_query, longest_candidate = (longer, shorter) if long_side == "queries" else (shorter, longer)

    queries = _family(rng, longest_query)
    candidates = None if symmetric else _family(rng, longest_candidate) + _extras(rng, longest_candidate, 12)
    if symmetric:
        queries += _extras(rng, longest_query, 4)
        longest_candidate = longest_query
    bound = bound_of(objective, linear, magnitude, longest_query, longest_candidate)
    step = magnitude * (2 if symmetric and objective == "global" else 1)  # a symmetric global call grows by two letters at a time
    assert (bound >= limit and bound - step < limit) if at_limit else (bound < limit <= bound + step), (bound, limit)

    if objective == "distance":
        expected = oracle.levenshtein(queries, candidates, *costs)
        reached = int(expected.max())
        result = Batch(None, costs, (-costs[2], -costs[3]), queries, candidates, bound, expected, objective, bool(affine), limit, aim)
    else:
        scorer = oracle.smith_waterman if objective == "local" else oracle.needleman_wunsch
        expected = scorer(queries, candidates, byte_to_class, class_costs, *costs)
        reached = int(expected.max()) if aim == "top" else -int(expected.min())
        result = Batch(byte_to_class, class_costs, costs, queries, candidates, bound, expected, objective, bool(affine), limit, aim)
    if aim is not None and not at_limit:
        assert reached >= FACTOR * limit, f"{objective} {costs} table {table}: the {aim} of the range is not reached: {reached} of {limit}"
    expected.setflags(write=False)
    return result


def flavours(objective, affine, wide):
    """The keyword arguments of the batches one (objective, gap model, order) is shown: every magnitude (128 from the table
    alone, 128 from a gap cost alone, 127, 40), every gap cost of the issue, both ends, the long side on either side.

    The TOP of a global score with gap costs <= 0 cannot pass 127 x min(rows, columns), about half the limit: that end is
    covered by the batches with POSITIVE gap costs, where the all-gap path earns 127 a letter.  The BOTTOM needs every path to
    be dear, so it wants both gap costs large: global batches whose extension (or opening) costs 1 cannot get near either end
    and run with `aim=None`, as does the distance with costs 0 / 127 / 1 / 1, which never exceeds rows + columns.  They are
    kept for what they put into the profile (entries of cost - gap = +-255) and the seeds."""
    mid = [] if wide else [40]  # 40: queries of several passes; the wide order's strings are long enough at 128
    if objective == "global" and not affine:
        chosen = [dict(table=128, costs=(-127, -127), aim="bottom"), dict(table=127, costs=(-128, -128), aim="bottom", long_side="candidates"),
                  dict(table=127, costs=(127, 127), aim="top"), dict(table=128, costs=(127, 127), aim="top", long_side="candidates")]
        chosen += [dict(table=m, costs=(-m, -m), aim="bottom") for m in mid]
    elif objective == "global":
        chosen = [dict(table=128, costs=(-128, -127), aim="bottom"), dict(table=127, costs=(127, -1), aim="top"),
                  dict(table=128, costs=(-128, -1), aim=None), dict(table=128, costs=(-1, -128), aim=None, long_side="candidates")]
        chosen += [dict(table=m, costs=(-m, -m + 1), aim="bottom", long_side="candidates") for m in mid]
    elif objective == "local" and not affine:
        chosen = [dict(table=128, costs=(0, 0), aim="top"), dict(table=127, costs=(-128, -128), aim="top", long_side="candidates"),
                  dict(table=128, costs=(-128, -128), aim="top")]
        chosen += [dict(table=m, costs=(-m, -m), aim="top", long_side="candidates") for m in mid]
    elif objective == "local":
        chosen = [dict(table=128, costs=(-128, -1), aim="top"), dict(table=127, costs=(-1, -128), aim="top", long_side="candidates")]
        chosen += [dict(table=m, costs=(-m, -3), aim="top") for m in mid]
    elif not affine:
        chosen = [dict(costs=(0, 127, 127, 127), aim="bottom"), dict(costs=(0, 127, 1, 1), aim=None, long_side="candidates")]
        chosen += [dict(costs=(0, m, m, m), aim="bottom", long_side="candidates") for m in mid]
    else:
        chosen = [dict(costs=(3, 127, 127, 126), aim="bottom"), dict(costs=(1, 126, 127, 1), aim=None, long_side="candidates")]
        chosen += [dict(costs=(2, m, m, m - 1), aim="bottom", long_side="candidates") for m in mid]
    return chosen

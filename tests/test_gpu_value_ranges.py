"""`-m gpu`: the 16-bit weighted kernels at the ENDS of their value ranges, on the hardware.

Four code paths keep cells or parked rows in 16 bits under a bound that only the host checks (host/dispatch.c, `szs_call_decide`):
the team tier's narrow order (hip/weighted_teams.hip: `v_pk_maximum3_f16` on biased patterns, an integer maximum only between
0x0400 and 0x7BFF), its wide order (`v_pk_max_u16`, one `v_add_u32` for both halves), hip/weighted_packed.hip (signed packed
halves, bound below 32000) and the `int16_t` parking of hip/weighted.hip's strip boundaries (the same bound).  Every other GPU
test feeds them costs of at most 11.  Here the costs are 127 / -128, the bound lies ONE length step below each limit and AT it,
and the scores come within a tenth of the limit (tests/value_range_cases.py asserts that from the oracle alone), so the
profile built from an `int8` table, the parked rows and the seeds of later passes, the pick of the result, the symmetric and
transposed writes and the distance profile all carry values next to the ends.  Which path ran is read off the call's profile.

The decision boundaries with a magnitude of 128 that comes from the table alone (-128 beside gap costs of 0 or -127) or from a
gap cost alone (-128 beside a table of +-127) are covered here too: `magnitude_of` (host/engines.c) off by one moves the first
length that takes the next regime, and the routing assertions at the limit fail.
"""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import stringzilla_amd as szs  # noqa: E402
from stringzilla_amd import _abi  # noqa: E402

import value_range_cases as cases  # noqa: E402


@contextlib.contextmanager
def knob(name, value):
    previous = _abi.tuning_set(name, value)
    try:
        yield
    finally:
        _abi.tuning_set(name, previous)


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return szs.DeviceScope(gpu_device=0)


def scored(gpu, batch):
    """The batch through the engine of its objective: (matrix as int64, profile of the call)."""
    if batch.objective == "distance":
        engine = szs.LevenshteinDistances(*batch.costs, capabilities=gpu)
    else:
        kind = szs.SmithWatermanScores if batch.objective == "local" else szs.NeedlemanWunschScores
        engine = kind(batch.byte_to_class, batch.costs, open=batch.gaps[0], extend=batch.gaps[1], capabilities=gpu)
    got = engine(batch.queries, device=gpu) if batch.candidates is None else engine(batch.queries, batch.candidates, device=gpu)
    return got.view(np.int64), engine.last_call_profile()


def agrees(got, batch, profile):
    wrong = np.argwhere(got != batch.expected.view(np.int64))
    others = batch.queries if batch.candidates is None else batch.candidates
    assert wrong.size == 0, (batch.objective, batch.costs, batch.gaps, batch.bound, profile.team, profile.team_wide, profile.cell_bits, profile.transposed,
                             [(len(batch.queries[q]), len(others[c]), int(got[q, c]), int(batch.expected.view(np.int64)[q, c])) for q, c in wrong[:5]])


SMALL, SQUARE, WAVE_WIDE = 41604, 161604, 643202  # 4 x 16: 64 rows a pass, the queries take 2 ... 8 (at 40: up to 24); 16 x 16; 64 x 32


def team_case(gpu, objective, wide, affine, shape, flavour):
    """Below the limit: this shape, this order, 16-bit cells.  At it: the wide order, or no team and 32-bit cells."""
    limit = cases.TEAM_LIMITS[objective][wide]  # hip/team_core.hpp: team_reach_limit
    for at_limit in (False, True):
        batch = cases.batch(objective, affine, limit, at_limit=at_limit, **flavour)
        with knob("team", shape), knob("tier", "lanes"), knob("swap", 0):
            got, profile = scored(gpu, batch)
        agrees(got, batch, profile)
        if not at_limit:
            assert (profile.team, profile.team_wide, profile.cell_bits) == (shape, wide, 16), (flavour, batch.bound, profile.team, profile.team_wide, profile.cell_bits)
        elif not wide:
            assert (profile.team, profile.team_wide, profile.cell_bits) == (shape, 1, 16), (flavour, batch.bound, profile.team, profile.team_wide, profile.cell_bits)
        else:
            assert (profile.team, profile.cell_bits) == (0, 32), (flavour, batch.bound, profile.team, profile.cell_bits)


@pytest.mark.parametrize("shape", [SMALL, SQUARE])
@pytest.mark.parametrize("affine", [0, 1], ids=["linear", "affine"])
@pytest.mark.parametrize("wide", [0, 1], ids=["narrow", "wide"])
@pytest.mark.parametrize("objective", ["global", "local", "distance"])
def test_team_tier_at_the_ends_of_its_ranges(gpu, oracle, objective, wide, affine, shape):
    for flavour in cases.flavours(objective, affine, wide):
        team_case(gpu, objective, wide, affine, shape, flavour)


@pytest.mark.parametrize("objective", ["global", "local", "distance"])
def test_wave_wide_teams_at_the_ends_of_their_ranges(gpu, oracle, objective):
    """64 x 32: a team is a whole wavefront, the hand-over crosses DPP rows."""
    for wide, affine in ((0, 1), (1, 0)):
        team_case(gpu, objective, wide, affine, WAVE_WIDE, cases.flavours(objective, affine, wide)[0])


@pytest.mark.parametrize("objective", ["global", "local", "distance"])
def test_team_tier_transposed_symmetric_and_host_planned(gpu, oracle, objective):
    """The candidates on the workgroups (the class table is asymmetric: the kernel must read its transpose), a symmetric call
    (the lower triangle, mirrored), and - a distance - a host-planned call, which counts no alphabet and keeps 32-bit cells."""
    limit = cases.TEAM_LIMITS[objective][0]
    flavour = dict(cases.flavours(objective, 1, 0)[1 if objective == "global" else 0])  # global: positive gap costs, the top of the range
    batch = cases.batch(objective, 1, limit, **flavour)
    with knob("team", SMALL), knob("tier", "lanes"), knob("swap", 1):
        got, profile = scored(gpu, batch)
    agrees(got, batch, profile)
    assert (profile.transposed, profile.team, profile.team_wide, profile.cell_bits) == (1, SMALL, 0, 16), (profile.transposed, profile.team, profile.team_wide)
    flavour.pop("long_side", None)
    square = cases.batch(objective, 1, limit, symmetric=True, **flavour)
    with knob("team", SMALL), knob("tier", "lanes"):
        got, profile = scored(gpu, square)
    agrees(got, square, profile)
    assert (profile.team, profile.team_wide, profile.cell_bits) == (SMALL, 0, 16), (profile.team, profile.team_wide, profile.cell_bits)
    if objective == "distance":
        with knob("team", SMALL), knob("tier", "lanes"), knob("swap", 0), knob("planner", "host"):
            got, profile = scored(gpu, batch)
        agrees(got, batch, profile)
        assert (profile.team, profile.cell_bits, profile.planner) == (0, 32, 0), (profile.team, profile.cell_bits, profile.planner)


def parked_flavours(objective, affine):
    """What hip/weighted_packed.hip and the `int16_t` parking are shown: the team tier's batches of the wide order (their
    strings are the longer ones), at the one limit both share."""
    return cases.flavours(objective, affine, 1)


@pytest.mark.parametrize("affine", [0, 1], ids=["linear", "affine"])
@pytest.mark.parametrize("objective", ["global", "local"])
def test_packed_kernel_at_the_ends_of_its_range(gpu, oracle, objective, affine):
    """Signed 16-bit halves: values next to +-32000; local gaps of (0, 0) and (-128, -128) through the saturating subtract.
    At the limit `d->narrow` goes and `d->packed` with it (host/dispatch.c:386-393), global and local alike: 32-bit cells."""
    for flavour in parked_flavours(objective, affine):
        for at_limit in (False, True):
            batch = cases.batch(objective, affine, cases.PARKED_LIMIT, at_limit=at_limit, **flavour)
            with knob("team", 0), knob("tier", "lanes"), knob("swap", 0):
                got, profile = scored(gpu, batch)
            agrees(got, batch, profile)
            assert (profile.team, profile.cell_bits) == (0, 32 if at_limit else 16), (flavour, at_limit, batch.bound, profile.team, profile.cell_bits)


@pytest.mark.parametrize("affine", [0, 1], ids=["linear", "affine"])
@pytest.mark.parametrize("objective", ["global", "local"])
def test_parked_rows_of_the_32_bit_kernel_at_the_ends_of_their_range(gpu, oracle, objective, affine):
    """hip/weighted.hip scores in 32 bits and parks the boundary rows of its 32-row strips as `int16_t` while the bound stays
    below 32000: queries of 4 ... 10 strips, parked values next to +-32000, then the first bound that parks 32 bits."""
    for flavour in parked_flavours(objective, affine):
        for at_limit in (False, True):
            batch = cases.batch(objective, affine, cases.PARKED_LIMIT, at_limit=at_limit, **flavour)
            with knob("packed", 0), knob("tier", "lanes"), knob("swap", 0):
                got, profile = scored(gpu, batch)
            agrees(got, batch, profile)
            assert (profile.team, profile.cell_bits) == (0, 32), (flavour, at_limit, profile.team, profile.cell_bits)


@pytest.mark.parametrize("gaps", [(127, 127), (127, -1)], ids=["linear", "affine"])
def test_local_scores_with_positive_gap_costs_at_magnitude_127(gpu, oracle, gaps):
    """A positive gap cost takes a local engine off every saturating path, to the signed 32-bit kernel of hip/weighted.hip:
    the one weighted path left that no other test feeds large costs.  No 16-bit bound applies; the strings are the packed
    kernel's."""
    shaped = cases.batch("local", 1, cases.PARKED_LIMIT, table=127, costs=(-127, -1), aim="top")
    expected = oracle.smith_waterman(shaped.queries, shaped.candidates, shaped.byte_to_class, shaped.costs, *gaps)
    batch = shaped._replace(gaps=gaps, expected=expected)
    assert expected.max() > 127 * max(map(len, batch.queries))  # gaps that pay: beyond any gapless alignment
    with knob("tier", "lanes"), knob("swap", 0):
        got, profile = scored(gpu, batch)
    agrees(got, batch, profile)
    assert (profile.team, profile.cell_bits) == (0, 32), (profile.team, profile.cell_bits)

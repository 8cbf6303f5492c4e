"""The team tier's arithmetic at the ENDS of its value ranges, on the CPU: the batches of tests/value_range_cases.py (costs
of 127 / -128, bounds one length step below each `team_reach_limit`, scores within a tenth of the limit) through the lane-by-lane
model of the kernel (tests/native/team_model.cpp over hip/team_core.hpp), bit for bit against the oracle - and the oracle
against the reference's serial engine, so that what it says at -128 and +127 rests on something other than itself.

The same batches run on the hardware in tests/test_gpu_value_ranges.py.  `szs_call_decide` has no probe that works without a
GPU (tests/test_host_logic.py), so the decision boundaries with a magnitude of 128 that comes from the table alone, or from a
gap cost alone, are checked there, through the profile of the call.
"""
import numpy as np
import pytest

import value_range_cases as cases
from oracle import binding
from test_team_model import model, run_model  # noqa: F401  (the fixture that compiles the model, and its caller)

# the compiled kernel shapes, and two that only the model has: one row of lanes with few registers, one lane
SHAPES = [(16, 32), (16, 16), (4, 32), (4, 16), (64, 32), (4, 8), (1, 4)]
COMBINATIONS = [(objective, affine, wide) for objective in ("global", "local", "distance") for affine in (0, 1) for wide in (0, 1)]


def batches_of(objective, affine, wide):
    limit = cases.TEAM_LIMITS[objective][wide]
    return [cases.batch(objective, affine, limit, **flavour) for flavour in cases.flavours(objective, affine, wide)]


@pytest.mark.parametrize("objective,affine,wide", COMBINATIONS)
def test_model_matches_the_oracle_at_the_ends_of_the_range(model, objective, affine, wide):  # noqa: F811
    for index, batch in enumerate(batches_of(objective, affine, wide)):
        lanes, registers = SHAPES[(COMBINATIONS.index((objective, affine, wide)) * 3 + index) % len(SHAPES)]  # every shape, every order
        if objective == "distance":
            match, mismatch = batch.costs[:2]
            byte_to_class, _ = cases.class_table(1)
            table = np.full((32, 32), -mismatch, np.int8)
            np.fill_diagonal(table, -match)
            got = -run_model(model, 2, affine, wide, lanes, registers, batch.queries, batch.candidates, byte_to_class, table, *batch.gaps)
        else:
            got = run_model(model, objective == "local", affine, wide, lanes, registers, batch.queries, batch.candidates, batch.byte_to_class,
                            batch.costs, *batch.gaps)
        wrong = np.argwhere(got != batch.expected.astype(np.int64))
        assert wrong.size == 0, (batch.costs, batch.gaps, lanes, registers, batch.bound,
                                 [(len(batch.queries[q]), len(batch.candidates[c]), int(got[q, c]), int(batch.expected[q, c])) for q, c in wrong[:5]])


@pytest.mark.skipif(not binding.reference_available(), reason="reference shim not built (no /root/reference on this box)")
@pytest.mark.parametrize("objective,affine,wide", COMBINATIONS)
def test_oracle_matches_the_reference_at_the_ends_of_the_range(objective, affine, wide):
    reference = binding.reference(tier=0)
    for batch in batches_of(objective, affine, wide):
        if objective == "distance":
            theirs = reference.levenshtein(batch.queries, batch.candidates, *batch.costs)
        else:
            scorer = reference.smith_waterman if objective == "local" else reference.needleman_wunsch
            theirs = scorer(batch.queries, batch.candidates, batch.byte_to_class, batch.costs, *batch.gaps)
        assert np.array_equal(theirs.view(np.int64), batch.expected.view(np.int64)), (batch.costs, batch.gaps, batch.bound)

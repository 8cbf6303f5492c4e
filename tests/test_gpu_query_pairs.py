"""`-m gpu`: two queries in one bit-vector (hip/lev_myers.hip, the fused short launch).

The launch that plans itself scores descending refs s and s + ceil(Q / 2) in one workgroup: in ONE vector when the pair takes no more
words than the two apart (at most ten), one after the other otherwise.  Whole matrices against the oracle, through both the fused
launch (planner mode 4) and the planned path (`fused` knob 0), for config-2 batches, odd query counts, queries that cannot pair,
empty strings and the transposed layout (more queries than candidates: the host swaps the roles).
"""
import contextlib
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import stringzilla_amd as szs  # noqa: E402
from stringzilla_amd import _abi  # noqa: E402


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


def _batch(rng, count, span, alphabet=bytes(range(32, 127))):
    return [bytes(rng.choice(alphabet) for _ in range(rng.randint(*span))) for _ in range(count)]


def _check(engine, gpu, oracle, queries, candidates):
    import torch

    q_tape, c_tape = szs.Strs(queries).to_device(0), szs.Strs(candidates).to_device(0)
    out = torch.full((len(queries), len(candidates)), -7, dtype=torch.int64, device="cuda:0")
    engine(q_tape, c_tape, device=gpu, out=out)
    got = out.cpu().numpy().view(np.uint64)
    expected = oracle.levenshtein(queries, candidates)
    wrong = np.argwhere(got != expected)
    assert not len(wrong), (len(wrong), wrong[:6].tolist(), [int(got[tuple(w)]) for w in wrong[:6]], [int(expected[tuple(w)]) for w in wrong[:6]])
    return int(engine.last_call_profile().planner)


CASES = {
    # name: (queries, candidates, query lengths, candidate lengths)
    "config2": (1024, 300, (96, 160), (96, 160)),
    "odd_count": (333, 257, (96, 160), (80, 170)),
    "cannot_pair": (101, 300, (150, 256), (90, 200)),  # pairs of 150+ bytes take more than ten words: one after the other
    "short_and_empty": (77, 300, (0, 40), (0, 60)),
    "mixed_widths": (200, 513, (0, 256), (0, 256)),
    "transposed": (600, 150, (96, 160), (96, 160)),  # more queries than candidates
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_pairs_score_what_the_oracle_scores(gpu, oracle, case):
    rows, columns, q_span, c_span = CASES[case]
    rng = random.Random(case)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    modes = []
    for _ in range(3):  # the first call of a shape is planned on the device; the next ones plan themselves inside the launch
        modes.append(_check(engine, gpu, oracle, _batch(rng, rows, q_span), _batch(rng, columns, c_span)))
    with knob("fused", 0):
        modes.append(_check(engine, gpu, oracle, _batch(rng, rows, q_span), _batch(rng, columns, c_span)))
    assert modes[3] != 4, modes
    if case in ("config2", "odd_count", "transposed"):  # the shapes of the headline take the launch that plans itself
        assert 4 in modes[:3], modes


def test_empty_queries_pair_with_anything(gpu, oracle):
    rng = random.Random(7)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    queries = [b""] * 9 + _batch(rng, 9, (1, 200))
    rng.shuffle(queries)
    candidates = _batch(rng, 260, (0, 120)) + [b""] * 3
    for _ in range(3):
        _check(engine, gpu, oracle, queries, candidates)

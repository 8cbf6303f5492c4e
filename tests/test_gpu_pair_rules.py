"""`-m gpu`: the pairing rule the query sorter of the short launch that plans itself chooses (csrc/hip/pair_rule.h, hip/lev_myers.hip).

Whole matrices against the oracle, three calls per shape so that the launch that plans itself runs (planner mode 4), and for every
such call the rule the sorter published (`szs_rocm_last_pairing`) against what the probe chooses on the lengths of the kernel's
query side - the caller's candidates when the host swapped the roles.  The shapes are the smallest at which the rule can go wrong: a
shift that wraps around the shorter half, an odd count, n = 1 and n = 0, pairs that do not fit ten words, swapped roles, empty
queries, equal lengths.
"""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import stringzilla_amd as szs  # noqa: E402
from stringzilla_amd import _abi  # noqa: E402

ALPHABET = bytes(range(32, 127))


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return szs.DeviceScope(gpu_device=0)


def _strings(rng, lengths):
    return [bytes(rng.choice(ALPHABET) for _ in range(length)) for length in lengths]


def _uniform(low, high):
    return lambda rng, count: [rng.randint(low, high) for _ in range(count)]


def _two_kinds(rng, count):  # (0,40) with (150,256): a long query fits one vector with a short one, never with another long one
    return [rng.randint(0, 40) if rng.random() < 0.5 else rng.randint(150, 256) for _ in range(count)]


def _with_empty(rng, count):
    return [0 if i % 5 == 0 else rng.randint(1, 200) for i in range(count)]


CASES = {
    # name: (queries, candidates, query lengths, candidate lengths)
    "shift_wraps": (64, 300, _uniform(96, 160), _uniform(96, 160)),
    "odd_count": (33, 300, _uniform(96, 160), _uniform(80, 170)),
    "two_queries": (2, 300, _uniform(96, 160), _uniform(96, 160)),  # n = 1
    "one_query": (1, 300, _uniform(96, 160), _uniform(96, 160)),  # n = 0: nothing is taken modulo n
    "cannot_always_pair": (40, 300, _two_kinds, _uniform(90, 200)),
    "transposed": (600, 150, _uniform(96, 160), _uniform(96, 160)),  # more queries than candidates: the host swaps the roles
    "empty_queries": (36, 260, _with_empty, _uniform(0, 120)),
    "equal_lengths": (64, 300, _uniform(128, 128), _uniform(96, 160)),
}


def _score(engine, gpu, oracle, queries, candidates):
    import torch

    q_tape, c_tape = szs.Strs(queries).to_device(0), szs.Strs(candidates).to_device(0)
    out = torch.full((len(queries), len(candidates)), -7, dtype=torch.int64, device="cuda:0")
    engine(q_tape, c_tape, device=gpu, out=out)
    got = out.cpu().numpy().view(np.uint64)
    expected = oracle.levenshtein(queries, candidates)
    wrong = np.argwhere(got != expected)
    assert not len(wrong), (len(wrong), wrong[:6].tolist(), [int(got[tuple(w)]) for w in wrong[:6]], [int(expected[tuple(w)]) for w in wrong[:6]])
    profile = engine.last_call_profile()
    return int(profile.planner), int(profile.transposed), int(_abi.lib.szs_rocm_last_pairing(engine.handle))


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_published_rule_is_the_probes_and_scores_what_the_oracle_scores(gpu, oracle, case):
    rows, columns, q_lengths, c_lengths = CASES[case]
    rng = random.Random(case)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    modes, shifted = [], 0
    for _ in range(3):  # the first call of a shape is planned on the device; the next ones plan themselves inside the launch
        of_queries, of_candidates = q_lengths(rng, rows), c_lengths(rng, columns)
        mode, transposed, pairing = _score(engine, gpu, oracle, _strings(rng, of_queries), _strings(rng, of_candidates))
        modes.append(mode)
        if mode != 4:
            assert pairing == 0, (modes, pairing)  # no sorter, no rule
            continue
        expected, chosen_total, _ = _abi.pair_rule_probe(of_candidates if transposed else of_queries)
        print(f"{case}: rule {pairing} published, {expected} expected ({chosen_total} words)")
        assert pairing == expected, (case, modes, transposed, pairing, expected)
        shifted += expected != 0
    assert 4 in modes, modes
    if case == "shift_wraps":  # every batch of this case's seed pairs better shifted (the test below); the last two with a shift beyond 0
        assert shifted == modes.count(4), (shifted, modes)
    if case == "equal_lengths":
        assert shifted == 0


def test_the_batches_of_the_wrapping_case_want_a_shift():
    """What `shift_wraps` relies on, without a GPU's help: the probe chooses a shifted rule for each of its batches, and for the two
    that plan themselves inside the launch a shift beyond 0 (a rule above 1), so that the second ranks wrap around the shorter half."""
    rows, columns, q_lengths, c_lengths = CASES["shift_wraps"]
    rng = random.Random("shift_wraps")
    for call in range(3):
        of_queries, of_candidates = q_lengths(rng, rows), c_lengths(rng, columns)
        _strings(rng, of_queries), _strings(rng, of_candidates)  # (the draws the scoring test makes in between)
        rule, _, pairs = _abi.pair_rule_probe(of_queries)
        assert rule > (1 if call else 0), (call, rule)
        rises = [s for s in range(len(pairs) - 1) if pairs[s, 1] < pairs[s + 1, 1]]  # second ranks fall with s, but for the wrap
        assert len(rises) == (rule > 1) and sorted(pairs[:, 1].tolist()) == list(range(32, 64)), (rule, rises)

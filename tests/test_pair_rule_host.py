"""The pairing rule of the short launch that plans itself (csrc/hip/pair_rule.h), through `szs_rocm_pair_rule_probe` - no GPU.

Queries ranked by descending length, slots = ceil(Q / 2), n = Q - slots.  Rule 0: slot s < n takes ranks s and slots + s; rule
delta + 1: ranks s and slots + ((n - 1 - s + delta) mod n).  The sorter evaluates rule 0 and sixteen evenly spaced shifts
(delta = k n // 16) and publishes the one with the fewest bit-vector words over all slots; ties go to rule 0, then to the smallest
shift.  A model of that in Python, the probe (the same header the kernel compiles) and the figures of DESIGN.md section 4.1.
"""
import numpy as np
import pytest

from stringzilla_amd import _abi

COUNTS = [0, 1, 2, 3, 5, 333, 1024]


def words(length):
    return (length + 31) // 32 if length else 1


def slot_words(a, b):
    shared = (a + b + 2 + 31) // 32
    return shared if shared <= words(a) + words(b) and shared <= 10 else words(a) + words(b)


def candidates(count):
    n = count - (count + 1) // 2
    return [0] + [1 + k * n // 16 for k in range(16)] if n else [0]


def model(lengths, rule=None):
    """(rule, total words, [(first rank, second rank or -1)]) - the chosen rule when `rule` is None."""
    ranked = sorted((int(x) for x in lengths), reverse=True)
    count, slots = len(ranked), (len(ranked) + 1) // 2
    n = count - slots

    def pairs_of(r):
        return [(s, (slots + s if r == 0 else slots + (n - 1 - s + r - 1) % n) if s < n else -1) for s in range(slots)]

    def total(r):
        return sum(slot_words(ranked[a], ranked[b]) if b >= 0 else words(ranked[a]) for a, b in pairs_of(r))

    if rule is None:
        rule = min(candidates(count), key=lambda r: (total(r), r))  # candidates ascend: ties to rule 0, then the smallest shift
    return rule, total(rule), pairs_of(rule)


def batches(count):
    rng = np.random.default_rng(count + 17)
    yield "U[96,160]", rng.integers(96, 161, count)
    yield "U[64,256]", rng.integers(64, 257, count)
    yield "U[1,100]", rng.integers(1, 101, count)
    yield "all 128", np.full(count, 128)
    yield "normal(128,20)", np.clip(np.rint(rng.normal(128, 20, count)), 1, 256).astype(np.int64)
    yield "(0,40) with (150,256)", np.where(rng.random(count) < 0.5, rng.integers(0, 41, count), rng.integers(150, 257, count))


@pytest.mark.parametrize("count", COUNTS)
def test_every_rank_sits_in_exactly_one_slot_under_every_rule(count):
    lengths = np.random.default_rng(count).integers(96, 161, count)
    for rule in candidates(count):
        got_rule, _, pairs = _abi.pair_rule_probe(lengths, rule)
        assert got_rule == rule and pairs.shape == ((count + 1) // 2, 2)
        ranks = [int(r) for r in pairs.ravel() if r >= 0]
        assert sorted(ranks) == list(range(count)), (count, rule)
        assert [int(s) for s in pairs[:, 0]] == list(range((count + 1) // 2))  # the longer half leads the slots, in order
        assert int((pairs[:, 1] < 0).sum()) == count % 2  # only the middle query of an odd count is alone


@pytest.mark.parametrize("count", COUNTS)
def test_the_probe_agrees_with_the_model_slot_for_slot(count):
    for name, lengths in batches(count):
        for rule in [None] + candidates(count):
            expected_rule, expected_total, expected_pairs = model(lengths, rule)
            got_rule, got_total, got_pairs = _abi.pair_rule_probe(lengths, _abi.PAIR_RULE_CHOOSE if rule is None else rule)
            assert (got_rule, got_total) == (expected_rule, expected_total), (name, count, rule)
            assert [tuple(int(x) for x in row) for row in got_pairs] == expected_pairs, (name, count, rule)


@pytest.mark.parametrize("count", [5, 333, 1000, 1024])
def test_the_choice_is_never_worse_than_rule_0(count):
    for name, lengths in batches(count):
        _, chosen_total, _ = _abi.pair_rule_probe(lengths)
        _, plain_total, _ = _abi.pair_rule_probe(lengths, 0)
        assert chosen_total <= plain_total, (name, count, chosen_total, plain_total)


@pytest.mark.parametrize("count", [2, 33, 1024])
@pytest.mark.parametrize("length", [0, 1, 128, 143, 256])
def test_equal_lengths_keep_rule_0(count, length):
    assert _abi.pair_rule_probe(np.full(count, length))[0] == 0


def test_the_headline_batch_saves_what_the_model_says():
    lengths = np.random.default_rng(2).integers(96, 161, 1024)  # 4160 against 4356 word-slots
    rule, chosen_total, _ = _abi.pair_rule_probe(lengths)
    _, plain_total, _ = _abi.pair_rule_probe(lengths, 0)
    print(f"rule {rule}: {chosen_total} words against {plain_total} under rule 0 ({chosen_total / plain_total:.4f})")
    assert rule != 0 and chosen_total <= 0.97 * plain_total, (rule, chosen_total, plain_total)


def test_sides_the_sorter_does_not_stage_keep_rule_0():
    rng = np.random.default_rng(5)
    assert _abi.pair_rule_probe(rng.integers(96, 161, 1025))[0] == 0  # more than 1024 queries: sorted in two passes, not in LDS
    assert _abi.pair_rule_probe(np.append(rng.integers(96, 161, 63), 257))[0] == 0  # a query beyond 256 bytes: the side is blank


def test_a_rule_beyond_the_second_half_is_refused():
    with pytest.raises(_abi.StringZillasError):
        _abi.pair_rule_probe([100, 90, 80, 70], 3)  # n = 2: rules 0, 1, 2

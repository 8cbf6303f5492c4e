"""`-m gpu`: the Myers column that takes HN << 1 from the adder's carries (hip/myers_core.hpp: myers_column), through every caller.

Every cell against the oracle.  Single patterns of every short width, at 32 W - 31 and 32 W bytes; pairs of queries whose shared vector
takes 3, 9 and 10 words with the lower separator row s0 on bit 31 (s1 on bit 0 of the next word), on bit 0 and mid-word, with no phantom
row, and with empty queries.  300 candidates of a two-letter alphabet - one full block and a partial one - of 0 ... 70 bytes, some of
exactly 8, 16 and 17, so that the 8-column main loop, the per-dword loop and the predicated tail all run.  Each batch goes through the
launch that plans itself (planner mode 4: paired bodies, and single ones for what does not pair) and then, on the same tapes, through
the plain short kernel (mode 3).  One small call each for the other callers: the queue kernel and a long-query launch, the tiny-token
kernel, the rerank kernel.
"""
import contextlib
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import stringzilla_amd as szs  # noqa: E402
from stringzilla_amd import _abi  # noqa: E402

PAIR_WORDS = 10  # szs_myers_pair_words_k


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


def _letters(rng, length, alphabet=b"ab"):
    return bytes(rng.choice(alphabet) for _ in range(length))


def _candidates(rng, queries):
    """300 texts: 0 ... 70 bytes, a few of exactly 8, 16 and 17, one equal to a query, one "a" * 64."""
    lengths = [rng.randint(0, 70) for _ in range(292)] + [8, 8, 16, 16, 17, 17]
    texts = [_letters(rng, length) for length in lengths] + [queries[0], b"a" * 64]
    rng.shuffle(texts)
    return texts


alive = []  # (every tape stays alive: a freed one's address handed to the next batch would look like "the same tapes")


def _score(engine, gpu, oracle, queries, candidates, tapes=None):
    import torch

    q_tape, c_tape = tapes or (szs.Strs(queries).to_device(0), szs.Strs(candidates).to_device(0))
    out = torch.full((len(queries), len(candidates)), -7, dtype=torch.int64, device="cuda:0")
    engine(q_tape, c_tape, device=gpu, out=out)
    got = out.cpu().numpy().view(np.uint64)
    expected = oracle.levenshtein(queries, candidates)
    wrong = np.argwhere(got != expected)
    assert not len(wrong), (len(wrong), wrong[:6].tolist(), [int(got[tuple(w)]) for w in wrong[:6]], [int(expected[tuple(w)]) for w in wrong[:6]])
    alive.append((q_tape, c_tape, out))
    return int(engine.last_call_profile().planner), (q_tape, c_tape)


def _three_calls(gpu, oracle, rng, lengths, expect_rule):
    """Two fresh batches of the same counts and lengths - the second plans itself inside its launch - and the second one's tapes again."""
    engine = szs.LevenshteinDistances(capabilities=gpu)
    modes = []
    for _ in range(2):
        queries = [_letters(rng, length) for length in lengths]
        candidates = _candidates(rng, queries)
        mode, tapes = _score(engine, gpu, oracle, queries, candidates)
        modes.append(mode)
    assert modes[1] == 4, modes
    if expect_rule:
        rule, _, pairs = _abi.pair_rule_probe(lengths)
        assert int(_abi.lib.szs_rocm_last_pairing(engine.handle)) == rule, (modes, rule)
        assert pairs[0].tolist() == [0, 1]  # two queries: one slot, both in it
    mode, _ = _score(engine, gpu, oracle, queries, candidates, tapes)
    assert mode == 3, (modes, mode)  # the same tapes again: the plain short kernel behind the guard, one query per workgroup


@pytest.mark.parametrize("words", range(1, 9))
def test_single_patterns_of_every_short_width(gpu, oracle, words):
    """Three queries: an odd count leaves one alone in its workgroup of the launch that plans itself whatever the other two do; the
    same tapes again score all three alone."""
    _three_calls(gpu, oracle, random.Random(words), [32 * words, 32 * words - 31, 32 * words - 31], expect_rule=False)


# (first length, second length): the longer query takes the lower rows, s0 sits at bit 32 W - 2 - (second length) of the W-word vector
PAIRS = {
    "3_words_mid_word": (40, 40),       # 82 rows where apart they take 4 words; s0 at bit 54
    "3_words_bit_31": (50, 31),         # s0 at bit 63, s1 at bit 0 of word 2
    "3_words_bit_0": (50, 30),          # s0 at bit 64
    "8_words_no_phantom_row": (129, 125),
    "9_words_mid_word": (140, 120),     # s0 at bit 166
    "9_words_bit_31": (140, 127),       # s0 at bit 159, s1 at bit 0 of word 5
    "9_words_bit_0": (140, 126),        # s0 at bit 160
    "10_words_mid_word": (160, 150),    # s0 at bit 168
    "10_words_bit_31": (170, 127),      # s0 at bit 191, s1 at bit 0 of word 6
    "10_words_bit_0": (170, 126),       # s0 at bit 192
    "10_words_no_phantom_row": (159, 159),  # s0 at bit 159, s1 at bit 0 of word 5, q1 from bit 0 up
    "empty_second": (40, 0),            # s0 and s1 on bits 62 and 63, nothing above them
    "empty_first": (0, 0),              # (the first query of a pair is its longer one) s0 on bit 30, nothing below it
}


@pytest.mark.parametrize("case", sorted(PAIRS))
def test_pairs_with_the_boundary_on_every_kind_of_bit(gpu, oracle, case):
    first, second = PAIRS[case]
    words_of = lambda length: (length + 31) // 32 if length else 1
    shared = (first + second + 2 + 31) // 32
    assert first >= second and shared <= min(PAIR_WORDS, words_of(first) + words_of(second))  # built to pair
    if case[0].isdigit():
        assert shared == int(case.split("_")[0])
        assert {"bit_31": (32 * shared - 2 - second) % 32 == 31, "bit_0": (32 * shared - 2 - second) % 32 == 0,
                "mid_word": 1 < (32 * shared - 2 - second) % 32 < 30, "no_phantom_row": 32 * shared == first + second + 2}[case.split("_", 2)[2]]
    _three_calls(gpu, oracle, random.Random(case), [first, second], expect_rule=True)


def test_the_queue_kernel_and_a_long_query_launch(gpu, oracle):
    rng = random.Random(48)
    queries = [_letters(rng, length) for length in [1, 600, 257, 256, 320, 33] + [rng.randint(1, 600) for _ in range(42)]]
    candidates = [_letters(rng, rng.randint(0, 300)) for _ in range(48)]
    engine = szs.LevenshteinDistances(capabilities=gpu)
    # (48 x 48 pairs: left alone, the planner may hand the batch to the chained tier or swap the roles)
    with knob("tier", "lanes"), knob("swap", 0):
        with knob("queue", 1):  # the one persistent launch: every width in the queue kernel's bodies
            _score(engine, gpu, oracle, queries, candidates)
            profile = engine.last_call_profile()
            assert profile.launches == 1 and profile.queue_items > 0, (profile.launches, profile.queue_items)
        with knob("queue", 0):  # one launch per width: the short kernel and the long-query launches of 10 ... 20 words
            _score(engine, gpu, oracle, queries, candidates)
            profile = engine.last_call_profile()
            assert profile.launches > 1 and profile.queue_items == 0, (profile.launches, profile.queue_items)


def test_the_tiny_token_kernel(gpu, oracle):
    rng = random.Random(64)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    words = lambda: [_letters(rng, rng.randint(1, 12), b"etaoinshr") for _ in range(64)]
    with knob("tiny", 1):
        modes = [_score(engine, gpu, oracle, words(), words())[0] for _ in range(2)]
    assert 5 in modes, modes


def test_one_rerank_call(gpu, oracle):
    rng = random.Random(8)
    queries = [_letters(rng, length) for length in (0, 1, 31, 32, 33, 64, 65, 128, 129, 225, 256, 97)]
    candidates = [_letters(rng, rng.randint(0, 90)) for _ in range(40)] + [b"a" * 64]
    indices = np.random.default_rng(8).integers(0, len(candidates), size=(len(queries), 8), dtype=np.uint64)
    matrix = oracle.levenshtein(queries, candidates)
    want = np.array([[matrix[q, int(i)] for i in row] for q, row in enumerate(indices)], dtype=np.uint64)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    got = engine.rerank(queries, candidates, indices, device=gpu)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()

"""`-m gpu`: the head and late loops of the short Myers bodies (hip/lev_myers.hip: myers_workgroup; csrc/hip/corner_cut.h).

Every cell against the oracle.  Single queries of 65, 96, 97, 128, 160 and 256 bytes - three of a length to a batch, which leaves one of
them alone in its workgroup of the launch that plans itself; pairs whose shared vector takes 6, 9 and 10 words, one whose top word
holds the separator rows (no head loop) and one with `pad + m1 < 32`, word 0 holding the separators (no late loop - with the longer
query below, as the launch orders a pair, such a vector has two words, so this one has no phase at all).  300 candidates, one full
block and a partial one: random ones over two letters; for every query of the batch - drawn from 95 letters, so that no chance match
undercuts them - the texts whose only optimal paths run along the band's edges, and texts a few edits away from the query's shifted
copies; an empty one, texts shorter than `head_until`, and runs of consecutive lengths around `head_until`, around `late_from` and
around the query's length - the launch sorts the candidates, so such a run fills neighbouring lanes of a wavefront with texts on either
side of the bound, and its lengths take every remainder of the loops' 8 columns.  Each batch goes through the launch that plans
itself (planner mode 4) and then, on the same tapes, through the plain short kernel (mode 3: one query per workgroup).  One small
call each for callers whose column keeps the whole vector: the codepoint kernel, the long-query launches and the queue kernel.
"""
import contextlib
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import stringzilla_amd as szs  # noqa: E402
from stringzilla_amd import _abi  # noqa: E402

PAIR_WORDS = 10  # szs_myers_pair_words_k
LETTERS = bytes(range(32, 127))  # the queries' 95 letters: chance matches must not undercut the paths along the band's edges
OUTSIDE = bytes(range(1, 32))  # letters no query holds


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


def words_of(length):
    return (length + 31) // 32 if length else 1


def _adversarial(query, rng):
    """m = n: L = U = m // 2.  The query without its first `a` letters and `a` foreign ones behind it - the only optimal path runs `a`
    rows below the diagonal - and the mirror image, for a = L - 15 ... L: the band's edge and the diagonals that an iteration of 8
    columns too many would cut.  All of the query's own length: sorted, they fill wavefronts whose shortest and longest texts are
    that long, so the bounds are as tight as the header makes them.  Then d = max(m, n) exactly, and d = 0."""
    m = len(query)
    edge = m // 2
    texts = []
    for a in range(max(0, edge - 15), edge + 1):
        texts += [query[a:] + _letters(rng, a, OUTSIDE), _letters(rng, a, OUTSIDE) + query[: m - a]]
    return texts + [_letters(rng, m, OUTSIDE), _letters(rng, m + 9, OUTSIDE), query]


def _close(query, rng):
    """Texts a few edits away from the query and from its shifted copies: their optimal paths hug a diagonal inside the band, at
    every distance from its edges, and a column that drops a word too early or too late changes their distance."""
    m = len(query)
    texts = []
    for shift in (m // 8, m // 4, (3 * m) // 8, m // 2 - 3, m // 2 + 1):
        texts += [query[shift:] + _letters(rng, shift // 2, OUTSIDE), _letters(rng, shift // 2, OUTSIDE) + query[: m - shift]]
    texts += [bytes(c if rng.random() < 0.9 else rng.choice(OUTSIDE) for c in query) for _ in range(2)]
    return texts


def _candidates(rng, queries, vector):
    """300 texts for the batch `queries`, scored in the vector `vector` = (first length, second length or None, words)."""
    first_length, second_length, words = vector
    longest = max(map(len, queries))
    head_until, late_from = _abi.corner_cut_probe(first_length, second_length, words, longest, longest)
    texts = [b""]
    for query in queries:
        texts += _adversarial(query, rng) + _close(query, rng)
    lengths = list(range(1, head_until, max(1, head_until // 4)))  # shorter than head_until: the head loop and then the tail alone
    for centre in (head_until, late_from if late_from != _abi.CORNER_CUT_NEVER else 2 * longest, longest):
        lengths += [n for n in range(centre - 10, centre + 11) if n >= 0]
    lengths += [rng.randint(0, min(300, 2 * longest + 8)) for _ in range(300 - len(texts) - len(lengths))]
    texts += [_letters(rng, n) for n in lengths]
    assert len(texts) == 300, len(texts)
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
    assert not len(wrong), (len(wrong), wrong[:6].tolist(), [int(got[tuple(w)]) for w in wrong[:6]], [int(expected[tuple(w)]) for w in wrong[:6]],
                            [len(candidates[w[1]]) for w in wrong[:6]])
    alive.append((q_tape, c_tape, out))
    return int(engine.last_call_profile().planner), (q_tape, c_tape)


def _three_calls(gpu, oracle, rng, lengths, vector, expect_rule):
    """Two fresh batches of the same counts and lengths - the second plans itself inside its launch - and the second one's tapes again."""
    engine = szs.LevenshteinDistances(capabilities=gpu)
    modes = []
    for _ in range(2):
        queries = [_letters(rng, length, LETTERS) for length in lengths]
        candidates = _candidates(rng, queries, vector)
        mode, tapes = _score(engine, gpu, oracle, queries, candidates)
        modes.append(mode)
    assert modes[1] == 4, modes
    if expect_rule:
        rule, _, pairs = _abi.pair_rule_probe(lengths)
        assert int(_abi.lib.szs_rocm_last_pairing(engine.handle)) == rule, (modes, rule)
        assert pairs[0].tolist() == [0, 1]  # two queries: one slot, both in it
    mode, _ = _score(engine, gpu, oracle, queries, candidates, tapes)
    assert mode == 3, (modes, mode)  # the same tapes again: the plain short kernel behind the guard, one query per workgroup


@pytest.mark.parametrize("length", [65, 96, 97, 128, 160, 256])
def test_single_queries(gpu, oracle, length):
    """Three queries of one length: whatever two of them do, the odd one is alone in its workgroup of the launch that plans itself;
    the same tapes again score all three alone."""
    _three_calls(gpu, oracle, random.Random(length), [length] * 3, (length, None, words_of(length)), expect_rule=False)


# (first length, second length): the longer query takes the lower rows
PAIRS = {
    "6_words": (100, 88),                     # both phases
    "9_words": (140, 120),                    # the top word alone in its 16-byte chunk of the mask row
    "10_words": (160, 150),
    "separator_in_the_top_word": (160, 20),   # 6 words, s0 at bit 170: no head loop
    "separator_in_word_0": (31, 31),          # pad + m1 = 31 < 32: 2 words, the bodies without phases
}


@pytest.mark.parametrize("case", sorted(PAIRS))
def test_pairs(gpu, oracle, case):
    first, second = PAIRS[case]
    shared = (first + second + 2 + 31) // 32
    assert first >= second and shared <= min(PAIR_WORDS, words_of(first) + words_of(second))  # built to pair
    pad = 32 * shared - (first + second + 2)
    bounds = _abi.corner_cut_probe(first, second, shared, first, first)
    if case[0].isdigit():
        assert shared == int(case.split("_")[0]) and bounds[0] > 8 and bounds[1] < 2 * first, bounds
    elif case == "separator_in_the_top_word":
        assert (pad + first) // 32 == shared - 1 and bounds[0] == 0 and bounds[1] < 2 * first, bounds
    else:
        assert pad + first < 32 and bounds == (0, _abi.CORNER_CUT_NEVER), bounds
    _three_calls(gpu, oracle, random.Random(case), [first, second], (first, second, shared), expect_rule=True)


def test_the_codepoint_kernel_keeps_its_loop(gpu, oracle):
    rng = random.Random(21)
    runes = "abü"
    word = lambda: "".join(rng.choice(runes) for _ in range(rng.randint(90, 170))).encode()
    queries, candidates = [word() for _ in range(3)], [word() for _ in range(40)]
    engine = szs.LevenshteinDistancesUTF8(capabilities=gpu)
    with knob("tiny", 0):
        got = engine(queries, candidates, device=gpu)
    expected = oracle.levenshtein_utf8(queries, candidates)
    assert np.array_equal(got, expected), np.argwhere(got != expected)[:5].tolist()
    assert engine.last_call_profile().planner != 5


def test_the_queue_kernel_and_a_long_query_launch_keep_theirs(gpu, oracle):
    rng = random.Random(48)
    queries = [_letters(rng, length) for length in [1, 600, 257, 256, 320, 128] + [rng.randint(1, 600) for _ in range(10)]]
    candidates = [_letters(rng, rng.randint(0, 300)) for _ in range(48)] + _adversarial(queries[5], rng) + _adversarial(queries[3], rng)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    with knob("tier", "lanes"), knob("swap", 0):
        with knob("queue", 1):  # the one persistent launch: every width in the queue kernel's bodies
            _score(engine, gpu, oracle, queries, candidates)
            profile = engine.last_call_profile()
            assert profile.launches == 1 and profile.queue_items > 0, (profile.launches, profile.queue_items)
        with knob("queue", 0):  # one launch per width: the short kernel and the long-query launches of 10 ... 20 words
            _score(engine, gpu, oracle, queries, candidates)
            profile = engine.last_call_profile()
            assert profile.launches > 1 and profile.queue_items == 0, (profile.launches, profile.queue_items)

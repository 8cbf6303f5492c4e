"""`-m gpu`: the two few-pairs tiers - hip/systolic.hip (NW, SW, weighted and codepoint Levenshtein) and hip/myers_chain.hip
(unit-cost bytes) - at the edges of their geometry, every cell against the oracle.

tests/chained_tier_cases.py holds the cases, tests/test_chained_tiers_model.py shows on the CPU that they are what they claim:
  a. one cross-product over EXACT lengths around every lane (8 / 32 rows), band (512 / 2048 rows), step (4 / 8 columns) and
     chunk (64 / 128 columns) edge, the first length with a steady chunk and the first with two, an empty string on each side;
  b. unit-cost contents whose deltas under a band's last row are runs of one value - a copy, foreign letters, shifted copies,
     prefixes and suffixes - with a band whose partial sum is negative handing over to one where it is positive;
  c. local optima planted so that `best` of one lane, `counted_rows` of a padded lane, `inside` of a ragged step or the
     atomic maximum over the bands alone decides the score;
  d. class tables and gap costs of 127 / -127 / -128 / 0, through the int8 profile, the saturating subtract and the affine seeds.
The random fuzz of tests/test_gpu_parity.py meets these by luck of the seed; here each is present by construction.

Every call pins the tier (and `swap`) and reads which kernel ran, and in which orientation, off the call's profile.  `tier=lanes`
runs the same cases as a control: the strip kernels park their deltas and rows too.  Nothing here provokes a stalled hand-over.
"""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import stringzilla_amd as szs  # noqa: E402
from stringzilla_amd import _abi  # noqa: E402

import chained_tier_cases as cases  # noqa: E402

LANES, SYSTOLIC, CHAIN = 0, 1, 2  # CallProfile.tier (host/szs_internal.h: SZS_TIER_*)


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


built = {}
alive = []  # tapes and matrices of every call: a freed one's address handed to the next batch would look like "the same tapes"


def engine_of(gpu, engine):
    if engine not in built:
        if engine.kind == "levenshtein":
            built[engine] = szs.LevenshteinDistances(*engine.costs, capabilities=gpu)
        elif engine.kind == "levenshtein_utf8":
            built[engine] = szs.LevenshteinDistancesUTF8(*engine.costs, capabilities=gpu)
        else:
            kind = szs.SmithWatermanScores if engine.kind == "smith_waterman" else szs.NeedlemanWunschScores
            built[engine] = kind(*cases.table_of(engine.table), open=engine.costs[0], extend=engine.costs[1], capabilities=gpu)
    return built[engine]


def tapes_of(queries, candidates=None):
    tapes = (szs.Strs(list(queries)).to_device(0), None if candidates is None else szs.Strs(list(candidates)).to_device(0))
    alive.append(tapes)
    return tapes


def scored(gpu, engine, tier, ran, queries, candidates=None, swap=0, tapes=None, knobs=()):
    """One call under `tier` and `swap`, every cell against the oracle; the profile must name the tier `ran` and the orientation.
    `candidates=None`: the symmetric call, which has nothing to swap."""
    q_tape, c_tape = tapes or tapes_of(queries, candidates)
    measure = (lambda text: len(text.decode())) if engine.kind == "levenshtein_utf8" else len
    with contextlib.ExitStack() as stack:
        for name, value in (("tier", tier), ("swap", swap)) + tuple(knobs):
            stack.enter_context(knob(name, value))
        native = engine_of(gpu, engine)
        got = native(q_tape, c_tape, device=gpu).view(np.int64)
        profile = native.last_call_profile()
    want = cases.expected(engine, tuple(queries), None if candidates is None else tuple(candidates))
    others = queries if candidates is None else candidates
    wrong = np.argwhere(got != want)
    assert not len(wrong), (engine, tier, swap, knobs, len(wrong), "of", want.size, "(m, n, got, expected):",
                            [(measure(queries[q]), measure(others[c]), int(got[q, c]), int(want[q, c])) for q, c in wrong[:8]])
    assert (profile.tier, profile.transposed) == (ran, swap if candidates is not None else 0), (engine, tier, profile.tier, profile.transposed)
    return q_tape, c_tape


# ---- a. the length grids -----------------------------------------------------------------------------------------------

PROTEIN = b"ARNDC"
SYSTOLIC_ENGINES = {
    "nw_linear": (cases.Engine("needleman_wunsch", "blosum62", (-4, -4)), PROTEIN),
    "nw_affine": (cases.Engine("needleman_wunsch", "blosum62", (-11, -2)), PROTEIN),
    "sw_saturating": (cases.Engine("smith_waterman", "blosum62", (-4, -1)), PROTEIN),
    "sw_signed": (cases.Engine("smith_waterman", "blosum62", (2, -1)), PROTEIN),  # a gap that pays: padded rows must not count
    "weighted_linear": (cases.Engine("levenshtein", None, (1, 3, 3, 3)), b"ACGT"),
    "weighted_affine": (cases.Engine("levenshtein", None, (0, 1, 4, 2)), b"ACGT"),
    "codepoints": (cases.Engine("levenshtein_utf8", None, (1, 2, 3, 3)), None),
    "nw_asymmetric": (cases.Engine("needleman_wunsch", "asymmetric", (-5, -1)), bytes(range(48, 80))),
}


@pytest.mark.parametrize("name", sorted(SYSTOLIC_ENGINES))
def test_systolic_length_grid(gpu, oracle, name):
    """18 x 26 exact lengths and an empty string a side in ONE launch, then the queries alone as the symmetric call; the engine
    with the asymmetric table again with the sides swapped: the grid's columns become the bands, the kernel reads the transpose."""
    engine, alphabet = SYSTOLIC_ENGINES[name]
    queries, candidates = cases.grid("systolic", runes=True) if alphabet is None else cases.grid("systolic", alphabet)
    tapes = scored(gpu, engine, "systolic", SYSTOLIC, queries, candidates)
    scored(gpu, engine, "systolic", SYSTOLIC, queries)
    if name == "nw_asymmetric":
        scored(gpu, engine, "systolic", SYSTOLIC, queries, candidates, swap=1, tapes=tapes)


UNIT = cases.Engine("levenshtein", None, (0, 1, 1, 1))


@pytest.mark.parametrize("waves", [4, 16])
def test_chain_length_grid(gpu, oracle, waves):
    """17 x 22 exact lengths: 4 and 16 candidates against one table of match masks (23 candidates: a last workgroup of 3 or 7)."""
    queries, candidates = cases.grid("chain")
    scored(gpu, UNIT, "chain", CHAIN, queries, candidates, knobs=(("chain_waves", waves),))
    scored(gpu, UNIT, "chain", CHAIN, queries, knobs=(("chain_waves", waves),))


def test_chain_length_grid_through_both_tiers_on_the_same_tapes(gpu, oracle):
    """The unit-cost engine under `tier=systolic` scores with the DP recurrences: the chain's grid up to 2049 rows (5 bands of
    512), both tiers on the same device tapes."""
    queries, candidates = cases.grid("chain")
    queries = tuple(query for query in queries if len(query) <= 2049)
    assert len(queries) == 13 and max(map(len, queries)) == 2049
    tapes = tapes_of(queries, candidates)
    scored(gpu, UNIT, "systolic", SYSTOLIC, queries, candidates, tapes=tapes)
    scored(gpu, UNIT, "chain", CHAIN, queries, candidates, tapes=tapes)
    scored(gpu, UNIT, "systolic", SYSTOLIC, queries, candidates, tapes=tapes)  # and back: the control words of an older epoch lie below


# ---- b. structured content ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("tier,ran", [("chain", CHAIN), ("systolic", SYSTOLIC), ("lanes", LANES)])
@pytest.mark.parametrize("m", cases.STRUCTURED_M)
def test_structured_contents(gpu, oracle, m, tier, ran):
    """Runs of one delta under a whole band hand-over, partial sums of both signs.  `tier=lanes`: beyond 2048 rows the strip
    kernel, whose parked deltas get the same runs."""
    query, _, candidates = cases.structured(m)
    scored(gpu, UNIT, tier, ran, (query,), candidates)
    if tier != "lanes":  # the candidates as the bands: every one of them a chain of its own against one text
        scored(gpu, UNIT, tier, ran, (query,), candidates, swap=1)


# ---- c. planted local optima -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("tier,ran", [("systolic", SYSTOLIC), ("lanes", LANES)])
@pytest.mark.parametrize("gaps", [(-4, -4), (-11, -2)], ids=["linear", "affine"])
@pytest.mark.parametrize("m", [1100, 1024])
def test_planted_optima(gpu, oracle, m, gaps, tier, ran):
    """Every placement scores 5 a row (tests/test_chained_tiers_model.py pins that on the oracle), its control less."""
    batch = cases.planted(m)
    engine = cases.Engine("smith_waterman", "planted", gaps)
    scored(gpu, engine, tier, ran, batch.queries, batch.candidates)
    want = cases.expected(engine, batch.queries, batch.candidates)
    for placement in batch.placements:
        assert want[placement.query, placement.candidate] == cases.MATCH * placement.length > want[placement.query, placement.candidate + 1], placement


# ---- d. large costs ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("engine", cases.LARGE_ENGINES, ids=lambda e: f"{e.kind}{e.costs}".replace(" ", ""))
def test_large_costs_through_systolic(gpu, oracle, engine):
    queries, candidates = cases.large()
    scored(gpu, engine, "systolic", SYSTOLIC, queries, candidates)
    scored(gpu, engine, "systolic", SYSTOLIC, queries)


def test_large_costs_through_the_lanes_tier_as_a_control(gpu, oracle):
    queries, candidates = cases.large()
    for engine in cases.LARGE_ENGINES:
        scored(gpu, engine, "lanes", LANES, queries, candidates, knobs=(("packed", 0),))


# ---- outputs -----------------------------------------------------------------------------------------------------------


def test_outputs_into_a_padded_device_matrix_and_a_host_matrix(gpu, oracle):
    import torch

    planted = cases.planted(1100)
    query, _, family = cases.structured(2049)
    for engine, tier, ran, queries, candidates in [(cases.Engine("smith_waterman", "planted", (-4, -4)), "systolic", SYSTOLIC, planted.queries, planted.candidates),
                                                   (UNIT, "chain", CHAIN, (query,) + cases.grid("chain")[0][:3], family)]:
        want = cases.expected(engine, tuple(queries), tuple(candidates))
        padded = torch.full((len(queries), len(candidates) + 9), -7, dtype=torch.int64, device="cuda:0")  # stride > columns
        host = np.full((len(queries), len(candidates)), -7, dtype=np.int64)  # staged through a dense device copy
        with knob("tier", tier), knob("swap", 0):
            native = engine_of(gpu, engine)
            native(list(queries), list(candidates), device=gpu, out=padded[:, : len(candidates)])
            profiles = [(native.last_call_profile().tier, native.last_call_profile().transposed)]
            native(list(queries), list(candidates), device=gpu, out=host)
            profiles.append((native.last_call_profile().tier, native.last_call_profile().transposed))
        assert profiles == [(ran, 0)] * 2, profiles
        assert np.array_equal(padded[:, : len(candidates)].cpu().numpy(), want) and (padded[:, len(candidates) :] == -7).all(), tier
        assert np.array_equal(host, want), tier
        alive.append(padded)

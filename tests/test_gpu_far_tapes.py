"""Every path that reads a tape ON THE DEVICE, on tapes whose offsets lie beyond, across and just below 2^32.

All other inputs of the suite are a few kilobytes, so `(u32)offset == offset` everywhere, and the one test with offsets above 2^32
(tests/test_gpu_round2.py::test_u64_tape_with_offsets_beyond_4_gib) predates the launch that plans itself, the tiny-token launch,
the UTF-8 front ends on multibyte text, top-k, rerank and every fuzzy call.  Here ONE zeroed buffer of 2^32 + 2^20 bytes holds every
tape (tests/far_tape_cases.py says where, and what a kernel that drops the high half of an offset would read instead: a decoy batch
of the same lengths).  Every test names the route it wants from `last_call_profile()` and takes its expected values from the oracle
or from the plain NumPy DPs of the fuzzy test modules - never from the same engine on a near tape.

kinds of a two-sided call (queries, candidates): `far` (both beyond 2^32 + 12345), `far_near` / `near_far` (one side an ordinary
tape of its own), `straddling` (the candidates lie across byte 2^32, one of them with `(u32)from > (u32)to`; `_queries`: the
queries do), `top` (32-bit offsets, the candidates' last one exactly 2^32 - 1; `_queries`: the queries').

The last two tests need no GPU: the layout's own assertions, and what a truncating kernel WOULD score on the decoys.
"""
import contextlib
import random

import numpy as np
import pytest

import far_tape_cases as cases
import stringzilla_amd as szs
from stringzilla_amd import _abi, matrices
from test_gpu_fuzzy_scan import oracle as scan_oracle
from test_gpu_fuzzy_scan_matches import _mutated, expected as matches_expected, last_rows
from test_gpu_fuzzy_scan_occurrences import Oracle as OccurrencesOracle
from test_gpu_fuzzy_search import select
from test_gpu_fuzzy_spans import dense, listed
from test_gpu_rerank import expected as listed_scores
from test_gpu_round5 import WORDS
from test_gpu_round6 import ODD_BYTES, _rune_count
from test_gpu_top_k import expected_top_k

on_gpu = pytest.mark.gpu  # (no module-wide mark: the last two tests run without one)

EMPTY = np.uint64(2**64 - 1)
ASCII = bytes(range(32, 127))  # the 95 letters of tests/test_gpu_pair_rules.py
RUNES = list("etaoin") + ["é", "ß", "中", "𝄞"]  # 1, 2, 3 and 4 bytes
CROSS = ("far", "far_near", "straddling", "top")
CROSS_EITHER_NEAR = ("far", "far_near", "near_far", "straddling", "top")  # the codepoint front ends: either side's base follows the other's span
ONE_TAPE = ("far", "straddling_queries", "top_queries")


@contextlib.contextmanager
def knob(name, value):
    previous = _abi.tuning_set(name, value)
    try:
        yield
    finally:
        _abi.tuning_set(name, previous)


def _draw(rng, alphabet, length):
    return bytes(rng.choice(alphabet) for _ in range(length))


def _runes(rng, count, letters=RUNES):
    return "".join(rng.choice(letters) for _ in range(count)).encode()


def same_matrix(got, expected, *context):
    """Every cell the oracle's; says where the first five differ, and how - the decoy tells which half of an offset was dropped."""
    wrong = np.argwhere(got != expected)
    assert not len(wrong), (context, len(wrong), wrong[:5].tolist(), [int(got[tuple(w)]) for w in wrong[:5]], [int(expected[tuple(w)]) for w in wrong[:5]])


def same_arrays(got, want, *context):
    assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), (context, [np.argwhere(g != w)[:6].tolist() for g, w in zip(got, want)])


_ONCE = {}


def once(key, compute):
    """A batch and its expected values: computed by the first test that asks, shared by every kind, never changed."""
    if key not in _ONCE:
        _ONCE[key] = compute()
    return _ONCE[key]


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return szs.DeviceScope(gpu_device=0)


class FarBuffer:
    """The one buffer: zeroed, so that what a truncated or wrapped offset reads is the same in every run."""

    def __init__(self):
        import torch

        self.data = torch.zeros(cases.SIZE, dtype=torch.uint8, device="cuda:0")

    def tapes(self, kind, queries, candidates=None, seed=0):
        """-> (queries, candidates or None) as `Strs` over the buffer at the places of `kind`, their decoys written too."""
        import torch

        plan = cases.plan(kind, queries, candidates, seed)
        sides = [plan.queries] + ([] if plan.candidates is None else [plan.candidates])
        for side in sides:
            for region in side.regions:
                self.data[region.start:region.stop].zero_()
        wide = any(side.offsets is not None and side.offsets.dtype == np.uint64 for side in sides)
        tapes = []
        for side in sides:
            for position, blob in side.writes:
                if len(blob):
                    self.data[position:position + len(blob)] = torch.from_numpy(blob).to(self.data.device)
            if side.offsets is None:  # near: an ordinary tape of its own, of the other side's offset width
                tapes.append(szs.Strs(side.strings, wide_offsets=wide).to_device(0))
            else:
                signed = side.offsets.view(np.int64 if side.offsets.dtype == np.uint64 else np.int32)
                tapes.append(szs.Strs.from_device(self.data, torch.from_numpy(signed).to(self.data.device)))
        torch.cuda.synchronize()  # torch's stream wrote the bytes, the calls run on the scope's own
        return tapes[0], (tapes[1] if len(tapes) > 1 else None)

    def text(self, content):
        """`content` written around byte 2^32; -> the slice of the buffer that holds it."""
        import torch

        region = cases.TEXT_REGION
        assert len(content) == cases.TEXT
        self.data[region.start:region.stop].zero_()
        self.data[region.start:region.start + len(content)] = torch.frombuffer(bytearray(content), dtype=torch.uint8).to(self.data.device)
        torch.cuda.synchronize()
        return self.data[region.start:region.start + len(content)]


@pytest.fixture(scope="module")
def far(gpu):
    import torch

    regions = cases.check_layout()  # no two regions overlap
    assert len(regions) == 9
    buffer = FarBuffer()
    yield buffer
    del buffer.data
    torch.cuda.empty_cache()


# ---- 1. the launch that plans itself (hip/lev_myers.hip: levenshtein_myers_short_fused_kernel, its sorter, its query pairs) --------------

FUSED = {"64x300": (64, 300), "600x150": (600, 150), "symmetric": (200, None)}  # (the host swaps the roles of 600 x 150)


def _fused_batches(oracle, shape):
    def compute():
        rows, columns = FUSED[shape]
        rng = random.Random("far " + shape)
        batches = []
        for _ in range(3):
            queries = [_draw(rng, ASCII, rng.randint(96, 160)) for _ in range(rows)]
            candidates = None if columns is None else [_draw(rng, ASCII, rng.randint(96, 160)) for _ in range(columns)]
            batches.append((queries, candidates, oracle.levenshtein(queries, candidates)))
        return batches

    return once(("fused", shape), compute)


@on_gpu
@pytest.mark.parametrize("shape,kind", [(shape, kind) for shape in FUSED for kind in (ONE_TAPE if shape == "symmetric" else CROSS)])
def test_the_launch_that_plans_itself(gpu, oracle, far, shape, kind):
    """Three calls of the same counts, fresh strings rewritten into the same places: `planner == 4` on at least one of them, every
    matrix the oracle's, and `cells` - the sorter reports the sums itself - the product of the summed lengths."""
    engine = szs.LevenshteinDistances(capabilities=gpu)
    modes = []
    for call, (queries, candidates, expected) in enumerate(_fused_batches(oracle, shape)):
        q_tape, c_tape = far.tapes(kind, queries, candidates, seed=call)
        got = engine(q_tape, c_tape, device=gpu)
        profile = engine.last_call_profile()
        modes.append((int(profile.planner), int(profile.launches)))
        same_matrix(got, expected, modes)
        lengths = np.array([len(query) for query in queries], dtype=np.int64)
        if candidates is None:
            cells = int((lengths.sum() ** 2 + (lengths ** 2).sum()) // 2)
        else:
            cells = int(lengths.sum()) * sum(len(candidate) for candidate in candidates)
        assert profile.cells == cells, (modes, int(profile.cells), cells)
    print(f"{shape} {kind}: (planner, launches) {modes}")
    assert (4, 1) in modes, modes


# ---- 2. tiny tokens (hip/myers_tiny.hip: tiny_offset / tiny_extent; hip/utf8.hip: utf8_narrow_kernel) -------------------------------------


def _tiny_batches(oracle, family):
    def compute():
        rng = random.Random("far tiny " + family)
        batches = []
        for _ in range(3):
            if family == "bytes":  # 0 ... 16 bytes, and a few of 17 ... 255 that ride along in the same launch
                queries = [_draw(rng, WORDS, rng.randint(0, 16)) for _ in range(66)] + [_draw(rng, WORDS, n) for n in (17, 40, 100, 255)]
                candidates = [_draw(rng, WORDS, rng.randint(0, 16)) for _ in range(290)] + [_draw(rng, WORDS, rng.randint(17, 255)) for _ in range(10)]
                score = oracle.levenshtein
            else:  # words of 0 ... 8 runes; beyond sixteen BYTES the wavefront decodes a string (its address goes through two __shfl halves)
                queries = [_runes(rng, rng.randint(0, 8)) for _ in range(67)] + [_runes(rng, n) for n in (17, 40)] + [ODD_BYTES[2]]
                candidates = [_runes(rng, rng.randint(0, 8)) for _ in range(295)] + [_runes(rng, n) for n in (5, 30, 64, 100)] + ["é".encode()]
                score = oracle.levenshtein_utf8
            rng.shuffle(queries), rng.shuffle(candidates)
            batches.append((queries, candidates, score(queries, candidates)))
        return batches

    return once(("tiny", family), compute)


@on_gpu
@pytest.mark.parametrize("family,kind", [("bytes", kind) for kind in CROSS] + [("codepoints", kind) for kind in CROSS_EITHER_NEAR])
def test_tiny_tokens(gpu, oracle, far, family, kind):
    """70 x 300 words straight from the tapes: from the second call of these counts on `planner == 5` and ONE launch - two for the
    codepoint engine, whose strings `utf8_narrow_kernel` writes as bytes first (the route test of tests/test_gpu_round6.py)."""
    engine = (szs.LevenshteinDistances if family == "bytes" else szs.LevenshteinDistancesUTF8)(capabilities=gpu)
    size = len if family == "bytes" else _rune_count
    modes = []
    with knob("tiny", 1):
        for call, (queries, candidates, expected) in enumerate(_tiny_batches(oracle, family)):
            assert len(queries) == 70 and len(candidates) == 300 and max(map(len, queries + candidates)) > 16
            q_tape, c_tape = far.tapes(kind, queries, candidates, seed=call)
            got = engine(q_tape, c_tape, device=gpu)
            profile = engine.last_call_profile()
            modes.append((int(profile.planner), int(profile.launches)))
            same_matrix(got, expected, modes)
            if call:
                assert modes[-1] == (5, 1 if family == "bytes" else 2), modes
                assert profile.cells == sum(map(size, queries)) * sum(map(size, candidates))
    print(f"{family} {kind}: (planner, launches) {modes}")


# ---- 3. the codepoint engine's general front end (hip/utf8.hip: transcode_tape_t::locate and span, the renumbering pass) -----------------


def _codepoint_batch(oracle):
    def compute():
        rng = random.Random("far codepoints")

        def line(most_bytes):  # whole runes, at most that many bytes
            made = b""
            while True:
                rune = rng.choice(RUNES).encode()
                if len(made) + len(rune) > most_bytes:
                    return made
                made += rune

        queries = [line(rng.randint(0, 700)) for _ in range(38)] + [line(700), ODD_BYTES[0], ODD_BYTES[7]]
        candidates = [line(rng.randint(0, 700)) for _ in range(58)] + [line(650), b""] + list(ODD_BYTES)
        assert len(queries[38]) > 512 and len(candidates[58]) > 512  # the window of eight 64-byte chunks refills
        return queries, candidates, oracle.levenshtein_utf8(queries, candidates)

    return once("codepoints", compute)


@on_gpu
@pytest.mark.parametrize("planner", ["device", "host"])
@pytest.mark.parametrize("kind", CROSS_EITHER_NEAR)
def test_codepoint_front_end(gpu, oracle, far, kind, planner):
    """Multibyte lines of 0 ... 700 bytes, transcoded from the far tapes: runes renumbered (`alphabet` 1) and kept (0).  The route:
    `planner` as pinned, and `cells` the product of the RUNE counts - an engine that fell through to the byte kernels counts bytes."""
    queries, candidates, expected = _codepoint_batch(oracle)
    cells = sum(map(_rune_count, queries)) * sum(map(_rune_count, candidates))
    assert cells != sum(map(len, queries)) * sum(map(len, candidates))
    engine = szs.LevenshteinDistancesUTF8(capabilities=gpu)
    q_tape, c_tape = far.tapes(kind, queries, candidates)
    for alphabet in (1, 0):
        with knob("alphabet", alphabet), knob("planner", planner):
            got = engine(q_tape, c_tape, device=gpu)
        profile = engine.last_call_profile()
        print(f"{kind} {planner} alphabet {alphabet}: planner {profile.planner}, launches {profile.launches}, cells {profile.cells}")
        same_matrix(got, expected, alphabet)
        assert profile.planner == 0 if planner == "host" else profile.planner in (1, 2), profile.planner
        assert profile.cells == cells, (int(profile.cells), cells)


# ---- 4. the one-launch kernel (hip/myers_queue.hip) and the strip launch behind it -----------------------------------------------------


def _queue_batch(oracle):
    def compute():
        rng = random.Random("far queue")
        queries = [_draw(rng, b"AB", n) for n in (0, 1, 32, 33, 256, 257, 512, 513, 2048)]
        candidates = [_draw(rng, b"AB", rng.randint(0, 300)) for _ in range(70)]
        longer = queries + [_draw(rng, b"AB", 2049)]
        return queries, longer, candidates, oracle.levenshtein(queries, candidates), oracle.levenshtein(longer, candidates)

    return once("queue", compute)


@on_gpu
@pytest.mark.parametrize("kind", CROSS)
def test_the_queue_kernel(gpu, oracle, far, kind):
    """Every width of the queue in ONE launch (`queue_items > 0`, `launches == 1`); a query of 2049 bytes adds the strip launch."""
    queries, longer, candidates, expected, expected_longer = _queue_batch(oracle)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    with knob("tier", "lanes"), knob("queue", 1), knob("swap", 0):  # (`swap` 0: the 2049-byte string stays a query of the kernel)
        q_tape, c_tape = far.tapes(kind, queries, candidates)
        got = engine(q_tape, c_tape, device=gpu)
        profile = engine.last_call_profile()
        same_matrix(got, expected)
        assert profile.queue_items > 0 and profile.launches == 1, (profile.queue_items, profile.launches)
        q_tape, c_tape = far.tapes(kind, longer, candidates, seed=1)
        got = engine(q_tape, c_tape, device=gpu)
        profile = engine.last_call_profile()
        same_matrix(got, expected_longer)
        assert profile.queue_items > 0 and profile.launches == 2, (profile.queue_items, profile.launches)  # the queue, and the strips


# ---- 5. top-k: every tile an engine call on a sub-tape (host/top_k.c: slice_input) ------------------------------------------------------


def _top_k_batch(oracle):
    def compute():
        rng = random.Random("far top-k")
        queries = [_draw(rng, b"ACGT", rng.randint(1, 40)) for _ in range(9)]
        candidates = [_draw(rng, b"ACGT", rng.randint(1, 40)) for _ in range(70)]
        return queries, candidates, oracle.levenshtein(queries, candidates)

    return once("top-k", compute)


@on_gpu
@pytest.mark.parametrize("tile", [3, None])
@pytest.mark.parametrize("kind", CROSS)
def test_top_k(gpu, oracle, far, kind, tile):
    """9 x 70 in tiles of 3 candidates - 24 sub-tapes whose first offset is far too, their lists merged - and in one tile.  The
    route: every pair scored once, and a scoring launch and a fold per tile."""
    queries, candidates, full = _top_k_batch(oracle)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    q_tape, c_tape = far.tapes(kind, queries, candidates)
    with knob("top_k_tile", tile):
        for k in (1, 7):
            indices, scores = engine.top_k(q_tape, c_tape, k=k, device=gpu)
            profile = engine.last_call_profile()
            same_arrays((indices, scores), expected_top_k(full, k, False), tile, k)
            tiles = -(-len(candidates) // tile) if tile else 1
            assert profile.pairs == len(queries) * len(candidates)
            assert profile.launches >= 2 * tiles + 1 if tile else profile.launches < 2 * 24 + 1, (tile, profile.launches)


# ---- 6. rerank and its strips (hip/rerank_core.hpp: rerank_fetch) ---------------------------------------------------------------------


def _rerank_batch(oracle):
    def compute():
        rng = random.Random("far rerank")
        queries = [_draw(rng, b"ACGT", n) for n in (0, 1, 31, 32, 33, 255, 256)] + [_draw(rng, b"ACGT", rng.randint(0, 200)) for _ in range(9)]
        documents = [_draw(rng, b"ACGT", n) for n in (257, 300, 513, 1025)]
        candidates = [_draw(rng, b"ACGT", rng.randint(0, 160)) for _ in range(100)]
        draws = np.random.default_rng(6)
        indices = draws.integers(0, len(candidates), size=(16, 8), dtype=np.uint64)
        indices[2, 0] = indices[5, 7] = indices[9, 3:6] = EMPTY
        indices[12, :] = EMPTY  # a row that lists nothing
        of_documents = draws.integers(0, len(candidates), size=(4, 8), dtype=np.uint64)
        of_documents[1, 2] = of_documents[3, 7] = EMPTY
        return (queries, documents, candidates, indices, of_documents, listed_scores(oracle.levenshtein(queries, candidates), indices),
                listed_scores(oracle.levenshtein(documents, candidates), of_documents))

    return once("rerank", compute)


@on_gpu
@pytest.mark.parametrize("setting", [None, 0])
@pytest.mark.parametrize("kind", CROSS)
def test_rerank_and_its_strips(gpu, oracle, far, kind, setting):
    """16 rows of 8 listed candidates out of 100, queries at every width up to 256, empty slots; then four documents of 257 ... 1025
    bytes against the same candidates.  The route: what `rerank_probe` says of these lengths under the knob - the listed-pairs
    kernel (1), the strips kernel (2), or with `rerank` 0 an engine call a row (0) - and the launches that go with it."""
    queries, documents, candidates, indices, of_documents, want, want_documents = _rerank_batch(oracle)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    longest = max(map(len, candidates))
    with knob("rerank", setting):
        for rows, listing, expected, route in ((queries, indices, want, 1), (documents, of_documents, want_documents, 2)):
            q_tape, c_tape = far.tapes(kind, rows, candidates, seed=route)
            got = engine.rerank(q_tape, c_tape, listing, device=gpu)
            profile = engine.last_call_profile()
            same_matrix(got, expected, route)
            routes = _abi.rerank_probe([len(row) for row in rows], listing.shape[1], longest)[0]
            filled = [bool(row) and bool((listing[at] != EMPTY).any()) for at, row in enumerate(rows)]
            print(f"{kind} rerank={setting} route {route}: routes {routes.tolist()}, launches {profile.launches}, pairs {profile.pairs}")
            assert set(routes[np.array([bool(row) for row in rows])].tolist()) == ({route} if setting is None else {0})
            assert profile.pairs == int((listing != EMPTY).sum())
            if setting is None:
                assert profile.launches <= (4 if route == 1 else 1), profile.launches
            else:
                assert profile.launches >= sum(filled), (profile.launches, sum(filled))


# ---- 7. fuzzy find, its spans, fuzzy search (the listed-pairs scaffold again; hip/myers_fuzzy_tile.hip) --------------------------------


def _fuzzy_batch():
    def compute():
        rng = random.Random("far fuzzy")
        queries = [_draw(rng, b"ACGT", n) for n in (0, 1, 32, 33, 256)]
        candidates = [_draw(rng, b"ACGT", rng.randint(0, 700)) for _ in range(40)]
        for at, query in enumerate(queries[1:]):  # a copy of every query under 0 ... 3 edits inside two of the texts
            for where in (3 + 5 * at, 20 + 4 * at):
                text, copy = candidates[where], _mutated(rng, query, b"ACGT", at)
                if len(text) < len(copy):
                    text += _draw(rng, b"ACGT", len(copy))
                cut = rng.randint(0, len(text) - len(copy))
                candidates[where] = text[:cut] + copy + text[cut + len(copy):]
        indices = np.random.default_rng(7).integers(0, len(candidates), size=(5, 12), dtype=np.uint64)
        indices[:, 0] = [3, 3, 8, 13, 18]  # the planted texts
        indices[1, 4] = indices[3, 11] = indices[4, 5:7] = EMPTY
        want = dense(queries, candidates)
        for matrix in want:
            matrix.setflags(write=False)
        return queries, candidates, indices, want

    return once("fuzzy", compute)


@on_gpu
@pytest.mark.parametrize("kind", CROSS)
def test_fuzzy_find_spans_and_search(gpu, far, kind):
    """Queries at the word boundaries, 40 texts of 0 ... 700 bytes with mutated copies planted, against the NumPy DP of
    tests/test_gpu_fuzzy_spans.py.  The routes: one launch for (distance, end), two with the starts, `pairs` the filled slots; the
    search of one tile scores, scans, emits and runs both passes of fuzzy find on its `k` winners: five launches."""
    queries, candidates, indices, want = _fuzzy_batch()
    engine = szs.LevenshteinDistances(capabilities=gpu)
    q_tape, c_tape = far.tapes(kind, queries, candidates)
    rows, count, filled = len(queries), len(candidates), int((indices != EMPTY).sum())
    cells = listed(want, indices)

    got = engine.fuzzy_find(q_tape, c_tape, indices, device=gpu)
    profile = engine.last_call_profile()
    same_arrays(got, (cells[0], cells[2]), "find")
    assert profile.launches == 1 and profile.pairs == filled, (profile.launches, profile.pairs)

    got = engine.fuzzy_find(q_tape, c_tape, indices, device=gpu, starts=True)
    profile = engine.last_call_profile()
    same_arrays(got, cells, "spans")
    assert profile.launches == 2 and profile.pairs == filled, (profile.launches, profile.pairs)

    got = engine.fuzzy_find(q_tape, c_tape, device=gpu, starts=True)  # the dense form: every query in every text
    profile = engine.last_call_profile()
    same_arrays(got, want, "dense spans")
    assert profile.launches == 2 and profile.pairs == rows * count

    got = engine.fuzzy_search(q_tape, c_tape, k=4, device=gpu, starts=True)
    profile = engine.last_call_profile()
    same_arrays(got, select(want, 4), "search")
    assert got[1][1:, 0].max() <= 3  # the planted copies are found
    assert profile.launches == 5 and profile.pairs == rows * count + rows * 4, (profile.launches, profile.pairs)


# ---- 8. the three scans: far queries, a text across byte 2^32 --------------------------------------------------------------------------


def _scan_batch():
    def compute():
        rng = random.Random("far scan")
        queries = [_draw(rng, b"ACGT", n) for n in (0, 1, 31, 32, 33, 64, 65, 128, 255, 256)] + [_draw(rng, b"ACGT", 48)]  # the last: planted nowhere
        text = bytearray(_draw(rng, b"ACGT", cases.TEXT))
        at = 5
        for turn in range(2):
            for query in queries[1:-1]:
                copy = _mutated(rng, query, b"ACGT", (turn + len(query)) % 4)
                text[at:at + len(copy)] = copy
                at += len(copy) + 23
            at += 300
        assert at < cases.TEXT
        middle = cases.TEXT // 2
        text[middle - 30:middle + 34] = queries[5]  # an exact copy of the 64-byte query across byte 2^32 itself
        text = bytes(text[:cases.TEXT])
        last = last_rows(queries, text)
        assert last[5, middle + 34] == 0  # ... and the DP finds it there
        return queries, text, scan_oracle(queries, text), last, OccurrencesOracle(queries, text)

    return once("scan", compute)


@on_gpu
@pytest.mark.parametrize("piece", [64, None])
@pytest.mark.parametrize("kind", ONE_TAPE)
def test_the_three_scans(gpu, far, kind, piece):
    """Far queries in a 5000-byte slice of the same buffer with byte 2^32 in its middle; pieces of 64 bytes - 79 of them, two
    workgroups a row, seams everywhere - and the automatic piece.  The routes: the cut `fuzzy_scan_probe` reports, and the launches
    of one block: scan + fold + reverse pass (3), count + prefix + store (3), and the reverse pass behind those (4).  The straddling
    and the top tape want the bytes that slice lies on: their queries scan the same text in a tensor of its own."""
    import torch

    queries, text, best, last, occurrences = _scan_batch()
    engine = szs.LevenshteinDistances(capabilities=gpu)
    q_tape, _ = far.tapes(kind, queries)
    if kind == "far":
        on_device = far.text(text)
        assert on_device.data_ptr() - far.data.data_ptr() == cases.LINE - cases.TEXT // 2
    else:
        on_device = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
    with knob("fuzzy_scan_piece", piece):
        size = piece or 4096
        assert _abi.fuzzy_scan_probe(len(queries), 256, len(text))[:2] == (size, -(-len(text) // size))
        got = engine.fuzzy_scan(q_tape, on_device, device=gpu, starts=True)
        same_arrays(got, best, "scan")
        assert engine.last_call_profile().launches == 3
        for max_distance in (0, 2):
            got = engine.fuzzy_scan_matches(q_tape, on_device, max_distance, limit=8, device=gpu)
            same_arrays(got, matches_expected(queries, last, max_distance, 8), "matches", max_distance)
            assert engine.last_call_profile().launches == 3
            got = engine.fuzzy_scan_occurrences(q_tape, on_device, max_distance, limit=8, device=gpu)
            same_arrays(got, occurrences.expected(max_distance, 8), "occurrences", max_distance)
            assert engine.last_call_profile().launches == 4


# ---- 9. the four families of tests/test_gpu_round2.py on the straddling and the top tapes -----------------------------------------------


def _family_batch(oracle):
    def compute():
        rng = random.Random("far families")
        queries = [_draw(rng, b"ACGT", rng.randint(0, 300)) for _ in range(40)]
        candidates = [_draw(rng, b"ACGT", rng.randint(0, 300)) for _ in range(40)]
        nuc = matrices.nuc44()
        return queries, candidates, {
            "levenshtein": oracle.levenshtein(queries, candidates), "levenshtein_utf8": oracle.levenshtein_utf8(queries, candidates),
            "needleman_wunsch": oracle.needleman_wunsch(queries, candidates, *nuc, -4, -1),
            "smith_waterman": oracle.smith_waterman(queries, candidates, *nuc, -4, -1)}

    return once("families", compute)


@on_gpu
@pytest.mark.parametrize("planner", ["device", "host"])
@pytest.mark.parametrize("kind", ["straddling", "straddling_queries", "top", "top_queries"])
def test_every_family_across_and_below_the_line(gpu, oracle, far, kind, planner):
    """One rectangular call per family, both planners (`profile.planner` says which ran); the existing test has the `far` tape."""
    queries, candidates, expected = _family_batch(oracle)
    nuc = matrices.nuc44()
    engines = {"levenshtein": szs.LevenshteinDistances(capabilities=gpu), "levenshtein_utf8": szs.LevenshteinDistancesUTF8(capabilities=gpu),
               "needleman_wunsch": szs.NeedlemanWunschScores(*nuc, open=-4, extend=-1, capabilities=gpu),
               "smith_waterman": szs.SmithWatermanScores(*nuc, open=-4, extend=-1, capabilities=gpu)}
    q_tape, c_tape = far.tapes(kind, queries, candidates)
    with knob("planner", planner):
        for family, engine in engines.items():
            same_matrix(engine(q_tape, c_tape, device=gpu).view(np.int64), expected[family].view(np.int64), family)
            profile = engine.last_call_profile()
            assert profile.planner == (0 if planner == "host" else 1), (family, profile.planner)  # a first call: planned and waited for


# ---- without a GPU: the layout, and what the decoys are for ---------------------------------------------------------------------------


def test_the_places_are_where_the_edges_are():
    """The layout's own assertion, and the three edges in the offsets `plan()` hands out for 300 strings of 0 ... 160 bytes."""
    cases.check_layout()
    rng = random.Random(1)
    lengths = [rng.randint(0, 160) for _ in range(300)]
    for place in ("far_a", "far_b"):
        offsets = cases.offsets_at(place, lengths)
        assert offsets.dtype == np.uint64 and int(offsets.min()) >= cases.LINE + 12345 and (offsets >> np.uint64(32)).all()
    offsets = cases.offsets_at("straddle", lengths).astype(object)
    across = [at for at in range(len(lengths)) if offsets[at] < cases.LINE <= offsets[at + 1]]
    assert len(across) == 1 and (offsets[across[0]] & 0xFFFFFFFF) > (offsets[across[0] + 1] & 0xFFFFFFFF)
    assert abs((cases.LINE - offsets[0]) - sum(lengths) // 2) <= max(lengths)  # about half of the bytes on either side
    assert offsets[0] < cases.LINE - 1000 and offsets[-1] > cases.LINE + 1000
    offsets = cases.offsets_at("top_a", lengths)
    assert offsets.dtype == np.uint32 and int(offsets[-1]) == 2**32 - 1 and int(offsets[0]) == 2**32 - 1 - sum(lengths)
    assert int(cases.offsets_at("top_b", lengths)[-1]) + cases.SLACK <= int(cases.offsets_at("top_a", [cases.CAPACITY])[0])


def test_a_kernel_that_dropped_the_high_half_would_not_pass(oracle):
    """The first batch of the 64 x 300 case on the `far` tapes, read the way a kernel would that kept only the low 32 bits of every
    offset - from the oracle alone, no GPU and no library: it finds strings of the same lengths (the decoys), and scores more than
    half of the cells differently.  A truncation cannot pass by accident."""
    queries, candidates, expected = _fused_batches(oracle, "64x300")[0]
    plan = cases.plan("far", queries, candidates, seed=0)
    low = cases.low_bytes(plan.queries, plan.candidates)
    read_queries, read_candidates = cases.truncated(plan.queries, low), cases.truncated(plan.candidates, low)
    assert [len(s) for s in read_queries] == [len(s) for s in queries] and [len(s) for s in read_candidates] == [len(s) for s in candidates]
    assert all(read and read != true for read, true in zip(read_queries + read_candidates, queries + candidates))
    scored = oracle.levenshtein(read_queries, read_candidates)
    differing = float((scored != expected).mean())
    print(f"cells a truncating kernel scores differently: {differing:.3f}")
    assert differing > 0.5

"""`-m gpu`: the HIP path, called through the C-ABI, against the CPU oracle, the committed golden matrices and the
reference's known answers.  Bit-exact everywhere: this path is integer arithmetic.

Mirrors the reference's own test plan for the path: KATs (test/similarities.cuh:609-625),
fuzz equivalence over cost schemes (:654-763), cross-product shapes incl. empties (:1283-1326), kernel-tier edges
(:1961-2108), closed forms (:1006-1153) and the input-format / error behaviour of the C shim.
"""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import stringzilla_amd as szs  # noqa: E402
from stringzilla_amd import _abi, matrices, workloads  # noqa: E402


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return szs.DeviceScope(gpu_device=0)


import contextlib  # noqa: E402
import os  # noqa: E402


@contextlib.contextmanager
def forced_env(name, value):
    """Pins one tuning knob of the library for the calls inside the block (`szs_rocm_tuning_set`, csrc/host/tuning.c: the
    environment itself is only read when the library is loaded), then restores the automatic choice."""
    from stringzilla_amd import _abi

    previous = _abi.tuning_set(name, value)
    try:
        yield
    finally:
        _abi.tuning_set(name, previous)  # nested blocks restore the outer setting, not "automatic"


def forced_tier(name):
    """The `tier` knob overrides the planner's cycle model (csrc/host/plan.c)."""
    return forced_env("SZS_ROCM_TIER", name)


def _unhex(items):
    return [bytes.fromhex(x) for x in items]


def _rand(rng, count, lo, hi, alphabet):
    return [bytes(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(count)]


# ---- known answers and golden matrices --------------------------------------------------------------------------------


def test_known_answers(gpu, golden):
    _, kats = golden
    engine = szs.LevenshteinDistances(capabilities=gpu)
    for group in ("levenshtein_unit", "levenshtein_unit_python"):
        firsts = [v[0].encode() for v in kats[group]["vectors"]]
        seconds = [v[1].encode() for v in kats[group]["vectors"]]
        matrix = engine(firsts, seconds, device=gpu)
        assert matrix.dtype == np.uint64
        assert np.diagonal(matrix).tolist() == [v[2] for v in kats[group]["vectors"]]
        for first, second, expected in kats[group]["vectors"]:  # and as 1x1 calls, like the reference emulates pairs
            assert int(engine([first.encode()], [second.encode()], device=gpu)[0, 0]) == expected
    match, mismatch, open_, extend = kats["levenshtein_custom_gaps"]["costs"]
    custom = szs.LevenshteinDistances(match=match, mismatch=mismatch, open=open_, extend=extend, capabilities=gpu)
    for first, second, expected in kats["levenshtein_custom_gaps"]["vectors"]:
        assert int(custom([first.encode()], [second.encode()], device=gpu)[0, 0]) == expected, (first, second)


def test_golden_reference_matrices(gpu, golden):
    """Every matrix the real reference engines produced (tests/golden/make_golden.py) must be reproduced exactly."""
    cases, _ = golden
    tables = {k: (np.array(v["byte_to_class"], np.uint8), np.array(v["class_costs"], np.int8).reshape(32, 32))
              for k, v in cases["tables"].items()}
    engines = {}
    for case in cases["cases"]:
        queries, candidates = _unhex(case["queries"]), _unhex(case["candidates"])
        if case["kind"] == "levenshtein":
            key = ("levenshtein", tuple(case["costs"]))
            if key not in engines:
                m, x, o, e = case["costs"]
                engines[key] = szs.LevenshteinDistances(match=m, mismatch=x, open=o, extend=e, capabilities=gpu)
            dtype = np.uint64
        else:
            key = (case["kind"], case["table"], tuple(case["gaps"]))
            if key not in engines:
                cls = szs.NeedlemanWunschScores if case["kind"] == "needleman_wunsch" else szs.SmithWatermanScores
                engines[key] = cls(*tables[case["table"]], open=case["gaps"][0], extend=case["gaps"][1], capabilities=gpu)
            dtype = np.int64
        engine = engines[key]
        got = engine(queries, candidates, device=gpu)
        expected = np.array(case["matrix"], dtype=dtype).reshape(len(queries), len(candidates))
        assert np.array_equal(got, expected), (case["kind"], case["name"], key)
        sym = engine(queries, device=gpu)
        expected_sym = np.array(case["symmetric"], dtype=dtype).reshape(len(queries), len(queries))
        assert np.array_equal(sym, expected_sym), (case["kind"], case["name"], key, "symmetric")


# ---- fuzz equivalence against the oracle -------------------------------------------------------------------------------


@pytest.mark.parametrize("costs", [(0, 1, 1, 1), (1, 3, 3, 3), (0, 1, 4, 2), (0, 4, 3, 2), (2, 5, 4, 1)])
def test_levenshtein_fuzz(gpu, oracle, costs):
    rng = random.Random(hash(costs) & 0xFFFF)
    engine = szs.LevenshteinDistances(*costs, capabilities=gpu)
    for alphabet, lo, hi, q_count, c_count in [
        (b"ABC", 1, 200, 16, 16),                # the reference's default fuzz config (test/stringzilla.hpp:395-400)
        (b"ACGT", 0, 40, 9, 300),                # more than one 256-candidate workgroup, empties included
        (bytes(range(256)), 25, 40, 5, 70),      # bytes >= 0x80 (parity trap 6)
        (b"AB", 120, 136, 7, 65),                # straddles the 4-word / 5-word kernels
    ]:
        queries, candidates = _rand(rng, q_count, lo, hi, alphabet), _rand(rng, c_count, lo, hi, alphabet)
        assert np.array_equal(engine(queries, candidates, device=gpu), oracle.levenshtein(queries, candidates, *costs))
        assert np.array_equal(engine(queries, device=gpu), oracle.levenshtein(queries, None, *costs))


def test_levenshtein_every_kernel_width(gpu, oracle):
    """Queries at both edges of every bit-parallel width (1..8 words inside the mixed-width short kernel, then each
    instantiated long width up to 64 words), plus queries beyond 2048 bytes that take the strip kernel - all in ONE call,
    so the planner's grouping is exercised too: 1 short + 8 long + 1 strip launch with the `queue` knob at 0, and since round 4
    ONE persistent launch for the nine bit-parallel widths (hip/myers_queue.hip) + the strip launch."""
    rng = random.Random(77)
    edges = [0, 1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 224, 225, 256, 257, 320, 321, 384, 385, 512, 513,
             640, 768, 769, 1024, 1025, 1536, 1537, 2048, 2049, 2500]
    queries = [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in edges]
    candidates = _rand(rng, 70, 0, 300, b"ACGT") + [queries[9], queries[-1][:2100]]
    engine = szs.LevenshteinDistances(capabilities=gpu)
    expected = oracle.levenshtein(queries, candidates)
    with forced_tier("lanes"):  # 34 x 72 pairs: left alone, the planner would hand this batch to the systolic tier
        got = engine(queries, candidates, device=gpu)
        assert np.array_equal(got, expected)
        profile = engine.last_call_profile()
        assert profile.launches == 2 and profile.queue_items > 0, profile.launches
        assert profile.cells == sum(map(len, queries)) * sum(map(len, candidates))
        with forced_env("queue", 0):
            assert np.array_equal(engine(queries, candidates, device=gpu), expected)
            assert engine.last_call_profile().launches == 10, engine.last_call_profile().launches


def test_levenshtein_beyond_2048_bytes_in_strips(gpu, oracle):
    """Unit-cost byte queries of more than 2048 bytes stay bit-parallel on the lanes tier: strips of 2048 rows whose
    last-row deltas are parked 16 columns to a dword (lev_myers.hip, `levenshtein_myers_banded_kernel`).  Strip edges
    (2048 k and k +- 1 rows), texts that end on and around the 4-column and 16-column boundaries, a wavefront whose
    shortest text ends inside a group, empties, bytes >= 0x80, symmetric calls, and a batch mixing every kernel width."""
    rng = random.Random(4096)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    with forced_tier("lanes"), forced_swap("0"):
        queries = [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in (2049, 2050, 3000, 4095, 4096, 4097, 6143, 6144, 6145, 7000)]
        candidates = [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in list(range(0, 70)) + [127, 128, 129, 1000, 2047, 2048, 2049, 5000, 6500]]
        assert np.array_equal(engine(queries, candidates, device=gpu), oracle.levenshtein(queries, candidates))
        assert engine.last_call_profile().cell_bits == 0 and engine.last_call_profile().tier == 0
        ragged = _rand(rng, 300, 20, 28, bytes(range(256))) + _rand(rng, 40, 3000, 3100, bytes(range(256)))  # 24: mid-group
        wide = _rand(rng, 3, 2100, 5000, bytes(range(256)))
        assert np.array_equal(engine(wide, ragged, device=gpu), oracle.levenshtein(wide, ragged))
        mixed = _rand(rng, 12, 1, 5000, b"AB") + [b""]
        assert np.array_equal(engine(mixed, device=gpu), oracle.levenshtein(mixed, None))
        assert np.array_equal(engine(mixed, mixed[:5], device=gpu), oracle.levenshtein(mixed, mixed[:5]))


@pytest.mark.parametrize("kind", ["needleman_wunsch", "smith_waterman"])
@pytest.mark.parametrize("gaps", [(-4, -4), (-4, -1), (-1, -1), (-11, -2), (-2, -5)])
def test_alignment_fuzz(gpu, oracle, kind, gaps):
    rng = random.Random(hash((kind, gaps)) & 0xFFFF)
    asym_map = np.array([rng.randint(0, 31) for _ in range(256)], dtype=np.uint8)
    asym_tab = np.array([[rng.randint(-9, 9) for _ in range(32)] for _ in range(32)], dtype=np.int8)
    cls = szs.NeedlemanWunschScores if kind == "needleman_wunsch" else szs.SmithWatermanScores
    for (byte_to_class, class_costs), alphabet in [
        (matrices.blosum62(), b"ARNDCQEGHILKMFPSTWYVBZX"),
        (matrices.nuc44(), b"ACGTN"),
        ((asym_map, asym_tab), bytes(range(256))),  # asymmetric table: the query must pick the ROW (parity trap 5)
    ]:
        engine = cls(byte_to_class, class_costs, open=gaps[0], extend=gaps[1], capabilities=gpu)
        for lo, hi, q_count, c_count in [(1, 200, 12, 12), (0, 50, 5, 280), (15, 17, 6, 20), (30, 70, 3, 40)]:
            queries, candidates = _rand(rng, q_count, lo, hi, alphabet), _rand(rng, c_count, lo, hi, alphabet)
            expected = getattr(oracle, kind)(queries, candidates, byte_to_class, class_costs, *gaps)
            got = engine(queries, candidates, device=gpu)
            assert got.dtype == np.int64 and np.array_equal(got, expected), (kind, gaps, lo, hi)
            expected_sym = getattr(oracle, kind)(queries, None, byte_to_class, class_costs, *gaps)
            assert np.array_equal(engine(queries, device=gpu), expected_sym), (kind, gaps, lo, hi, "symmetric")


def test_alignment_wide_and_narrow_boundaries(gpu, oracle):
    """The strip boundary is parked in 16 bits when the host can bound every parked value (reach < 32000 for global,
    shortest side x largest cost for saturating local scores) and in 32 bits otherwise: score both regimes, plus local
    alignment with a POSITIVE gap cost, which takes the generic signed kernel instead of the saturating one."""
    rng = random.Random(91)
    table = matrices.blosum62()
    for lo, hi, q_count, c_count, gaps in [(1450, 1600, 2, 70, (-4, -4)), (1450, 1600, 2, 70, (-11, -2)),   # reach > 32000
                                           (100, 180, 4, 300, (-4, -1)), (3000, 3300, 1, 65, (-4, -1))]:
        queries = _rand(rng, q_count, lo, hi, b"ARNDCQEGHILKMFPSTWYV")
        candidates = _rand(rng, c_count, lo, hi, b"ARNDCQEGHILKMFPSTWYV")
        for kind in ("needleman_wunsch", "smith_waterman"):
            cls = szs.NeedlemanWunschScores if kind == "needleman_wunsch" else szs.SmithWatermanScores
            engine = cls(*table, open=gaps[0], extend=gaps[1], capabilities=gpu)
            expected = getattr(oracle, kind)(queries, candidates, *table, *gaps)
            assert np.array_equal(engine(queries, candidates, device=gpu), expected), (kind, lo, hi, gaps)
    queries, candidates = _rand(rng, 5, 20, 90, b"ACGT"), _rand(rng, 70, 20, 90, b"ACGT")
    for gaps in [(1, 1), (2, -1), (-3, 1)]:
        engine = szs.SmithWatermanScores(*matrices.nuc44(), open=gaps[0], extend=gaps[1], capabilities=gpu)
        expected = oracle.smith_waterman(queries, candidates, *matrices.nuc44(), *gaps)
        assert np.array_equal(engine(queries, candidates, device=gpu), expected), gaps


@pytest.mark.parametrize("kind", ["needleman_wunsch", "smith_waterman"])
def test_packed_and_wide_cells_agree(gpu, oracle, kind):
    """Class-table engines whose values provably fit 16 bits run hip/weighted_packed.hip (two cells per operation, the
    lower half of a strip one column behind the upper one); `SZS_ROCM_PACKED=0` pins the 32-bit kernel.  Both must give
    the oracle's matrix: every strip shape (1..70 query rows: empty lower half, ragged last strip), candidates shorter
    than one batch, empties, a 32-class asymmetric table (largest pair profile), symmetric mode, swapped sides."""
    rng = random.Random(77 if kind == "needleman_wunsch" else 78)
    asym_map = np.array([rng.randint(0, 31) for _ in range(256)], dtype=np.uint8)
    asym_map[:32] = np.arange(32, dtype=np.uint8)  # every class in use
    asym_tab = np.array([[rng.randint(-9, 9) for _ in range(32)] for _ in range(32)], dtype=np.int8)
    cls = szs.NeedlemanWunschScores if kind == "needleman_wunsch" else szs.SmithWatermanScores
    for (byte_to_class, class_costs), alphabet in [(matrices.blosum62(), b"ARNDCQEGHILKMFPSTWYVBZX*"), (matrices.nuc44(), b"ACGTN"),
                                                   ((asym_map, asym_tab), bytes(range(256)))]:
        for gaps in [(-4, -4), (-5, -1), (-1, -3)]:
            engine = cls(byte_to_class, class_costs, open=gaps[0], extend=gaps[1], capabilities=gpu)
            queries = [bytes(rng.choice(alphabet) for _ in range(length)) for length in list(range(0, 36)) + [47, 48, 49, 63, 64, 65, 70]]
            candidates = _rand(rng, 300, 0, 90, alphabet) + _rand(rng, 40, 0, 3, alphabet)
            expected = getattr(oracle, kind)(queries, candidates, byte_to_class, class_costs, *gaps)
            expected_sym = getattr(oracle, kind)(queries, None, byte_to_class, class_costs, *gaps)
            for pinned, bits in [("1", 16), ("0", 32)]:
                with forced_env("SZS_ROCM_PACKED", pinned), forced_tier("lanes"):
                    assert np.array_equal(engine(queries, candidates, device=gpu), expected), (kind, gaps, pinned)
                    assert engine.last_call_profile().cell_bits == bits
                    assert np.array_equal(engine(queries, device=gpu), expected_sym), (kind, gaps, pinned, "symmetric")
                    with forced_env("SZS_ROCM_SWAP", "1"):
                        assert np.array_equal(engine(queries, candidates, device=gpu), expected), (kind, gaps, pinned, "swapped")
                        assert engine.last_call_profile().transposed == 1 and engine.last_call_profile().cell_bits == bits
    # beyond 16 bits the packed kernel is not an option: reach (1600 + 1600 + 3) x 11 > 32000
    engine = cls(*matrices.blosum62(), open=-11, extend=-2, capabilities=gpu)
    queries, candidates = _rand(rng, 2, 1500, 1600, b"ARNDCQEGHILKMFPSTWYV"), _rand(rng, 65, 1500, 1600, b"ARNDCQEGHILKMFPSTWYV")
    expected = getattr(oracle, kind)(queries, candidates, *matrices.blosum62(), -11, -2)
    with forced_tier("lanes"):
        assert np.array_equal(engine(queries, candidates, device=gpu), expected)
        assert engine.last_call_profile().cell_bits == (32 if kind == "needleman_wunsch" else 16)


def test_cross_product_shapes(gpu, oracle):
    """1xN, Nx1, 1x1, ragged with empties, rectangular, empty sides (test/similarities.cuh:1283-1326)."""
    rng = random.Random(5)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    nw = szs.NeedlemanWunschScores(*matrices.blosum62(), open=-4, extend=-1, capabilities=gpu)
    for q_count, c_count in [(1, 9), (9, 1), (1, 1), (6, 6), (3, 11), (0, 4), (4, 0), (0, 0)]:
        queries, candidates = _rand(rng, q_count, 0, 30, b"ARND"), _rand(rng, c_count, 0, 30, b"ARND")
        if q_count == 6:
            queries[2] = b""
            candidates[4] = b""
        got = engine(queries, candidates, device=gpu)
        assert got.shape == (q_count, c_count)
        assert np.array_equal(got, oracle.levenshtein(queries, candidates))
        got = nw(queries, candidates, device=gpu)
        assert np.array_equal(got, oracle.needleman_wunsch(queries, candidates, *matrices.blosum62(), -4, -1))


def test_symmetric_universals(gpu):
    rng = random.Random(9)
    strings = _rand(rng, 300, 0, 90, b"ACGT")
    matrix = szs.LevenshteinDistances(capabilities=gpu)(strings, device=gpu)
    assert np.array_equal(matrix, matrix.T) and not np.diagonal(matrix).any()  # test/similarities.cuh:1259-1264


def test_closed_forms(gpu):
    rng = random.Random(10)
    strings = _rand(rng, 40, 0, 400, b"ACGT")
    lengths = np.array([len(s) for s in strings], dtype=np.int64)
    unit = szs.LevenshteinDistances(capabilities=gpu)
    assert np.array_equal(unit(strings, [b""], device=gpu)[:, 0], lengths.astype(np.uint64))        # d(x, "") = |x|
    assert not np.diagonal(unit(strings, strings, device=gpu)).any()                                 # d(x, x) = 0
    weird = szs.LevenshteinDistances(match=0, mismatch=2, open=5, extend=2, capabilities=gpu)
    expected = np.where(lengths > 0, 5 + 2 * (lengths - 1), 0).astype(np.uint64)                    # serial.hpp:165-175
    assert np.array_equal(weird([b""], strings, device=gpu)[0], expected)
    table = matrices.nuc44()
    sw = szs.SmithWatermanScores(*table, open=-4, extend=-1, capabilities=gpu)
    assert not sw(strings, [b""], device=gpu).any()                                                 # serial.hpp:3077-3080
    assert np.array_equal(np.diagonal(sw(strings, strings, device=gpu)), 5 * lengths)               # all matches
    nw = szs.NeedlemanWunschScores(*table, open=-4, extend=-4, capabilities=gpu)
    assert np.array_equal(nw(strings, [b""], device=gpu)[:, 0], -4 * lengths)


# ---- the C shim's formats and error behaviour -------------------------------------------------------------------------


def test_input_formats_and_result_placement(gpu, oracle):
    import torch

    rng = random.Random(21)
    queries, candidates = _rand(rng, 7, 0, 150, b"ACGT"), _rand(rng, 300, 0, 150, b"ACGT")
    expected = oracle.levenshtein(queries, candidates)
    engine = szs.LevenshteinDistances(capabilities=gpu)

    wide_q, wide_c = szs.Strs(queries, wide_offsets=True), szs.Strs(candidates, wide_offsets=True)
    assert np.array_equal(engine(wide_q, wide_c, device=gpu), expected)                   # *_u64tape

    out = np.full((7, 300), 0xDEADBEEF, dtype=np.uint64)                                  # plain host results: staged copy
    assert engine(queries, candidates, device=gpu, out=out) is out and np.array_equal(out, expected)

    padded = torch.full((7, 320), -7, dtype=torch.int64, device="cuda")                   # stride > columns
    view = padded[:, :300]
    engine(queries, candidates, device=gpu, out=view)
    assert np.array_equal(view.cpu().numpy().view(np.uint64), expected)
    assert (padded[:, 300:] == -7).all()                                                  # padding never written (cuda.cuh:2201-2203)

    # Unified memory from the library's own allocator, host-written, device-read, host-read back.
    q_tape, c_tape = szs.Strs(queries), szs.Strs(candidates)
    blocks = []

    def unified_copy(array):
        pointer = _abi.lib.szs_unified_alloc(max(array.nbytes, 1))
        assert pointer
        ctypes.memmove(pointer, array.ctypes.data, array.nbytes)
        blocks.append((pointer, array.nbytes))
        return pointer

    results_pointer = _abi.lib.szs_unified_alloc(7 * 300 * 8)
    q_struct = _abi.U32Tape(unified_copy(q_tape.data), unified_copy(q_tape.offsets), 7)
    c_struct = _abi.U32Tape(unified_copy(c_tape.data), unified_copy(c_tape.offsets), 300)
    error = ctypes.c_char_p()
    status = _abi.lib.szs_levenshtein_distances_u32tape(engine.handle, gpu.handle, ctypes.byref(q_struct), ctypes.byref(c_struct),
                                                        results_pointer, 300, ctypes.byref(error))
    assert status == 0, error.value
    unified = np.ctypeslib.as_array(ctypes.cast(results_pointer, ctypes.POINTER(ctypes.c_uint64)), shape=(7, 300))
    assert np.array_equal(unified, expected)
    for pointer, size in blocks:
        _abi.lib.szs_unified_free(pointer, size)
    _abi.lib.szs_unified_free(results_pointer, 7 * 300 * 8)


def test_callback_sequences(gpu, oracle):
    """`sz_sequence_t`: strings reached through host callbacks, each at its own device address."""
    import torch

    rng = random.Random(22)
    queries, candidates = _rand(rng, 5, 1, 60, b"ACGT"), _rand(rng, 9, 1, 60, b"ACGT")
    keep = []

    def sequence_of(strings):
        tensors = [torch.tensor(list(s), dtype=torch.uint8, device="cuda") for s in strings]
        starts = [t.data_ptr() for t in tensors]
        lengths = [len(s) for s in strings]
        get_start = _abi.MEMBER_START(lambda handle, i: starts[i])
        get_length = _abi.MEMBER_LENGTH(lambda handle, i: lengths[i])
        keep.extend([tensors, get_start, get_length])
        return _abi.Sequence(None, len(strings), get_start, get_length)

    q_seq, c_seq = sequence_of(queries), sequence_of(candidates)
    results = torch.zeros((5, 9), dtype=torch.int64, device="cuda")
    engine = szs.LevenshteinDistances(capabilities=gpu)
    error = ctypes.c_char_p()
    status = _abi.lib.szs_levenshtein_distances(engine.handle, gpu.handle, ctypes.byref(q_seq), ctypes.byref(c_seq),
                                                results.data_ptr(), 9, ctypes.byref(error))
    assert status == 0, error.value
    assert np.array_equal(results.cpu().numpy().view(np.uint64), oracle.levenshtein(queries, candidates))


def test_error_behaviour(gpu):
    engine = szs.LevenshteinDistances(capabilities=gpu)
    strs = szs.Strs([b"abc", b"abd"]).to_device(0)
    with pytest.raises(szs.StringZillasError) as failure:  # GPU engine + CPU scope (levenshtein.cuh:86)
        engine(strs, strs, device=szs.DeviceScope(cpu_cores=2))
    assert failure.value.status_name == "device_code_mismatch"

    host_data = np.frombuffer(b"abcabd", dtype=np.uint8).copy()  # plain host memory (cuda.cuh:4268-4272)
    host_offsets = np.array([0, 3, 6], dtype=np.uint32)
    tape = _abi.U32Tape(host_data.ctypes.data, host_offsets.ctypes.data, 2)
    out = np.zeros((2, 2), dtype=np.uint64)
    error = ctypes.c_char_p()
    status = _abi.lib.szs_levenshtein_distances_u32tape(engine.handle, gpu.handle, ctypes.byref(tape), ctypes.byref(tape),
                                                        out.ctypes.data, 2, ctypes.byref(error))
    assert status == -18 and error.value == b"Use device-reachable or unified memory"

    untouched = np.full((2, 2), 7, dtype=np.uint64)  # empty side: success, nothing written (cuda.cuh:4257)
    assert engine(strs, szs.Strs([]), device=gpu).shape == (2, 0)
    empty = _abi.U32Tape(host_data.ctypes.data, host_offsets.ctypes.data, 0)
    status = _abi.lib.szs_levenshtein_distances_u32tape(engine.handle, gpu.handle, ctypes.byref(empty), ctypes.byref(tape),
                                                        untouched.ctypes.data, 2, ctypes.byref(error))
    assert status == 0 and (untouched == 7).all()

    assert engine(strs, strs)[0, 1] == 1  # default scope lazily binds GPU 0 (stringzillas.cuh:303-320)
    assert "cuda" in szs.DeviceScope(gpu_device=0).capabilities and "cuda" in szs.__capabilities__

    with pytest.raises(szs.StringZillasError):
        szs.DeviceScope(gpu_device=64)


# ---- BASELINE.json configs: scaled against the oracle, full size through size-independent properties -------------------


@pytest.mark.parametrize("index,scale", [(1, 1.0), (2, 1 / 8), (3, 1 / 32), (4, 1 / 128), (5, 1 / 24)])
def test_baseline_configs_scaled(gpu, oracle, index, scale):
    load = workloads.config(index, scale=scale)
    queries = [load.queries[i] for i in range(len(load.queries))]
    candidates = [load.candidates[i] for i in range(len(load.candidates))]
    if load.kind == "levenshtein":
        engine = szs.LevenshteinDistances(**load.costs, capabilities=gpu)
        expected = oracle.levenshtein(queries, candidates, **load.costs)
    else:
        table = matrices.by_name(load.table)
        cls = szs.NeedlemanWunschScores if load.kind == "needleman_wunsch" else szs.SmithWatermanScores
        engine = cls(*table, **load.costs, capabilities=gpu)
        expected = getattr(oracle, load.kind)(queries, candidates, *table, load.costs["open"], load.costs["extend"])
    got = engine(load.queries, load.candidates, device=gpu)
    assert np.array_equal(got, expected), load.name
    assert engine.last_call_profile().cells == load.cells


def test_config2_full_size_properties(gpu, oracle):
    """1,048,576 pairs: too many for the CPU oracle in seconds, so check (a) a random sample of rows exactly,
    (b) the transposed call gives the transposed matrix, (c) the triangle inequality bounds |len(q) - len(c)| <= d <=
    max(len), (d) the self-similarity call is symmetric with a zero diagonal."""
    load = workloads.config(2)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    matrix = engine(load.queries, load.candidates, device=gpu)
    assert matrix.shape == (1024, 1024)
    rng = np.random.default_rng(0)
    rows = rng.choice(1024, size=6, replace=False)
    candidates = [load.candidates[i] for i in range(1024)]
    expected = oracle.levenshtein([load.queries[int(r)] for r in rows], candidates)
    assert np.array_equal(matrix[rows], expected)
    assert np.array_equal(engine(load.candidates, load.queries, device=gpu), matrix.T)
    q_len, c_len = load.queries.lengths()[:, None], load.candidates.lengths()[None, :]
    assert (matrix.astype(np.int64) >= np.abs(q_len - c_len)).all() and (matrix.astype(np.int64) <= np.maximum(q_len, c_len)).all()
    self_matrix = engine(load.queries, device=gpu)
    assert np.array_equal(self_matrix, self_matrix.T) and not np.diagonal(self_matrix).any()
    assert engine.last_call_profile().pairs == 1024 * 1025 // 2


@pytest.mark.parametrize("index", [3, 4, 5, 6])
def test_full_size_configs_whole_rows(gpu, oracle, index):
    """Configs 3, 4, 5 (and 5 at the codepoint level) at BASELINE.json's FULL size: the whole matrix is computed on the GPU
    and WHOLE ROWS of it - the longest, the shortest and the median query, and three more at random, each against EVERY
    candidate - are recomputed on the CPU: every lane position of every candidate block and every strip phase of the
    kernels is covered at the sizes the configs name (the reference checks every timed batch the same way,
    bench/similarities.cuh:410-423).  The checker is the reference's own engine (oracle/_ref, all host threads) when it is
    built, the plain-C oracle otherwise; the candidates take the row role there so that the threads have rows to share
    (all tables and costs of these configs are symmetric).  Size-independent properties are checked on all of it."""
    import os

    from oracle import binding

    load = workloads.config(index)
    threads = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    checker = binding.reference(tier=binding.reference_best_tier(), threads=threads) if binding.reference_available() else oracle
    if load.kind in ("levenshtein", "levenshtein_utf8"):
        cls = szs.LevenshteinDistances if load.kind == "levenshtein" else szs.LevenshteinDistancesUTF8
        engine = cls(**load.costs, capabilities=gpu)
        scorer = checker.levenshtein if load.kind == "levenshtein" else checker.levenshtein_utf8
        score = lambda rows, columns: scorer(rows, columns, **load.costs)
    else:
        table = matrices.by_name(load.table)
        cls = szs.NeedlemanWunschScores if load.kind == "needleman_wunsch" else szs.SmithWatermanScores
        engine = cls(*table, **load.costs, capabilities=gpu)
        score = lambda rows, columns: getattr(checker, load.kind)(rows, columns, *table, load.costs["open"], load.costs["extend"])
    matrix = engine(load.queries, load.candidates, device=gpu)
    assert matrix.shape == (len(load.queries), len(load.candidates))

    lengths = load.queries.lengths()
    order = np.argsort(lengths, kind="stable")
    rng = np.random.default_rng(index)
    picked = {int(order[-1]), int(order[0]), int(order[len(order) // 2])} | {int(i) for i in rng.integers(0, len(lengths), 3)}
    picked = sorted(picked)
    candidates = [load.candidates[i] for i in range(len(load.candidates))]
    expected = score(candidates, [load.queries[i] for i in picked])  # (candidates x picked rows): transposed roles
    assert np.array_equal(matrix[picked].view(np.int64), expected.T.view(np.int64)), load.name

    if index != 4:  # config 4's transposed call is another second of GPU time for no new code path
        assert np.array_equal(engine(load.candidates, load.queries, device=gpu), matrix.T)
    if load.kind == "smith_waterman":
        shortest = np.minimum(load.queries.lengths()[:, None], load.candidates.lengths()[None, :])
        assert (matrix >= 0).all() and (matrix <= 5 * shortest).all()  # NUC.4.4: a match scores 5


# ---- codepoint-level Levenshtein (szs_levenshtein_distances_utf8*) ----------------------------------------------------


@pytest.fixture(scope="module")
def golden_utf8():
    import json
    import os

    with open(os.path.join(os.path.dirname(__file__), "golden", "reference_utf8_matrices.json")) as f:
        return json.load(f)


def test_utf8_known_answers(gpu, golden):
    _, kats = golden
    unit = szs.LevenshteinDistancesUTF8(capabilities=gpu)
    for first, second, expected in kats["levenshtein_utf8_runes"]["vectors"]:
        assert int(unit([first.encode()], [second.encode()], device=gpu)[0, 0]) == expected, (first, second)
    match, mismatch, open_, extend = kats["levenshtein_utf8_custom_gaps"]["costs"]
    custom = szs.LevenshteinDistancesUTF8(match=match, mismatch=mismatch, open=open_, extend=extend, capabilities=gpu)
    for first, second, expected in kats["levenshtein_utf8_custom_gaps"]["vectors"]:
        assert int(custom([first.encode()], [second.encode()], device=gpu)[0, 0]) == expected, (first, second)


def test_utf8_golden_reference_matrices(gpu, golden_utf8):
    """Matrices produced by the reference's own UTF-8 engines (linear and affine, unit and non-unit costs, 1-4 byte
    runes, queries on both sides of the 256-rune bit-parallel limit, the degenerate corpus of test/similarities.py)."""
    engines = {}
    for case in golden_utf8["cases"]:
        costs = tuple(case["costs"])
        if costs not in engines:
            m, x, o, e = costs
            engines[costs] = szs.LevenshteinDistancesUTF8(match=m, mismatch=x, open=o, extend=e, capabilities=gpu)
        queries, candidates = _unhex(case["queries"]), _unhex(case["candidates"])
        got = engines[costs](queries, candidates, device=gpu)
        expected = np.array(case["matrix"], dtype=np.uint64).reshape(len(queries), len(candidates))
        assert got.dtype == np.uint64 and np.array_equal(got, expected), (case["name"], costs)
        sym = engines[costs](queries, device=gpu)
        expected_sym = np.array(case["symmetric"], dtype=np.uint64).reshape(len(queries), len(queries))
        assert np.array_equal(sym, expected_sym), (case["name"], costs, "symmetric")


@pytest.mark.parametrize("costs", [(0, 1, 1, 1), (1, 3, 3, 3), (0, 1, 4, 2)])
def test_utf8_fuzz(gpu, oracle, costs):
    rng = random.Random(hash(costs) & 0xFFF)
    engine = szs.LevenshteinDistancesUTF8(*costs, capabilities=gpu)
    pools = ["AÉ中😀", "abc абв", "日本語中文字漢", "aé中😀bñ語🚀 ", "".join(chr(0x4E00 + i) for i in range(400))]
    for pool in pools:
        for lo, hi, q_count, c_count in [(0, 48, 7, 300), (200, 300, 3, 70), (1, 20, 64, 5)]:
            text = lambda: "".join(rng.choice(pool) for _ in range(rng.randint(lo, hi))).encode()
            queries, candidates = [text() for _ in range(q_count)], [text() for _ in range(c_count)]
            expected = oracle.levenshtein_utf8(queries, candidates, *costs)
            assert np.array_equal(engine(queries, candidates, device=gpu), expected), (pool[:4], lo, hi)
    # ASCII corpus: the byte kernels take over and must agree with both oracles
    strings = [bytes(rng.choice(b"ACGT ") for _ in range(rng.randint(0, 90))) for _ in range(40)]
    assert np.array_equal(engine(strings, device=gpu), oracle.levenshtein_utf8(strings, None, *costs))
    assert np.array_equal(engine(strings, device=gpu), oracle.levenshtein(strings, None, *costs))


def test_utf8_long_queries_stay_bit_parallel(gpu, oracle):
    """Queries of 257..2048 runes take the long rune kernels (dense rune ids in dynamic LDS): every instantiated width,
    texts whose distinct runes exceed the id table (the overflow runes are matched against the pattern directly) both
    naturally - 1500 distinct CJK runes in one query - and with the table shrunk to 5 ids, symmetric calls, empties."""
    rng = random.Random(2049)
    small = "abcdefghij klmno\u00e9\u00f1\u0436\u0444\u4e2d\u6587\U0001F600"
    wide = [chr(c) for c in range(0x4E00, 0x4E00 + 3000)]
    def text(alphabet, runes):
        return "".join(rng.choice(alphabet) for _ in range(runes)).encode("utf-8")
    engine = szs.LevenshteinDistancesUTF8(capabilities=gpu)
    queries = [text(small, n) for n in (257, 300, 320, 321, 384, 385, 500, 512, 513, 640, 700, 768, 769, 1000, 1024, 1025, 1500, 1536, 1537, 2000, 2048)]
    candidates = [text(small, rng.randint(0, 2100)) for _ in range(30)] + [b"", text(small, 1), text(wide, 900)]
    expected = oracle.levenshtein_utf8(queries, candidates)
    with forced_tier("lanes"), forced_swap("0"):
        assert np.array_equal(engine(queries, candidates, device=gpu), expected)
        assert engine.last_call_profile().cell_bits == 0  # no DP kernel ran: bit-parallel all the way
        with forced_env("SZS_ROCM_RUNE_IDS", "5"):
            assert np.array_equal(engine(queries, candidates, device=gpu), expected)
        rich = [text(wide, n) for n in (300, 900, 1500, 2048)] + [text(small, 1200)]
        others = [text(wide, rng.randint(200, 2048)) for _ in range(10)] + rich[:2]
        assert np.array_equal(engine(rich, others, device=gpu), oracle.levenshtein_utf8(rich, others))
        assert np.array_equal(engine(rich, device=gpu), oracle.levenshtein_utf8(rich, None))
    # beyond 2048 runes: strips of 2048 runes, the rune table rebuilt per strip - still no DP kernel
    longer = [text(small, 2049), text(small, 2500), text(small, 4096), text(small, 4097), text(wide, 5000), text(small, 6200)]
    texts = candidates[:9] + [text(wide, 900), text(wide, 3000), text(small, 17), text(small, 16), text(small, 33)]
    with forced_tier("lanes"), forced_swap("0"):  # (left alone, the planner would put the shorter side on the bit-vectors)
        assert np.array_equal(engine(longer, texts, device=gpu), oracle.levenshtein_utf8(longer, texts))
        assert engine.last_call_profile().cell_bits == 0
        with forced_env("SZS_ROCM_RUNE_IDS", "5"):  # nearly every rune overflows the table: masks straight from the pattern
            assert np.array_equal(engine(longer[:3], texts[:6], device=gpu), oracle.levenshtein_utf8(longer[:3], texts[:6]))
        assert np.array_equal(engine(longer[:4], device=gpu), oracle.levenshtein_utf8(longer[:4], None))  # symmetric


def test_utf8_malformed_bytes_follow_the_unchecked_contract(gpu, oracle):
    """`sz_rune_decode_unchecked`: stray continuation bytes, unvalidated tails, over-long leads - never an error."""
    engine = szs.LevenshteinDistancesUTF8(capabilities=gpu)
    strings = [b"\x80\xbfabc", b"\xc3\x41\xc3", b"ab\xe4\xb8", b"\xf8\x80\x80\x80A", "é中".encode(), b"", b"\xff\xfe\xfd\xfc\xfb"]
    assert np.array_equal(engine(strings, strings, device=gpu), oracle.levenshtein_utf8(strings, strings))


# ---- the systolic (few-pairs) tier: hip/systolic.hip -----------------------------------------------------------------


def test_systolic_known_answers_and_golden_matrices(gpu, golden):
    """Everything the real reference engines produced must come out of the systolic tier as well."""
    cases, kats = golden
    with forced_tier("systolic"):
        engine = szs.LevenshteinDistances(capabilities=gpu)
        for group in ("levenshtein_unit", "levenshtein_unit_python"):
            firsts = [v[0].encode() for v in kats[group]["vectors"]]
            seconds = [v[1].encode() for v in kats[group]["vectors"]]
            assert np.diagonal(engine(firsts, seconds, device=gpu)).tolist() == [v[2] for v in kats[group]["vectors"]]
            assert engine.last_call_profile().tier == 1
        tables = {k: (np.array(v["byte_to_class"], np.uint8), np.array(v["class_costs"], np.int8).reshape(32, 32))
                  for k, v in cases["tables"].items()}
        engines = {}
        for case in cases["cases"]:
            queries, candidates = _unhex(case["queries"]), _unhex(case["candidates"])
            if case["kind"] == "levenshtein":
                key = ("levenshtein", tuple(case["costs"]))
                if key not in engines:
                    m, x, o, e = case["costs"]
                    engines[key] = szs.LevenshteinDistances(match=m, mismatch=x, open=o, extend=e, capabilities=gpu)
                dtype = np.uint64
            else:
                key = (case["kind"], case["table"], tuple(case["gaps"]))
                if key not in engines:
                    cls = szs.NeedlemanWunschScores if case["kind"] == "needleman_wunsch" else szs.SmithWatermanScores
                    engines[key] = cls(*tables[case["table"]], open=case["gaps"][0], extend=case["gaps"][1], capabilities=gpu)
                dtype = np.int64
            got = engines[key](queries, candidates, device=gpu)
            expected = np.array(case["matrix"], dtype=dtype).reshape(len(queries), len(candidates))
            assert np.array_equal(got, expected), (case["kind"], case["name"], key)
            sym = engines[key](queries, device=gpu)
            expected_sym = np.array(case["symmetric"], dtype=dtype).reshape(len(queries), len(queries))
            assert np.array_equal(sym, expected_sym), (case["kind"], case["name"], key, "symmetric")


@pytest.mark.parametrize("kind", ["needleman_wunsch", "smith_waterman"])
@pytest.mark.parametrize("gaps", [(-4, -4), (-4, -1), (-11, -2), (2, -1)])
def test_systolic_alignment_fuzz(gpu, oracle, kind, gaps):
    """Band edges (512 rows per wavefront), lane edges (8 rows per lane), the 64-column hand-over chunks, empties, more
    candidates than lanes, asymmetric tables; local alignment with a positive gap cost takes the non-saturating form.
    Random lengths and letters: the exact edges, planted optima and large costs are in tests/test_gpu_chained_tiers.py."""
    rng = random.Random(hash((kind, gaps)) & 0xFFFF)
    asym_map = np.array([rng.randint(0, 31) for _ in range(256)], dtype=np.uint8)
    asym_tab = np.array([[rng.randint(-9, 9) for _ in range(32)] for _ in range(32)], dtype=np.int8)
    cls = szs.NeedlemanWunschScores if kind == "needleman_wunsch" else szs.SmithWatermanScores
    if kind == "needleman_wunsch" and gaps[0] > 0:
        pytest.skip("positive gap costs are exercised on the local form only")
    with forced_tier("systolic"):
        for (byte_to_class, class_costs), alphabet in [
            (matrices.blosum62(), b"ARNDCQEGHILKMFPSTWYVBZX"),
            (matrices.nuc44(), b"ACGTN"),
            ((asym_map, asym_tab), bytes(range(256))),
        ]:
            engine = cls(byte_to_class, class_costs, open=gaps[0], extend=gaps[1], capabilities=gpu)
            for lo, hi, q_count, c_count in [(0, 20, 9, 9), (1, 200, 6, 12), (500, 530, 4, 5), (1000, 1100, 2, 3),
                                             (60, 70, 3, 70), (1530, 1540, 1, 2)]:
                queries, candidates = _rand(rng, q_count, lo, hi, alphabet), _rand(rng, c_count, lo, hi, alphabet)
                expected = getattr(oracle, kind)(queries, candidates, byte_to_class, class_costs, *gaps)
                got = engine(queries, candidates, device=gpu)
                assert engine.last_call_profile().tier == 1
                assert np.array_equal(got, expected), (kind, gaps, lo, hi)
                expected_sym = getattr(oracle, kind)(queries, None, byte_to_class, class_costs, *gaps)
                assert np.array_equal(engine(queries, device=gpu), expected_sym), (kind, gaps, lo, hi, "symmetric")


@pytest.mark.parametrize("costs", [(0, 1, 1, 1), (1, 3, 3, 3), (0, 1, 4, 2), (2, 5, 4, 1)])
def test_systolic_levenshtein_fuzz(gpu, oracle, costs):
    """Weighted and codepoint Levenshtein through hip/systolic.hip, random lengths and letters; the exact lane, band, step and
    chunk edges are in tests/test_gpu_chained_tiers.py."""
    rng = random.Random(hash(costs) & 0xFFFF)
    with forced_tier("systolic"):
        engine = szs.LevenshteinDistances(*costs, capabilities=gpu)
        for alphabet, lo, hi, q_count, c_count in [(b"ABC", 0, 200, 8, 8), (bytes(range(256)), 25, 40, 5, 70),
                                                   (b"ACGT", 505, 520, 3, 4), (b"AB", 1020, 1030, 2, 3)]:
            queries, candidates = _rand(rng, q_count, lo, hi, alphabet), _rand(rng, c_count, lo, hi, alphabet)
            assert np.array_equal(engine(queries, candidates, device=gpu), oracle.levenshtein(queries, candidates, *costs))
            assert engine.last_call_profile().tier == 1
            assert np.array_equal(engine(queries, device=gpu), oracle.levenshtein(queries, None, *costs))
        runes = szs.LevenshteinDistancesUTF8(*costs, capabilities=gpu)
        for pool in ["AÉ中😀", "aé中😀bñ語🚀 ", "".join(chr(0x4E00 + i) for i in range(400))]:
            for lo, hi, q_count, c_count in [(0, 48, 5, 9), (500, 530, 2, 3)]:
                text = lambda: "".join(rng.choice(pool) for _ in range(rng.randint(lo, hi))).encode()
                queries, candidates = [text() for _ in range(q_count)], [text() for _ in range(c_count)]
                expected = oracle.levenshtein_utf8(queries, candidates, *costs)
                assert np.array_equal(runes(queries, candidates, device=gpu), expected), (pool[:4], lo, hi)
                assert runes.last_call_profile().tier == 1


def test_systolic_long_pairs_pick_the_tier_themselves(gpu, oracle):
    """A handful of long pairs: the planner's cycle model must route them to the systolic tier on its own (a band chain of
    ten wavefronts per pair here), and a million short pairs must stay on the lanes tier."""
    rng = random.Random(123)
    queries, candidates = _rand(rng, 2, 4800, 5200, b"ACGT"), _rand(rng, 3, 4800, 5200, b"ACGT")
    table = matrices.nuc44()
    for cls, kind, gaps in [(szs.NeedlemanWunschScores, "needleman_wunsch", (-4, -4)),
                            (szs.SmithWatermanScores, "smith_waterman", (-4, -1)),
                            (szs.NeedlemanWunschScores, "needleman_wunsch", (-5, -2))]:
        engine = cls(*table, open=gaps[0], extend=gaps[1], capabilities=gpu)
        got = engine(queries, candidates, device=gpu)
        assert engine.last_call_profile().tier == 1, kind
        assert np.array_equal(got, getattr(oracle, kind)(queries, candidates, *table, *gaps)), (kind, gaps)
    unit = szs.LevenshteinDistances(capabilities=gpu)
    assert np.array_equal(unit(queries, candidates, device=gpu), oracle.levenshtein(queries, candidates))
    assert unit.last_call_profile().tier == 2  # unit costs: the bit-parallel band chain (hip/myers_chain.hip)
    load = workloads.config(2, scale=1 / 4)
    unit(load.queries, load.candidates, device=gpu)
    assert unit.last_call_profile().tier == 0


def test_myers_chain_fuzz(gpu, oracle):
    """hip/myers_chain.hip: band edges (2048 rows per wavefront), word edges (32 rows per lane), the 8-column steps and
    128-column hand-over chunks, empties, bytes >= 0x80, ragged batches, symmetric calls, swapped sides.  Random lengths and
    letters: the exact edges and the structured contents (runs of one delta, partial sums of both signs) are in
    tests/test_gpu_chained_tiers.py."""
    rng = random.Random(2048)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    with forced_tier("chain"):
        for alphabet, lo, hi, q_count, c_count in [(b"ABC", 0, 70, 9, 9), (bytes(range(256)), 25, 40, 5, 70), (b"ACGT", 120, 136, 7, 5),
                                                   (b"AB", 2040, 2056, 3, 4), (b"ACGT", 4090, 4100, 2, 3), (b"ACGT", 1, 6200, 6, 6),
                                                   (b"ACGT", 500, 530, 64, 3)]:
            queries, candidates = _rand(rng, q_count, lo, hi, alphabet), _rand(rng, c_count, lo, hi, alphabet)
            assert np.array_equal(engine(queries, candidates, device=gpu), oracle.levenshtein(queries, candidates)), (lo, hi)
            assert engine.last_call_profile().tier == 2
            assert np.array_equal(engine(queries, device=gpu), oracle.levenshtein(queries, None)), (lo, hi, "symmetric")
        with forced_swap("1"):
            queries, candidates = _rand(rng, 3, 100, 2500, b"ACGT"), _rand(rng, 5, 100, 5000, b"ACGT")
            assert np.array_equal(engine(queries, candidates, device=gpu), oracle.levenshtein(queries, candidates))
            assert engine.last_call_profile().transposed == 1


@pytest.mark.parametrize("waves", ["4", "8", "16"])
def test_myers_chain_shares_one_mask_table_between_candidates(gpu, oracle, waves):
    """A workgroup of hip/myers_chain.hip scores 4 / 8 / 16 candidates against ONE query band (one 64 KB match-mask table):
    candidate counts that do not fill the last workgroup, queries of one and of several bands in one batch, symmetric
    calls (wavefronts above the diagonal leave after the table is built), and the launcher's own choice at a size where
    it picks 16.  The exact-length grid under 4 and 16 wavefronts is in tests/test_gpu_chained_tiers.py."""
    rng = random.Random(int(waves))
    engine = szs.LevenshteinDistances(capabilities=gpu)
    with forced_tier("chain"), forced_env("SZS_ROCM_CHAIN_WAVES", waves), forced_swap("0"):
        for q_count, c_count, lo, hi in [(3, 1, 10, 300), (5, 13, 0, 2300), (9, 37, 1900, 2200), (2, 70, 4000, 4300)]:
            queries, candidates = _rand(rng, q_count, lo, hi, b"ACGT"), _rand(rng, c_count, lo, hi, b"ACGTN")
            assert np.array_equal(engine(queries, candidates, device=gpu), oracle.levenshtein(queries, candidates)), (q_count, c_count)
            assert engine.last_call_profile().tier == 2
        queries = _rand(rng, 21, 1500, 2600, b"ACGT")
        assert np.array_equal(engine(queries, device=gpu), oracle.levenshtein(queries, None))
    if waves == "16":  # 70 x 70 x 2 bands = 9800 wavefronts: the launcher goes to 16 per workgroup by itself
        queries, candidates = _rand(rng, 70, 2100, 2300, b"ACGT"), _rand(rng, 70, 2100, 2300, b"ACGT")
        with forced_tier("chain"), forced_swap("0"):
            assert np.array_equal(engine(queries, candidates, device=gpu), oracle.levenshtein(queries, candidates))


def test_systolic_single_very_long_pair(gpu, oracle):
    """1 x 1 call of two 40 KB strings (the reference's `score_across_cuda_device_` regime, cuda.cuh:715-716):
    79 bands in flight, checked exactly; then both orders of an uneven pair."""
    rng = random.Random(321)
    first, second = _rand(rng, 1, 40000, 40000, b"ACGT"), _rand(rng, 1, 40500, 40500, b"ACGT")
    nw = szs.NeedlemanWunschScores(*matrices.nuc44(), open=-4, extend=-1, capabilities=gpu)
    expected = oracle.needleman_wunsch(first, second, *matrices.nuc44(), -4, -1)
    assert np.array_equal(nw(first, second, device=gpu), expected)
    assert nw.last_call_profile().tier == 1
    assert np.array_equal(nw(second, first, device=gpu), expected.T)  # NUC.4.4 is symmetric
    unit = szs.LevenshteinDistances(capabilities=gpu)
    short = [first[0][:700]]
    assert np.array_equal(unit(first, short, device=gpu), oracle.levenshtein(first, short))
    assert np.array_equal(unit(short, first, device=gpu), oracle.levenshtein(short, first))


# ---- orientation: the planner may put the candidates on workgroups and the queries on lanes -----------------------------


def forced_swap(value):
    return forced_env("SZS_ROCM_SWAP", value)


@pytest.mark.parametrize("tier", ["lanes", "systolic"])
def test_swapped_sides_give_the_same_matrix(gpu, oracle, tier):
    """Forced swap on every engine family, with an ASYMMETRIC class table (the kernel must then see its transpose),
    ragged rectangular shapes, a padded device matrix and a staged host matrix."""
    import torch

    rng = random.Random(404)
    asym_map = np.array([rng.randint(0, 31) for _ in range(256)], dtype=np.uint8)
    asym_tab = np.array([[rng.randint(-9, 9) for _ in range(32)] for _ in range(32)], dtype=np.int8)
    queries, candidates = _rand(rng, 7, 0, 120, bytes(range(256))), _rand(rng, 70, 0, 90, bytes(range(256)))
    with forced_tier(tier), forced_swap("1"):
        for costs in [(0, 1, 1, 1), (1, 3, 3, 3), (0, 2, 4, 1)]:
            engine = szs.LevenshteinDistances(*costs, capabilities=gpu)
            assert np.array_equal(engine(queries, candidates, device=gpu), oracle.levenshtein(queries, candidates, *costs))
            assert engine.last_call_profile().transposed == 1
        for kind, cls in [("needleman_wunsch", szs.NeedlemanWunschScores), ("smith_waterman", szs.SmithWatermanScores)]:
            for gaps in [(-3, -3), (-5, -1)]:
                engine = cls(asym_map, asym_tab, open=gaps[0], extend=gaps[1], capabilities=gpu)
                expected = getattr(oracle, kind)(queries, candidates, asym_map, asym_tab, *gaps)
                assert np.array_equal(engine(queries, candidates, device=gpu), expected), (kind, gaps)
                assert engine.last_call_profile().transposed == 1
                padded = torch.full((7, 80), -7, dtype=torch.int64, device="cuda")  # stride > columns
                engine(queries, candidates, device=gpu, out=padded[:, :70])
                assert np.array_equal(padded[:, :70].cpu().numpy(), expected) and (padded[:, 70:] == -7).all()
                host = np.zeros((7, 70), dtype=np.int64)                             # staged through a dense device copy
                engine(queries, candidates, device=gpu, out=host)
                assert np.array_equal(host, expected)
                with forced_swap("0"):  # the same engine, back in the caller's orientation: the table is re-uploaded
                    assert np.array_equal(engine(queries, candidates, device=gpu), expected)
                    assert engine.last_call_profile().transposed == 0
        utf8 = szs.LevenshteinDistancesUTF8(capabilities=gpu)
        texts = lambda count, lo, hi: ["".join(rng.choice("aé中😀bñ") for _ in range(rng.randint(lo, hi))).encode() for _ in range(count)]
        q, c = texts(5, 0, 60), texts(9, 0, 40)
        assert np.array_equal(utf8(q, c, device=gpu), oracle.levenshtein_utf8(q, c))


def test_tall_cross_products_are_turned_on_their_side(gpu, oracle):
    rng = random.Random(405)
    queries, candidates = _rand(rng, 6000, 90, 140, b"ACGT"), _rand(rng, 2, 90, 140, b"ACGT")  # 6000 one-lane wavefronts, or 188 full ones
    engine = szs.LevenshteinDistances(capabilities=gpu)
    assert np.array_equal(engine(queries, candidates, device=gpu), oracle.levenshtein(queries, candidates))
    assert engine.last_call_profile().transposed == 1 and engine.last_call_profile().tier == 0
    assert np.array_equal(engine(candidates, queries, device=gpu), oracle.levenshtein(candidates, queries))
    assert engine.last_call_profile().transposed == 0


# ---- rolling MinHash / Count-Min fingerprints (szs_fingerprints_*; hip/fingerprints.hip) ------------------------------


def test_fingerprints_golden_reference(gpu):
    """What the reference's serial engines produced (64-dimension slices and per-dimension fallback alike)."""
    import json

    with open(os.path.join(os.path.dirname(__file__), "golden", "reference_fingerprints.json")) as f:
        cases = json.load(f)["cases"]
    for case in cases:
        engine = szs.Fingerprints(case["dimensions"], window_widths=case["window_widths"], seed=case["seed"], capabilities=gpu)
        hashes, counts = engine(_unhex(case["texts"]), device=gpu)
        assert hashes.dtype == np.uint32 and hashes.shape == (len(case["texts"]), case["dimensions"])
        assert np.array_equal(hashes, np.array(case["min_hashes"], dtype=np.uint32)), case["name"]
        assert np.array_equal(counts, np.array(case["min_counts"], dtype=np.uint32)), case["name"]


def test_fingerprints_fuzz(gpu):
    """Empty texts, texts shorter than / equal to a window, several 4096-position segments per text (merged on the
    device), every byte value, odd dimension counts (idle lanes), wide tapes, NumPy `out=` buffers (staged copy)."""
    from oracle import binding

    rng = random.Random(64)
    for dimensions, widths, seed in [(64, [7], 0), (512, None, 1), (1024, None, 2), (100, None, 3), (13, [2, 4, 31], 4), (320, [3, 1024], 5)]:
        texts = [bytes(rng.randrange(256) for _ in range(n))
                 for n in [0, 1, 2, 3, 6, 7, 8, 30, 31, 32, 100, 1023, 1024, 1025, 4095, 4096, 4097, 9000, rng.randint(0, 20000)]]
        engine = szs.Fingerprints(dimensions, window_widths=widths, seed=seed, capabilities=gpu)
        expected = binding.oracle_fingerprints(texts, dimensions, widths, seed)
        got = engine(texts, device=gpu)
        assert np.array_equal(got[0], expected[0]) and np.array_equal(got[1], expected[1]), (dimensions, widths)
        wide = engine(szs.Strs(texts, wide_offsets=True), device=gpu)
        assert np.array_equal(wide[0], expected[0]) and np.array_equal(wide[1], expected[1]), (dimensions, "u64tape")
        out = (np.zeros((len(texts), dimensions), np.uint32), np.zeros((len(texts), dimensions), np.uint32))
        engine(texts, device=gpu, out=out)
        assert np.array_equal(out[0], expected[0]) and np.array_equal(out[1], expected[1]), (dimensions, "out=")
    assert szs.Fingerprints(64, capabilities=gpu)([], device=gpu)[0].shape == (0, 64)
    # windows wider than the 1024 bytes the kernel stages in LDS read the text in place (round 4): wider than a segment of 4096
    # window ends, wider than most of the texts, mixed with narrow ones
    for dimensions, widths, seed in [(128, [1025], 6), (192, [3, 5000, 31], 7), (64, [20000], 8), (70, [4097, 2, 65536], 9)]:
        texts = [bytes(rng.randrange(256) for _ in range(n)) for n in [0, 5, 1024, 1025, 1026, 4096, 5000, 5001, 9000, 20000, 20001, 30000]]
        engine = szs.Fingerprints(dimensions, window_widths=widths, seed=seed, capabilities=gpu)
        expected = binding.oracle_fingerprints(texts, dimensions, widths, seed)
        got = engine(texts, device=gpu)
        assert np.array_equal(got[0], expected[0]) and np.array_equal(got[1], expected[1]), (dimensions, widths)
    with pytest.raises(szs.StringZillasError):
        szs.Fingerprints(64, window_widths=[65537], capabilities=gpu)
    with pytest.raises(szs.StringZillasError):
        szs.Fingerprints(64, window_widths=[1], capabilities=gpu)  # the reference asserts width > 1
    with pytest.raises(szs.StringZillasError):
        szs.Fingerprints(64, capabilities=("serial",))


def test_fingerprints_callback_sequences_and_unified_outputs(gpu):
    """`szs_fingerprints_sequence` (strings reached through host callbacks, each at its own device address) and outputs in
    unified memory with a padded row stride."""
    import torch

    from oracle import binding

    rng = random.Random(65)
    texts = [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in (0, 5, 64, 300, 5000)]
    tensors = [torch.tensor(list(t) or [0], dtype=torch.uint8, device="cuda") for t in texts]
    starts, lengths = [t.data_ptr() for t in tensors], [len(t) for t in texts]
    get_start = _abi.MEMBER_START(lambda handle, i: starts[i])
    get_length = _abi.MEMBER_LENGTH(lambda handle, i: lengths[i])
    sequence = _abi.Sequence(None, len(texts), get_start, get_length)
    engine = szs.Fingerprints(128, window_widths=[4, 9], seed=11, capabilities=gpu)
    stride = 128 * 4 + 32
    hashes_pointer = _abi.lib.szs_unified_alloc(len(texts) * stride)
    counts_pointer = _abi.lib.szs_unified_alloc(len(texts) * stride)
    ctypes.memset(hashes_pointer, 0xEE, len(texts) * stride), ctypes.memset(counts_pointer, 0xEE, len(texts) * stride)
    error = ctypes.c_char_p()
    status = _abi.lib.szs_fingerprints_sequence(engine.handle, gpu.handle, ctypes.byref(sequence), hashes_pointer, stride,
                                                counts_pointer, stride, ctypes.byref(error))
    assert status == 0, error.value
    expected = binding.oracle_fingerprints(texts, 128, [4, 9], seed=11)
    for pointer, want in ((hashes_pointer, expected[0]), (counts_pointer, expected[1])):
        raw = np.ctypeslib.as_array(ctypes.cast(pointer, ctypes.POINTER(ctypes.c_uint32)), shape=(len(texts), stride // 4))
        assert np.array_equal(raw[:, :128], want)
        assert (raw[:, 128:] == 0xEEEEEEEE).all()  # padding never written
    _abi.lib.szs_unified_free(hashes_pointer, len(texts) * stride), _abi.lib.szs_unified_free(counts_pointer, len(texts) * stride)

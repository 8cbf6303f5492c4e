"""Cases for the two few-pairs tiers, hip/systolic.hip and hip/myers_chain.hip, at the edges of their geometry: exact lengths
around every band, lane, step and chunk boundary; contents whose deltas under a band's last row are runs of one value; local
optima planted where one mechanism alone decides the score; costs of 127 / -128.  Nothing here is random but the letters, and
those come from fixed seeds.

A plain module: no fixtures, no settings, no GPU.  tests/test_chained_tiers_model.py (CPU: the cases are what they claim to be)
and tests/test_gpu_chained_tiers.py (the kernels against the oracle) import it.  The oracle's matrices are cached and shared
between tests: they must not be written to.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

from oracle import binding

# hip/systolic.hip
SYSTOLIC_ROWS = 8            # systolic_rows_k: query rows a lane
SYSTOLIC_BAND = 512          # systolic_band_rows_k: 64 lanes x 8 rows, one wavefront
SYSTOLIC_COLUMNS = 4         # systolic_columns_k: columns a lane scores per step
SYSTOLIC_CHUNK = 16 * 4      # systolic_chunk_steps_k steps = 64 columns between two hand-overs
SYSTOLIC_FIRST_STEADY = 320  # run_chunk: `chunk_first >= 64 && K * (chunk_first + 16) <= n`, the first n with a steady chunk
# hip/myers_chain.hip
CHAIN_WORD = 32              # rows a lane: one 32-bit word of VP / VN
CHAIN_BAND = 2048            # chain_band_rows_k: 64 lanes x 32 rows
CHAIN_COLUMNS = 8            # chain_columns_k
CHAIN_CHUNK = 16 * 8         # chain_chunk_steps_k steps = 128 columns
CHAIN_FIRST_STEADY = 640     # the same condition with K = 8

SYSTOLIC_M = (1, 7, 8, 9, 15, 16, 17, 504, 505, 511, 512, 513, 520, 1023, 1024, 1025, 1536, 1537)
SYSTOLIC_N = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 66, 67, 68, 127, 128, 129, 255, 256, 257, 319, 320, 321, 383, 384, 385)
CHAIN_M = (1, 31, 32, 33, 63, 64, 65, 2016, 2017, 2047, 2048, 2049, 2080, 2081, 4095, 4096, 4097)
CHAIN_N = (1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 135, 136, 137, 255, 256, 257, 639, 640, 641, 767, 768, 769)

RUNES = "aé中😀"  # 1, 2, 3 and 4 bytes


def _letters(rng, length, alphabet):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), size=length)].tobytes()


# ---- a. length grids ---------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def grid(tier, alphabet=b"ACGT", runes=False):
    """(queries, candidates) of ONE cross-product: a string of every listed length, in the listed order, and an empty one at
    the end of each side.  `runes`: the letters are drawn from RUNES and the lengths count codepoints."""
    rows, columns = (SYSTOLIC_M, SYSTOLIC_N) if tier == "systolic" else (CHAIN_M, CHAIN_N)
    rng = np.random.default_rng(len(tier) + 17 * len(alphabet) + runes)
    if runes:
        draw = lambda length: "".join(RUNES[i] for i in rng.integers(0, len(RUNES), size=length)).encode()
    else:
        draw = lambda length: _letters(rng, length, alphabet)
    return tuple(draw(m) for m in rows) + (b"",), tuple(draw(n) for n in columns) + (b"",)


def grid_lengths(tier):
    rows, columns = (SYSTOLIC_M, SYSTOLIC_N) if tier == "systolic" else (CHAIN_M, CHAIN_N)
    return rows + (0,), columns + (0,)


# ---- the engines, and the oracle's matrix of a batch ---------------------------------------------------------------------


class Engine(NamedTuple):
    kind: str  # "needleman_wunsch" | "smith_waterman" | "levenshtein" | "levenshtein_utf8"
    table: Optional[str]  # a name `table_of` knows, for the two class-table kinds
    costs: tuple  # (open, extend), or (match, mismatch, open, extend)


@functools.lru_cache(maxsize=None)
def _table(name):
    if name == "blosum62":
        return binding.blosum62()
    if name == "planted":
        return planted_table()
    if name == "large":
        return large_table()
    assert name == "asymmetric", name
    rng = np.random.default_rng(404)
    return rng.integers(0, 32, size=256).astype(np.uint8), rng.integers(-9, 10, size=(32, 32)).astype(np.int8)


def table_of(name):
    return _table(name)


@functools.lru_cache(maxsize=None)
def expected(engine, queries, candidates=None):
    """The oracle's matrix as int64; `candidates=None`: the symmetric call.  Tuples in, a read-only array out."""
    oracle = binding.oracle()
    q, c = list(queries), None if candidates is None else list(candidates)
    if engine.kind in ("levenshtein", "levenshtein_utf8"):
        matrix = getattr(oracle, engine.kind)(q, c, *engine.costs)
    else:
        matrix = getattr(oracle, engine.kind)(q, c, *table_of(engine.table), *engine.costs)
    matrix = matrix.view(np.int64)
    matrix.setflags(write=False)
    return matrix


# ---- b. structured content for unit costs ------------------------------------------------------------------------------

STRUCTURED_M = (513, 2049, 4097)
OWN, FOREIGN = b"ACGT", b"WXYZ"  # the query's letters, and letters it does not hold


@functools.lru_cache(maxsize=None)
def structured(m):
    """(query, labels, candidates): the candidates whose horizontal deltas under a band's last row hold runs of one value."""
    rng = np.random.default_rng(m)
    query = _letters(rng, m, OWN)
    foreign = lambda length: _letters(rng, length, FOREIGN)
    family = [("itself", query), ("foreign, as long", foreign(m)), ("foreign, 9 longer", foreign(m + 9))]
    for s in (1, 31, 32, 33):
        family += [(f"shifted up by {s}", query[s:] + foreign(s)), (f"shifted down by {s}", foreign(s) + query[: m - s])]
    for length in sorted({m - 1, m // 2, 2048, 2047}, reverse=True):
        if length < m:
            family += [(f"prefix of {length}", query[:length]), (f"suffix of {length}", query[m - length :])]
    replaced = bytearray(query)
    replaced[63::64] = foreign(len(replaced[63::64]))
    family.append(("every 64th byte replaced", bytes(replaced)))
    return query, tuple(label for label, _ in family), tuple(text for _, text in family)


# ---- c. planted local optima -------------------------------------------------------------------------------------------

SEGMENT_ROWS = 12
MATCH = 5
BACKGROUND = b"ab"
SEGMENT_LETTERS = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ012"  # 29 letters, a class each: 3 ... 31


def planted_table():
    """Background letters score -3 against everything, themselves included; a segment letter scores +5 against itself."""
    byte_to_class = np.zeros(256, np.uint8)
    for index, letter in enumerate(BACKGROUND + SEGMENT_LETTERS):
        byte_to_class[letter] = index + 1
    table = np.full((32, 32), -3, np.int8)
    for index in range(len(SEGMENT_LETTERS)):
        table[3 + index, 3 + index] = MATCH
    return byte_to_class, table


class Placement(NamedTuple):
    name: str
    query: int  # index into the batch's queries
    last_row: int  # 1-based DP row and column of the optimum's last cell
    last_column: int
    length: int  # letters of the segment that the candidate holds: its last ones
    candidate: int  # index into the batch's candidates; the segment-free control follows it


class PlantedBatch(NamedTuple):
    queries: tuple
    candidates: tuple
    placements: tuple


COLUMNS, MIDDLE = 400, 200  # a candidate's length and where its segment ends, unless the placement is about columns


@functools.lru_cache(maxsize=None)
def planted(m):
    """The batch of one query length: 1100 (three bands, 76 rows in the last: lanes 0 ... 9, the last of them with 4 real rows;
    beside it a query of 1097 and one of 1103 rows, whose lane 9 holds 1 and 7) or 1024 (two whole bands).  A query holds
    several segments, each a 12-mer of its own over the 29 segment letters, no letter twice; a candidate holds ONE segment of one
    query - or only its last letter -, and is followed by its control: the same background without the segment."""
    assert m in (1100, 1024), m
    rng = np.random.default_rng(m)
    padded = m % SYSTOLIC_BAND != 0
    last_band_row = m - 40 if padded else 800
    # rows where a segment ENDS, per query; segments of one query never overlap
    plans = [(m, {"band 0": 300, "row 512": 512, "band 1": 800, "the last row": m}),
             (m, {"row 513": 513}),
             (m, {"rows 507 ... 518": 518})]
    if padded:
        plans[0][1]["the last band"] = last_band_row
        plans[1][1]["a lane with 4 real rows"] = m - 2  # 1098: row 1 of lane 9
        plans += [(m - 3, {"a lane with 1 real row": m - 3}), (m + 3, {"a lane with 7 real rows": m + 2})]
    queries, segments = [], {}
    for index, (rows, ends) in enumerate(plans):
        query = bytearray(_letters(rng, rows, BACKGROUND))
        for name, end in ends.items():
            segment = bytes(SEGMENT_LETTERS[i] for i in rng.permutation(len(SEGMENT_LETTERS))[:SEGMENT_ROWS])
            query[end - SEGMENT_ROWS : end] = segment
            segments[name] = (index, end, segment)
        queries.append(bytes(query))

    candidates, placements = [], []

    def place(name, segment_name, columns=COLUMNS, last_column=MIDDLE, length=SEGMENT_ROWS):
        query, last_row, segment = segments[segment_name]
        background = _letters(rng, columns, BACKGROUND)
        text = bytearray(background)
        text[last_column - length : last_column] = segment[SEGMENT_ROWS - length :]
        placements.append(Placement(name, query, last_row, last_column, length, len(candidates)))
        candidates.extend([bytes(text), background])

    for name in segments:
        place(name, name)
    place("column 1", "rows 507 ... 518", last_column=1, length=1)  # that query holds one segment: its last letter occurs once
    place("columns 1 ... 12", "band 0", last_column=SEGMENT_ROWS)
    for columns in (201, 202, 203, 204):  # the last step holds 1, 2, 3 and 4 columns
        place(f"column n = {columns}", "band 0", columns=columns, last_column=columns)
        place(f"column n = {columns}, the last row", "the last row", columns=columns, last_column=columns)
    # lane 0 of band 1 (row 513) scores columns 257 ... 320 and 321 ... 384 in the steady body, the rest in the predicated one
    for last_column in (256, 257, 320, 321, 384, 385):
        place(f"row 513, column {last_column}", "row 513", last_column=last_column)
    # lane 9 of the padded band is in a steady chunk under columns 285 ... 348: the body that counts `my_rows` rows, unpredicated
    for name in ("the last row", "a lane with 1 real row", "a lane with 4 real rows", "a lane with 7 real rows"):
        if name in segments:
            place(f"{name}, column 300", name, last_column=300)
    return PlantedBatch(tuple(queries), tuple(candidates), tuple(placements))


# ---- d. large costs ----------------------------------------------------------------------------------------------------

LARGE_M, LARGE_N = (9, 512, 513, 1025), (5, 64, 65, 321)


def large_table():
    """Three letters, entries from {127, -127, -128, 0}, asymmetric; every other byte is class 0 and costs 0."""
    byte_to_class = np.zeros(256, np.uint8)
    for index, letter in enumerate(b"ABC"):
        byte_to_class[letter] = index + 1
    table = np.zeros((32, 32), np.int8)
    table[1:4, 1:4] = [[127, -128, 0], [-127, 127, -127], [-128, 0, 127]]
    return byte_to_class, table


LARGE_ENGINES = tuple(Engine(kind, "large", gaps) for kind in ("needleman_wunsch", "smith_waterman")
                      for gaps in ((-128, -128), (-128, -1), (-1, -128), (0, 0))) + (
    Engine("smith_waterman", "large", (127, -1)),  # a gap that pays: the signed local form
    Engine("levenshtein", None, (0, 127, 127, 127)),
    Engine("levenshtein", None, (1, 127, 100, 27)),
)


@functools.lru_cache(maxsize=None)
def large():
    """(queries, candidates): the queries are prefixes of one text, the candidates pieces of it - a run of 212 matches ends on
    row 512, a piece straddles it - so values far beyond 127 x 64 are parked under a band's last row and picked up below."""
    rng = np.random.default_rng(127)
    base = _letters(rng, max(LARGE_M), b"ABC")
    piece = bytearray(base[300:621])
    for at in range(49, len(piece), 50):
        piece[at] = b"ABC"[(b"ABC".index(piece[at]) + 1) % 3]
    candidates = {5: base[:5], 64: base[480:544], 65: base[448:513], 321: bytes(piece)}
    assert tuple(sorted(candidates)) == LARGE_N and all(len(text) == n for n, text in candidates.items())
    return tuple(base[:m] for m in LARGE_M), tuple(candidates[n] for n in LARGE_N)

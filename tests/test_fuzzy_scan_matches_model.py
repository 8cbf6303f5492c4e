"""Fuzzy scan matches (`szs_rocm_fuzzy_scan_matches*`) in plain Python - runs anywhere.  The piece rule of
hip/myers_fuzzy_matches.hip - piece p owns columns (p P, min(n, (p + 1) P)], its lane walks from s = p P - min(p P, 2 m) and reports
owned columns only - against the full DP with a free start in the text, and the two-pass capacity rule - counts per piece, prefix
sums over chunks of 64 pieces and within them, the hits whose slot is below `limit` - against the leftmost hits."""
import functools
import random

EMPTY = 2**64 - 1
PIECES = (1, 2, 3, 5, 8, 16, 64)
CASES = 3000


def last_row(query, text):
    """D[m][j] for j = 0 ... n of the unit-cost DP with a free start in the text."""
    column = list(range(len(query) + 1))
    row = [len(query)]
    for symbol in text:
        diagonal, column[0] = column[0], 0
        for i, wanted in enumerate(query, 1):
            diagonal, column[i] = column[i], min(diagonal + (wanted != symbol), column[i] + 1, column[i - 1] + 1)
        row.append(column[-1])
    return row


def hits_of(query, text, bound):
    """What the call returns in full: every (j, D[m][j]) with j in [1, n] and D[m][j] <= bound; a query of no bytes has none."""
    if not query:
        return []
    return [(j, d) for j, d in enumerate(last_row(query, text)) if j >= 1 and d <= bound]


def piece_hits(query, text, piece, bound, warm_of):
    """The kernel's rule: per piece the (j, L[j]) of its OWNED columns with L[j] <= bound, L the DP started `warm_of(m)` bytes early."""
    n, m = len(text), len(query)
    found = []
    for p in range(-(-n // piece)):
        begin, end = p * piece, min(n, (p + 1) * piece)
        start = begin - min(begin, warm_of(m))
        row = last_row(query, text[start:end]) if m else []
        found.append([(j, row[j - start]) for j in range(begin + 1, end + 1) if m and row[j - start] <= bound])
    return found


def two_passes(per_piece, limit):
    """The count per piece, the exclusive prefix over chunks of 64 pieces and within a chunk, then every lane stores its hits into
    slots offset, offset + 1, ... while they are below `limit`.  Returns (count, ends, distances), the rows `limit` long."""
    counts = [len(found) for found in per_piece]
    chunks = [sum(counts[at:at + 64]) for at in range(0, len(counts), 64)]
    ends, distances, before = [EMPTY] * limit, [EMPTY] * limit, 0
    for chunk, total in enumerate(chunks):
        if before < limit and total:  # else the workgroup returns before it builds a table
            offset = before
            for found in per_piece[64 * chunk:64 * chunk + 64]:
                for slot, (j, d) in enumerate(found, offset):
                    if slot < limit:
                        assert ends[slot] == EMPTY  # one writer a slot
                        ends[slot], distances[slot] = j, d
                offset += len(found)
        before += total
    return before, ends, distances


def _case(rng):
    letters = "ab" if rng.random() < 0.3 else "abc" if rng.random() < 0.5 else "abcd"
    m = 0 if rng.random() < 0.03 else rng.randint(1, 12)
    n = 0 if rng.random() < 0.03 else rng.randint(1, 90)
    query = "".join(rng.choice(letters) for _ in range(m))
    text = [rng.choice(letters) for _ in range(n)]
    for _ in range(rng.randint(0, 3) if m and n else 0):  # planted copies with up to two edits, anywhere - also across pieces
        copy = list(query)
        for _ in range(rng.randint(0, 2)):
            kind, at = rng.randint(0, 2), rng.randrange(len(copy)) if copy else 0
            if kind == 0 and copy:
                copy[at] = rng.choice(letters)
            elif kind == 1 and len(copy) > 1:
                del copy[at]
            else:
                copy.insert(at, rng.choice(letters))
        at = rng.randrange(n)
        text[at:at + len(copy)] = copy
    text = "".join(text[:n])
    bound = rng.choice((0, 0, 1, 1, 2, 3, m // 2, m, m + 3))
    return query, text, rng.choice(PIECES), bound


@functools.lru_cache(maxsize=None)
def cases():
    rng = random.Random(412)
    return tuple(_case(rng) for _ in range(CASES))


@functools.lru_cache(maxsize=None)
def truth():
    """hits_of every case: computed once, read-only."""
    return tuple(tuple(hits_of(query, text, bound)) for query, text, _, bound in cases())


WARM_UPS = {"2m": lambda m: 2 * m, "m": lambda m: m, "m-1": lambda m: max(m - 1, 0)}


@functools.lru_cache(maxsize=None)
def cut(warm_up):
    """piece_hits of every case under one warm-up rule: computed once, read-only."""
    return tuple(tuple(tuple(found) for found in piece_hits(query, text, piece, bound, WARM_UPS[warm_up]))
                 for query, text, piece, bound in cases())


def _mismatches(warm_up):
    return sum(tuple(hit for found in per_piece for hit in found) != want for per_piece, want in zip(cut(warm_up), truth()))


def test_the_generator_covers_what_it_must():
    drawn = cases()
    assert any(not query for query, _, _, _ in drawn) and any(not text for _, text, _, _ in drawn)
    assert any(query and bound >= len(query) for query, _, _, bound in drawn)
    assert {piece for _, _, piece, _ in drawn} == set(PIECES)
    found = [len(want) for want in truth()]
    assert any(count > 3 for count in found)  # more hits than a limit of 3
    without, with_hits = sum(count == 0 for count in found), sum(count > 0 for count in found)
    assert without >= CASES // 5 and with_hits >= CASES // 5, (without, with_hits)
    # a query of no bytes and an empty text have no hit, whatever the bound; a bound of m or more makes every column one
    for query, text, _, bound in drawn:
        if not query or not text:
            assert hits_of(query, text, bound) == []
        elif bound >= len(query):
            assert [j for j, _ in hits_of(query, text, bound)] == list(range(1, len(text) + 1))


def test_a_warm_up_of_two_m_is_exact():
    assert _mismatches("2m") == 0


def test_a_warm_up_of_m_is_not():
    """It is for the MINIMUM of fuzzy scan (tests/test_fuzzy_scan_model.py), not for every column."""
    assert _mismatches("m") >= 1
    assert _mismatches("m-1") >= _mismatches("m")


def test_no_piece_reports_too_little_and_each_hit_has_one_owner():
    for (query, text, piece, bound), per_piece in zip(cases()[:600], cut("2m")):
        row = last_row(query, text) if query else []
        seen = set()
        for p, found in enumerate(per_piece):
            for j, d in found:
                assert d == row[j] and j not in seen and p * piece < j <= (p + 1) * piece
                seen.add(j)


def test_the_two_passes_keep_the_leftmost_hits():
    for limit in (0, 1, 3, 1000):
        over = under = 0
        for per_piece, want in zip(cut("2m"), truth()):
            count, ends, distances = two_passes(per_piece, limit)
            kept = list(want[:limit])
            assert count == len(want)  # the full count, also above the limit
            assert ends == [j for j, _ in kept] + [EMPTY] * (limit - len(kept))
            assert distances == [d for _, d in kept] + [EMPTY] * (limit - len(kept))
            over, under = over + (len(want) > limit), under + (0 < len(want) <= limit)
        assert (over or limit == 1000) and (under or limit == 0)  # rows above and below the limit (no text has 1000 columns)


def test_the_two_passes_cross_chunks_of_64_pieces():
    """Pieces of one byte over 90 columns: two chunks - the second writes only where the first left slots."""
    query, text = "ab", "ab" * 45
    per_piece = piece_hits(query, text, 1, 0, lambda m: 2 * m)
    assert len(per_piece) == 90 and [j for found in per_piece for j, _ in found] == list(range(2, 91, 2))
    for limit in (0, 1, 31, 32, 33, 45, 64):
        count, ends, distances = two_passes(per_piece, limit)
        kept = list(range(2, 91, 2))[:limit]
        assert count == 45 and ends == kept + [EMPTY] * (limit - len(kept)) and distances == [0] * len(kept) + [EMPTY] * (limit - len(kept))

"""Fuzzy scan occurrences (`szs_rocm_fuzzy_scan_occurrences*`) in plain Python - runs anywhere.  The rule -
column j in [1, n] is an occurrence end iff D[m][j] <= bound, D[m][j] < D[m][j - 1] and (j == n or D[m][j] <= D[m][j + 1]) - over the
full DP with a free start in the text, against the decomposition of hip/myers_fuzzy_occurrences.hip: piece p owns columns
(p P, min(n, (p + 1) P)], its lane walks from s = p P - min(p P, 2 m), one TAIL column behind its last owned column where the piece is
not the last, and decides column c - 1 at column c from the scores of three columns; the lane of the last piece decides column n
behind its walk."""
import functools
import itertools
import random

PIECES = (1, 2, 3, 5, 8)
TRIALS = 2  # per (m, n, alphabet): 6 x 41 x 2 x TRIALS pairs, each under every piece and every bound


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


def occurrences_of(row, bound):
    """The rule over a whole bottom row: every (j, D[m][j]) that is an occurrence end."""
    n = len(row) - 1
    return [(j, row[j]) for j in range(1, n + 1) if row[j] <= bound and row[j] < row[j - 1] and (j == n or row[j] <= row[j + 1])]


def lane_rows(query, text, piece, tail=True):
    """Per piece what its lane sees: (s, warm, tail, L) - L[c] the bottom row of the DP started at s, for c = 0 ... warm + own + tail."""
    n, m = len(text), len(query)
    lanes = []
    for p in range(-(-n // piece)):
        begin, end = p * piece, min(n, (p + 1) * piece)
        warm = min(begin, 2 * m)
        has_tail = tail and end < n
        lanes.append((begin - warm, warm, has_tail, last_row(query, text[begin - warm:end + has_tail])))
    return lanes


def lane_occurrences(lanes, bound):
    """The kernel's walk: two scores kept, column c - 1 decided at column c where it is owned; a lane without a tail column decides its
    last column behind the walk as the column with no right neighbour.  Absolute (j, score), piece by piece."""
    found = []
    for start, warm, has_tail, row in lanes:
        held = left = row[0]
        taken = 0
        for c in range(1, len(row)):
            score, taken = row[c], c
            if c - 1 > warm and held <= bound and held < left and held <= score:
                found.append((start + c - 1, held))
            left, held = held, score
        if not has_tail and taken > warm and held <= bound and held < left:
            found.append((start + taken, held))
    return found


@functools.lru_cache(maxsize=None)
def cases():
    """(query, text) for every m in 1..6, n in 0..40 and alphabets of 2 and 3 letters, seeded; half of them with a planted copy."""
    rng = random.Random(1317)
    drawn = []
    for m, n, letters in itertools.product(range(1, 7), range(41), ("ab", "abc")):
        for trial in range(TRIALS):
            query = "".join(rng.choice(letters) for _ in range(m))
            text = [rng.choice(letters) for _ in range(n)]
            if trial % 2 and n:
                at = rng.randrange(n)
                text[at:at + m] = query
            drawn.append((query, "".join(text[:n])))
    return tuple(drawn)


@functools.lru_cache(maxsize=None)
def truth():
    """The bottom row of every case: computed once, read-only."""
    return tuple(tuple(last_row(query, text)) for query, text in cases())


def test_the_decomposition_equals_the_rule():
    """Every piece size, every bound 0 ... m: the lanes report exactly the rule's occurrence ends, each once, with its distance."""
    reported = plateaus = at_piece_end = at_piece_start = 0
    for (query, text), row in zip(cases(), truth()):
        for piece in PIECES:
            lanes = lane_rows(query, text, piece)
            for bound in range(len(query) + 1):
                want = occurrences_of(row, bound)
                assert lane_occurrences(lanes, bound) == want, (query, text, piece, bound)
                reported += len(want)
                plateaus += sum(j < len(text) and row[j + 1] == d for j, d in want)
                at_piece_end += sum(j % piece == 0 and j < len(text) for j, _ in want)
                at_piece_start += sum(j % piece == 1 % piece and j > 1 for j, _ in want)
    assert min(reported, plateaus, at_piece_end, at_piece_start) > 1000  # the sweep exercises what the cut has to get right


def test_the_neighbours_a_lane_sees_are_exact():
    """Why it holds: on its owned columns, on column p P to their left and on the tail column a lane's row IS the bottom row."""
    for (query, text), row in zip(cases()[::3], truth()[::3]):
        for piece in PIECES:
            for start, warm, has_tail, seen in lane_rows(query, text, piece):
                assert list(row[start + warm:start + len(seen)]) == seen[warm:], (query, text, piece, start)


def _first_without_the_tail():
    """The first case of the sweep, smallest piece and bound first, where a lane that ends at its last owned column - and decides it
    as the last piece decides column n - departs from the rule."""
    for (query, text), row in zip(cases(), truth()):
        for piece in PIECES:
            lanes = lane_rows(query, text, piece, tail=False)
            for bound in range(len(query) + 1):
                got, want = lane_occurrences(lanes, bound), occurrences_of(row, bound)
                if got != want:
                    return query, text, piece, bound, got, want
    return None


def test_without_the_tail_column_it_goes_wrong():
    query, text, piece, bound, got, want = _first_without_the_tail()
    # pinned: the search's own first find.  The bottom row of "ab" in "ab" is 2 1 0; with pieces of one byte the lane of piece 0 ends
    # at column 1, sees 1 < 2 and no right neighbour, and reports a column the rule does not: the row keeps descending to column 2.
    assert (query, text, piece, bound) == PINNED[:4], (query, text, piece, bound, got, want)
    assert (got, want) == PINNED[4:]
    # a step down that keeps descending, cut by a piece boundary: reported without the right neighbour, not an occurrence with it
    extra = [pair for pair in got if pair not in want]
    assert extra and all(j % piece == 0 and j < len(text) for j, _ in extra) and not [pair for pair in want if pair not in got]


PINNED = ("ab", "ab", 1, 1, [(1, 1), (2, 0)], [(2, 0)])


def test_every_occurrence_is_a_hit_with_its_distance():
    for row in truth():
        for bound in range(row[0] + 1):
            hits = {(j, d) for j, d in enumerate(row) if j >= 1 and d <= bound}
            found = occurrences_of(row, bound)
            assert set(found) <= hits and [j for j, _ in found] == sorted(j for j, _ in found)


def test_the_best_match_is_the_leftmost_occurrence_of_minimum_distance():
    """fuzzy scan's (d*, end) - the minimum of the bottom row and the smallest column that attains it - under d* <= bound, d* < m."""
    compared = nothing = 0
    for row in truth():
        m, best = row[0], min(row)
        end = row.index(best)
        for bound in range(m + 1):
            found = occurrences_of(row, bound)
            if best < m and best <= bound:
                least = min(d for _, d in found)
                assert (least, next(j for j, d in found if d == least)) == (best, end)
                compared += 1
            elif best == m:  # nothing better than m anywhere: no occurrence, even at a bound of m
                assert found == [] and occurrences_of(row, m + 5) == []
                nothing += 1
    assert compared > 1000 and nothing > 50

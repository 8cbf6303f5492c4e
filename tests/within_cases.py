"""What the bounded searches must return (`szs_rocm_within*`, `szs_rocm_fuzzy_search_within*`), in plain numpy:
no GPU, no library.  tests/test_within_host.py checks a model of the device's two passes against `expected_within`, the GPU tests the
calls themselves - `within` over the oracle's matrices, `fuzzy_search_within` over the semi-global DP below."""
import numpy as np

EMPTY = np.uint64(2**64 - 1)
UNTOUCHED = 0x5A5A5A5A5A5A5A5A
QUERY_LENGTHS = (0, 1, 31, 32, 33, 64, 65, 128, 255, 256)  # every word boundary of the tile kernel's eight widths


def hits_of(matrix, bound, descending, self_search=False):
    """The boolean (rows, columns) matrix of hits: a distance hits iff bound >= 0 and cell <= bound, a score iff the signed cell >= bound;
    the own column of a self-search never hits."""
    matrix = np.asarray(matrix)
    if descending:
        hits = matrix.astype(np.int64) >= int(bound)
    elif bound < 0:
        hits = np.zeros(matrix.shape, bool)
    else:
        hits = matrix.astype(np.uint64) <= np.uint64(bound)
    if self_search:
        hits = hits & ~np.eye(*matrix.shape, dtype=bool)
    return hits


def expected_within(matrix, bound, descending, limit, self_search=False, dtype=np.uint64):
    """(counts, indices, scores): the hits of every row among ALL columns, and the leftmost `limit` of them in ascending column order
    with their cells; the slots behind hold (2^64 - 1, 0)."""
    matrix = np.asarray(matrix)
    hits = hits_of(matrix, bound, descending, self_search)
    rows = matrix.shape[0]
    counts = hits.sum(axis=1).astype(np.uint64)
    indices = np.full((rows, limit), EMPTY, dtype=np.uint64)
    scores = np.zeros((rows, limit), dtype=dtype)
    for q in range(rows):
        columns = np.flatnonzero(hits[q])[:limit]
        indices[q, :len(columns)] = columns
        scores[q, :len(columns)] = matrix[q, columns]
    return counts, indices, scores


def _columns(pattern, texts, lengths, free_start):
    """The last row of the unit-cost DP of `pattern` against every text, column by column: yields (j, D[m][j] per text)."""
    m, rows = len(pattern), np.arange(len(pattern) + 1)
    padded = np.zeros((len(texts), max(int(lengths.max(initial=0)), 1)), np.uint8)
    for at, text in enumerate(texts):
        padded[at, :len(text)] = np.frombuffer(text, np.uint8)
    column = np.tile(rows, (len(texts), 1))
    for j in range(1, int(lengths.max(initial=0)) + 1):
        step = np.full_like(column, 0 if free_start else j)  # row zero: free start in the text, or D[0][j] = j
        step[:, 1:] = np.minimum(column[:, :-1] + (pattern[None, :] != padded[:, j - 1, None]), column[:, 1:] + 1)
        column = np.minimum.accumulate(step - rows, axis=1) + rows  # the insertions down the column
        yield j, column[:, m]


def spans(query, texts):
    """(distances, starts, ends) of `query` inside every text: D[0][j] = 0, D[i][0] = i, unit costs; distance = the minimum of the last
    row, end = the smallest j that attains it, start = where the shortest match that ends there begins."""
    m, pattern = len(query), np.frombuffer(query, np.uint8)
    lengths = np.array([len(text) for text in texts], dtype=np.int64)
    best, end = np.full(len(texts), m, np.int64), np.zeros(len(texts), np.int64)
    for j, last in _columns(pattern, texts, lengths, free_start=True):
        better = (j <= lengths) & (last < best)
        best[better], end[better] = last[better], j
    heads = [text[:int(e)][::-1] for text, e in zip(texts, end)]  # c[:end] reversed, against the reversed query
    least, back = np.full(len(texts), m, np.int64), np.zeros(len(texts), np.int64)
    for t, last in _columns(pattern[::-1], heads, end, free_start=False):
        better = (t <= end) & (last < least)
        least[better], back[better] = last[better], t  # strictly smaller: the smallest t, the shortest match
    assert np.array_equal(least, best)
    return best, end - back, end


def dense(queries, candidates):
    """The (queries x candidates) matrices of distances, starts and ends, read-only."""
    if not candidates:
        return tuple(np.zeros((len(queries), 0), np.uint64) for _ in range(3))
    triples = [spans(query, candidates) for query in queries]
    parts = tuple(np.array([triple[part] for triple in triples], dtype=np.uint64).reshape(len(queries), len(candidates)) for part in range(3))
    for matrix in parts:
        matrix.setflags(write=False)
    return parts


def expected_fuzzy_within(want, max_distance, limit, skip_own=False):
    """(counts, indices, distances, starts, ends) from `dense`'s matrices: a hit is a distance <= max_distance; the leftmost `limit` hits
    a row in ascending column order; missing slots: (2^64 - 1, 0, 0, 0)."""
    counts, indices, distances = expected_within(want[0], min(max_distance, 2**63 - 1), False, limit, self_search=skip_own)
    starts, ends = np.zeros_like(distances), np.zeros_like(distances)
    for q in range(indices.shape[0]):
        held = int(min(counts[q], limit))
        starts[q, :held], ends[q, :held] = want[1][q, indices[q, :held]], want[2][q, indices[q, :held]]
    return counts, indices, distances, starts, ends


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))

"""What the alignment tests share (tests/test_alignments_model.py, tests/test_gpu_alignments.py): the CANONICAL edit script of
`szs_rocm_alignments*` by the plain suffix DP of include/stringzillas/stringzillas_rocm.h, vectorised per row with NumPy, and what a
script does to a query."""
import numpy as np

OPS = {"=": ord("="), "X": ord("X"), "I": ord("I"), "D": ord("D")}
QUERY_LENGTHS = (0, 1, 31, 32, 33, 64, 65, 128, 255, 256)  # every word boundary of the bit-vector
LONGEST_SPAN = 512


def suffix_table(query: bytes, span: bytes) -> np.ndarray:
    """S[i][j] = lev(query[i:], span[j:]): S[m][j] = t - j, S[i][t] = m - i, S[i][j] = min(S[i+1][j+1] + (q[i] != s[j]), S[i+1][j] + 1,
    S[i][j+1] + 1).  A row at a time: the third term is a running minimum from the right of (the other two + j) - j."""
    m, t = len(query), len(span)
    q, s = np.frombuffer(query, dtype=np.uint8), np.frombuffer(span, dtype=np.uint8)
    table = np.zeros((m + 1, t + 1), dtype=np.int64)
    columns = np.arange(t + 1, dtype=np.int64)
    table[m] = t - columns
    for i in range(m - 1, -1, -1):
        below = table[i + 1]
        cell = below + 1                                                   # S[i+1][j] + 1
        cell[:t] = np.minimum(cell[:t], below[1:] + (s != q[i]))           # S[i+1][j+1] + (q[i] != s[j])
        table[i] = np.minimum.accumulate((cell + columns)[::-1])[::-1] - columns  # ... and S[i][j'] + (j' - j) for every j' > j
    return table


def canonical_script(query: bytes, span: bytes):
    """(distance, script): the walk from (0, 0) to (m, t) that takes the first of diagonal, 'I', 'D' that holds; the script as bytes
    of `= X I D`."""
    m, t = len(query), len(span)
    table = suffix_table(query, span).tolist()
    script = bytearray()
    i = j = 0
    while i < m or j < t:
        here = table[i][j]
        if i < m and j < t and table[i + 1][j + 1] + (query[i] != span[j]) == here:
            script.append(OPS["="] if query[i] == span[j] else OPS["X"])
            i, j = i + 1, j + 1
        elif i < m and table[i + 1][j] + 1 == here:
            script.append(OPS["I"])
            i += 1
        else:
            script.append(OPS["D"])
            j += 1
    return table[0][0], bytes(script)


def canonical_scripts(query: bytes, spans):
    """`canonical_script` of one query against many spans at once, every step vectorised over the spans: (distances, lengths, ops) -
    two int64 vectors and a uint8 (spans, m + longest span) array, each script followed by zeros."""
    m, n = len(query), len(spans)
    q = np.frombuffer(query, dtype=np.uint8)
    t = np.array([len(span) for span in spans], dtype=np.int64)
    longest = int(t.max(initial=0))
    padded = np.zeros((n, max(longest, 1)), dtype=np.uint8)
    for at, span in enumerate(spans):
        padded[at, :len(span)] = np.frombuffer(span, dtype=np.uint8)
    far = np.int32(1 << 20)  # beyond a span's own columns: never the minimum of anything
    columns = np.arange(longest + 1, dtype=np.int32)
    beyond = columns[None, :] > t[:, None]
    table = np.empty((n, m + 1, longest + 1), dtype=np.int32)
    table[:, m] = np.where(beyond, far, t[:, None] - columns[None, :])
    for i in range(m - 1, -1, -1):
        below = table[:, i + 1]
        cell = below + 1
        cell[:, :longest] = np.minimum(cell[:, :longest], below[:, 1:] + (padded[:, :longest] != q[i]))
        cell[beyond] = far
        table[:, i] = np.minimum.accumulate((cell + columns)[:, ::-1], axis=1)[:, ::-1] - columns
    ops = np.zeros((n, m + longest), dtype=np.uint8)
    each = np.arange(n)
    i, j = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    lengths = np.zeros(n, dtype=np.int64)
    for step in range(m + longest):
        active = (i < m) | (j < t)
        if not active.any():
            break
        here = table[each, i, j]
        i1, j1 = np.minimum(i + 1, m), np.minimum(j + 1, longest)
        differ = (q[np.minimum(i, m - 1)] if m else np.zeros(n, dtype=np.uint8)) != padded[each, np.minimum(j, max(longest, 1) - 1)]
        diagonal = (i < m) & (j < t) & (table[each, i1, j1] + differ == here)
        query_alone = ~diagonal & (i < m) & (table[each, i1, j] + 1 == here)
        op = np.where(diagonal, np.where(differ, OPS["X"], OPS["="]), np.where(query_alone, OPS["I"], OPS["D"])).astype(np.uint8)
        ops[active, step] = op[active]
        lengths += active
        i += active & (diagonal | query_alone)
        j += active & ~query_alone
    return table[:, 0, 0].astype(np.int64), lengths, ops


def apply_script(query: bytes, script: bytes, span: bytes) -> bytes:
    """What the script makes of the query: '=' copies a query byte, 'X' replaces it by the span's, 'I' drops it (a byte the query has
    and the span has not), 'D' takes a byte of the span alone.  The span's bytes come from `span` - a script names no bytes."""
    made = bytearray()
    i = j = 0
    for op in script:
        if op == OPS["="]:
            made.append(query[i])
            i, j = i + 1, j + 1
        elif op == OPS["X"]:
            assert query[i] != span[j]
            made.append(span[j])
            i, j = i + 1, j + 1
        elif op == OPS["I"]:
            i += 1
        else:
            assert op == OPS["D"]
            made.append(span[j])
            j += 1
    assert i == len(query)
    return bytes(made)


def span_lengths(m: int):
    """t in {0, 1, m - 1, m, m + 1, 2 m}, capped at the longest span."""
    return sorted({min(max(t, 0), LONGEST_SPAN) for t in (0, 1, m - 1, m, m + 1, 2 * m)})

"""The alignment kernel's arithmetic on the CPU (hip/myers_alignments.hip) - runs anywhere.

Two things stand side by side: the CANONICAL script by the plain suffix DP (tests/alignment_cases.py), and a word-by-word model of
exactly what the kernel computes - the reversed query right-aligned over ZERO phantom rows in W words of 32 bits, the span walked
from its last byte down under myers_prefix_column_traced, `VP'` and the true diagonal-zero vector `D0 | VN` kept per column, then the
traceback from the bottom-right corner: diagonal iff the bytes are equal or the D0 bit is clear, else 'I' iff the VP' bit is set,
else 'D'; row zero takes 'D's only, column zero 'I's only.  The walk of the reversed problem emits the ops in forward order."""
import random

import pytest

import alignment_cases as cases

MASK = 0xFFFFFFFF


def _reversed_table(query: bytes, words: int):
    """Byte i of the query at bit pad + (m - 1 - i) of its byte's row; the phantom low rows are zero rows."""
    pad = 32 * words - len(query)
    table = {}
    for i, byte in enumerate(query):
        position = pad + (len(query) - 1 - i)
        table.setdefault(byte, [0] * words)[position >> 5] |= 1 << (position & 31)
    return table


def _bits_from(pad: int, words: int):
    return [sum(1 << (bit - 32 * w) for bit in range(max(pad, 32 * w), 32 * w + 32)) for w in range(words)]


def _traced_column(vp, vn, eq, with_vn=True):
    """myers_prefix_column_traced, word by word: returns (hp | hn << 1 of the last row, the diagonal-zero words); vp and vn updated."""
    words = len(vp)
    carry = hp_below = hn_below = 0
    diagonal_zero = [0] * words
    for w in range(words):
        xv = eq[w] | vn[w]
        total = (eq[w] & vp[w]) + vp[w] + carry
        carry, total = total >> 32, total & MASK
        d0 = (total ^ vp[w]) | eq[w]
        diagonal_zero[w] = (d0 | vn[w]) if with_vn else d0
        hp = (vn[w] | ~(d0 | vp[w])) & MASK
        hn = vp[w] & d0
        hp_shifted = ((hp << 1) | (1 if w == 0 else hp_below >> 31)) & MASK
        hn_shifted = ((hn << 1) | (0 if w == 0 else hn_below >> 31)) & MASK
        hp_below, hn_below = hp, hn
        vp[w] = (hn_shifted | ~(xv | hp_shifted)) & MASK
        vn[w] = hp_shifted & xv
    return (hp_below >> 31) | ((hn_below >> 31) << 1), diagonal_zero


def model_script(query: bytes, span: bytes, words: int, with_vn=True):
    """(distance, script, phantom rows stayed zero) as the kernel computes them at `words` words."""
    m, t = len(query), len(span)
    pad = 32 * words - m
    table, zeros = _reversed_table(query, words), [0] * words
    vp, vn = _bits_from(pad, words), [0] * words
    phantom = [MASK ^ word for word in vp]  # the bits below `pad`
    score, inert, trace = m, True, []
    for taken in range(1, t + 1):  # column `taken` of the reversed problem: the span's byte t - taken
        top, diagonal_zero = _traced_column(vp, vn, table.get(span[t - taken], zeros), with_vn)
        score += (top & 1) - (top >> 1)
        inert = inert and not any((vp[w] | vn[w]) & phantom[w] for w in range(words))
        trace.append((list(vp), diagonal_zero))
    script = bytearray()
    row, column = m, t  # of the reversed problem: real row `row` is bit pad + row - 1
    while row or column:
        if not row:
            script.append(cases.OPS["D"])
            column -= 1
            continue
        if not column:
            script.append(cases.OPS["I"])
            row -= 1
            continue
        bit = pad + row - 1
        new_vp, diagonal_zero = trace[column - 1]
        equal = query[m - row] == span[t - column]
        if equal or not (diagonal_zero[bit >> 5] >> (bit & 31)) & 1:
            script.append(cases.OPS["="] if equal else cases.OPS["X"])
            row, column = row - 1, column - 1
        elif (new_vp[bit >> 5] >> (bit & 31)) & 1:
            script.append(cases.OPS["I"])
            row -= 1
        else:
            script.append(cases.OPS["D"])
            column -= 1
        if len(script) > m + t:  # a wrong trace must not walk for ever
            break
    return score, bytes(script), inert


def _pairs():
    """(alphabet, m, t) at every word boundary of m and every t of the issue; two strings per case, one random and one a mutation."""
    for alphabet in (2, 26):
        for m in cases.QUERY_LENGTHS:
            for t in cases.span_lengths(m):
                yield alphabet, m, t


def _strings(alphabet, m, t):
    generator = random.Random(1000003 * alphabet + 521 * m + t)
    letters = bytes(range(ord("a"), ord("a") + alphabet))
    query = bytes(generator.choice(letters) for _ in range(m))
    mutated = bytearray(query)
    for _ in range(max(1, m // 8)):  # close to the query: long diagonal runs with edits between them
        at = generator.randrange(len(mutated) + 1)
        kind = generator.randrange(3)
        if kind == 0 and at < len(mutated):
            mutated[at] = generator.choice(letters)
        elif kind == 1 and at < len(mutated):
            del mutated[at]
        else:
            mutated.insert(at, generator.choice(letters))
    near = (bytes(mutated) + bytes(generator.choice(letters) for _ in range(t)))[:t]
    far = bytes(generator.choice(letters) for _ in range(t))
    return query, (near, far)


_canonical = {}


def _canonical_of(query, span):
    if (query, span) not in _canonical:
        _canonical[(query, span)] = cases.canonical_script(query, span)
    return _canonical[(query, span)]


@pytest.mark.parametrize("words", range(1, 9))
def test_model_script_is_the_canonical_script(words):
    checked = 0
    for alphabet, m, t in _pairs():
        if m > 32 * words:
            continue
        query, spans = _strings(alphabet, m, t)
        for span in spans:
            distance, script = _canonical_of(query, span)
            model_distance, model, inert = model_script(query, span, words)
            assert inert, (words, alphabet, m, t)
            assert (model_distance, model) == (distance, script), (words, alphabet, m, t)
            checked += 1
    assert checked >= 2 * 2 * 3 * 4


def test_canonical_script_is_a_shortest_edit_script():
    for alphabet, m, t in _pairs():
        query, spans = _strings(alphabet, m, t)
        for span in spans:
            distance, script = _canonical_of(query, span)
            assert max(m, t) <= len(script) <= m + t
            assert cases.apply_script(query, script, span) == span
            assert sum(op != cases.OPS["="] for op in script) == distance
            assert script.count(b"I") + script.count(b"=") + script.count(b"X") == m
            assert script.count(b"D") + script.count(b"=") + script.count(b"X") == t


def test_canonical_script_of_small_known_pairs():
    assert cases.canonical_script(b"", b"") == (0, b"")
    assert cases.canonical_script(b"abc", b"") == (3, b"III")
    assert cases.canonical_script(b"", b"ab") == (2, b"DD")
    assert cases.canonical_script(b"abc", b"abc") == (0, b"===")
    assert cases.canonical_script(b"abc", b"axc") == (1, b"=X=")
    assert cases.canonical_script(b"ab", b"b") == (1, b"I=")     # 'I' before 'D' ...
    assert cases.canonical_script(b"b", b"ab") == (1, b"D=")
    assert cases.canonical_script(b"ab", b"ba") == (2, b"XX")    # ... and the diagonal before either


def test_the_rule_needs_the_vn_term():
    """The same rule fed `(sum ^ VP) | Eq` - the `d0` that is enough for HP and HN - goes wrong: where VN is set the cell equals its
    diagonal neighbour whatever Eq says, and without the term the walk takes a mismatch the DP does not pay for."""
    wrong = 0
    for alphabet, m, t in _pairs():
        if m > 64:
            continue
        query, spans = _strings(alphabet, m, t)
        for span in spans:
            _, script = _canonical_of(query, span)
            wrong += model_script(query, span, 2, with_vn=False)[1] != script
    assert wrong >= 1


def test_the_batched_reference_is_the_plain_one():
    """tests/alignment_cases.py's `canonical_scripts` - what the GPU tests compare against, vectorised over the spans - against the
    walk of `canonical_script`, spans of every length side by side, the empty query and no spans at all included."""
    for alphabet, m in ((2, 0), (2, 33), (26, 64), (2, 5)):
        query, _ = _strings(alphabet, m, 0)
        spans = [span for t in (0, 1, 7, m, m + 1, 2 * m, 97) for span in _strings(alphabet, m, t)[1]]
        distances, lengths, ops = cases.canonical_scripts(query, spans)
        for at, span in enumerate(spans):
            distance, script = cases.canonical_script(query, span)
            assert (int(distances[at]), int(lengths[at])) == (distance, len(script))
            assert ops[at, :len(script)].tobytes() == script and not ops[at, len(script):].any()
    distances, lengths, ops = cases.canonical_scripts(b"abc", [b""])
    assert (distances.tolist(), lengths.tolist(), ops.tobytes()) == ([3], [3], b"III")
    assert cases.canonical_scripts(b"abc", [])[2].shape == (0, 3)

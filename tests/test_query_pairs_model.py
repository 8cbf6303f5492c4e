"""Two queries in one Myers bit-vector (hip/myers_core.hpp: myers_column with pattern_pair_t; hip/lev_myers.hip: the paired bodies).

1. A bit-level model of the packed column - the kernel's formulas on a 32 W-bit integer whose add is the W-word carry chain - scored
   against the oracle's Levenshtein: the boundary inside one word, s0 at bit 31 and s1 at bit 0, W = 8, 9 and 10, empty q1 or q2,
   pairs that fill their words exactly.
2. The pairing of the fused launch: slot s of ceil(Q / 2) takes descending refs s and s + ceil(Q / 2); every query is scored exactly
   once, and on config-2 lengths more of the scored bits are real rows than with one query per vector.
3. The code object: the fused and plain short kernels keep no scratch, and every main loop of four words or more - single patterns
   and pairs - spends at most 7.3 logic VALU instructions per word-step (the Myers column needs 7).
"""
import os
import random
import re
import shutil
import subprocess
from collections import Counter, defaultdict

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR_WORDS = 10  # szs_myers_pair_words_k


def bits_in_word(low_bit, high_bit, w):
    """hip/lev_myers.hip: bits_in_word - the bits of [low_bit, high_bit) that fall into word w."""
    low, high = max(low_bit, 32 * w), min(high_bit, 32 * w + 32)
    if low >= high:
        return 0
    return (0xFFFFFFFF if high - low == 32 else (1 << (high - low)) - 1) << (low - 32 * w)


def pair_distances(first, second, text, words):
    """The paired body of myers_workgroup for one lane, word masks assembled as the kernel assembles them."""
    l1, l2 = len(first), len(second)
    pad = 32 * words - (l1 + l2 + 2)
    assert pad >= 0
    second_row = pad + l1 + 2
    full = (1 << (32 * words)) - 1
    join = lambda per_word: sum(per_word(w) << (32 * w) for w in range(words))
    sep = join(lambda w: bits_in_word(second_row - 2, second_row, w))
    top = join(lambda w: bits_in_word(second_row - 3, second_row - 2, w) if l1 else 0)
    peq = defaultdict(int)
    for i, c in enumerate(first):
        peq[c] |= 1 << (pad + i)
    for i, c in enumerate(second):
        peq[c] |= 1 << (second_row + i)
    vp, vn = join(lambda w: bits_in_word(pad, 32 * words, w)) & ~sep, 0
    for c in text:
        eq = peq[c]
        xv = eq | vn | sep
        total = ((eq & vp) + vp) & full
        d0 = (total ^ vp) | eq
        hp = (vn | ~(d0 | vp)) & full
        hn = vp & d0 & ~top
        hp_shifted, hn_shifted = ((hp << 1) | 1) & full, (hn << 1) & full
        vp = (hn_shifted | ~(xv | hp_shifted)) & full
        vn = hp_shifted & xv & ~sep
        assert not (vp | vn) & sep  # the separator rows stay inert
    mine, theirs = join(lambda w: bits_in_word(pad, pad + l1, w)), join(lambda w: bits_in_word(second_row, 32 * words, w))
    count = lambda x: bin(x).count("1")
    return (len(text) + count(vp & mine) - count(vn & mine), len(text) + count(vp & theirs) - count(vn & theirs))


def _cases():
    rng = random.Random(2026)
    letters = lambda n, alphabet=b"ACGT": bytes(rng.choice(alphabet) for _ in range(n))
    cases = []
    for words in (8, 9, 10):
        room = 32 * words - 2
        for _ in range(6):  # anywhere in the vector
            l1 = rng.randint(0, room)
            cases.append((letters(l1), letters(rng.randint(0, room - l1)), words))
        l2 = rng.randint(1, 100)
        cases.append((letters(room - l2), letters(l2), words))  # q1 at exactly 32 k - 2 - L2: no phantom row
    cases.append((letters(60), letters(95), 8))    # s0 at bit 159 = bit 31 of word 4, s1 at bit 0 of word 5
    cases.append((letters(90), letters(100), 8))   # s0 and s1 inside word 4
    cases.append((letters(127), letters(127), 8))  # both 127: s0 at bit 127, s1 at bit 128
    cases.append((b"", letters(150), 9))           # empty q1
    cases.append((letters(150), b"", 9))           # empty q2
    cases.append((b"", b"", 1))
    cases.append((letters(15), letters(15), 1))    # one word, full
    return cases


def test_the_packed_column_scores_what_the_oracle_scores(oracle):
    rng = random.Random(11)
    texts = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 180))) for _ in range(24)] + [b""]
    for first, second, words in _cases():
        expected = oracle.levenshtein([first, second], texts)
        for j, text in enumerate(texts):
            got = pair_distances(first, second, text, words)
            assert got == (int(expected[0, j]), int(expected[1, j])), (len(first), len(second), words, len(text))


def test_random_alphabets_and_lengths(oracle):
    rng = random.Random(5)
    for _ in range(40):
        alphabet = bytes(rng.sample(range(256), rng.randint(1, 6)))
        word = lambda n: bytes(rng.choice(alphabet) for _ in range(n))
        words = rng.randint(1, PAIR_WORDS)
        l1 = rng.randint(0, 32 * words - 2)
        first, second = word(l1), word(rng.randint(0, 32 * words - 2 - l1))
        texts = [word(rng.randint(0, 70)) for _ in range(6)]
        expected = oracle.levenshtein([first, second], texts)
        for j, text in enumerate(texts):
            assert pair_distances(first, second, text, words) == (int(expected[0, j]), int(expected[1, j]))


def words_of(length):
    return (length + 31) // 32 if length else 1


def slots(descending):
    """myers_short_body: slot s -> (query rank s, query rank s + ceil(Q / 2) or None, words of the pair's vector or None when the
    two run one after the other)."""
    count = len(descending)
    half = (count + 1) // 2
    for s in range(half):
        if s + half >= count:
            yield s, None, None
            continue
        l1, l2 = descending[s], descending[s + half]
        pair = (l1 + l2 + 2 + 31) // 32
        yield s, s + half, pair if pair <= words_of(l1) + words_of(l2) and pair <= PAIR_WORDS else None


def test_every_query_is_scored_exactly_once():
    rng = random.Random(3)
    for count in (1, 2, 3, 7, 1024, 1025):
        lengths = sorted((rng.randint(0, 256) for _ in range(count)), reverse=True)
        used = Counter()
        for first, second, _ in slots(lengths):
            used[first] += 1
            if second is not None:
                used[second] += 1
        assert sorted(used) == list(range(count)) and set(used.values()) == {1}


def test_pairs_use_more_of_the_vector_on_config_2_lengths():
    rng = np.random.default_rng(2)
    lengths = sorted(rng.integers(96, 161, size=1024).tolist(), reverse=True)
    real = sum(lengths)
    single = sum(32 * words_of(n) for n in lengths)
    paired = 0
    for first, second, pair in slots(lengths):
        if second is None:
            paired += 32 * words_of(lengths[first])
        elif pair is None:
            paired += 32 * (words_of(lengths[first]) + words_of(lengths[second]))
        else:
            paired += 32 * pair
    assert real / single < 0.9 and real / paired > 0.93, (real / single, real / paired)


# ---- the code object


def _functions(assembly):
    current, body = None, []
    for line in assembly.splitlines():
        start = re.match(r"^(_Z\w+):", line)
        if start and current is None:
            current, body = start.group(1), []
        elif current is not None:
            if line.startswith(".Lfunc_end"):
                yield current, body
                current = None
            else:
                body.append(line)


def _loops(body):
    loops, header, block = defaultdict(Counter), None, None
    for line in body:
        label = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", line)
        if label:
            block, comment = label.group(1), label.group(2) or ""
            inside = re.search(r"in Loop: Header=(BB\d+_\d+)", comment)
            header = ".L" + inside.group(1) if inside else (block if "Loop Header" in comment else None)
            continue
        if re.match(r"^\s*;\s*=>.*Loop Header", line) and block:
            header = block
            continue
        token = line.strip().split(None, 1)[0] if line.strip() else ""
        if header and token.startswith("v_"):
            loops[header][re.sub(r"_e(32|64)$", "", token)] += 1
    return loops


LOGIC = {"v_and_b32", "v_or_b32", "v_xor_b32", "v_not_b32", "v_bitop3_b32", "v_xnor_b32", "v_or3_b32", "v_and_or_b32"}


@pytest.fixture(scope="module")
def assembly():
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc is needed to build the library, and so to check what it compiles to"
    source = os.path.join(ROOT, "stringzilla_amd", "csrc", "hip", "lev_myers.hip")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-S", "--cuda-device-only"]
    return subprocess.run([hipcc, *flags, source, "-o", "-"], check=True, capture_output=True, text=True).stdout


@pytest.mark.parametrize("kernel", ["levenshtein_myers_short_fused_kernelILb0E", "levenshtein_myers_short_kernelILb0E"])
def test_short_kernels_keep_the_column_at_its_instruction_floor(assembly, kernel):
    bodies = {name: body for name, body in _functions(assembly) if kernel in name}
    assert len(bodies) == 1, sorted(bodies)
    (name, body), = bodies.items()
    descriptor = assembly.index(".amdhsa_kernel " + name)
    scratch = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", assembly[descriptor:])
    assert scratch and int(scratch.group(1)) == 0, (name, scratch and scratch.group(1))
    seen = {}
    for header, opcodes in _loops(body).items():
        steps = opcodes["v_add_co_u32"] + opcodes["v_addc_co_u32"]  # one carry link per word-step
        if steps < 32:  # the main loops of four words and more: 8 columns x W words
            continue
        seen[header] = sum(opcodes[k] for k in LOGIC) / steps
    assert seen, name
    worst = max(seen.values())
    assert worst <= 7.3, (name, sorted(seen.items(), key=lambda kv: -kv[1])[:4])

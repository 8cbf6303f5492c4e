"""Seeded batches that drive the fingerprint kernels (hip/fingerprints.hip) to the ENDS of their hash arithmetic.

The kernel does one fused update per byte, x = hash * multiplier + (new + 1) + complement * (old + 1), and reduces it with ONE
Barrett step whose reciprocal is rounded down, followed by ONE `residue >= modulo ? residue - modulo : residue`.  On random
bytes the hash is uniform in [0, modulo), so neither the equality of that `>=` (x an exact multiple of the modulo) nor the top
of the range (x next to its bound of ~896 modulo) nor a repeated minimum is ever met.  Here they are PLANTED: the parameters of
a dimension are integer functions of `seed + dimension`, so the last six bytes of a window can be solved (meet in the middle,
3 + 3 bytes) for the window to hash to any chosen residue - 0, modulo - 1, or one whose low 32 bits are 0xFFFFFFFF, the value
that also marks "text shorter than the window".

What is here:
  - the exact integer model (Python ints): `splitmix64`, `parameters`, `window_hash`, `fingerprint`, `export`.  It is the
    high-precision reference and imports nothing of the library under test;
  - `plant()`, the planter, and `search()`, which picks the window a batch uses;
  - `batches()`: every batch with its aims, each aim asserted from integers alone;
  - `write()` (`python -m tests.fingerprint_range_cases --write`): runs the planter and stores the solved bytes together with
    what the reference's serial engines return for every batch in tests/golden/fingerprint_ranges.json.  Tests read that file;
    only one model test runs the planter, once.

Quotients x // modulo that the planted "top" steps reach (a property of the inputs, found on the CPU; `write()` prints them,
tests/test_fingerprint_ranges_model.py asserts them): the step that LEAVES a planted window - hash modulo - 1, 0xFF entering,
0xFF leaving - has x = (modulo - 1) * multiplier + 256 + 256 * complement, the dimension's own bound: 765 to 868 over the eight
planted (engine, width) pairs, 868 in 128 dimensions of width 7, seed 1, dimension 112; the step that ENTERS it reaches 743 to
840.  Per width the dimension with the largest bound is taken, out of the 21 to 128 that have the width; width 6 is left out,
six solved bytes leave no room for the leading 0xFF.  No input can take any dimension beyond 895 modulo (multiplier 639,
complement modulo - 1).

A plain module: no fixtures, no settings.  tests/test_fingerprint_ranges_model.py (CPU) and tests/test_gpu_fingerprint_ranges.py
import it.
"""
import base64
import functools
import json
import os
import sys
from typing import NamedTuple

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fingerprint_ranges.json")
SEGMENT = 4096  # window END positions a workgroup hashes (hip/fingerprints.hip: fingerprint_segment_k)
STAGED_WIDEST = 1024  # windows up to here are staged in LDS, wider ones are read in place (fingerprint_max_width_k)
SKIPPED = (0xFFFFFFFF, 0)  # what a text shorter than the window exports
MASK64 = (1 << 64) - 1

# ---- the exact integer model ----------------------------------------------------------------------------------------------


def splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) & MASK64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


@functools.lru_cache(maxsize=None)
def parameters(dimensions, widths, seed):
    """[(width, multiplier, modulo)] per dimension.  `widths`: a tuple.  A dimension's width is `widths[(dim // 64) % count]`
    when `dimensions` is a whole multiple of 64 x count (the sliced engines), else `widths[dim % count]`."""
    count = len(widths)
    sliced = dimensions % count == 0 and (dimensions // count) % 64 == 0
    result = []
    for dim in range(dimensions):
        mixed = splitmix64((seed + dim) & MASK64)
        result.append((widths[(dim // 64 if sliced else dim) % count], 256 + mixed % 384, 4503599626977 - splitmix64(mixed) % (1 << 20)))
    return result


def window_hash(window, multiplier, modulo):
    """sum (byte_i + 1) multiplier^(width - 1 - i)  mod  modulo."""
    value = 0
    for byte in window:
        value = (value * multiplier + byte + 1) % modulo
    return value


def complement_of(width, multiplier, modulo):
    return -pow(multiplier, width, modulo) % modulo


def bound_of(width, multiplier, modulo):
    """The largest quotient x // modulo a rolled step of this dimension can have: hash modulo - 1, 0xFF entering and leaving."""
    return ((modulo - 1) * multiplier + 256 + 256 * complement_of(width, multiplier, modulo)) // modulo


def fingerprint(text, width, multiplier, modulo):
    """(minimum, count, largest x // modulo of the rolled steps) over all windows; None when the text is shorter than one."""
    if len(text) < width:
        return None
    complement = complement_of(width, multiplier, modulo)
    value = window_hash(text[:width], multiplier, modulo)
    minimum, count, largest = value, 1, 0
    terms = [byte + 1 for byte in text]
    for entering, leaving in zip(terms[width:], terms):
        x = value * multiplier + entering + complement * leaving
        if x > largest:
            largest = x
        value = x % modulo
        if value < minimum:
            minimum, count = value, 1
        elif value == minimum:
            count += 1
    return minimum, count, largest // modulo


def export(state):
    """(hash, count) as the engines return them: the low 32 bits of the minimum."""
    return SKIPPED if state is None else (state[0] & 0xFFFFFFFF, state[1])


# ---- the planter ----------------------------------------------------------------------------------------------------------


def entering_quotient(window, before, multiplier, modulo):
    """x // modulo of the rolled step that completes `window` when the byte `before` precedes it."""
    previous = window_hash(bytes([before]) + window[:-1], multiplier, modulo)
    x = previous * multiplier + window[-1] + 1 + complement_of(len(window), multiplier, modulo) * (before + 1)
    return x // modulo


def plant(multiplier, modulo, target, prefix=b"", before=0xFF):
    """Every window `prefix` + six bytes whose hash is `target`, in the order of the six bytes, as (window, quotient): the
    quotient x // modulo of the rolled step that completes the window after the byte `before`.  Meet in the middle: the 2^24
    three-byte tails sorted by value, the value each three-byte head still needs looked up among them."""
    digits = np.arange(1, 257, dtype=np.uint64)
    triples = (digits[:, None, None] * np.uint64(multiplier * multiplier) + digits[None, :, None] * np.uint64(multiplier) + digits[None, None, :]).reshape(-1)
    order = np.argsort(triples, kind="stable")  # a triple's index is its three bytes, big end first
    tails = triples[order]
    needed = (target - window_hash(prefix, multiplier, modulo) * pow(multiplier, 6, modulo)) % modulo
    needs = (np.uint64(needed + modulo) - (triples * np.uint64(multiplier**3)) % np.uint64(modulo)) % np.uint64(modulo)  # below 2^55 throughout
    heads = np.flatnonzero(needs <= tails[-1])
    at = np.minimum(np.searchsorted(tails, needs[heads]), len(tails) - 1)
    hit = tails[at] == needs[heads]
    found = []
    for head, tail in zip(heads[hit].tolist(), order[at[hit]].tolist()):
        window = prefix + head.to_bytes(3, "big") + tail.to_bytes(3, "big")
        assert window_hash(window, multiplier, modulo) == target
        found.append((window, entering_quotient(window, before, multiplier, modulo)))
    return found


def filler(count, *salt):
    """`count` bytes that depend on `salt` alone."""
    return np.random.default_rng([int(s) for s in salt]).integers(0, 256, size=count, dtype=np.uint8).tobytes()


class Plant(NamedTuple):
    dimensions: int
    widths: tuple
    seed: int
    dim: int
    kind: str  # "zero", "top" or "ones"

    def describe(self):
        width, multiplier, modulo = parameters(self.dimensions, self.widths, self.seed)[self.dim]
        target = {"zero": 0, "top": modulo - 1, "ones": (3 << 32) | 0xFFFFFFFF}[self.kind]
        lead = b"\xff" if self.kind == "top" else b""  # a top window starts with 0xFF: the step that leaves it is the bound itself
        prefix = lead + filler(width - 6 - len(lead), self.seed, self.dim, width, len(self.kind))
        return width, multiplier, modulo, target, prefix


def search(plant_):
    """The six bytes this plant uses: the planter's first solution, for a top window the one whose entering step is largest."""
    width, multiplier, modulo, target, prefix = plant_.describe()
    found = plant(multiplier, modulo, target, prefix)
    window, quotient = max(found, key=lambda entry: entry[1]) if plant_.kind == "top" else found[0]
    return window[-6:], quotient, len(found)


def top_dimension(dimensions, widths, seed, width, skip=0):
    """The dimension of this width whose bound is largest (`skip`: the next best ones)."""
    ranked = sorted((-bound_of(*p), dim) for dim, p in enumerate(parameters(dimensions, widths, seed)) if p[0] == width)
    return ranked[skip][1]


# Engines: the sliced path; the per-dimension path with idle lanes; the widest staged window; the kernel that reads in place.
SLICED, FALLBACK, STAGED, IN_PLACE, MIXED, NARROW = (128, (7,)), (100, (6, 9, 31)), (128, (1024,)), (64, (1025,)), (70, (7, 4097, 65536)), (256, (2, 3, 4, 5))
ZERO_PLANTS = [  # dimensions of both wavefronts of an engine, of every template
    Plant(*SLICED, 1, 3, "zero"), Plant(*SLICED, 2, 70, "zero"), Plant(*FALLBACK, 1, 4, "zero"), Plant(*FALLBACK, 2, 66, "zero"),
    Plant(*FALLBACK, 2, 98, "zero"), Plant(*STAGED, 2, 100, "zero"), Plant(*IN_PLACE, 1, 37, "zero"), Plant(*MIXED, 2, 66, "zero"),
    Plant(*MIXED, 2, 1, "zero"), Plant(*MIXED, 1, 68, "zero")]
ONES_PLANTS = [Plant(*SLICED, 1, 70, "ones"), Plant(*FALLBACK, 1, 98, "ones"), Plant(*IN_PLACE, 2, 5, "ones")]
TOP_ENGINES = [(SLICED, 1), (FALLBACK, 2), (STAGED, 1), (IN_PLACE, 2), (MIXED, 1)]  # a top plant per width of each
RUN_ENGINES = [(SLICED, 2), (FALLBACK, 1), (NARROW, 1), (STAGED, 2), (IN_PLACE, 1), (MIXED, 2)]
LONGEST_RUN = 1 << 20


def top_plants(windows=None):
    """Per (engine, width) the dimension with the largest bound - the next one where no solution's entering step reaches three
    quarters of it (chance below 10^-6 with 50 solutions).  With stored `windows` the choice made at generation is read back."""
    chosen = []
    for (dimensions, widths), seed in TOP_ENGINES:
        for width in widths:
            if width < 7:  # six solved bytes after the leading 0xFF
                continue
            for skip in range(4):
                candidate = Plant(dimensions, widths, seed, top_dimension(dimensions, widths, seed, width, skip), "top")
                if windows is not None and candidate in windows:
                    break
                if windows is None and 4 * search(candidate)[1] >= 3 * bound_of(*parameters(dimensions, widths, seed)[candidate.dim]):
                    break
            else:
                raise AssertionError(f"no top window for {dimensions} {widths} seed {seed} width {width}")
            chosen.append(candidate)
    return chosen


# ---- the batches ----------------------------------------------------------------------------------------------------------


class Aim(NamedTuple):
    text: int  # index into the batch's texts
    dim: int
    hash: int  # what the engines must return there ...
    count: int  # ... and how often
    why: str


class Batch(NamedTuple):
    name: str
    dimensions: int
    widths: tuple
    seed: int
    texts: list
    aims: list
    planted: tuple  # the dimensions the integer model is compared on for every text of the batch
    quotients: tuple  # top batches: (dimension's bound, quotient of the entering step, of the leaving step)

    def model(self, text, dim):
        return export(fingerprint(self.texts[text], *parameters(self.dimensions, self.widths, self.seed)[dim]))


def stored_windows():
    with open(GOLDEN) as handle:
        stored = json.load(handle)
    return {Plant(w["dimensions"], tuple(w["widths"]), w["seed"], w["dim"], w["kind"]): bytes.fromhex(w["solved"]) for w in stored["windows"]}


def _window(windows, plant_):
    width, multiplier, modulo, target, prefix = plant_.describe()
    window = prefix + windows[plant_]
    assert len(window) == width and window_hash(window, multiplier, modulo) == target, plant_
    return window


def _placed(window, starts, length, *salt):
    """Filler of `length` bytes with `window` written at every start."""
    text = bytearray(filler(length, *salt))
    for start in starts:
        assert start >= 0 and start + len(window) <= length
        text[start:start + len(window)] = window
    return bytes(text)


def _zero_batch(windows, plant_):
    width, multiplier, modulo, _, _ = plant_.describe()
    zero = _window(windows, plant_)
    salt = (plant_.seed, plant_.dim, width)
    later_end = max(SEGMENT, -(-width // SEGMENT) * SEGMENT)  # the first window a later segment owns ends here
    texts, plants, whys = [], [], []

    def add(why, starts, length):
        texts.append(_placed(zero, starts, length, *salt, len(texts)))
        plants.append(starts), whys.append(why)

    add("the whole text (first-window loop)", [0], width)
    add("the first window of a longer text (first-window loop)", [0], width + 300)
    add("deep inside a text (rolled loop)", [300], width + 500)
    add("the first window of a later segment", [later_end - width + 1], later_end + 1 + max(100, SEGMENT + width - later_end) + 50)
    if width <= 5000:  # (wider: one text of three plants is all a 65536-byte window needs)
        if 3 * width + 300 < SEGMENT:
            add("twice within one segment (tie in the rolled loop)", [100, 150 + width], 2 * width + 210)
            add("three times within one segment", [100, 150 + width, 200 + 2 * width], 3 * width + 260)
            add("once in each of three segments (ties in the merge)", [200, SEGMENT + 300, 2 * SEGMENT + 10], 2 * SEGMENT + 90 + width)
        add("in the last segment only (merge: replace)", [2 * SEGMENT + 80], 2 * SEGMENT + 100 + width)
        add("in the first segment with windows only (merge: ignore)", [5], 2 * SEGMENT + 100 + width)
    if 3 * width + 300 >= SEGMENT:
        add("three times, each in a segment of its own (ties in the merge)", [40, 140 + width, 240 + 2 * width], 3 * width + 300)
    aims = []
    for index, (text, starts, why) in enumerate(zip(texts, plants, whys)):
        ends = [start + width - 1 for start in starts]
        assert all(text[start:start + width] == zero for start in starts)
        if "first-window loop" in why:
            assert starts == [0]
        if "rolled loop" in why or "within one segment" in why:
            assert len({end // SEGMENT for end in ends}) == 1 and min(ends) > max(width - 1, min(ends) // SEGMENT * SEGMENT)
        if "later segment" in why:
            assert ends[0] % SEGMENT == 0 and ends[0] > width - 1 and len(text) > SEGMENT + width
        if "merge" in why and len(starts) == 3:
            assert len({end // SEGMENT for end in ends}) == 3
        if "replace" in why:
            assert ends[0] // SEGMENT == (len(text) - 1) // SEGMENT > (width - 1) // SEGMENT
        if "ignore" in why:
            assert ends[0] // SEGMENT == (width - 1) // SEGMENT < (len(text) - 1) // SEGMENT
        state = fingerprint(text, width, multiplier, modulo)
        assert state[:2] == (0, len(starts)), (plant_, why, state)  # from integers alone: the minimum is 0, once per plant
        aims.append(Aim(index, plant_.dim, 0, len(starts), why))
    return Batch(f"zero/{plant_.dimensions}/{plant_.seed}/{plant_.dim}/w{width}", plant_.dimensions, plant_.widths, plant_.seed, texts, aims, (plant_.dim,), ())


def _top_batch(windows, plant_):
    width, multiplier, modulo, _, _ = plant_.describe()
    top = _window(windows, plant_)
    assert top[0] == 0xFF
    bound, entering = bound_of(width, multiplier, modulo), entering_quotient(top, 0xFF, multiplier, modulo)
    assert 4 * entering >= 3 * bound, (plant_, entering, bound)
    salt = (plant_.seed, plant_.dim, width, 7)
    texts = []
    if width <= 5000:
        texts.append(_placed(b"\xff" + top + b"\xff", [120], width + 300, *salt, 0))
    texts.append(_placed(b"\xff" + top + b"\xff", [120], width + 2 * SEGMENT + 300, *salt, 1))  # two more segments of later windows
    aims = []
    for index, text in enumerate(texts):
        minimum, count, largest = fingerprint(text, width, multiplier, modulo)
        assert largest == bound, (plant_, largest, bound)  # the step that leaves the window IS the bound: nothing larger exists
        assert minimum < modulo - 1  # the planted window is never the minimum: a wrong state shows in the windows after it
        assert len(text) - (121 + width) >= (2 * SEGMENT if index == len(texts) - 1 else 1)
        aims.append(Aim(index, plant_.dim, minimum & 0xFFFFFFFF, count, "every window after a step at the dimension's bound"))
    return Batch(f"top/{plant_.dimensions}/{plant_.seed}/{plant_.dim}/w{width}", plant_.dimensions, plant_.widths, plant_.seed, texts, aims, (plant_.dim,),
                 (bound, entering, bound))


def _ones_batch(windows, plant_):
    width = plant_.describe()[0]
    ones = _window(windows, plant_)
    texts = [ones, ones[:-1]]
    aims = [Aim(0, plant_.dim, 0xFFFFFFFF, 1, "a hash whose low 32 bits are all ones, met once")]
    aims += [Aim(1, dim, *SKIPPED, "one byte short of the window") for dim, p in enumerate(parameters(plant_.dimensions, plant_.widths, plant_.seed)) if p[0] == width]
    batch = Batch(f"ones/{plant_.dimensions}/{plant_.seed}/{plant_.dim}/w{width}", plant_.dimensions, plant_.widths, plant_.seed, texts, aims, (plant_.dim,), ())
    assert batch.model(0, plant_.dim) == (0xFFFFFFFF, 1) and all(batch.model(1, aim.dim) == SKIPPED for aim in aims[1:])
    return batch


def _run_batch(dimensions, widths, seed, longest=False):
    """Texts of one byte value: every window is the same, so the count is n - width + 1 in EVERY dimension - widths 2 to 5
    included, which cannot be planted.  Then texts of period 2, 3 and 64, whose counts the integer model derives."""
    every = parameters(dimensions, widths, seed)
    sample = tuple(sorted({min(dim for dim, p in enumerate(every) if p[0] == width) for width in widths} | {dimensions - 1}))
    if longest:  # 256 segments of one text: the counts of all of them summed in the merge
        text = b"\xff" * LONGEST_RUN
        aims = [Aim(0, dim, window_hash(text[:p[0]], p[1], p[2]) & 0xFFFFFFFF, LONGEST_RUN - p[0] + 1, "a run: every window alike") for dim, p in enumerate(every)]
        return Batch(f"runs/longest/{dimensions}/{seed}", dimensions, widths, seed, [text], aims, sample[1:3], ())
    lengths = sorted({n for width in widths for n in (width - 1, width, width + 1, SEGMENT + width - 1)} | {SEGMENT - 1, SEGMENT, SEGMENT + 1, 3 * SEGMENT + 5})
    values = (0x00, 0xFF, ord("A")) if max(widths) <= 5000 else (0xFF,)
    texts = [bytes([value]) * n for value in values for n in lengths]
    aims, alike = [], {}
    for index, text in enumerate(texts):
        for dim in range(dimensions):
            width, multiplier, modulo = every[dim]
            if len(text) < width:
                aims.append(Aim(index, dim, *SKIPPED, "a run shorter than the window"))
                continue
            if (text[0], dim) not in alike:
                alike[text[0], dim] = window_hash(text[:width], multiplier, modulo) & 0xFFFFFFFF
            aims.append(Aim(index, dim, alike[text[0], dim], len(text) - width + 1, "a run: every window alike"))
    periodic = SEGMENT + 77 + (max(widths) if max(widths) <= 5000 else 0)
    for period in (b"\x00\xff", b"abc", filler(64, seed, dimensions)):
        texts.append((period * (periodic // len(period) + 1))[:periodic])
        for dim in sample:
            aims.append(Aim(len(texts) - 1, dim, *export(fingerprint(texts[-1], *every[dim])), f"period {len(period)}"))
            width = every[dim][0]
            assert width > periodic or aims[-1].count >= (periodic - width + 1) // len(period)  # every window recurs with the period
    return Batch(f"runs/{dimensions}/{seed}/w{'-'.join(map(str, widths))}", dimensions, widths, seed, texts, aims, sample, ())


def batches(windows=None):
    """Every batch.  `windows`: {Plant: six solved bytes}; None reads the stored ones."""
    return list(_batches(windows)) if windows is not None else _stored_batches()


@functools.lru_cache(maxsize=None)
def _stored_batches():
    return list(_batches(stored_windows()))  # shared between tests: not to be written to


def _batches(windows):
    for plant_ in ZERO_PLANTS:
        yield _zero_batch(windows, plant_)
    for plant_ in top_plants(windows):
        yield _top_batch(windows, plant_)
    for plant_ in ONES_PLANTS:
        yield _ones_batch(windows, plant_)
    for (dimensions, widths), seed in RUN_ENGINES:
        yield _run_batch(dimensions, widths, seed)
    yield _run_batch(12, (3, 7, 31), 2, longest=True)


# ---- the stored file ------------------------------------------------------------------------------------------------------


def pack(matrix):
    """A uint32 matrix as its distinct rows (base64 of little-endian words) and the row each line is."""
    rows, of = [], []
    for row in np.ascontiguousarray(matrix, dtype="<u4"):
        encoded = base64.b64encode(row.tobytes()).decode()
        if encoded not in rows:
            rows.append(encoded)
        of.append(rows.index(encoded))
    return {"rows": rows, "of": of}


def unpack(packed, dimensions):
    rows = [np.frombuffer(base64.b64decode(row), dtype="<u4") for row in packed["rows"]]
    return np.array([rows[index] for index in packed["of"]], dtype=np.uint32).reshape(len(packed["of"]), dimensions)


def stored_results():
    """{batch name: (min_hashes, min_counts)} of the reference's serial engines, as recorded."""
    with open(GOLDEN) as handle:
        stored = json.load(handle)
    return {name: (unpack(r["min_hashes"], r["dimensions"]), unpack(r["min_counts"], r["dimensions"])) for name, r in stored["results"].items()}


def render():
    """The text of tests/golden/fingerprint_ranges.json: runs the planter, then the reference's engines on every batch."""
    from oracle import binding

    plants = ZERO_PLANTS + top_plants() + ONES_PLANTS
    windows, entries = {}, []
    for plant_ in plants:
        solved, quotient, solutions = search(plant_)
        width, multiplier, modulo, target, _ = plant_.describe()
        windows[plant_] = solved
        entries.append({"dimensions": plant_.dimensions, "widths": list(plant_.widths), "seed": plant_.seed, "dim": plant_.dim, "kind": plant_.kind,
                        "width": width, "target": target, "solved": solved.hex(), "solutions": solutions})
        if plant_.kind == "top":
            print(f"top: {plant_.dimensions} dimensions {list(plant_.widths)} seed {plant_.seed} dimension {plant_.dim} width {width}: "
                  f"entering step {quotient}, leaving step and bound {bound_of(width, multiplier, modulo)}, {solutions} solutions")
    results = {}
    for batch in batches(windows):
        hashes, counts, kind = binding.reference_fingerprints(batch.texts, batch.dimensions, list(batch.widths), batch.seed)
        results[batch.name] = {"dimensions": batch.dimensions, "reference_engine": kind, "min_hashes": pack(hashes), "min_counts": pack(counts)}
    return json.dumps({"generator": "python -m tests.fingerprint_range_cases --write", "windows": entries, "results": results}, separators=(",", ":")) + "\n"


def write():
    text = render()
    with open(GOLDEN, "w") as handle:
        handle.write(text)
    print(f"wrote {GOLDEN}: {len(text)} bytes")


if __name__ == "__main__":
    if "--write" not in sys.argv:
        sys.exit("usage: python -m tests.fingerprint_range_cases --write")
    write()

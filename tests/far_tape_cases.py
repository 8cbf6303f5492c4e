"""Where the tapes of tests/test_gpu_far_tapes.py lie inside ONE buffer of 2^32 + 2^20 bytes, and what is written there.

A tape is a byte buffer plus `count + 1` offsets.  Every kernel that reads one on the device turns `offsets[i]`, `offsets[i + 1]` and
the buffer's address into a pointer and a 32-bit length; an offset kept in 32 bits on the way, or a sum of two of them, shows on no
input of a few kilobytes.  `plan()` places a batch so that it does:

  place       offsets                                                    what a 32-bit slip does there
  far_a/b     u64, all of them >= 2^32 + 12345                            reads `offset - 2^32`: the DECOY, see below
  straddle    u64, the string that holds the batch's middle byte lies     that string: `(u32)from > (u32)to`; the strings behind it
              across byte 2^32, about half of the bytes on either side    read the decoy, the ones before it are read correctly
  top_a       u32, the last offset is exactly 2^32 - 1                    `from + length`, `align4(from - first) + 8 i` wrap to ~0
  top_b       u32, ends 64 bytes below top_a's first byte                 (the other side of a two-sided call on `top`)
  text        no tape: 5000 bytes around byte 2^32, the scans' one text

DECOYS.  For every byte of a u64 tape at a position p >= 2^32 another byte lies at p - 2^32: the batch's own bytes, shuffled by a
seeded generator - the same lengths, the same alphabet, other strings.  A kernel that drops the high half of an offset scores valid
but WRONG strings: a clean mismatch, never a fault and never garbage.  The rest of the buffer is zero, and every place is zeroed
before it is written, so what a wrapped sum reads is the same in every run.

The regions are laid out once, below; `check_layout()` asserts that no two of them overlap - payloads (with 64 bytes of slack behind
each: the byte kernels read whole aligned dwords), decoys and the text.  One exception cannot be avoided and is asserted instead: the
bytes just BELOW 2^32 serve the straddling tape, the top tapes or the text - a tape that ends at 2^32 - 1 and a string that holds
byte 2^32 - 1 want the same bytes - so a call uses the straddling tape, the two top tapes or the text, never two of these, and
what one call uses lies apart.

A plain module: NumPy only, no GPU, no fixtures.
"""
from typing import NamedTuple, Optional

import numpy as np

LINE = 1 << 32
SIZE = LINE + (1 << 20)  # the buffer
SLACK = 64  # bytes kept free behind the last string of a tape
CAPACITY = 160 * 1024  # the bytes of one side's batch, at most
TEXT = 5000


class Region(NamedTuple):
    name: str
    start: int
    stop: int  # slack included


def _region(name, start, payload=CAPACITY):
    return Region(name, start, start + payload + SLACK)


# payloads; the order of the far places leaves the straddling tape's upper half free
STRADDLE = Region("straddle", LINE - CAPACITY, LINE + CAPACITY + SLACK)
FAR_A = _region("far_a", STRADDLE.stop + 12345)
FAR_B = _region("far_b", FAR_A.stop + 3)  # odd: the two sides of a call start at different byte alignments
TOP_A = Region("top_a", LINE - 1 - CAPACITY, LINE - 1 + SLACK)
TOP_B = Region("top_b", TOP_A.start - SLACK - CAPACITY, TOP_A.start)
TEXT_REGION = Region("text", LINE - TEXT // 2, LINE - TEXT // 2 + TEXT + SLACK)
PLACES = {region.name: region for region in (STRADDLE, FAR_A, FAR_B, TOP_A, TOP_B)}
BELOW_THE_LINE = ("straddle", "top_a", "top_b", "text")  # one of them at a time
WIDE = {"straddle": True, "far_a": True, "far_b": True, "top_a": False, "top_b": False}


def decoy_of(region):
    """Where the decoy of a u64 place lies: its bytes at and above 2^32, moved down by 2^32."""
    return Region("decoy of " + region.name, max(region.start, LINE) - LINE, region.stop - LINE)


DECOYS = {name: decoy_of(PLACES[name]) for name in ("straddle", "far_a", "far_b")}

# (place of the queries, place of the candidates); None: an ordinary tape of its own, offsets from 0
KINDS = {
    "far": ("far_a", "far_b"),
    "far_near": ("far_a", None),
    "near_far": (None, "far_b"),
    "straddling": ("far_a", "straddle"),
    "straddling_queries": ("straddle", "far_b"),
    "top": ("top_b", "top_a"),
    "top_queries": ("top_a", "top_b"),
}


def check_layout():
    """No two regions overlap, but for the places below the line, of which a plan uses one; all of them inside the buffer."""
    regions = list(PLACES.values()) + list(DECOYS.values()) + [TEXT_REGION]
    for region in regions:
        assert 0 <= region.start < region.stop <= SIZE, region
    apart = lambda one, other: one.stop <= other.start or other.stop <= one.start
    for at, one in enumerate(regions):
        for other in regions[at + 1:]:
            if one.name in BELOW_THE_LINE and other.name in BELOW_THE_LINE and {one.name, other.name} != {"top_a", "top_b"}:
                continue
            assert apart(one, other), (one, other)
    for name in ("far_a", "far_b"):
        assert PLACES[name].start >= LINE + 12345
    for kind, (q_place, c_place) in KINDS.items():  # what one call uses lies apart, decoys included
        used = [region for place in (q_place, c_place) if place for region in (PLACES[place], DECOYS.get(place)) if region]
        assert all(apart(one, other) for at, one in enumerate(used) for other in used[at + 1:]), kind
    assert apart(TEXT_REGION, FAR_A) and apart(TEXT_REGION, DECOYS["far_a"])  # the scans: far queries and the text
    return regions


class Side(NamedTuple):
    place: Optional[str]  # None: near
    strings: list
    offsets: Optional[np.ndarray]  # uint64 or uint32, `count + 1` of them; None: near
    writes: list  # (position in the buffer, uint8 array): the payload, then its decoy
    regions: list  # what to zero before writing


class Plan(NamedTuple):
    kind: str
    queries: Side
    candidates: Optional[Side]


def offsets_at(place, lengths):
    """The offsets of strings of these lengths at `place`: the far places begin at their region's first byte, the top ones END at
    its last, and the straddling one puts byte 2^32 inside the string that holds the middle byte of the batch."""
    lengths = np.asarray(lengths, dtype=np.int64)
    ends = np.cumsum(lengths)
    total = int(ends[-1]) if len(ends) else 0
    assert total <= CAPACITY, (place, total)
    region = PLACES[place]
    if place.startswith("far"):
        first = region.start
    elif place.startswith("top"):
        first = region.stop - SLACK - total
    else:
        assert total > 0, "a batch of no bytes straddles nothing"
        across = int(np.searchsorted(ends, total // 2, side="right"))  # the string that holds byte total // 2: it is not empty
        before = int(ends[across] - lengths[across])
        first = LINE - before - max(1, int(lengths[across]) // 2)
        assert first + before < LINE <= first + int(ends[across])
    offsets = np.zeros(len(lengths) + 1, dtype=np.uint64)
    offsets[0] = first
    offsets[1:] = ends.astype(np.uint64) + np.uint64(first)
    assert region.start <= first and first + total + SLACK <= region.stop
    if not WIDE[place]:
        assert int(offsets[-1]) < LINE
        offsets = offsets.astype(np.uint32)
    return offsets


def side_at(place, strings, seed):
    strings = [bytes(string) for string in strings]
    if place is None:
        return Side(None, strings, None, [], [])
    offsets = offsets_at(place, [len(string) for string in strings])
    first = int(offsets[0])
    payload = np.frombuffer(b"".join(strings), dtype=np.uint8).copy()
    writes, regions = [(first, payload)], [PLACES[place]]
    if place in DECOYS:
        shuffled = np.random.default_rng(seed).permutation(payload)  # the same lengths and letters, other strings
        above = max(LINE - first, 0)  # the bytes below the line have no place 2^32 further down
        writes.append((first + above - LINE, shuffled[above:]))
        regions.append(DECOYS[place])
    return Side(place, strings, offsets, writes, regions)


def plan(kind, queries, candidates=None, seed=0):
    """Where the two sides of a call of `kind` go (`candidates` None: a symmetric call, the queries' place alone)."""
    q_place, c_place = KINDS[kind]
    return Plan(kind, side_at(q_place, queries, 2 * seed + 1), None if candidates is None else side_at(c_place, candidates, 2 * seed + 2))


def truncated(side, low):
    """The strings a kernel would read that kept only the low 32 bits of this side's offsets, from `low`: the first 2^20 bytes of the
    buffer as the side's writes leave them.  (A string whose truncated end lies before its start reads as empty.)"""
    assert side.place in ("far_a", "far_b"), "only a side that lies above the line as a whole has all of its decoy in `low`"
    offsets = side.offsets.astype(np.uint64) & np.uint64(LINE - 1)
    return [low[int(a):int(b)].tobytes() if b >= a else b"" for a, b in zip(offsets[:-1], offsets[1:])]


def low_bytes(*sides):
    """The first 2^20 bytes of a zeroed buffer after the writes of `sides`."""
    low = np.zeros(1 << 20, dtype=np.uint8)
    for side in sides:
        for position, blob in side.writes:
            if position < len(low):
                low[position:position + len(blob)] = blob
    return low

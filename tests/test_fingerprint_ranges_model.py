"""The fingerprint kernels' hash arithmetic at its ends, WITHOUT a GPU: the stored windows and every batch's aims by exact
integers, one run of the planter, the C oracle and (where built) the reference's engines against the integer model, and the
kernel's one-step Barrett reduction restated in `float64` and swept over every multiple of every modulo it can meet.
tests/test_gpu_fingerprint_ranges.py shows the same batches to the hardware."""
import functools
import json

import numpy as np
import pytest

from oracle import binding

import fingerprint_range_cases as cases


def test_stored_windows_hit_their_targets_and_batches_reach_their_aims():
    """`batches()` asserts every aim while it builds the texts; here: each stored window against its recorded target, the kinds
    of aim that must be present, and the quotients of the top steps the documents quote."""
    with open(cases.GOLDEN) as handle:
        stored = json.load(handle)
    for entry in stored["windows"]:
        plant = cases.Plant(entry["dimensions"], tuple(entry["widths"]), entry["seed"], entry["dim"], entry["kind"])
        width, multiplier, modulo, target, prefix = plant.describe()
        assert (width, target) == (entry["width"], entry["target"]) and len(prefix) == width - 6
        assert cases.window_hash(prefix + bytes.fromhex(entry["solved"]), multiplier, modulo) == target
        assert target == {"zero": 0, "top": modulo - 1}.get(plant.kind, target) and (plant.kind != "ones" or target & 0xFFFFFFFF == 0xFFFFFFFF and target < modulo)
    batches = cases.batches()
    assert {batch.name for batch in batches} == set(stored["results"])
    whys = {aim.why for batch in batches for aim in batch.aims}
    for needed in ("first-window loop", "rolled loop", "later segment", "twice within one segment", "three times within one segment",
                   "each of three segments", "replace", "ignore", "bound", "all ones", "one byte short", "a run: every window alike", "period 64"):
        assert any(needed in why for why in whys), needed
    planted = {(batch.dimensions, batch.widths, dim // 64) for batch in batches if batch.name.startswith("zero") for dim in batch.planted}
    assert {(128, (7,), 0), (128, (7,), 1), (100, (6, 9, 31), 0), (100, (6, 9, 31), 1), (128, (1024,), 1), (64, (1025,), 0), (70, (7, 4097, 65536), 1)} <= planted
    assert {batch.seed for batch in batches} == {1, 2}
    assert {max(batch.widths) > cases.STAGED_WIDEST for batch in batches if batch.name.startswith(("zero", "top"))} == {False, True}  # both kernel templates
    tops = [batch.quotients for batch in batches if batch.name.startswith("top")]
    assert len(tops) == 8 and all(leaving == bound and 4 * entering >= 3 * bound for bound, entering, leaving in tops)
    assert (min(t[2] for t in tops), max(t[2] for t in tops), min(t[1] for t in tops), max(t[1] for t in tops)) == (765, 868, 743, 840)
    assert max(len(text) for batch in batches for text in batch.texts if max(batch.widths) < 65536) == cases.LONGEST_RUN  # the one long run
    assert sorted({len(text) for batch in batches for text in batch.texts if max(batch.widths) < 65536})[-2] <= 16384


def test_one_planter_run_reproduces_a_stored_window():
    plant = cases.ZERO_PLANTS[0]
    width, multiplier, modulo, target, prefix = plant.describe()
    found = cases.plant(multiplier, modulo, target, prefix)
    assert len(found) >= 30  # 2^48 six-byte endings over a modulo of 2^42: 64 expected
    assert found[0][0][-6:] == cases.stored_windows()[plant] == cases.search(plant)[0]
    complement = cases.complement_of(width, multiplier, modulo)
    for window, quotient in found:  # the quotient it reports is that of the rolled step after 0xFF, and that step lands on the target
        x = cases.window_hash(b"\xff" + window[:-1], multiplier, modulo) * multiplier + window[-1] + 1 + complement * 256
        assert (x // modulo, x % modulo) == (quotient, target)


def _agrees(got, batch, who):
    """`got` = (hashes, counts) of all dimensions: the integer model on every dimension of a small text, on the planted
    dimensions (a run batch: one per width and the last) of a long one, and every aim."""
    hashes, counts = got
    for index, text in enumerate(batch.texts):
        for dim in range(batch.dimensions) if len(text) <= 1200 else batch.planted:
            assert (int(hashes[index, dim]), int(counts[index, dim])) == batch.model(index, dim), (who, batch.name, index, len(text), dim)
    for aim in batch.aims:
        assert (int(hashes[aim.text, aim.dim]), int(counts[aim.text, aim.dim])) == (aim.hash, aim.count), (who, batch.name, aim)


@functools.lru_cache(maxsize=None)
def _oracle(index):
    batch = cases.batches()[index]
    return binding.oracle_fingerprints(batch.texts, batch.dimensions, list(batch.widths), batch.seed)


@pytest.mark.parametrize("kind", ["zero", "top", "ones", "runs"])
def test_oracle_equals_the_integer_model(kind):
    for index, batch in enumerate(cases.batches()):
        if batch.name.startswith(kind):
            _agrees(_oracle(index), batch, "oracle")


def test_reference_engines_agree_and_the_stored_results_are_theirs():
    """Needs the reference's engines built (oracle/_ref); where they are not, the stored results are still held against the
    oracle, dimension by dimension."""
    stored = cases.stored_results()
    for index, batch in enumerate(cases.batches()):
        hashes, counts = stored[batch.name]
        expected = _oracle(index)
        assert np.array_equal(hashes, expected[0]) and np.array_equal(counts, expected[1]), batch.name
        if binding.reference_available():
            live = binding.reference_fingerprints(batch.texts, batch.dimensions, list(batch.widths), batch.seed)
            assert np.array_equal(live[0], hashes) and np.array_equal(live[1], counts), batch.name


# ---- the kernel's arithmetic, restated ------------------------------------------------------------------------------------


def _reduce(x, modulo, reciprocal, fix_up=np.greater_equal):
    """hip/fingerprints.hip `reduce`: every operand is an integer below 2^53, so `fma(-quotient, modulo, x)` is x - quotient x
    modulo exactly and plain `float64` arithmetic restates it."""
    quotient = np.floor(x * reciprocal)
    residue = x - quotient * modulo
    return residue if fix_up is None else np.where(fix_up(residue, modulo), residue - modulo, residue)


def _sweep():
    """-> (x, modulo, k) as float64 vectors: 256 dimensions of two seeds, every k from 0 to the largest quotient a dimension can
    meet WHATEVER its width (hash modulo - 1, two bytes of 0xFF, a complement of modulo - 1), x in {k modulo - 1, k modulo,
    k modulo + 1} within that bound."""
    xs, modulos, ks = [], [], []
    for seed in (1, 2):
        for _, multiplier, modulo in cases.parameters(256, (7,), seed):
            top = (modulo - 1) * multiplier + 256 + 256 * (modulo - 1)
            assert top < 1 << 52
            k = np.arange(0, top // modulo + 1, dtype=np.int64)
            for offset in (-1, 0, 1):
                x = k * modulo + offset
                keep = (x >= 0) & (x <= top)
                xs.append(x[keep]), modulos.append(np.full(int(keep.sum()), modulo, np.int64)), ks.append(k[keep])
    return np.concatenate(xs), np.concatenate(modulos), np.concatenate(ks)


def test_restated_kernel_arithmetic_lands_on_the_canonical_residue():
    """The update and the one-step Barrett of hip/fingerprints.hip in `float64`, the reciprocal formed exactly as
    host/fingerprint_engines.c forms it, on the values where a quotient can go wrong: next to every multiple of the modulo.

    Pinned counter-examples: with `>` in place of `>=` every x = k modulo (k >= 1) comes out as the modulo itself; with no
    fix-up at all, the same.  Both because the rounded-down reciprocal makes the quotient k - 1 there.

    Finding about the margin (measured, not chosen): the UNROUNDED reciprocal `1.0 / modulo` never overshoots in this sweep
    either - of its 1 061 785 values not one gets a quotient above x // modulo, up to k = 894; at x = k modulo - 1 the
    product's rounding error stays below the 1 / modulo ~ 2^-42 that separates it from k.  What it does not give is a
    quotient one can predict: on 353 505 of the 353 587 multiples it is k exactly, on the other 82 it is k - 1.  The scale
    by 1 - 2^-50 makes the quotient k - 1 on EVERY multiple (and on 213 742 of the x = k modulo + 1, where the residue
    modulo + 1 takes the same fix-up), so the equality of the `>=` is no rare path but the only one a multiple takes."""
    x, modulo, k = _sweep()
    assert len(x) == 1_061_785 and k.max() == 894
    xf, mf = x.astype(np.float64), modulo.astype(np.float64)
    assert np.array_equal(xf.astype(np.int64), x)
    reciprocal = (1.0 / mf) * (1.0 - 2.0**-50)
    canonical = x % modulo
    assert np.array_equal(_reduce(xf, mf, reciprocal).astype(np.int64), canonical)
    quotient = np.floor(xf * reciprocal).astype(np.int64)
    assert ((quotient == x // modulo) | (quotient == x // modulo - 1)).all()  # never overshoots, never more than one short
    multiples = (x % modulo == 0) & (k >= 1)
    assert (quotient[multiples] == k[multiples] - 1).all()  # the `>=` with equality: taken at EVERY multiple
    # the two counter-examples
    wrong = _reduce(xf, mf, reciprocal, np.greater).astype(np.int64) != canonical
    assert np.array_equal(wrong, multiples)
    wrong = _reduce(xf, mf, reciprocal, None).astype(np.int64) != canonical
    assert wrong[multiples].all() and int(wrong.sum()) == 567_329  # and wherever else the quotient is one short
    # the finding
    unrounded = np.floor(xf * (1.0 / mf)).astype(np.int64)
    overshoots = int((unrounded > x // modulo).sum())
    print("unrounded reciprocal: overshoots", overshoots, "of", len(x), "| exact at multiples:", int((unrounded[multiples] == k[multiples]).sum()), "of", int(multiples.sum()))
    assert overshoots == 0 and int((unrounded[multiples] == k[multiples]).sum()) == 353_505 and int(multiples.sum()) == 353_587


def test_restated_update_follows_the_integer_model_through_a_top_batch():
    """The fused update itself - fma(complement, old + 1, fma(hash, multiplier, new + 1)) - is exact below 2^53: restated in
    `float64` it walks a top batch's text, its step at the dimension's bound included, hash for hash with the integers."""
    batch = next(b for b in cases.batches() if b.name.startswith("top/128/1/"))
    dim = batch.planted[0]
    width, multiplier, modulo = cases.parameters(batch.dimensions, batch.widths, batch.seed)[dim]
    text = batch.texts[0]
    reciprocal = np.float64(1.0 / modulo) * np.float64(1.0 - 2.0**-50)
    complement = float(cases.complement_of(width, multiplier, modulo))
    value, exact, largest = np.float64(cases.window_hash(text[:width], multiplier, modulo)), cases.window_hash(text[:width], multiplier, modulo), 0
    for at in range(width, len(text)):
        x = value * multiplier + (text[at] + 1.0) + complement * (text[at - width] + 1.0)
        exact_x = exact * multiplier + text[at] + 1 + int(complement) * (text[at - width] + 1)
        assert int(x) == exact_x
        value, exact, largest = _reduce(x, np.float64(modulo), reciprocal), exact_x % modulo, max(largest, exact_x // modulo)
        assert int(value) == exact
    assert largest == batch.quotients[0]

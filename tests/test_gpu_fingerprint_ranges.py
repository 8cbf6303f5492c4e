"""`-m gpu`: the fingerprint kernels (hip/fingerprints.hip) at the ENDS of their hash arithmetic, on the hardware.

Every other test of these kernels feeds them random bytes, on which the hash is uniform below a modulo of ~2^42: the equality of
the one `residue >= modulo` after the rounded-down Barrett step (x an exact multiple of the modulo), an x next to the bound of
~896 modulo, and a minimum that repeats are then never met.  tests/fingerprint_range_cases.py PLANTS them - windows that hash to
0, to modulo - 1 between bytes of 0xFF, to a residue whose low 32 bits are 0xFFFFFFFF - in the first-window loop, the rolled
loop, the first window of a later segment, several times in one segment and across the merge, in dimensions of both
wavefronts, of the staged kernel and of the one that reads in place; and runs of one byte, whose count is known in every
dimension.  The windows come from tests/golden/fingerprint_ranges.json: no search runs here.

Three references, from the narrowest to the widest: the exact integer model on the planted dimensions, the C oracle on all
dimensions, the stored results of the reference's serial engines.  The aims are then asserted on the GPU's own numbers.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import stringzilla_amd as szs  # noqa: E402
from oracle import binding  # noqa: E402

import fingerprint_range_cases as cases  # noqa: E402

KINDS = ["zero", "top", "ones", "runs"]


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return szs.DeviceScope(gpu_device=0)


def of_kind(kind):
    return [batch for batch in cases.batches() if batch.name.startswith(kind)]


def engine_of(gpu, batch):
    return szs.Fingerprints(batch.dimensions, window_widths=list(batch.widths), seed=batch.seed, capabilities=gpu)


_computed = {}


def computed(gpu, batch):
    """(hashes, counts) of the batch on the GPU, once per batch."""
    if batch.name not in _computed:
        hashes, counts = engine_of(gpu, batch)(batch.texts, device=gpu)
        assert hashes.dtype == counts.dtype == np.uint32 and hashes.shape == counts.shape == (len(batch.texts), batch.dimensions)
        _computed[batch.name] = (hashes, counts)
    return _computed[batch.name]


@functools.lru_cache(maxsize=None)
def stored():
    return cases.stored_results()


def same(got, expected, batch, who):
    for name, ours, theirs in (("hashes", got[0], expected[0]), ("counts", got[1], expected[1])):
        wrong = np.argwhere(ours != theirs)
        assert wrong.size == 0, (who, batch.name, name, [(int(t), len(batch.texts[t]), int(d), int(ours[t, d]), int(theirs[t, d])) for t, d in wrong[:5]])


@pytest.mark.parametrize("kind", KINDS)
def test_planted_dimensions_equal_the_integer_model_and_reach_their_aims(gpu, kind):
    """Hash 0 with count = plants; 0xFFFFFFFF with count 1 next to 0xFFFFFFFF with count 0; every window after a step at the
    dimension's bound; runs with count n - width + 1 in every dimension: read off the GPU's own output."""
    for batch in of_kind(kind):
        hashes, counts = computed(gpu, batch)
        for index in range(len(batch.texts)):
            for dim in batch.planted:
                assert (int(hashes[index, dim]), int(counts[index, dim])) == batch.model(index, dim), (batch.name, index, len(batch.texts[index]), dim)
        for aim in batch.aims:
            assert (int(hashes[aim.text, aim.dim]), int(counts[aim.text, aim.dim])) == (aim.hash, aim.count), (batch.name, aim)
        if kind == "zero":
            assert all((aim.hash, aim.count) == (0, batch.texts[aim.text].count(batch.texts[0])) for aim in batch.aims)
        if kind == "ones":
            assert (int(hashes[0, batch.planted[0]]), int(counts[0, batch.planted[0]])) == (0xFFFFFFFF, 1)
            assert (int(hashes[1, batch.planted[0]]), int(counts[1, batch.planted[0]])) == (0xFFFFFFFF, 0)
        if kind == "runs":
            widths = np.array([p[0] for p in cases.parameters(batch.dimensions, batch.widths, batch.seed)], dtype=np.int64)
            for index, text in enumerate(batch.texts):
                if len(set(text)) == 1:
                    assert np.array_equal(counts[index], np.maximum(len(text) - widths + 1, 0)), (batch.name, len(text))


@pytest.mark.parametrize("kind", KINDS)
def test_all_dimensions_equal_the_oracle_and_the_stored_reference(gpu, kind):
    for batch in of_kind(kind):
        got = computed(gpu, batch)
        same(got, binding.oracle_fingerprints(batch.texts, batch.dimensions, list(batch.widths), batch.seed), batch, "oracle")
        same(got, stored()[batch.name], batch, "stored reference")


@pytest.mark.parametrize("kind", KINDS)
def test_wide_tapes_and_padded_out_buffers(gpu, kind):
    """The same batches through a tape of 64-bit offsets, and into NumPy `out=` buffers whose rows are 8 words longer than the
    fingerprint: the padding stays as it was."""
    for batch in of_kind(kind):
        engine, expected = engine_of(gpu, batch), stored()[batch.name]
        same(engine(szs.Strs(batch.texts, wide_offsets=True), device=gpu), expected, batch, "wide tape")
        padded = [np.full((len(batch.texts), batch.dimensions + 8), 0xEEEEEEEE, np.uint32) for _ in range(2)]
        out = (padded[0][:, :batch.dimensions], padded[1][:, :batch.dimensions])
        assert out[0].strides == (4 * (batch.dimensions + 8), 4)
        engine(batch.texts, device=gpu, out=out)
        same(out, expected, batch, "padded out=")
        assert all((matrix[:, batch.dimensions:] == 0xEEEEEEEE).all() for matrix in padded), batch.name


def test_texts_sharing_a_planted_window_match_in_its_dimension(gpu):
    """End to end: texts that share a window hashing to 0 have hash 0 there whatever else they hold, so `Fingerprints.matches`
    counts that dimension for every pair of them - and counts what a comparison of the rows counts."""
    for batch in of_kind("zero")[:3]:
        hashes, _ = computed(gpu, batch)
        dim = batch.planted[0]
        assert (hashes[:, dim] == 0).all()
        matrix = engine_of(gpu, batch).matches(hashes, device=gpu)
        assert np.array_equal(matrix, (hashes[:, None, :] == hashes[None, :, :]).sum(axis=2))
        without = hashes.copy()
        without[::2, dim] = 1  # every other text loses the shared minimum: exactly the mixed pairs lose one match
        lost = matrix.astype(np.int64) - engine_of(gpu, batch).matches(without, device=gpu)
        rows = np.arange(len(batch.texts)) % 2
        assert np.array_equal(lost, (rows[:, None] != rows[None, :]).astype(np.int64)) and matrix.min() >= 1

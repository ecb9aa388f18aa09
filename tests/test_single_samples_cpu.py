"""CPU tier of MCSamples.makeSingleSamples / WeightedSamples.random_single_samples_indices: the host logic (argument
handling, default thinning from max_scatter_points, the two threshold modes, the file layout, what happens to the caller's
generator, the route of a generator that is not PCG64) runs over a numpy double of Context.draw_single_rows / gather_rows
and is held to the reference's rows, arrays and file texts in tests/golden/single_samples.npz."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import single_cases  # noqa: E402
from fake_ctx import FakeBuf, FakeContext  # noqa: E402


class DrawContext(FakeContext):
    """FakeContext + numpy statements of gd_draw_single_rows / gd_gather_rows.  The PCG64 route rebuilds numpy's own
    generator from the (state, inc) it is handed, so it shares no code with csrc/pcg64.hpp."""

    calls = []

    def draw_single_rows(self, a, b, mode=0, pcg=None, rand=None, capacity=None):
        assert (pcg is None) != (rand is None)
        if pcg is not None:
            bg = np.random.PCG64()
            st = bg.state
            st["state"] = dict(state=int(pcg[0]), inc=int(pcg[1]))
            st["has_uint32"], st["uinteger"] = 0, 0
            bg.state = st
            rand = np.random.Generator(bg).random(self.N)
        w = np.ones(self.N) if self.w is None else self.w
        a, b = np.float64(a), np.float64(b)
        keep = np.nonzero(rand <= ((w / a) / b if mode else w / (a * b)))[0]
        type(self).calls.append(dict(route="pcg" if pcg is not None else "rand", mode=mode, a=float(a), b=float(b),
                                     capacity=capacity, K=len(keep)))
        if capacity is not None and len(keep) > capacity:
            return None, len(keep)
        return FakeBuf(keep.astype(np.int32)), len(keep)

    def gather_rows(self, rows, K, cols):
        return self.s[np.asarray(rows.a[:K], dtype=np.int64)][:, list(cols)]


@pytest.fixture(scope="module")
def gold():
    return single_cases.load_golden()


@pytest.fixture(scope="module")
def samples():
    from getdist_amd.mcsamples import MCSamples

    return {fx: single_cases.build(MCSamples, fx, _context_factory=DrawContext) for fx in single_cases.CALLS_FOR}


def test_entries_exported_and_bound():
    from getdist_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_native()
    lib = _lib.load_library()
    for name in ("gd_draw_single_rows", "gd_gather_rows"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert hasattr(_lib.Context, "draw_single_rows") and hasattr(_lib.Context, "gather_rows")


def test_golden_covers_the_cases(gold):
    assert sorted(gold.files) == sorted("%s/%s" % c for c in single_cases.all_cases())
    assert os.path.getsize(single_cases.GOLDEN) < 512 * 1024


@pytest.mark.parametrize("fx,call", list(single_cases.all_cases()))
def test_matches_reference(samples, gold, tmp_path, fx, call):
    """unweighted, integer-weight and real-weight sets; defaults, thin=, max_samples=, single_thin=, the file branch"""
    want = gold["%s/%s" % (fx, call)]
    got = single_cases.run(samples[fx], call, tmp_path)
    if want.dtype.kind == "U":
        assert isinstance(got, str) and got == str(want)  # byte-equal text: %16.7E of weight 1, loglike, parameters
    else:
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got, want)


def test_default_thin_comes_from_max_scatter_points(samples):
    mc = samples["int"]
    assert mc.max_scatter_points == 450
    DrawContext.calls.clear()
    mc.makeSingleSamples(random_state=1)
    c = DrawContext.calls[-1]
    assert c["mode"] == 0 and c["a"] == mc.max_mult
    assert c["b"] == max(1, mc.norm / mc.max_mult / 450) and c["b"] > 1
    mc.random_single_samples_indices(random_state=1, max_samples=100)
    assert DrawContext.calls[-1]["b"] == mc.norm / mc.max_mult / 100
    mc.random_single_samples_indices(random_state=1)
    assert DrawContext.calls[-1]["b"] == 1
    mc.random_single_samples_indices(random_state=1, max_samples=10**9)
    assert DrawContext.calls[-1]["b"] == 1  # max(1, ...)


def test_file_branch_uses_the_other_division_order(samples, tmp_path):
    DrawContext.calls.clear()
    samples["real"].makeSingleSamples(filename=str(tmp_path / "a.txt"), random_state=2)
    assert DrawContext.calls[-1]["mode"] == 1
    samples["real"].makeSingleSamples(random_state=2)
    assert DrawContext.calls[-1]["mode"] == 0


def test_thin_and_max_samples_together_raise(samples):
    from getdist_amd.chains import WeightedSampleError

    with pytest.raises(WeightedSampleError, match="Cannot set thin and max_samples"):
        samples["int"].random_single_samples_indices(thin=2, max_samples=100)


def test_indices_are_int64_and_ascending(samples):
    ix = samples["real"].random_single_samples_indices(random_state=11)
    assert ix.dtype == np.int64 and np.all(np.diff(ix) > 0)


def _pending_uint32(seed):
    g = np.random.default_rng(seed)
    g.integers(0, 2**32, dtype=np.uint32, endpoint=False)
    assert g.bit_generator.state["has_uint32"] == 1
    return g


@pytest.mark.parametrize("make", [lambda: np.random.default_rng(21), lambda: _pending_uint32(22)],
                         ids=["fresh", "pending_uint32"])
def test_pcg64_generator_is_left_where_the_reference_leaves_it(samples, make, tmp_path):
    mc = samples["int"]
    for call in (lambda g: mc.random_single_samples_indices(random_state=g, thin=2),
                 lambda g: mc.makeSingleSamples(random_state=g),
                 lambda g: mc.makeSingleSamples(filename=str(tmp_path / "g.txt"), random_state=g)):
        mine, twin = make(), make()
        DrawContext.calls.clear()
        call(mine)
        assert DrawContext.calls[-1]["route"] == "pcg"
        twin.random(mc.numrows)
        assert mine.bit_generator.state == twin.bit_generator.state
        assert mine.random() == twin.random()
        assert mine.integers(0, 2**32, dtype=np.uint32) == twin.integers(0, 2**32, dtype=np.uint32)


def test_bit_generator_argument_is_advanced_too(samples):
    mc = samples["unit"]
    bg, twin = np.random.PCG64(5), np.random.PCG64(5)
    ix = mc.random_single_samples_indices(random_state=bg, thin=2)
    rand = np.random.Generator(twin).random(mc.numrows)
    assert np.array_equal(ix, np.nonzero(rand <= np.ones(mc.numrows) / (1.0 * 2))[0])
    assert bg.state == twin.state


@pytest.mark.parametrize("bitgen", [np.random.Philox, np.random.MT19937, np.random.PCG64DXSM, np.random.SFC64])
def test_other_generators_take_the_vector_route(samples, bitgen):
    mc = samples["real"]
    mine, twin = np.random.Generator(bitgen(31)), np.random.Generator(bitgen(31))
    DrawContext.calls.clear()
    ix = mc.random_single_samples_indices(random_state=mine, thin=1.5)
    assert [c["route"] for c in DrawContext.calls] == ["rand"]
    rand = twin.random(mc.numrows)
    assert np.array_equal(ix, np.nonzero(rand <= mc.weights / (np.max(mc.weights) * 1.5))[0])
    assert mine.bit_generator.state["state"].keys() == twin.bit_generator.state["state"].keys()
    assert mine.random() == twin.random()


def test_short_buffer_is_answered_by_one_exact_retry(samples):
    """The first buffer is sized from the expected count; a draw that keeps more is repeated with exactly its count."""
    mc = samples["unit"]
    norm = mc.norm
    DrawContext.calls.clear()
    try:
        mc.norm = np.float64(10.0)  # makes the estimate far too small
        ix = mc.random_single_samples_indices(random_state=3, thin=1.25)
    finally:
        mc.norm = norm
    first, second = DrawContext.calls
    assert first["capacity"] < first["K"] and second["capacity"] == first["K"] == second["K"] == len(ix)
    assert np.array_equal(ix, mc.random_single_samples_indices(random_state=3, thin=1.25))

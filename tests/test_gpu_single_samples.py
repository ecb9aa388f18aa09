"""GPU tier of the weight-one draws: gd_draw_single_rows / gd_gather_rows against numpy alone --
np.nonzero(default_rng(seed).random(N) <= w / (max(w) * thin))[0], compared with array_equal: the draw is the reference's,
bit for bit -- and MCSamples.makeSingleSamples / random_single_samples_indices end to end against the golden rows."""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import single_cases  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 2048         # rows per block of the draw kernels (csrc/draw.hip: DRAW_TILE)
SCAN_PASS = 1024    # tile counts per pass of the one-block scan
ROW_COUNTS = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 7]
MANY_TILES = TILE * SCAN_PASS + TILE + 5  # 1026 tiles: the scan takes a second pass and carries the first one's total


def _weights(kind, N, seed=0):
    r = np.random.default_rng([77, seed, N])
    if kind == "none":
        return None
    if kind == "int":
        return r.integers(1, 9, N).astype(float)
    if kind == "real":
        return np.exp(r.standard_normal(N)) * r.uniform(0.1, 2.0, N)
    if kind == "zeros":
        w = r.integers(1, 5, N).astype(float)
        w[r.random(N) < 0.4] = 0.0
        w[0] = 3.0  # (not all zero at N = 1)
        return w
    if kind == "max_last":
        w = r.uniform(0.5, 1.0, N)
        w[-1] = 7.25
        return w
    raise KeyError(kind)


@pytest.fixture(scope="module")
def ctx():
    from getdist_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


def _upload(ctx, N, w):
    ctx.upload(np.zeros((N, 1)), w)
    return np.ones(N) if w is None else w


def _expected(seed, w, thin):
    return np.nonzero(np.random.default_rng(seed).random(len(w)) <= w / (np.max(w) * thin))[0]


def _pcg(seed):
    s = np.random.default_rng(seed).bit_generator.state["state"]
    return s["state"], s["inc"]


def _rows(buf, K):
    out = buf.to_host((K,), dtype=np.int32).astype(np.int64) if K else np.zeros(0, dtype=np.int64)
    buf.free()
    return out


def _check_draw(ctx, N, kind, thin, seed):
    w = _upload(ctx, N, _weights(kind, N, seed))
    want = _expected(seed, w, thin)
    buf, K = ctx.draw_single_rows(np.max(w), thin, 0, pcg=_pcg(seed))
    got = _rows(buf, K)
    assert K == len(want) and np.array_equal(got, want)
    # the vector route over the same variates gives the same list
    buf, K = ctx.draw_single_rows(np.max(w), thin, 0, rand=np.random.default_rng(seed).random(N))
    assert np.array_equal(_rows(buf, K), want)
    return want


@pytest.mark.parametrize("N", ROW_COUNTS)
@pytest.mark.parametrize("kind", ["none", "real"])
def test_row_counts(ctx, N, kind):
    _check_draw(ctx, N, kind, 1.0 if kind == "none" else 1.7, seed=N)


@pytest.mark.parametrize("kind", ["none", "int", "real", "zeros", "max_last"])
@pytest.mark.parametrize("thin", [1, 3.5, 1e300])
def test_weights_and_thin(ctx, kind, thin):
    want = _check_draw(ctx, 3 * TILE + 7, kind, thin, seed=5)
    if thin == 1e300:
        assert len(want) == 0  # K = 0: nothing kept, nothing written
    elif kind == "none" and thin == 1:
        assert len(want) == 3 * TILE + 7
    else:
        assert 0 < len(want) < 3 * TILE + 7


def test_more_tiles_than_one_scan_pass(ctx):
    want = _check_draw(ctx, MANY_TILES, "real", 3.5, seed=12345)
    assert want[-1] >= TILE * SCAN_PASS  # rows of the tiles behind the first scan pass are there


def test_threshold_modes_round_differently(ctx):
    """w / (a * b) and (w / a) / b differ in the last bit on some rows; with rand set to the larger of the two there, each
    mode keeps exactly the rows of its own expression."""
    N = 3 * TILE + 7
    w = _upload(ctx, N, _weights("real", N, 9))
    a, b = np.float64(np.max(w)), np.float64(3.7)
    t0, t1 = w / (a * b), (w / a) / b
    differ = np.nonzero(t0 != t1)[0]
    assert differ.size > 20
    rand = np.random.default_rng(1).random(N)
    rand[differ] = np.maximum(t0, t1)[differ]
    want0, want1 = np.nonzero(rand <= t0)[0], np.nonzero(rand <= t1)[0]
    assert np.setdiff1d(want0, want1).size > 0 and np.setdiff1d(want1, want0).size > 0
    for mode, want in ((0, want0), (1, want1)):
        buf, K = ctx.draw_single_rows(a, b, mode, rand=rand)
        assert np.array_equal(_rows(buf, K), want), mode


def test_capacity_is_never_exceeded(ctx):
    from getdist_amd import _lib

    N = 3 * TILE + 7
    w = _upload(ctx, N, _weights("int", N, 3))
    want = _expected(8, w, 2.0)
    K = len(want)
    state, inc = _pcg(8)
    m64 = (1 << 64) - 1
    st = (ctypes.c_uint64 * 4)(state >> 64, state & m64, inc >> 64, inc & m64)
    guard = np.int32(-1234567)
    buf = ctx.alloc((K + 1) * 4)
    n = ctypes.c_int64()

    def call(capacity):
        buf.from_host(np.full(K + 1, guard, dtype=np.int32))
        rc = ctx.lib.gd_draw_single_rows(ctx.h, st, None, float(np.max(w)), 2.0, 0, buf.ptr, capacity, ctypes.byref(n))
        return rc, buf.to_host((K + 1,), dtype=np.int32)

    rc, held = call(K - 1)  # one short: the count and its status come back, not a single word is written
    assert rc == _lib.GD_DRAW_MORE_ROWS and n.value == K
    assert np.all(held == guard)
    rc, held = call(K)  # exact fit: the word behind the buffer is untouched
    assert rc == 0 and n.value == K
    assert np.array_equal(held[:K], want) and held[K] == guard
    buf.free()
    # the wrapper reports the short buffer as (None, K)
    assert ctx.draw_single_rows(np.max(w), 2.0, 0, pcg=(state, inc), capacity=K - 1) == (None, K)


@pytest.fixture(scope="module")
def table(ctx):
    """A resident (250 000, 5) sample set of its own context, and the host copy."""
    from getdist_amd._lib import Context

    c = Context(0)
    s = np.random.default_rng(2).standard_normal((250_000, 5))
    c.upload(s, None)
    yield c, s
    c.close()


@pytest.mark.parametrize("K", [0, 1, 65, 200_000])  # 200 000 x 3 entries: more than one sweep of the capped grid
@pytest.mark.parametrize("cols", [[0, 2], [4, 1, 3, 0, 2], [1, 1, 3]], ids=["subset", "permuted", "repeat"])
def test_gather_rows(table, K, cols):
    c, s = table
    ix = np.random.default_rng(K).integers(0, len(s), K).astype(np.int32)  # any order, repeats allowed
    d_ix = c.alloc(max(K, 1) * 4)
    if K:
        d_ix.from_host(ix)
    got = c.gather_rows(d_ix, K, cols)
    d_ix.free()
    assert got.shape == (K, len(cols)) and np.array_equal(got, s[ix][:, cols])


@pytest.fixture(scope="module")
def big():
    from getdist_amd.mcsamples import MCSamples

    return single_cases.build(MCSamples, "big_int"), single_cases.fixtures()["big_int"]


def test_end_to_end_make_single_samples(big):
    mc, f = big
    s, w = f["samples"], f["weights"]
    got = mc.makeSingleSamples(random_state=6)
    thin = max(1, np.sum(w) / np.max(w) / 2000)
    live = s[np.random.default_rng(6).random(len(w)) <= w / (np.max(w) * thin)]
    assert np.array_equal(got, live)
    assert np.array_equal(got, single_cases.load_golden()["big_int/arr_default"])


def test_end_to_end_indices(big):
    mc, f = big
    w = f["weights"]
    gold = single_cases.load_golden()
    got = mc.random_single_samples_indices(max_samples=500, random_state=5)
    assert got.dtype == np.int64
    assert np.array_equal(got, _expected(5, w, max(1, np.sum(w) / np.max(w) / 500)))
    assert np.array_equal(got, gold["big_int/ix_max"])
    # a generator that is not PCG64 draws on the host; the kernels read the uploaded vector
    got = single_cases.run(mc, "ix_philox", None)
    assert np.array_equal(got, gold["big_int/ix_philox"])
    # a caller's PCG64 generator ends where random(numrows) leaves it
    mine, twin = np.random.default_rng(44), np.random.default_rng(44)
    mc.random_single_samples_indices(random_state=mine, thin=2)
    twin.random(mc.numrows)
    assert mine.bit_generator.state == twin.bit_generator.state


def test_end_to_end_file_branch(tmp_path):
    from getdist_amd.mcsamples import MCSamples

    mc = single_cases.build(MCSamples, "int")
    gold = single_cases.load_golden()
    for call in ("file_default", "file_thin"):
        assert single_cases.run(mc, call, tmp_path) == str(gold["int/" + call])

"""GPU tier of the chain export: gd_format_matrix / gd_format_rows against Python's ``%`` operator byte for byte (random bit
patterns with NaN / inf / subnormals, constructed exact ties, tile and scan boundaries, strides, row lists, both row
selectors, the capacity contract), the reference's files of tests/golden/export.npz through the real context, the
streaming writer against np.savetxt, and a save / load round trip of a set mutated on the device."""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import export_cases  # noqa: E402

pytestmark = pytest.mark.gpu

FORMATS = [(0, 8, False), (16, 7, True), (0, 17, False)]  # "%.8e" (saveAsText), "%16.7E" (makeSingleSamples), the widest digits
FORMAT_IDS = ["%.8e", "%16.7E", "%.17e"]
SCAN_PASS = 1024  # tile counts per pass of the one-block scan (csrc/export.hip: k_tile_scan (tilescan.hpp))
# rows x fields.  A tile is 64 rows while it fits 64 KB of LDS (csrc/export.hip: 64 rows up to 5 fields, 32 or 16 rows for
# 52 fields depending on the format): 63 / 64 / 65, 31 / 32 / 33 and 15 / 16 / 17 straddle every tile size in use, 4097 rows
# are many tiles, and 64 * 2048 + 5 rows of 2 fields are 2049 tiles: three passes of the scan.
SHAPES = [(1, 1), (1, 3), (63, 3), (64, 52), (65, 52), (4097, 5), (15, 52), (16, 52), (17, 52), (31, 52), (32, 52), (33, 52),
          (64 * 2 * SCAN_PASS + 5, 2)]


def spec_string(width, prec, upper):
    return "%%%s.%d%s" % (width if width else "", prec, "E" if upper else "e")


def python_text(table, width, prec, upper, sep):
    spec = spec_string(width, prec, upper)
    row = (" " if sep else "").join([spec] * table.shape[1]) + "\n"
    return "".join([row % tuple(r) for r in table.tolist()]).encode()


def ties(rng, count):
    """exact ties at 8 and 9 significant digits: (10 d + 5) 10^j (scaled by a negative power of ten: the exact path) and
    d + 1/2"""
    out = []
    for prec in (7, 8):
        d = rng.integers(10 ** prec, 10 ** (prec + 1), size=count)
        for j in range(0, 6):
            v = (10 * d + 5) * 10 ** j
            out.append(v[v < 2 ** 53].astype(np.float64))
        out.append(d + 0.5)
    out.append(np.array([1234567.125, 1234567125000.0, 9.999999995e99, 1e100, 9.999999995e-101, 1e-100, 5e-324, 0.0, -0.0,
                         np.inf, -np.inf, np.nan, -np.nan, 2.2250738585072014e-308, 1.7976931348623157e308]))
    return np.concatenate(out)


def content(K, m, seed):
    """(K, m) doubles: random bit patterns (NaN, inf and subnormals stay in), every fourth value a directed case"""
    rng = np.random.default_rng([99, seed, K, m])
    x = rng.integers(0, 2 ** 64, size=K * m, dtype=np.uint64, endpoint=False).view(np.float64).copy()
    t = ties(rng, 50)
    pick = rng.integers(0, len(t), size=len(x[::4]))
    x[::4] = t[pick] * rng.choice([1.0, -1.0], size=len(pick))
    return x.reshape(K, m)


@pytest.fixture(scope="module")
def ctx():
    from getdist_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


def _text(buf, n):
    out = buf.to_host((n,), dtype=np.uint8).tobytes() if n else b""
    buf.free()
    return out


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_format_matrix(ctx, shape, fmt):
    x = content(*shape, seed=1)
    for sep in (True, False):
        buf, n = ctx.format_matrix(x, *fmt, sep=sep)
        assert _text(buf, n) == python_text(x, *fmt, sep)


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_format_matrix_strides(ctx, fmt):
    x = content(70, 9, seed=2)
    d = ctx.alloc(x.nbytes)
    d.from_host(x)
    # the transpose: a column-major view of the same memory
    buf, n = ctx.format_matrix(d, *fmt, shape=(9, 70), strides=(1, 9))
    assert _text(buf, n) == python_text(x.T, *fmt, True)
    # a sub-matrix: rows 3..67 step 2, columns 1..8 step 3
    sub = x[3:68:2, 1:9:3]
    dsub = type("View", (), {"ptr": d.ptr + 8 * (3 * 9 + 1), "nbytes": 0})()
    buf, n = ctx.format_matrix(dsub, *fmt, shape=sub.shape, strides=(18, 3))
    assert _text(buf, n) == python_text(sub, *fmt, True)
    d.free()


N_ROWS = 4097 + 64
W, Z, ONE = -1, -2, -3


@pytest.fixture(scope="module")
def resident():
    """A resident set of its own context: 5 columns of mixed content, real weights, a loglike vector in a spare column"""
    from getdist_amd._lib import Context

    c = Context(0)
    s = content(N_ROWS, 5, seed=3)
    rng = np.random.default_rng(4)
    w = np.exp(rng.standard_normal(N_ROWS)) * rng.uniform(0.1, 2.0, N_ROWS)
    ll = rng.uniform(0, 50, N_ROWS) * 10.0 ** rng.integers(-3, 4, N_ROWS)
    c.upload(s, w)
    llcol = c.set_extra_column(c.EXTRA_COLS - 1, ll)
    srcs = [W, llcol, 0, 1, 2, 3, 4, Z, ONE, 2]
    table = np.column_stack([w, ll, s, np.zeros(N_ROWS), np.ones(N_ROWS), s[:, 2]])
    yield c, srcs, table
    c.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("lo,hi", [(0, 1), (0, 63), (0, 64), (0, 65), (0, N_ROWS), (5, 70), (33, 4000), (N_ROWS - 1, N_ROWS)])
def test_format_rows_ranges(resident, lo, hi, fmt):
    c, srcs, table = resident
    for sep in (True, False):
        buf, n = c.format_rows(srcs, lo=lo, hi=hi, width=fmt[0], prec=fmt[1], upper=fmt[2], sep=sep)
        assert _text(buf, n) == python_text(table[lo:hi], *fmt, sep)


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_format_rows_list(resident, fmt):
    """an unsorted device row list with repeats; a row number outside the set gives nan in every field"""
    c, srcs, table = resident
    rng = np.random.default_rng(6)
    ix = rng.integers(0, N_ROWS, 300).astype(np.int32)
    ix[10], ix[11], ix[200] = ix[9], N_ROWS + 5, -1
    d = c.alloc(ix.nbytes)
    d.from_host(ix)
    want = table[np.clip(ix, 0, N_ROWS - 1)].copy()
    want[(ix < 0) | (ix >= N_ROWS)] = np.nan
    for sep in (True, False):
        buf, n = c.format_rows(srcs, rows=d, K=len(ix), width=fmt[0], prec=fmt[1], upper=fmt[2], sep=sep)
        assert _text(buf, n) == python_text(want, *fmt, sep)
    buf, n = c.format_rows(srcs, rows=d, K=100, row_offset=150, width=fmt[0], prec=fmt[1], upper=fmt[2])
    assert _text(buf, n) == python_text(want[150:250], *fmt, True)
    d.free()


def test_unweighted_set_writes_unit_weights(ctx):
    s = np.random.default_rng(8).standard_normal((70, 2))
    ctx.upload(s, None)
    buf, n = ctx.format_rows([W, Z, 0, 1], lo=0, hi=70)
    assert _text(buf, n) == python_text(np.column_stack([np.ones(70), np.zeros(70), s]), 0, 8, False, True)


def test_capacity_and_bad_arguments(resident):
    from getdist_amd import _lib

    c, srcs, table = resident
    lo, hi = 7, 207
    want = python_text(table[lo:hi], 0, 8, False, True)
    need = len(want)
    arr = np.asarray(srcs, dtype=np.int32)
    psrc = arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    guard = 0xA5
    buf = c.alloc(need + 64)
    n = ctypes.c_int64()

    def call(capacity, srcs_p=psrc, m=len(srcs), lo=lo, hi=hi, rows=None, K=0, width=0, prec=8):
        buf.from_host(np.full(need + 64, guard, dtype=np.uint8))
        rc = c.lib.gd_format_rows(c.h, srcs_p, m, lo, hi, rows, K, width, prec, 0, 1, buf.ptr, capacity, ctypes.byref(n))
        return rc, buf.to_host((need + 64,), dtype=np.uint8)

    rc, held = call(need - 1)  # one byte short: the size and its status come back, not a byte is written
    assert rc == _lib.GD_FORMAT_MORE_BYTES and n.value == need
    assert np.all(held == guard)
    rc, held = call(need)  # exact fit: the bytes behind the text are untouched
    assert rc == 0 and n.value == need
    assert held[:need].tobytes() == want and np.all(held[need:] == guard)
    # the wrapper reports the short buffer as (None, bytes needed)
    small = c.alloc(need - 1)
    assert c.format_rows(srcs, lo=lo, hi=hi, out=small) == (None, need)
    small.free()

    bad = _lib.GD_ERR_BADARG
    for col in (c.n + c.EXTRA_COLS, -4):
        a2 = np.array([0, col], dtype=np.int32)
        assert call(need, a2.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 2)[0] == bad
    assert call(need, lo=5, hi=5)[0] == bad                      # empty interval (and: neither selector)
    assert call(need, lo=0, hi=0)[0] == bad
    assert call(need, lo=-1, hi=5)[0] == bad
    assert call(need, lo=0, hi=N_ROWS + 1)[0] == bad             # out of range
    rows = c.alloc(16)
    rows.from_host(np.arange(4, dtype=np.int32))
    assert call(need, lo=0, hi=4, rows=rows.ptr, K=4)[0] == bad  # both selectors
    assert call(need, lo=0, hi=0, rows=rows.ptr, K=4)[0] == 0
    rows.free()
    for width, prec in ((0, 18), (0, -1), (33, 8), (-1, 8)):
        assert call(need, width=width, prec=prec)[0] == bad
    assert call(need, m=0)[0] == bad
    assert np.all(call(need, lo=5, hi=5)[1] == guard)            # refused before any launch: nothing written
    buf.free()
    # matrix entry: same contract
    x = np.ascontiguousarray(table[:50, :4])
    d = c.alloc(x.nbytes)
    d.from_host(x)
    want = python_text(x, 16, 7, True, False)
    out = c.alloc(len(want) + 16)
    out.from_host(np.full(len(want) + 16, guard, dtype=np.uint8))
    rc = c.lib.gd_format_matrix(c.h, d.ptr, 50, 4, 4, 1, 16, 7, 1, 0, out.ptr, len(want) - 1, ctypes.byref(n))
    assert rc == _lib.GD_FORMAT_MORE_BYTES and n.value == len(want) and np.all(out.to_host((len(want) + 16,), dtype=np.uint8) == guard)
    rc = c.lib.gd_format_matrix(c.h, d.ptr, 50, 4, 4, 1, 16, 7, 1, 0, out.ptr, len(want), ctypes.byref(n))
    held = out.to_host((len(want) + 16,), dtype=np.uint8)
    assert rc == 0 and held[:len(want)].tobytes() == want and np.all(held[len(want):] == guard)
    assert c.lib.gd_format_matrix(c.h, d.ptr, 50, 0, 4, 1, 16, 7, 1, 0, out.ptr, len(want), ctypes.byref(n)) == bad
    assert c.lib.gd_format_matrix(c.h, d.ptr, 50, 4, 4, 1, 16, 18, 1, 0, out.ptr, len(want), ctypes.byref(n)) == bad
    d.free()
    out.free()


def test_no_samples_is_a_bad_argument():
    from getdist_amd import _lib

    c = _lib.Context(0)
    n = ctypes.c_int64()
    src = (ctypes.c_int32 * 1)(0)
    buf = c.alloc(64)
    assert c.lib.gd_format_rows(c.h, src, 1, 0, 1, None, 0, 0, 8, 0, 1, buf.ptr, 64, ctypes.byref(n)) == _lib.GD_ERR_BADARG
    buf.free()
    c.close()


@pytest.fixture(scope="module")
def gold():
    return export_cases.load_golden()


@pytest.mark.parametrize("fx,call", list(export_cases.all_cases()))
def test_golden_files(gold, tmp_path, fx, call):
    from getdist_amd.mcsamples import MCSamples

    want = gold[(fx, call)]
    got = export_cases.run(export_cases.build(MCSamples, fx), call, tmp_path)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], "%s/%s: %s differs from the reference's file" % (fx, call, name)


@pytest.fixture(scope="module")
def stream_case(tmp_path_factory):
    from getdist_amd._lib import Context

    s = np.random.default_rng(12).standard_normal((100_003, 6)) * [1.0, 1e-3, 1e3, 1.0, 1e120, 1e-120]
    path = str(tmp_path_factory.mktemp("stream") / "want.txt")
    np.savetxt(path, s, fmt="%.8e")
    c = Context(0)
    c.upload(s, None)
    yield c, open(path, "rb").read()
    c.close()


@pytest.mark.parametrize("chunk_rows", [None, 1000, 7])  # 7 is less than a tile: more than 14 000 chunks
def test_streaming_writer_equals_savetxt(stream_case, tmp_path, chunk_rows):
    from getdist_amd import chainfiles

    c, want = stream_case
    path = str(tmp_path / "got.txt")
    chainfiles.write_text_rows(path, c, list(range(6)), (0, 100_003), chunk_rows=chunk_rows)
    assert open(path, "rb").read() == want
    assert os.listdir(str(tmp_path)) == ["got.txt"]


def _rounded(a):
    a = np.asarray(a, dtype=np.float64)
    return np.array([float("%.8e" % v) for v in a.reshape(-1).tolist()]).reshape(a.shape)


def _check_round_trip(mc, root):
    from getdist_amd.chainfiles import loadMCSamples

    mc.saveChainsAsText(root)
    back = loadMCSamples(root, no_cache=True)
    assert np.array_equal(back.samples, _rounded(mc.samples))
    assert np.array_equal(back.weights, _rounded(mc.weights if mc.weights is not None else np.ones(mc.numrows)))
    assert np.array_equal(back.loglikes, _rounded(mc.loglikes))
    assert np.array_equal(back.chain_offsets, mc.chain_offsets)
    assert back.paramNames.list() == mc.paramNames.list()
    assert back.paramNames.labels() == mc.paramNames.labels()
    assert [p.isDerived for p in back.paramNames.names] == [p.isDerived for p in mc.paramNames.names]
    assert [p.comment for p in back.paramNames.names] == [p.comment for p in mc.paramNames.names]
    for name in mc.paramNames.list():
        assert back.ranges.getLower(name) == mc.ranges.getLower(name) and back.ranges.getUpper(name) == mc.ranges.getUpper(name)
    back.ctx.close()


def test_round_trip_of_the_resident_set(tmp_path):
    from getdist_amd.mcsamples import MCSamples

    mc = export_cases.build(MCSamples, "chains3")
    os.makedirs(str(tmp_path / "a"))
    _check_round_trip(mc, str(tmp_path / "a" / "chain"))
    # what is saved is the resident, mutated set
    before = mc.samples.shape
    mc.thin(3)
    mc.filter(mc.samples[:, 0] > 0.2)
    assert mc.weights is None and 0 < mc.numrows and mc.samples.shape != before
    os.makedirs(str(tmp_path / "b"))
    _check_round_trip(mc, str(tmp_path / "b" / "chain"))

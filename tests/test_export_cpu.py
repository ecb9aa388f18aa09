"""CPU tier of the chain export (saveAsText, saveChainsAsText, saveTextMetadata, writeCovMatrix, writeCorrelationMatrix,
chainfiles.write_text_rows): the product's Python layer runs over a context double whose format_rows / format_matrix call
the g++ build of csrc/fmtdouble.hpp -- the formatter the device kernels run -- and every file is held byte for byte to what
the reference wrote (tests/golden/export.npz)."""

import logging
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "native"))
import export_cases  # noqa: E402
from fake_ctx import FakeBuf, FakeContext  # noqa: E402

SRC_WEIGHT, SRC_ZERO, SRC_ONE = -1, -2, -3


class HarnessContext(FakeContext):
    """FakeContext + gd_format_rows / gd_format_matrix stated with numpy for the table and the host build of the formatter
    for the text."""

    calls = []

    def _text(self, table, width, prec, upper, sep):
        import build_fmt

        table = np.ascontiguousarray(table, dtype=np.float64)
        flat, _ = build_fmt.format_array(table.reshape(-1).view(np.uint64), width, prec, upper, tail=10)
        fields = flat.split(b"\n")[:-1]
        m = table.shape[1]
        return b"".join((b" " if sep else b"").join(fields[i:i + m]) + b"\n" for i in range(0, len(fields), m))

    def _deliver(self, text, out, host):
        if out is not None and len(text) > out.nbytes:
            return None, len(text)
        buf = out if out is not None else FakeBuf(None, len(text))
        buf.a = np.frombuffer(text, dtype=np.uint8)
        if host is not None:
            host[:len(text)] = buf.a
        return buf, len(text)

    def format_rows(self, srcs, lo=None, hi=None, rows=None, K=None, row_offset=0, width=0, prec=8, upper=False, sep=True,
                    out=None, host=None):
        assert (rows is None) != (lo is None)
        index = np.arange(lo, hi) if rows is None else np.asarray(rows.a[row_offset:row_offset + K], dtype=np.int64)
        type(self).calls.append(dict(rows=len(index), width=width, prec=prec, upper=upper, sep=sep))
        w = np.ones(self.N) if self.w is None else self.w
        cols = [self.s[index, s] if s >= 0 else w[index] if s == SRC_WEIGHT else np.full(len(index), float(s == SRC_ONE))
                for s in srcs]
        return self._deliver(self._text(np.column_stack(cols), width, prec, upper, sep), out, host)

    def format_matrix(self, x, width=0, prec=8, upper=False, sep=True, out=None, host=None, shape=None, strides=None):
        return self._deliver(self._text(np.atleast_2d(x), width, prec, upper, sep), out, host)

    def fetch_bytes_async(self, buf, host, nbytes):
        host[:nbytes] = buf.a[:nbytes]


@pytest.fixture(scope="module")
def gold():
    return export_cases.load_golden()


def build(fx):
    from getdist_amd.mcsamples import MCSamples

    return export_cases.build(MCSamples, fx, _context_factory=HarnessContext)


def test_constants_match_the_header():
    from getdist_amd import _lib

    text = open(os.path.join(os.path.dirname(HERE), "include", "gdhip.h")).read()
    for name, value in (("GD_FMT_SRC_WEIGHT", SRC_WEIGHT), ("GD_FMT_SRC_ZERO", SRC_ZERO), ("GD_FMT_SRC_ONE", SRC_ONE),
                        ("GD_FORMAT_MORE_BYTES", -22)):
        assert "#define %s (%d)" % (name, value) in text
        assert getattr(_lib, name) == value
    assert hasattr(_lib.Context, "format_rows") and hasattr(_lib.Context, "format_matrix")


def test_golden_covers_the_cases(gold):
    assert sorted(gold) == sorted(export_cases.all_cases())
    assert os.path.getsize(export_cases.GOLDEN) < 512 * 1024


@pytest.mark.parametrize("fx,call", list(export_cases.all_cases()))
def test_files_equal_the_references(gold, tmp_path, fx, call):
    want = gold[(fx, call)]
    got = export_cases.run(build(fx), call, tmp_path)
    assert sorted(got) == sorted(want)  # the same set of files (no temporary left behind)
    for name in want:
        assert got[name] == want[name], "%s/%s: %s differs from the reference's file" % (fx, call, name)


def test_device_route_and_host_route(tmp_path, caplog):
    """%.8e and %.5e are formatted by the formatter under test, %.6f by np.savetxt with one logging line"""
    HarnessContext.calls.clear()
    build("prec5").saveAsText(str(tmp_path / "a"))
    assert [(c["width"], c["prec"], c["upper"], c["sep"]) for c in HarnessContext.calls] == [(0, 5, False, True)]
    HarnessContext.calls.clear()
    from getdist_amd import chainfiles

    chainfiles._host_route_logged.clear()
    with caplog.at_level(logging.INFO, logger="getdist_amd.chainfiles"):
        mc = build("prec6f")
        mc.saveAsText(str(tmp_path / "b"))
        mc.saveAsText(str(tmp_path / "c"))
    assert HarnessContext.calls == []
    assert len([r for r in caplog.records if "np.savetxt" in r.getMessage()]) == 1


def test_format_spec_parser():
    from getdist_amd.chainfiles import parse_device_format

    assert parse_device_format("%.8e") == (0, 8, False)
    assert parse_device_format("%16.7E") == (16, 7, True)
    assert parse_device_format("%15.7E") == (15, 7, True)
    assert parse_device_format("%e") == (0, 6, False)
    assert parse_device_format("%12e") == (12, 6, False)
    assert parse_device_format("%.0e") == (0, 0, False)
    assert parse_device_format("%32.17e") == (32, 17, False)
    for host in ("%.6f", "%g", "%.8g", "%-16.7e", "%+.8e", "% .8e", "%016.7e", "%#.3e", "%.18e", "%33.8e", "%.8e %.8e", "%.e",
                 "x%.8e", "%.8e\n", "%d", "", ["%.8e", "%.3e"], None):
        assert parse_device_format(host) is None, host


@pytest.mark.parametrize("chunk_rows", [None, 64, 7, 1])
def test_chunks_join_to_one_text(gold, tmp_path, chunk_rows):
    from getdist_amd import chainfiles

    mc = build("real")
    srcs, host_rows = mc._text_sources()
    path = str(tmp_path / "x.txt")
    HarnessContext.calls.clear()
    chainfiles.write_text_rows(path, mc.ctx, srcs, (0, mc.numrows), chunk_rows=chunk_rows)
    assert len(HarnessContext.calls) == (1 if chunk_rows is None else -(-mc.numrows // chunk_rows))
    assert open(path, "rb").read() == gold[("real", "save")]["chain.txt"]
    sub = str(tmp_path / "sub.txt")  # a range that starts and ends inside the set
    chainfiles.write_text_rows(sub, mc.ctx, srcs, (13, 301), chunk_rows=chunk_rows)
    assert open(sub, "rb").read() == b"".join(gold[("real", "save")]["chain.txt"].splitlines(True)[13:301])


def test_zero_rows_give_an_empty_file(tmp_path):
    from getdist_amd import chainfiles

    mc = build("unit")
    srcs, _ = mc._text_sources()
    path = str(tmp_path / "empty.txt")
    chainfiles.write_text_rows(path, mc.ctx, srcs, (5, 5))
    assert os.path.getsize(path) == 0


class _FailingFile:
    def __init__(self, f, fail_at):
        self.f, self.left = f, fail_at

    def write(self, data):
        self.left -= 1
        if self.left < 0:
            raise OSError("disk full")
        return self.f.write(data)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.f.close()


@pytest.mark.parametrize("where", ["sink", "formatter"])
def test_interrupted_save_leaves_no_file(tmp_path, monkeypatch, where):
    """The text goes to path.tmp<pid> and is renamed when complete: a failure half way leaves neither a truncated chain nor
    the temporary."""
    from getdist_amd import chainfiles

    mc = build("real")
    srcs, _ = mc._text_sources()
    path = str(tmp_path / "chain_1.txt")
    if where == "sink":
        monkeypatch.setattr(chainfiles, "open", lambda name, mode: _FailingFile(open(name, mode), 2), raising=False)
        with pytest.raises(OSError, match="disk full"):
            chainfiles.write_text_rows(path, mc.ctx, srcs, (0, mc.numrows), chunk_rows=50)
    else:
        real, count = mc.ctx.format_rows, [0]

        def failing(*a, **k):
            count[0] += 1
            if count[0] == 3:
                raise RuntimeError("device lost")
            return real(*a, **k)

        monkeypatch.setattr(mc.ctx, "format_rows", failing)
        with pytest.raises(RuntimeError, match="device lost"):
            chainfiles.write_text_rows(path, mc.ctx, srcs, (0, mc.numrows), chunk_rows=50)
    assert os.listdir(str(tmp_path)) == []
    # and an existing file survives a failed overwrite untouched
    monkeypatch.undo()
    chainfiles.write_text_rows(path, mc.ctx, srcs, (0, 10))
    before = open(path, "rb").read()
    monkeypatch.setattr(mc.ctx, "format_rows", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("device lost")))
    with pytest.raises(RuntimeError):
        chainfiles.write_text_rows(path, mc.ctx, srcs, (0, mc.numrows))
    assert open(path, "rb").read() == before and os.listdir(str(tmp_path)) == ["chain_1.txt"]


def test_chain_view_saves_its_rows_without_metadata(gold, tmp_path):
    mc = build("chains3")
    views = mc.getSeparateChains()
    views[1].saveAsText(str(tmp_path / "v"), chain_index=1)
    assert os.listdir(str(tmp_path)) == ["v_2.txt"]
    assert open(str(tmp_path / "v_2.txt"), "rb").read() == gold[("chains3", "chains")]["sub/dir/chain_2.txt"]


def test_param_strings():
    from getdist_amd.paramnames import ParamInfo, ParamNames
    from getdist_amd.parampriors import ParamBounds

    p = ParamInfo("omegab", "\\Omega_b")
    assert str(p) == p.string() == "omegab\t\\Omega_b"
    p.isDerived, p.comment = True, "baryons"
    assert p.string() == "omegab*\t\\Omega_b\t#baryons" and p.string(wantComments=False) == "omegab*\t\\Omega_b"
    names = ParamNames(["a", "b"], ["A", None])
    assert str(names) == "a\tA\nb\t\n"  # no label given: the reference holds "" there
    b = ParamBounds()
    b.setRange("x", (None, 1.0))
    b.setRange("phi", (0.0, 6.25, "periodic"))
    b.setRange("ignored", (None, None))
    b.setFixed("f", 2.0)
    assert str(b) == ("%22s%17s%17s\n" % ("x", "    N", "%15.7E" % 1.0) + "%22s%17s%17s%10s\n" % ("phi", "%15.7E" % 0.0, "%15.7E" % 6.25, "periodic")
                      + "%22s%17s%17s\n" % ("f", "%15.7E" % 2.0, "%15.7E" % 2.0))

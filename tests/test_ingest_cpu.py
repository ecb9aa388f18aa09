"""CPU tests of the host route of the chain ingestion (chainfiles.loadNumpyTxt / read_root with a context): a context that
cannot parse leaves today's behaviour, a context that declines falls back to the host parser for the whole file, and a
fix list is patched with float() of the named bytes."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from getdist_amd import chainfiles  # noqa: E402


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture()
def root(tmp_path):
    rng = np.random.default_rng(3)
    r = str(tmp_path / "chain")
    for k, n in enumerate((40, 55)):
        x = np.column_stack([rng.integers(1, 4, n), rng.random(n) * 10, rng.standard_normal((n, 3))])
        np.savetxt("%s_%d.txt" % (r, k + 1), x, fmt="%.8e")
    with open(r + ".paramnames", "w") as f:
        f.write("a\nb\nc\n")
    return r


def test_a_context_that_cannot_parse_changes_nothing(root):
    import fake_ctx

    fake = fake_ctx.FakeContext(0)
    assert not hasattr(fake, "parse_text")
    fname = root + "_1.txt"
    assert same_bits(chainfiles.loadNumpyTxt(fname, None, ctx=fake), chainfiles.loadNumpyTxt(fname))
    assert same_bits(chainfiles.loadNumpyTxt(fname, 3, fake), chainfiles.loadNumpyTxt(fname, 3))
    a = chainfiles.read_root(root, None, True, ctx=fake)
    b = chainfiles.read_root(root, None, True)
    assert a["names"] == b["names"] and len(a["samples"]) == 2
    for key in ("samples", "weights", "loglikes"):
        assert all(same_bits(x, y) for x, y in zip(a[key], b[key]))


class Declines:
    def __init__(self):
        self.calls = []

    def parse_text(self, source, skiprows=0, **kw):
        self.calls.append((source, skiprows, kw))
        return None


def test_a_declined_file_takes_the_host_route(root, tmp_path, capsys):
    stub = Declines()
    fname = root + "_2.txt"
    assert same_bits(chainfiles.loadNumpyTxt(fname, 2, ctx=stub), np.loadtxt(fname, skiprows=2))
    assert stub.calls == [(fname, 2, {})]
    loaded = chainfiles.read_root(root, None, True, ctx=stub)
    assert len(stub.calls) == 3 and [c.shape[0] for c in loaded["samples"]] == [40, 55]
    ragged = str(tmp_path / "ragged.txt")
    with open(ragged, "w") as f:
        f.write("1 2 3\n4 5\n")
    capsys.readouterr()
    with pytest.raises(ValueError) as with_stub:
        chainfiles.loadNumpyTxt(ragged, ctx=stub)
    assert capsys.readouterr().out.count("Error reading") == 1
    with pytest.raises(ValueError) as without:
        chainfiles.loadNumpyTxt(ragged)
    assert str(with_stub.value) == str(without.value)
    empty = str(tmp_path / "empty.txt")
    open(empty, "w").close()
    assert chainfiles.loadNumpyTxt(empty, ctx=stub).shape == (0, 0)
    assert len(stub.calls) == 4  # an empty file never reaches the context


class SkipsLikeTheDevice:
    """Skips lines the way Context.parse_text does (skipped_text_bytes on the binary file) and parses the rest exactly."""

    def __init__(self):
        self.declined = []

    def parse_text(self, source, skiprows=0, **kw):
        import io

        from getdist_amd._lib import skipped_text_bytes

        with open(source, "rb") as f:
            start = skipped_text_bytes(f, skiprows)
            self.declined.append(start is None)
            if start is None:
                return None
            f.seek(start)
            return dict(array=np.loadtxt(io.BytesIO(f.read()), ndmin=2), fixes=[])


def test_skipped_lines_end_where_text_mode_ends_them(tmp_path):
    """A lone CR inside the skipped lines is a line end for np.loadtxt and pandas, which open the file as text: the
    device route must decline, not skip through the next LF and lose a row."""
    import io

    from getdist_amd._lib import skipped_text_bytes

    lone = str(tmp_path / "lone_cr.txt")
    with open(lone, "wb") as f:
        f.write(b"x y z\r1 2 3\n4 5 6\n7 8 9\n")
    want = np.atleast_2d(np.loadtxt(lone, skiprows=1))
    assert want.shape == (3, 3)
    stub = SkipsLikeTheDevice()
    assert same_bits(chainfiles.loadNumpyTxt(lone, 1, ctx=stub), want)
    assert same_bits(chainfiles.loadNumpyTxt(lone, 1), want)
    assert stub.declined == [True]
    crlf = str(tmp_path / "crlf.txt")
    with open(crlf, "wb") as f:
        f.write(b"x y z\r\n# c\r\n1 2 3\r\n4 5 6\r\n")
    for skip in (1, 2, 3):  # CRLF is one line end in both modes
        stub = SkipsLikeTheDevice()
        assert same_bits(chainfiles.loadNumpyTxt(crlf, skip, ctx=stub), np.atleast_2d(np.loadtxt(crlf, skiprows=skip)))
        assert stub.declined == [False]
    cases = [(b"a\nb\nc\n", 2, 4), (b"a\nb", 1, 2), (b"a\nb", 5, 3), (b"a\n", 0, 0), (b"a\r\nb\n", 1, 3), (b"a\r\r\nb\n", 1, None),
             (b"a\rb\n", 1, None), (b"a\n\rb\nc\n", 1, 2), (b"a\n\rb\nc\n", 2, None), (b"a\xc3\xa9\nb\n", 1, None), (b"a\x00\nb\n", 1, None),
             (b"a\r", 1, None)]
    for text, skip, expect in cases:
        assert skipped_text_bytes(io.BytesIO(text), skip) == expect, (text, skip)


def test_a_fix_list_is_patched_with_float_of_the_named_bytes(tmp_path):
    text = b"# head\n1.5 2.5 9007199254740993.5\n4 1e23 6\n"
    fname = str(tmp_path / "fix.txt")
    with open(fname, "wb") as f:
        f.write(text)

    class Parses:
        def parse_text(self, source, skiprows=0, **kw):
            assert source == fname and skiprows == 1
            arr = np.array([[1.5, 2.5, np.nan], [4.0, np.nan, 6.0]])
            return dict(array=arr, fixes=[(0, 2, text.index(b"9007"), len(b"9007199254740993.5")), (1, 1, text.index(b"1e23"), 4)])

    got = chainfiles.loadNumpyTxt(fname, 1, ctx=Parses())
    assert same_bits(got, np.loadtxt(fname, skiprows=1))

    class TwoColumns:
        def parse_text(self, source, skiprows=0, **kw):
            return dict(array=np.zeros((2, 2)), fixes=[])

    two = str(tmp_path / "two.txt")
    with open(two, "wb") as f:
        f.write(b"1 2\n3 4\n")
    assert same_bits(chainfiles.loadNumpyTxt(two, ctx=TwoColumns()), np.array([[1.0, 2.0], [3.0, 4.0]]))

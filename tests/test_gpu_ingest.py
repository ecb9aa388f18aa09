"""GPU tier of the chain ingestion: gd_parse_scan / gd_parse_rows (csrc/ingest.hip, csrc/parsedouble.hpp) and the host
route built on them (Context.parse_text, chainfiles.loadNumpyTxt with a context) against np.loadtxt bit for bit: tile
boundaries, line ends and separators, comments, the fix list of undecided tokens, the declines (each leaving the output
block untouched), bad arguments, chunked files whose lines straddle every chunk boundary, and a save / load round trip."""

import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

pytestmark = pytest.mark.gpu

TILE_BYTES = 24576  # csrc/ingest.hip ING_TB: a block owns the lines that start in its 24 KiB of the text
MAX_LINE = 8192     # include/gdhip.h GD_PARSE_MAX_LINE


@pytest.fixture(scope="module")
def ctx():
    from getdist_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


def values(K, m, seed):
    rng = np.random.default_rng([7, seed, K, m])
    x = rng.standard_normal(K * m) * 10.0 ** rng.uniform(-30, 30, size=K * m)
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 5e-324, 1.7976931348623157e308, 1.0, -1.0, 1e22, 1e23, 0.5])
    pick = rng.integers(0, K * m, size=max(K * m // 7, 1))
    x[pick] = special[rng.integers(0, len(special), size=len(pick))]
    return x.reshape(K, m)


def make_text(x, fmt):
    if fmt == "repr":
        return "".join(" ".join(map(repr, r)) + "\n" for r in x.tolist()).encode()
    if fmt == "%.0e":
        return "".join(" ".join("%.0e" % v for v in r) + "\n" for r in x.tolist()).encode()
    sep = "" if fmt == "%16.7E" else " "  # makeSingleSamples writes its "%16.7E" fields back to back
    row = sep.join([fmt] * x.shape[1]) + "\n"
    return "".join(row % tuple(r) for r in x.tolist()).encode()


def reference(text, **kw):
    return np.loadtxt(io.BytesIO(text), ndmin=2, **kw)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def device_parse(ctx, text, **kw):
    """(array with the fix list applied, number of fixes) or (None, 0) when the device declines"""
    from getdist_amd.chainfiles import patch_fixes

    res = ctx.parse_text(text, **kw)
    if res is None:
        return None, 0
    arr = patch_fixes(res["array"], res["fixes"], lambda off, ln: text[off:off + ln])
    return arr, len(res["fixes"])


def check_text(ctx, text, **kw):
    got, nfix = device_parse(ctx, text, **kw)
    assert got is not None, "the device declined the text"
    want = reference(text)
    assert same_bits(got, want), "shapes %r / %r" % (got.shape, want.shape)
    return nfix


SHAPES = [(1, 1), (1, 3), (2, 52), (63, 3), (64, 52), (65, 52), (4097, 5)]


@pytest.mark.parametrize("fmt", ["%.8e", "%16.7E", "repr", "%.0e"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_parse_text_shapes(ctx, shape, fmt):
    # "%.0e" tokens are 5 to 7 bytes: a tile of 4097 x 5 of them holds more values than it collects in LDS (direct stores)
    check_text(ctx, make_text(values(shape[0], shape[1], 1), fmt))


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_tile_height(ctx, delta):
    """52 fields of "%16.7E" are 833 bytes a line, every line: the first tile owns the 30 lines that start in its 24 KiB."""
    line = 52 * 16 + 1
    height = -(-TILE_BYTES // line)
    for tiles in (1, 3):
        x = values(tiles * height + delta, 52, 2)
        text = make_text(x, "%16.7E")
        assert len(text) == x.shape[0] * line
        check_text(ctx, text)


def test_line_starting_on_a_tile_boundary(ctx):
    """8 fields of "%15.7E" and 7 blanks are 128 bytes a line: line 192 starts on the first byte of the second tile"""
    x = values(192 * 2 + 3, 8, 3)
    text = make_text(x, "%15.7E")
    assert len(text) == 128 * x.shape[0]
    check_text(ctx, text)


@pytest.mark.parametrize("fmt", ["%.8e", "repr"])
def test_line_ends_separators_and_comments(ctx, fmt):
    x = values(300, 5, 4)
    plain = make_text(x, fmt)
    lines = plain.split(b"\n")[:-1]
    rng = np.random.default_rng(5)
    check_text(ctx, plain[:-1])                              # no final newline
    check_text(ctx, b"\r\n".join(lines) + b"\r\n")           # CRLF
    check_text(ctx, b"\r\n".join(lines))                     # CRLF, none at the end
    blanks = [b" ", b"\t", b"   ", b" \t ", b"\x0b", b"\x0c "]
    out = []
    for k, ln in enumerate(lines):
        toks = ln.split()
        s = b"".join(t + blanks[int(rng.integers(0, len(blanks)))] for t in toks)
        out.append(blanks[k % len(blanks)] * (k % 3) + s.rstrip() + b" " * (k % 4))
    check_text(ctx, b"\n".join(out) + b"\n")                 # tabs, runs of blanks, leading and trailing blanks
    out = [b"# a header line", b"#"]
    for k, ln in enumerate(lines):
        out.append(ln + (b" # trailing " + ln if k % 3 == 0 else b"#x" if k % 3 == 1 else b""))
        if k % 5 == 0:
            out += [b"", b"   ", b"# 1 2 3 4 5 6 7", b"\t"]
    check_text(ctx, b"\n".join(out) + b"\n")                 # comments and blank lines
    check_text(ctx, b"\n\n" + b"\n".join(out))


def _upload(ctx, data):
    buf = ctx.alloc(max(len(data), 16))
    buf.from_host(np.frombuffer(data, dtype=np.uint8))
    return buf


def test_row_offset_and_ld(ctx):
    x = values(70, 4, 6)
    text = make_text(x, "%.8e")
    want = reference(text)
    for shift in (0, 5):  # a block that does not start on a 16-byte boundary
        d_text = _upload(ctx, b"\n" * shift + text)
        rc, rows, m, used = ctx.parse_scan(d_text, len(text), last=True, offset=shift)
        assert (rc, rows, m, used) == (0, 70, 4, len(text))
        ld, off = 100, 13
        before = np.random.default_rng(1).random(4 * ld)
        out = ctx.alloc(before.nbytes)
        out.from_host(before)
        rc, fixes, count = ctx.parse_rows(d_text, len(text), rows, m, out, ld, row_offset=off, offset=shift)
        assert rc == 0 and count == len(fixes)
        got = out.to_host((4, ld))
        for r, j, _, _ in fixes:
            assert off <= r < off + 70
            got[j, r] = want[r - off, j]
        expect = before.reshape(4, ld).copy()
        expect[:, off:off + 70] = want.T
        assert same_bits(got, expect)  # the rest of the block is unchanged
        out.free()
        d_text.free()


def undecided_text():
    """Rows of tokens among which the CPU harness finds undecided ones (exact ties scaled by negative powers of ten,
    tokens of more than 19 digits, values below 1e-310), and how many it finds."""
    import build_parse

    toks = [b"9007199254740993.5", b"1.5", b"4503599627370497.5", b"0.1", b"9007199254740993.00000000000000000001", b"2e-320",
            b"5e-324", b"1e23", b"123456789012345678901234567890", b"1.7976931348623158e308", b"2.5", b"1e-311",
            b"1.00000000000000011102230246251565404236316680908203125", b"7", b"1.2345678e+00"]
    rows = [toks[k:] + toks[:k] for k in range(len(toks))] * 3
    _, verdict, ok = build_parse.parse_tokens([t for r in rows for t in r])
    assert ok.all()
    return b"".join(b" ".join(r) + b"\n" for r in rows), int((verdict == build_parse.UNDECIDED).sum()), len(rows), len(toks)


def test_fix_list(ctx):
    text, expected, K, m = undecided_text()
    assert expected >= K  # every row holds at least one
    res = ctx.parse_text(text)
    assert res is not None and len(res["fixes"]) == expected
    flat = res["array"]
    for r, j, off, ln in res["fixes"]:
        assert np.isnan(flat[r, j])  # the placeholder
        assert text[off:off + ln] in text.split() and (off == 0 or text[off - 1:off] in b" \n")
    assert check_text(ctx, text) == expected
    # fix_capacity 0 reports the count and writes no entry; a short list makes parse_text decline
    d_text = _upload(ctx, text)
    out = ctx.alloc(8 * K * m)
    rc, fixes, count = ctx.parse_rows(d_text, len(text), K, m, out, K, fix_capacity=0)
    assert rc == 0 and count == expected and len(fixes) == 0
    rc, fixes, count = ctx.parse_rows(d_text, len(text), K, m, out, K, fix_capacity=3)
    assert rc == 0 and count == expected and len(fixes) == 3
    out.free()
    d_text.free()
    saved = ctx.PARSE_FIX_CAPACITY
    try:
        ctx.PARSE_FIX_CAPACITY = 3
        assert ctx.parse_text(text) is None
    finally:
        ctx.PARSE_FIX_CAPACITY = saved


def _long_line(nbytes):
    return b"1 2" + b" " * (nbytes - 5) + b"3\n"


DECLINES = {
    "ragged first": b"1 2\n1 2 3\n4 5 6\n" + b"7 8 9\n" * 50,
    "ragged middle": b"7 8 9\n" * 25 + b"1 2 3 4\n" + b"7 8 9\n" * 25,
    "ragged last": b"7 8 9\n" * 50 + b"1 2",
    "ragged across tiles": b"7 8 9\n" * 5000 + b"1 2\n" + b"7 8 9\n" * 5000,
    "lone CR": b"1 2 3\n4 5\r6\n7 8 9\n",
    "CR at the end": b"1 2 3\n4 5 6\r",
    "byte 0xC3": b"1 2 3\n4 5 \xc3\xa9\n",
    "byte 0xC3 in a comment": b"1 2 3 # caf\xc3\xa9\n4 5 6\n",
    "NUL": b"1 2 3\n4 \x00 6\n",
    "1_0": b"1 2 3\n4 1_0 6\n",
    "hex": b"1 2 3\n4 0x10 6\n",
    "bare e": b"1 2 3\n4 5 1e\n",
    # 4000 lines of three 1-byte tokens in the first tile are twice what the scan notes in its list (ING_SCAP = 6144); the
    # rest have their grammar checked inside the walk.  Which tokens the list takes is the order the lanes arrive in, so
    # the bad token stands once behind all others and once among them
    "1_0 behind the scan's token list": b"7 8 9\n" * 4000 + b"7 1_0 9\n",
    "1_0 behind the list, more rows after it": b"7 8 9\n" * 4000 + b"7 1_0 9\n" + b"7 8 9\n" * 4000,
    "long line": b"1 2 3\n" + _long_line(MAX_LINE + 1) + b"4 5 6\n",
    "long last line": b"1 2 3\n" * 5000 + _long_line(9000)[:-1],
}


@pytest.mark.parametrize("case", list(DECLINES))
def test_declines_leave_the_output_untouched(ctx, case):
    from getdist_amd._lib import GD_PARSE_NOT_PLAIN

    text = DECLINES[case]
    d_text = _upload(ctx, text)
    rc = ctx.parse_scan(d_text, len(text), last=True)[0]
    assert rc == GD_PARSE_NOT_PLAIN
    rows = text.count(b"\n") + 1
    before = np.random.default_rng(2).random(4 * rows)
    out = ctx.alloc(before.nbytes)
    out.from_host(before)
    rc, fixes, count = ctx.parse_rows(d_text, len(text), rows, 3, out, rows)
    assert rc == GD_PARSE_NOT_PLAIN and len(fixes) == 0
    assert same_bits(out.to_host((4 * rows,)), before)
    out.free()
    d_text.free()
    assert ctx.parse_text(text) is None


def test_short_tokens_overflow_the_scan_list(ctx):
    """Tokens of 1 to 2 bytes: a tile holds about 12 000 of them, more than the scan notes in its list (6144) and more
    than the parse collects in LDS (1792), so the scan checks the later ones inside its walk and the parse stores directly."""
    rng = np.random.default_rng(31)
    toks = np.array([b"0", b"1", b"2", b"3", b"4", b"5", b"6", b"7", b"8", b"9", b"-1", b".5", b"1.", b"+2", b"-0"], dtype=object)
    pick = toks[rng.integers(0, len(toks), size=(9000, 3))]
    text = b"".join(b" ".join(r) + b"\n" for r in pick.tolist())
    assert 3 * TILE_BYTES // 8 > 6144 and len(text) > 2 * TILE_BYTES
    assert check_text(ctx, text) == 0


def test_longest_line_is_taken(ctx):
    text = b"1 2 3\n" + _long_line(MAX_LINE) + b"4 5 6\n" + _long_line(MAX_LINE)[:-1]
    assert len(_long_line(MAX_LINE)) == MAX_LINE
    check_text(ctx, text)


def test_scan_of_a_block_that_goes_on(ctx):
    """Without `last` the scan stops behind the last newline and leaves the unfinished line -- whatever it holds -- alone."""
    text = b"1 2 3\n4 5 6\r\n# c\n7 8 9\n10 11 1e"
    d_text = _upload(ctx, text)
    rc, rows, m, used = ctx.parse_scan(d_text, len(text), last=False)
    assert (rc, rows, m, used) == (0, 3, 3, text.rindex(b"\n") + 1)
    rc, rows, m, used = ctx.parse_scan(d_text, 4, last=False)
    assert (rc, rows, m, used) == (0, 0, 0, 0)
    rc, rows, m, used = ctx.parse_scan(d_text, 0, last=True)
    assert (rc, rows, m, used) == (0, 0, 0, 0)
    d_text.free()


def test_bad_arguments(ctx):
    from getdist_amd._lib import GD_ERR_BADARG, GdhipError

    text = b"1 2 3\n4 5 6\n"
    d_text = _upload(ctx, text)
    out = ctx.alloc(8 * 3 * 10)

    def bad(call):
        with pytest.raises(GdhipError) as e:
            call()
        assert e.value.code == GD_ERR_BADARG

    bad(lambda: ctx.parse_scan(d_text, -1))
    bad(lambda: ctx.parse_scan(None, 5))
    bad(lambda: ctx.parse_rows(d_text, len(text), 2, 3, out, 1))                  # ld < rows
    bad(lambda: ctx.parse_rows(d_text, len(text), 2, 3, out, 10, row_offset=9))   # ld < row_offset + rows
    bad(lambda: ctx.parse_rows(d_text, len(text), 2, 3, out, 10, row_offset=-1))
    bad(lambda: ctx.parse_rows(d_text, -1, 2, 3, out, 10))
    bad(lambda: ctx.parse_rows(None, len(text), 2, 3, out, 10))
    bad(lambda: ctx.parse_rows(d_text, len(text), 2, 3, None, 10))
    bad(lambda: ctx.parse_rows(d_text, len(text), 3, 3, out, 10))                 # not what the scan reports
    bad(lambda: ctx.parse_rows(d_text, len(text), 2, 2, out, 10))
    rc, fixes, count = ctx.parse_rows(d_text, len(text), 2, 3, out, 10)
    assert rc == 0 and count == 0
    out.free()
    d_text.free()


@pytest.fixture(scope="module")
def chain_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ingest") / "chain_1.txt")
    text = b"# weight like a b c d e\n\n" + make_text(values(3000, 7, 8), "%.8e")
    lines = text.split(b"\n")
    lines[5] += b"  # five"
    with open(path, "wb") as f:
        f.write(b"\n".join(lines))
    return path


@pytest.mark.parametrize("skiprows", [0, 1, 5])
def test_load_numpy_txt_in_small_chunks(ctx, chain_file, skiprows):
    from getdist_amd import chainfiles

    calls = []
    spy = type("Spy", (), {"parse_text": lambda self, *a, **k: calls.append(1) or ctx.parse_text(*a, **k)})()
    # 4096-byte chunks against lines of about 100 bytes: a line straddles every chunk boundary
    got = chainfiles.loadNumpyTxt(chain_file, skiprows, ctx=spy, _parse_args=dict(chunk_bytes=4096))
    want = np.atleast_2d(np.loadtxt(chain_file, skiprows=skiprows))
    assert calls and same_bits(got, want)
    res = ctx.parse_text(chain_file, skiprows=skiprows, chunk_bytes=4096)
    assert res is not None and res["array"].shape == want.shape  # the device route was not declined
    assert same_bits(chainfiles.loadNumpyTxt(chain_file, skiprows, ctx=ctx), want)  # one chunk


def test_skipped_lines_that_only_text_mode_can_count(ctx, tmp_path):
    """np.loadtxt and pandas skip lines of a file opened as text, where a lone CR ends a line too; the device never
    sees the skipped bytes, so parse_text declines and the host route's rows come back."""
    from getdist_amd import chainfiles

    lone = str(tmp_path / "lone_cr.txt")
    with open(lone, "wb") as f:
        f.write(b"x y z\r1 2 3\n4 5 6\n7 8 9\n")
    want = np.atleast_2d(np.loadtxt(lone, skiprows=1))
    assert want.shape == (3, 3)
    assert ctx.parse_text(lone, skiprows=1) is None
    assert same_bits(chainfiles.loadNumpyTxt(lone, 1, ctx=ctx), want)
    assert same_bits(chainfiles.loadNumpyTxt(lone, 1, ctx=ctx), chainfiles.loadNumpyTxt(lone, 1))
    crlf = str(tmp_path / "crlf.txt")
    with open(crlf, "wb") as f:
        f.write(b"x y z\r\n1 2 3\r\n4 5 6\r\n7 8 9\r\n")
    for skip in (1, 2):  # CRLF is one line end for both: the device route takes it
        res = ctx.parse_text(crlf, skiprows=skip)
        assert res is not None and not res["fixes"]
        assert same_bits(res["array"], np.loadtxt(crlf, skiprows=skip, ndmin=2))
    accent = str(tmp_path / "accent.txt")
    with open(accent, "wb") as f:
        f.write(b"# caf\xc3\xa9\n1 2 3\n4 5 6\n")
    assert ctx.parse_text(accent, skiprows=1) is None  # whether the skipped bytes decode is the text reader's to say


def test_an_allocation_that_fails_declines(ctx, chain_file, monkeypatch):
    """GD_ERR_NOMEM inside parse_text (the share of free memory was there, one block of it was not) takes the host
    route, as before the device route existed; any other device error still raises."""
    from getdist_amd import chainfiles
    from getdist_amd._lib import GD_ERR_HIP, GD_ERR_NOMEM, GdhipError

    want = np.atleast_2d(np.loadtxt(chain_file))
    real = ctx.alloc
    state = {"calls": 0, "code": GD_ERR_NOMEM}

    def failing(nbytes):
        state["calls"] += 1
        if state["calls"] == 2:  # the output block: the text is on the device and scanned by then
            raise GdhipError(state["code"], "no block of %d bytes" % nbytes)
        return real(nbytes)

    monkeypatch.setattr(ctx, "alloc", failing)
    assert ctx.parse_text(chain_file) is None
    state["calls"] = 0
    assert same_bits(chainfiles.loadNumpyTxt(chain_file, ctx=ctx), want)
    state.update(calls=0, code=GD_ERR_HIP)
    with pytest.raises(GdhipError):
        ctx.parse_text(chain_file)
    monkeypatch.undo()
    assert same_bits(chainfiles.loadNumpyTxt(chain_file, ctx=ctx), want)


def test_load_numpy_txt_ragged_and_empty(ctx, tmp_path, capsys):
    from getdist_amd import chainfiles

    ragged = str(tmp_path / "ragged.txt")
    with open(ragged, "wb") as f:
        f.write(make_text(values(40, 5, 9), "%.8e") + b"1.0 2.0\n")
    with pytest.raises(ValueError) as without:
        chainfiles.loadNumpyTxt(ragged)
    capsys.readouterr()
    with pytest.raises(ValueError) as with_ctx:
        chainfiles.loadNumpyTxt(ragged, ctx=ctx)
    assert str(with_ctx.value) == str(without.value)
    assert capsys.readouterr().out.count("Error reading") == 1
    empty = str(tmp_path / "empty.txt")
    open(empty, "wb").close()
    got = chainfiles.loadNumpyTxt(empty, ctx=ctx)
    assert got.shape == (0, 0)
    two = str(tmp_path / "two.txt")  # fewer than 3 columns: the host route's array
    with open(two, "wb") as f:
        f.write(b"1 2\n3 4\n")
    assert same_bits(chainfiles.loadNumpyTxt(two, ctx=ctx), chainfiles.loadNumpyTxt(two))


def test_round_trip_through_the_device_route(tmp_path):
    from getdist_amd._lib import Context
    from getdist_amd.mcsamples import MCSamples

    rng = np.random.default_rng(12)
    samples = rng.standard_normal((1500, 4)) * np.array([1.0, 1e-3, 1e5, 1e-12])
    mc = MCSamples(samples=[samples[:700], samples[700:]], weights=[rng.integers(1, 5, size=700).astype(float),
                                                                   rng.integers(1, 5, size=800).astype(float)],
                   loglikes=[rng.random(700) * 30, rng.random(800) * 30], names=["a", "b", "c", "d"],
                   settings={"ignore_rows": 0})
    root = str(tmp_path / "chain")
    mc.saveChainsAsText(root)
    mc.ctx.close()
    calls = []

    def factory(device):
        c = Context(device)
        inner = c.parse_text

        def spy(*a, **k):
            res = inner(*a, **k)
            calls.append(res is not None)
            return res

        c.parse_text = spy
        return c

    back = MCSamples(root=root, settings={"ignore_rows": 0}, _no_cache=True, _context_factory=factory)
    files = sorted(f for f in os.listdir(str(tmp_path)) if f.endswith(".txt"))
    assert len(files) == 2
    want = np.vstack([np.loadtxt(str(tmp_path / f)) for f in files])
    assert calls == [True, True]  # both chain files took the device route
    assert same_bits(back.weights, want[:, 0]) and same_bits(back.loglikes, want[:, 1]) and same_bits(back.samples, want[:, 2:])
    back.ctx.close()

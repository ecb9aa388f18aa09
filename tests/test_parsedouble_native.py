"""
CPU tests of getdist_amd/csrc/parsedouble.hpp, the integer-only decimal -> double conversion that runs inside the ingestion
kernels (csrc/ingest.hip), compiled for the host by tests/native/build_parse.py.  Every token is held to np.loadtxt bit
for bit (uint64 view, NaNs included): the contract of the chain ingestion is the reference's doubles, not close ones.
A token may come back *undecided*; it then takes the fix-up rule of the host route (float() of its bytes) and the final
bits are held to the same oracle.
"""

import io
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

FORMATS = ["repr", "%.8e", "%16.7E", "%.17e", "%.0e"]


@pytest.fixture(scope="module")
def par():
    import build_parse

    build_parse.load()
    return build_parse


def text_of(values, fmt):
    """One token per value (no blanks: "%16.7E" pads on the left, and a token has none)."""
    vals = np.asarray(values, dtype=np.float64).tolist()
    if fmt == "repr":
        return [repr(v).encode() for v in vals]
    return [(fmt % v).strip().encode() for v in vals]


def oracle_bits(tokens):
    arr = np.loadtxt(io.BytesIO(b"\n".join(tokens) + b"\n"), ndmin=1)
    assert arr.shape == (len(tokens),)
    return arr.view(np.uint64)


def check(par, tokens, want=None):
    """Harness + fix-up rule against np.loadtxt; returns the mask of undecided tokens."""
    bits, verdict, ok = par.parse_tokens(tokens)
    want = oracle_bits(tokens) if want is None else want
    assert not (verdict == par.NOT_A_NUMBER).any(), "rejected: %r" % tokens[int(np.argmax(verdict == par.NOT_A_NUMBER))]
    assert ok.all(), "the grammar check rejects %r" % tokens[int(np.argmin(ok))]
    und = verdict == par.UNDECIDED
    final = bits.copy()
    for i in np.flatnonzero(und):
        final[i] = np.float64(float(tokens[i])).view(np.uint64)  # the host route's fix-up
    bad = np.flatnonzero(final != want)
    assert bad.size == 0, "token %r: got %016x, np.loadtxt gives %016x (undecided: %s)" % (
        tokens[bad[0]], int(final[bad[0]]), int(want[bad[0]]), bool(und[bad[0]]))
    return und


def decimal_exponent(tok):
    """q of a "d.ddde+XX" token: the power of ten that scales its digits read as an integer."""
    mant, _, ex = tok.lower().partition(b"e")
    return int(ex) - len(mant.partition(b".")[2])


def bits_of(values):
    return np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)


def powers():
    p10 = np.array([float("1e%d" % e) for e in range(-323, 309)]).view(np.uint64)
    p2 = bits_of([2.0 ** e for e in range(-1073, 1024)])
    both = np.concatenate([p10, p2])
    return np.concatenate([both - np.uint64(1), both, both + np.uint64(1)]).view(np.float64)


@pytest.mark.parametrize("fmt", FORMATS)
def test_random_bit_patterns(par, fmt):
    bits = np.random.default_rng(2024).integers(0, 2 ** 64, size=2_000_000, dtype=np.uint64, endpoint=False)
    tokens = text_of(bits.view(np.float64), fmt)
    und = check(par, tokens)
    print("%s: %d of %d random bit patterns undecided" % (fmt, int(und.sum()), len(tokens)))
    if fmt in ("%.8e", "%16.7E"):
        q = np.array([decimal_exponent(t) if t[-1:].isdigit() else 0 for t in tokens])
        inside = (q >= -22) & (q <= 22)
        assert not und[inside].any()


@pytest.mark.parametrize("fmt", FORMATS)
def test_scaled_normals(par, fmt):
    rng = np.random.default_rng(77)
    x = rng.standard_normal(1_000_000) * 10.0 ** rng.uniform(-30, 30, size=1_000_000)
    tokens = text_of(x, fmt)
    und = check(par, tokens)
    print("%s: %d of %d scaled normals undecided" % (fmt, int(und.sum()), len(tokens)))
    if fmt in ("%.8e", "%16.7E"):
        # at most 9 digits: w < 2^30 cannot form a 54-bit tie, and the nearest halfway point is further than the window
        q = np.array([decimal_exponent(t) for t in tokens])
        inside = (q >= -22) & (q <= 22)
        assert inside.sum() > 100_000
        assert not und[inside].any(), "undecided inside -22 <= q <= 22: %r" % tokens[int(np.flatnonzero(und & inside)[0])]
    if fmt == "%.17e":
        # q inside the table: the window is 2^-73 of an ulp wide, so "everything undecided" cannot pass
        assert und.sum() * 10_000 <= len(tokens)


@pytest.mark.parametrize("fmt", FORMATS)
def test_powers_and_neighbours(par, fmt):
    tokens = text_of(powers(), fmt)
    und = check(par, tokens)
    print("%s: %d powers of ten / two and neighbours undecided" % (fmt, int(und.sum())))
    if fmt in ("%.8e", "%16.7E"):
        q = np.array([decimal_exponent(t) for t in tokens])
        inside = (q >= -22) & (q <= 22)
        assert inside.sum() > 500
        print("%s: %d of %d tokens inside -22 <= q <= 22 undecided" % (fmt, int(und[inside].sum()), int(inside.sum())))
        assert not und[inside].any(), "undecided inside -22 <= q <= 22: %r" % tokens[int(np.flatnonzero(und & inside)[0])]


def test_around_half_the_least_subnormal(par):
    """Tokens on both sides of 2^-1075 = 2.4703282292062327...e-324, where 0 and the least subnormal meet, at 1 to 20
    digits.  Their q lies below the table (w >= 1 and q >= -310 make 1e-310 at the least, so decide() itself never sees a
    value that small: its guard for that range is there for soundness alone); they are undecided and the fix-up settles them."""
    from fractions import Fraction

    half = Fraction(1, 2 ** 1075)
    tokens = []
    for nd in range(1, 21):
        scaled = half * Fraction(10) ** (323 + nd)  # nd digits in front of the point
        w = int(scaled)
        for d in (-2, -1, 0, 1, 2):
            if w + d > 0:
                tokens.append(("%de-%d" % (w + d, 323 + nd)).encode())
    und = check(par, tokens)
    print("subnormal boundary: %d of %d undecided" % (int(und.sum()), len(tokens)))


def test_extremes(par):
    tokens = [b"5e-324", b"4.9406564584124654e-324", b"2.4703282292062328e-324", b"2.4703282292062329e-324",
              b"2.4703282292062327e-324", b"1.7976931348623157e308", b"1.7976931348623158e308", b"1.7976931348623159e308",
              b"1e400", b"-1e-400", b"2.2250738585072014e-308", b"2.2250738585072011e-308", b"1e-345", b"9.9e-346", b"1e309",
              b"1e308", b"0.5", b".125", b"1.", b"+1", b"-0", b"0e999", b"-0.0e-999", b"1e99999999999999999999",
              b"1e-99999999999999999999", b"00000000000000000000000000001", b"0.00000000000000000000000000000000001"]
    und = check(par, tokens)
    bits, verdict, _ = par.parse_tokens(tokens)
    assert int(bits[tokens.index(b"-0")]) == 0x8000000000000000
    assert int(bits[tokens.index(b"2.4703282292062328e-324")]) == 0 or und[tokens.index(b"2.4703282292062328e-324")]
    print("extremes: %d of %d undecided" % (int(und.sum()), len(tokens)))


def test_nan_and_inf_patterns(par):
    tokens = [b"nan", b"-NaN", b"+nan", b"NAN", b"Infinity", b"-inf", b"+INF", b"-iNfInItY", b"inf"]
    und = check(par, tokens)
    assert not und.any()
    bits, _, _ = par.parse_tokens(tokens)
    python = np.array([float(t.decode()) for t in tokens]).view(np.uint64)
    assert (bits == python).all()  # -nan keeps the sign Python gives it


def halfway_tokens():
    """Exact ties: odd 54-bit integers h (2^53 + 1 style) at several binary exponents, written out in full, and their
    neighbours one digit longer (...5 -> ...50001 and ...49999)."""
    from fractions import Fraction

    rng = np.random.default_rng(19)
    out = []
    odd = [2 ** 53 + 1, 2 ** 54 - 1] + [int(v) | 1 | (1 << 53) for v in rng.integers(0, 2 ** 53, size=40)]
    for h in odd:
        for e in (0, 1, 7, 30, 63, 200, -1, -2, -10, -40, -54, -60):
            v = Fraction(h) * Fraction(2) ** e
            if v.denominator == 1:
                s = str(v.numerator)
                out += [s, s + ".0", s + ".00000000000000000001", str(v.numerator - 1) + ".99999999999999999999"]
            else:  # h / 2^k = h 5^k / 10^k: a finite decimal
                k = -e
                digits = str(h * 5 ** k)
                digits = digits.rjust(k + 1, "0")
                s = digits[:-k] + "." + digits[-k:]
                assert s.endswith("5")
                out += [s, s + "0001", s[:-1] + "49999", s + "000000000000000000000000"]
    return [t.encode() for t in out]


def test_exact_halfway_cases(par):
    tokens = halfway_tokens()
    assert len(tokens) > 1500
    und = check(par, tokens)
    print("halfway cases: %d of %d undecided" % (int(und.sum()), len(tokens)))


def test_long_tokens(par):
    """25-40 digits and long runs of leading and trailing zeros."""
    rng = np.random.default_rng(23)
    tokens = []
    for nd in range(25, 41):
        for _ in range(200):
            d = "".join(map(str, rng.integers(0, 10, size=nd)))
            cut = int(rng.integers(0, nd + 1))
            tokens.append((d[:cut] + "." + d[cut:] + "e%d" % int(rng.integers(-40, 40))).encode())
            tokens.append(("0" * int(rng.integers(1, 30)) + d[:cut] + "0" * int(rng.integers(0, 30))).encode() or b"0")
            tokens.append(("0." + "0" * int(rng.integers(1, 30)) + d + "0" * int(rng.integers(0, 30))).encode())
            tokens.append((str(int(rng.integers(1, 10 ** 9))) + "0" * int(rng.integers(10, 40)) + ".000").encode())
    tokens = [t for t in tokens if any(c in b"0123456789" for c in t)]
    und = check(par, tokens)
    print("long tokens: %d of %d undecided" % (int(und.sum()), len(tokens)))
    assert und.sum() < len(tokens) // 2


REJECTED = [b"1_0", b"0x10", b"1d5", b"1e", b"1e+", b".", b"+", b"1.2.3", b"1j", b"--1", b"", b"1\xc3\xa9", b"\xc3\xa9", b"1\xff",
            b"e5", b".e5", b"na", b"nanx", b"infi", b"infinityy", b"1e5.", b"1e5e5", b"+-1", b"1+1", b"0b1", b"1f"]


def test_rejections(par):
    bits, verdict, ok = par.parse_tokens(REJECTED)
    for t, v, g in zip(REJECTED, verdict, ok):
        assert v == par.NOT_A_NUMBER and not g, "%r is taken for a number" % t
    for t in REJECTED:  # the yardstick rejects each of them too
        if t and all(c < 0x80 for c in t):
            with pytest.raises(ValueError):
                np.loadtxt(io.BytesIO(t + b"\n"))
    # a NUL byte inside a token
    bits, verdict, ok = par.parse_tokens([b"1\x002"])
    assert verdict[0] == par.NOT_A_NUMBER and not ok[0]


def test_sanitizer_program(par):
    """The same source as a stand-alone program under AddressSanitizer + UBSan: every token is read from a heap block of
    exactly its length.  A child process; nothing is loaded into this interpreter."""
    exe = par.sanitizer_program()
    if exe is None:
        pytest.skip("g++ has no sanitizer runtime on this machine")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout

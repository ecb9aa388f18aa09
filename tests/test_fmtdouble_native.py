"""
CPU tests of getdist_amd/csrc/fmtdouble.hpp, the integer-only "%W.Pe" formatter that runs inside the export kernels
(csrc/export.hip), compiled for the host by tests/native/build_fmt.py.  Every value is held to Python's ``%`` operator
byte for byte: the contract of the chain export is equality with the reference's files, not numbers that parse close.
"""

import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

SPECS = [(0, 8, False), (16, 7, True), (15, 7, True), (0, 0, False), (0, 17, False), (25, 16, False)]
SPEC_IDS = ["%%%d.%d%s" % (w, p, "E" if u else "e") for w, p, u in SPECS]


@pytest.fixture(scope="module")
def fmt():
    import build_fmt

    build_fmt.load()
    return build_fmt


def spec_string(width, prec, upper):
    return "%%%s.%d%s" % (width if width else "", prec, "E" if upper else "e")


def python_text(values, width, prec, upper):
    spec = spec_string(width, prec, upper) + "\n"
    return "".join([spec % v for v in values.tolist()]).encode()


def check(fmt, bits, width, prec, upper, slow=False):
    """The harness and Python agree on every byte; returns how many values left the fast path."""
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    got, taken = fmt.format_array(bits, width, prec, upper, tail=10, slow=slow)
    want = python_text(bits.view(np.float64), width, prec, upper)
    if got != want:
        g, w = got.split(b"\n"), want.split(b"\n")
        for i, (a, b) in enumerate(zip(g, w)):
            assert a == b, "value %r (bits %016x) as %s: got %r, Python gives %r" % (
                bits.view(np.float64)[i], int(bits[i]), spec_string(width, prec, upper), a, b)
        assert len(g) == len(w)
    return taken


def bits_of(values):
    return np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)


def powers_of_ten():
    p = np.array([float("1e%d" % e) for e in range(-323, 309)]).view(np.uint64)
    return np.concatenate([p - 1, p, p + 1])


def powers_of_two():
    return bits_of([2.0 ** e for e in range(-1074, 1024)])


def extremes():
    b = [0x0000000000000001, 0x000FFFFFFFFFFFFF, 0x0010000000000000, 0x7FEFFFFFFFFFFFFF,  # subnormal / normal ends
         0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,  # +-0, +-inf
         0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001,  # NaNs: both signs, payloads
         0x7FFFFFFFFFFFFFFF, 0xFFF8000000ABCDEF, 0x7FF4000000000000]
    b = np.array(b, dtype=np.uint64)
    return np.concatenate([b, b[:4] | np.uint64(1 << 63)])


def carry_cases():
    x = np.array([9.999999995e99, 9.999999995e-101, 9.99999995e99, 9.99999995e-101, 9.5e99, 9.5e-100, 1e100, 1e-100, 1e-99, 9.9999999999999999e99])
    b = x.view(np.uint64)
    return np.concatenate([b - 2, b - 1, b, b + 1, b + 2])


def constructed_ties(prec, rng, per_j=40):
    """Doubles on or next to an EXACT tie at ``prec``.  Returns (near, far).  ``far``: (10 d + 5) 10^j for random
    (prec + 1)-digit d and every j >= 0 whose product is still a double (d 5^(j+1) < 2^53 or so): these are scaled by
    10^q with q = -1 - j < 0, where the table entry is inexact.  ``near``: d + 1/2 (a tie at q = 0), d + 1/8, and odd
    numerators over small powers of two -- few fractional bits, q >= 0, decided exactly by the fast path."""
    lo, hi = 10 ** prec, 10 ** (prec + 1)
    near, far = [], []
    j = 0
    while True:
        got = 0
        for d in rng.integers(lo, hi, size=per_j).tolist():
            v = (10 * d + 5) * 10 ** j
            if v >> ((v & -v).bit_length() - 1) < 2 ** 53:  # the odd part fits the significand: v is a double
                assert int(float(v)) == v
                far.append(float(v))
                got += 1
        if got == 0:
            break
        j += 1
    for d in rng.integers(lo, hi, size=per_j).tolist():
        near += [d + 0.5, d + 0.125, d + 0.375, (d // 1000) + 0.0625]
    for shift in range(1, 12):
        for d in rng.integers(lo, hi, size=per_j).tolist():
            near.append((2 * d + 1) / 2.0 ** shift)
    return np.array(near), np.array(far)


def test_directed_cases(fmt):
    rng = np.random.default_rng(11)
    sets = [powers_of_ten(), powers_of_two(), extremes(), carry_cases(), bits_of(np.arange(0, 10001, dtype=np.float64)),
            bits_of(-np.arange(0, 10001, dtype=np.float64)),
            bits_of([1234567.125, 1234567125000.0, 0.5, 1.5, 2.5, 0.125, 1e22, 1e23, 5e-324, -5e-324])]
    for prec in (7, 8):
        near, far = constructed_ties(prec, rng)
        sets += [bits_of(near), bits_of(far), bits_of(-far)]
    allbits = np.concatenate(sets)
    for w, p, u in SPECS:
        check(fmt, allbits, w, p, u)
        check(fmt, allbits, w, p, u, slow=True)  # the exact path alone gives the same bytes


def test_documented_examples(fmt):
    def one(x, w, p, u):
        return fmt.format_array(bits_of([x]), w, p, u)[0]

    assert one(1234567.125, 0, 8, False) == b"1.23456712e+06"       # tie, to even
    assert one(1234567125000.0, 0, 8, False) == b"1.23456712e+12"   # tie with q < 0
    assert one(9.999999995e99, 0, 8, False) == b"9.99999999e+99"
    assert one(np.nextafter(9.999999995e99, np.inf), 0, 8, False) == b"1.00000000e+100"
    assert one(5e-324, 0, 8, False) == b"4.94065646e-324"
    assert one(-0.0, 0, 8, False) == b"-0.00000000e+00"
    assert one(3.0, 0, 0, False) == b"3e+00"
    assert one(float("-inf"), 16, 7, True) == b"            -INF"
    assert one(-float("nan"), 16, 7, True) == b"             NAN"
    assert one(-float("nan"), 0, 8, False) == b"nan"


def test_exact_ties_take_the_exact_path(fmt):
    """A tie scaled by a negative power of ten sits exactly on the boundary the truncated table cannot decide."""
    rng = np.random.default_rng(5)
    for prec in (7, 8):
        _, far = constructed_ties(prec, rng)
        assert far.size > 100
        taken = check(fmt, bits_of(far), 0, prec, False)
        assert taken >= 1, "no constructed tie with q < 0 left the fast path"
        print("P = %d: %d of %d constructed ties with q < 0 took the exact path" % (prec, taken, far.size))


@pytest.mark.parametrize("spec", SPECS, ids=SPEC_IDS)
def test_random_bit_patterns(fmt, spec):
    bits = np.random.default_rng(2024).integers(0, 2 ** 64, size=2_000_000, dtype=np.uint64, endpoint=False)
    check(fmt, bits, *spec)


@pytest.mark.parametrize("spec", SPECS, ids=SPEC_IDS)
def test_scaled_normals(fmt, spec):
    rng = np.random.default_rng(77)
    x = rng.standard_normal(1_000_000) * 10.0 ** rng.uniform(-30, 30, size=1_000_000)
    check(fmt, bits_of(x), *spec)


def test_plain_normals_stay_on_the_fast_path(fmt):
    """standard_normal x 1 at P = 8 scales by 10^8..10^13 or so: an exact table entry, so the exact path is never needed;
    the error bound allows about 2^-60 per value where the entry is inexact."""
    x = np.random.default_rng(3).standard_normal(1_000_000)
    taken = check(fmt, bits_of(x), 0, 8, False)
    print("standard_normal x 1, 1e6 values at %%.8e: %d took the exact path" % taken)
    assert taken == 0  # every draw is above 1e-47 in magnitude: 0 <= q <= 55, where the table is exact


def test_sanitizer_program(fmt):
    """The same source as a stand-alone program under AddressSanitizer + UBSan: every value goes into a heap block of
    exactly max(W, P + 8) bytes.  A child process; nothing is loaded into this interpreter."""
    exe = fmt.sanitizer_program()
    if exe is None:
        pytest.skip("g++ has no sanitizer runtime on this machine")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout

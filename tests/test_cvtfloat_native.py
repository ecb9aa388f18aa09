"""CPU test of getdist_amd/csrc/cvtfloat.hpp -- the narrowing conversions of device-array output (csrc/devexport.hip) --
compiled for the host by tests/native/build_cvt.py.  fp16 and fp32 are held bit for bit to numpy's ``astype`` (IEEE
round-to-nearest-even in one step from the double), bf16 to a model in Python integers that decides by the exact
remainder (devexport_cases.bf16_model).  NaN inputs: numpy's software fp16 path keeps a signalling payload as it is, the
header quiets it like the hardware conversions do, so for NaNs the sign, the NaN-ness and the quiet bit are checked."""

import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))
import devexport_cases as xc  # noqa: E402


@pytest.fixture(scope="module")
def cvt():
    import build_cvt

    build_cvt.load()
    return build_cvt


@pytest.fixture(scope="module")
def patterns():
    """1e5 random bit patterns (every exponent, NaNs and subnormals included), values dense around the fp16 / bf16 / fp32
    ranges, and the targeted values"""
    r = np.random.default_rng(11)
    raw = r.integers(0, 1 << 64, 100_000, dtype=np.uint64)
    scaled = (r.standard_normal(20_000) * np.exp2(r.integers(-160, 130, 20_000).astype(np.float64))).view(np.uint64)
    # exact ties and their neighbours on the fp16 grid: k / 2048 in [1, 2) is a tie for odd k
    ties = 1 + np.arange(1, 4096, dtype=np.float64) / 4096
    near = np.concatenate([ties, np.nextafter(ties, 0), np.nextafter(ties, 4)]).view(np.uint64)
    return np.concatenate([raw, scaled, near, xc.targeted_values().view(np.uint64)])


def check(bits, f16, bf16, f32):
    x = bits.view(np.float64)
    nan = np.isnan(x)
    want16, want32 = xc.narrowed(x, np.float16), xc.narrowed(x, np.float32)
    assert np.array_equal(f16[~nan], want16[~nan])
    assert np.array_equal(f32[~nan], want32[~nan])
    assert np.array_equal(bf16[~nan], xc.bf16_model(x[~nan]))
    sign = (bits[nan] >> np.uint64(63)).astype(np.uint16)
    assert np.all((f16[nan] & 0x7E00) == 0x7E00) and np.array_equal(f16[nan] >> 15, sign)
    assert np.all((bf16[nan] & 0x7FC0) == 0x7FC0) and np.array_equal(bf16[nan] >> 15, sign)
    assert np.all(np.isnan(f32[nan].view(np.float32))) and np.array_equal((f32[nan] >> 31).astype(np.uint16), sign)
    assert np.array_equal(bf16[nan], xc.bf16_model(x[nan]))


def test_bit_equal_to_astype_and_the_exact_model(cvt, patterns):
    check(patterns, *cvt.convert(patterns))


def test_the_single_step_is_not_cosmetic(cvt):
    """the two values a detour over fp32 gets wrong, and the bf16 ties"""
    x = np.array([65519.999, 1 + 2.0**-11 + 2.0**-40, 65520.0, 1 + 2.0**-11, 1 + 3 * 2.0**-11])
    f16, bf16, _ = cvt.convert(x.view(np.uint64))
    assert list(f16.view(np.float16)) == [65504.0, 1 + 2.0**-10, np.inf, 1.0, 1 + 2.0**-9]
    with np.errstate(over="ignore"):
        through = x.astype(np.float32).astype(np.float16)
    assert through[0] == np.inf and through[1] == 1.0  # what the two-step route gives
    y = np.array([1 + 2.0**-8, 1 + 3 * 2.0**-8, 1 + 2.0**-8 + 2.0**-50, -0.0, 2.0**-134, 2.0**-134 * (1 + 2.0**-40)])
    _, bf16, _ = cvt.convert(y.view(np.uint64))
    assert list(bf16) == [0x3F80, 0x3F82, 0x3F81, 0x8000, 0x0000, 0x0001]


def test_subnormal_results_survive(cvt):
    x = np.array([6e-8, 2.0**-25, 2.0**-25 * (1 + 2.0**-30), 1e-40, -1e-40, 7e-46, 1e-45])
    f16, _, f32 = cvt.convert(x.view(np.uint64))
    assert list(f16[:3]) == [0x0001, 0x0000, 0x0001]
    assert np.array_equal(f32.view(np.float32), x.astype(np.float32)) and np.all(f32[3:5].view(np.float32) != 0)
    assert f32[5] == 0 and f32[6] == 1


def test_sanitizer_program(cvt, patterns, tmp_path):
    """The same source as a stand-alone program under AddressSanitizer + UBSan, on the same vectors: inputs and outputs lie
    in heap blocks of exactly their size.  A child process; nothing is loaded into this interpreter."""
    exe = cvt.sanitizer_program()
    if exe is None:
        pytest.skip("g++ has no sanitizer runtime on this machine")
    src, dst = tmp_path / "patterns.bin", tmp_path / "narrowed.bin"
    patterns.tofile(src)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    n = patterns.size
    raw = np.fromfile(dst, dtype=np.uint8)
    assert raw.size == 8 * n
    f16, bf16 = raw[:2 * n].view(np.uint16), raw[2 * n:4 * n].view(np.uint16)
    check(patterns, f16, bf16, raw[4 * n:].view(np.uint32))

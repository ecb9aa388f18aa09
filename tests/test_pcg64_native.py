"""
CPU tests of getdist_amd/csrc/pcg64.hpp, the PCG64 that runs inside the weight-one draw kernels (csrc/draw.hip), compiled
for the host by tests/native/build_pcg64.py: every double, the jump-ahead and the stride form are held to numpy's
np.random.default_rng bit for bit -- the draw's contract is equality with the reference's rows, not statistical equivalence.
"""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

SEEDS = [0, 7, 12345, 2**63 + 11]
OFFSETS = [0, 1, 2, 2**32 + 5, 10**7 - 1]
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def lib():
    import build_pcg64

    return build_pcg64.load()


def words(bit_generator):
    """{state_hi, state_lo, inc_hi, inc_lo} of a PCG64 bit generator, as the C entry points take it"""
    s = bit_generator.state["state"]
    return (ctypes.c_uint64 * 4)(s["state"] >> 64, s["state"] & M64, s["inc"] >> 64, s["inc"] & M64)


def with_pending_uint32(seed):
    """A generator that holds a buffered 32-bit half (has_uint32 = 1)."""
    g = np.random.default_rng(seed)
    g.integers(0, 2**32, dtype=np.uint32, endpoint=False)
    assert g.bit_generator.state["has_uint32"] == 1
    return g


def generators():
    out = [("seed%d" % s, lambda s=s: np.random.default_rng(s)) for s in SEEDS]
    out.append(("pending_uint32", lambda: with_pending_uint32(99)))
    return out


@pytest.mark.parametrize("name,make", generators(), ids=[n for n, _ in generators()])
def test_next_double_at_offsets(lib, name, make):
    st = words(make().bit_generator)
    for off in OFFSETS:
        twin = make()
        twin.bit_generator.advance(off)
        if name == "pending_uint32":  # numpy's advance() drops the buffered half; the doubles never look at it
            assert twin.bit_generator.state["has_uint32"] == 0
        want = twin.random()
        got = lib.pcg64_double_at(st, off)
        assert got == want, (name, off, got, want)


@pytest.mark.parametrize("name,make", generators(), ids=[n for n, _ in generators()])
def test_consecutive_doubles(lib, name, make):
    n = 5000
    out = np.empty(n)
    lib.pcg64_doubles(words(make().bit_generator), n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert np.array_equal(out, make().random(n))


def test_large_offset_by_vector_draw(lib):
    """offset 10**7 - 1 against the vector numpy actually draws (not through numpy's own advance)"""
    for seed in SEEDS[:3]:
        want = np.random.default_rng(seed).random(10**7)[-1]
        assert lib.pcg64_double_at(words(np.random.default_rng(seed).bit_generator), 10**7 - 1) == want


@pytest.mark.parametrize("seed", SEEDS)
def test_stride_form_equals_single_steps(lib, seed):
    T, steps = 256, 1000
    st = words(np.random.default_rng(seed).bit_generator)
    hop = np.empty(steps, dtype=np.uint64)
    one = np.empty(T * steps, dtype=np.uint64)
    pu = ctypes.POINTER(ctypes.c_uint64)
    lib.pcg64_stride_walk(st, T, steps, hop.ctypes.data_as(pu))
    lib.pcg64_single_steps(st, T * steps, one.ctypes.data_as(pu))
    assert np.array_equal(hop, one[T - 1::T])
    # and the single steps are numpy's raw 64-bit outputs
    assert np.array_equal(one[:4096], np.random.default_rng(seed).bit_generator.random_raw(4096))


@pytest.mark.parametrize("n", [1, 63, 20000, 10**6 + 3])
def test_advance_equals_state_after_random(lib, n):
    for name, make in generators():
        g = make()
        st = words(g.bit_generator)
        g.random(n)
        after = g.bit_generator.state["state"]["state"]
        got = (ctypes.c_uint64 * 2)()
        lib.pcg64_advance(st, n, got)
        assert (int(got[0]) << 64) | int(got[1]) == after, (name, n)


def test_pending_uint32_survives_random_but_not_advance():
    """What the host layer has to restore: random(n) keeps a buffered 32-bit half, bit_generator.advance(n) drops it."""
    a, b = with_pending_uint32(5), with_pending_uint32(5)
    a.random(100)
    b.bit_generator.advance(100)
    sa, sb = a.bit_generator.state, b.bit_generator.state
    assert sa["state"] == sb["state"]
    assert sa["has_uint32"] == 1 and sb["has_uint32"] == 0

"""The scratch layout of getdist_amd/csrc/scratchplan.hpp, on the host: the header compiles with g++ as it does with hipcc,
against a stub of the allocation call.  Offsets and totals are checked against prefix sums computed here."""
import os
import signal
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
COUNTS = [0, 1, 255, 256, 257, 4096, (1 << 33) + 1]
TYPES = {"char": (1, 0), "short": (2, 256), "int": (4, 512), "double": (8, 64), "rec24": (24, 0)}  # name: (sizeof, pad)
GD_ERR_NOMEM = -2


def up(b):
    return (b + 255) // 256 * 256


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(HERE, "native", "scratchplan_check.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "scratchplan_check")
        subprocess.run(["g++", "-O2", "-std=c++17", src, "-o", path], check=True)
        yield path


def test_offsets_are_prefix_sums_of_sizes_rounded_up_to_256(exe):
    r = subprocess.run([exe, "layout"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    bufs, totals, rest = {}, {}, {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "buf":
            bufs.setdefault(f[1], []).append((int(f[2]), int(f[3]), int(f[4])))
        elif f[0] == "total":
            totals[f[1]] = (int(f[2]), int(f[3]))
        else:
            rest[f[0]] = [int(v) for v in f[1:]]
    assert set(bufs) == set(TYPES) == set(totals)
    for name, (size, pad) in TYPES.items():
        assert [(s, c) for s, c, _ in bufs[name]] == [(size, c) for c in COUNTS]
        off = 0
        for (_, count, got), nxt in zip(bufs[name], bufs[name][1:] + [None]):
            assert got == off, (name, count, got, off)
            if count == 0 and nxt is not None:
                assert nxt[2] == got  # a zero-sized buffer shares its successor's offset
            off += up(count * size)
        assert totals[name] == (pad, off + pad)
    assert rest["big"] == [1 << 34]  # take<double>(1 << 31): no 32-bit wrap
    # tail<int>(3) behind take<int>(3): 12 bytes, not rounded; the sub-layout sits behind one rounded byte of the outer block
    assert rest["tail"] == [256, 256 + 12, 256 + 256 + 12]


@pytest.mark.parametrize("mode", [["fail"], ["fail", "zero-sized"], ["early"], ["unbound"]])
def test_a_buffer_without_a_block_stops_in_the_assert(exe, mode):
    r = subprocess.run([exe] + mode, capture_output=True, text=True)
    assert r.returncode == -signal.SIGABRT, (r.returncode, r.stdout, r.stderr)
    assert "unreachable" not in r.stdout
    assert "scratch buffer used before ScratchPlan::get" in r.stderr
    if mode[0] == "fail":  # the failing allocation came back as the error code, from either block
        assert r.stdout.split() == ["rc", str(GD_ERR_NOMEM), str(GD_ERR_NOMEM)]

"""Builds the host-only (g++) harness of getdist_amd/csrc/fmtdouble.hpp on demand: load() returns a ctypes handle with
prototypes, sanitizer_program() the path of the stand-alone AddressSanitizer/UBSan executable (None when g++ has no
sanitizer runtime here), format_array() formats a vector of doubles the way the device kernels do."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libfmt_harness.so")
EXE = os.path.join(HERE, "fmt_harness_asan")
SRC = os.path.join(HERE, "fmt_harness.cpp")
CSRC = os.path.join(HERE, "..", "..", "getdist_amd", "csrc")
HEADERS = [os.path.join(CSRC, "fmtdouble.hpp"), os.path.join(CSRC, "fmtdouble_pow10.inc")]

_lib = None


def _stale(target):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(f) for f in [SRC] + HEADERS)


def load():
    global _lib
    if _lib is not None:
        return _lib
    for h in HEADERS:
        if not os.path.exists(h):
            raise FileNotFoundError(h)
    if _stale(SO):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", SRC, "-o", SO], check=True)
    lib = ctypes.CDLL(SO)
    pu64, pc = ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p
    lib.fmt_array.restype = ctypes.c_int64
    lib.fmt_array.argtypes = [pu64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, pc, ctypes.c_int64,
                              ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)]
    lib.fmt_array_slow.restype = ctypes.c_int64
    lib.fmt_array_slow.argtypes = [pu64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, pc, ctypes.c_int64]
    _lib = lib
    return lib


def sanitizer_program():
    """Path of the stand-alone sanitizer build of the harness, or None when it cannot be linked here."""
    if _stale(EXE):
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DFMT_HARNESS_MAIN", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", SRC, "-o", EXE], capture_output=True, text=True)
        if r.returncode != 0:
            if "asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr:
                return None
            raise RuntimeError(r.stderr)
    return EXE


def format_array(bits, width, prec, upper, tail=-1, slow=False):
    """(bytes, values that left the fast path) of the uint64 patterns ``bits`` as "%W.P{e|E}", each followed by the byte
    ``tail`` when it is >= 0.  ``slow`` sends every finite non-zero value through the exact path."""
    lib = load()
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    room = (max(width, prec + 8) + 1) * max(bits.size, 1)
    out = np.empty(room, dtype=np.uint8)
    pb = bits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    if slow:
        n = lib.fmt_array_slow(pb, bits.size, width, prec, int(upper), tail, out.ctypes.data, room)
        taken = bits.size
    else:
        cnt = ctypes.c_int64(0)
        n = lib.fmt_array(pb, bits.size, width, prec, int(upper), tail, out.ctypes.data, room, None, ctypes.byref(cnt))
        taken = cnt.value
    if n < 0:
        raise RuntimeError("a value exceeded max(width, prec + 8) bytes")
    return out[:n].tobytes(), taken

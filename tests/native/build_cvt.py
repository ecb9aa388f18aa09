"""Builds the host-only (g++) harness of getdist_amd/csrc/cvtfloat.hpp on demand: load() returns a ctypes handle with
prototypes, sanitizer_program() the path of the stand-alone AddressSanitizer/UBSan executable (None when g++ has no
sanitizer runtime here), convert() narrows a vector of double bit patterns the way the device kernels do."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libcvt_harness.so")
EXE = os.path.join(HERE, "cvt_harness_asan")
SRC = os.path.join(HERE, "cvt_harness.cpp")
HEADERS = [os.path.join(HERE, "..", "..", "getdist_amd", "csrc", "cvtfloat.hpp")]

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
    lib.cvt_array.restype = None
    lib.cvt_array.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    _lib = lib
    return lib


def sanitizer_program():
    """Path of the stand-alone sanitizer build of the harness, or None when it cannot be linked here."""
    if _stale(EXE):
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DCVT_HARNESS_MAIN", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", SRC, "-o", EXE], capture_output=True, text=True)
        if r.returncode != 0:
            if "asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr:
                return None
            raise RuntimeError(r.stderr)
    return EXE


def convert(bits):
    """(fp16 bits, bf16 bits, fp32 bits) of the uint64 patterns ``bits``"""
    lib = load()
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    f16, bf16, f32 = np.empty(bits.size, np.uint16), np.empty(bits.size, np.uint16), np.empty(bits.size, np.uint32)
    lib.cvt_array(bits.ctypes.data, bits.size, f16.ctypes.data, bf16.ctypes.data, f32.ctypes.data)
    return f16, bf16, f32

"""Builds the host-only (g++) harness of getdist_amd/csrc/pcg64.hpp on demand; returns a ctypes handle with prototypes."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libpcg64_harness.so")
SRC = os.path.join(HERE, "pcg64_harness.cpp")
HEADER = os.path.join(HERE, "..", "..", "getdist_amd", "csrc", "pcg64.hpp")


def load():
    if not os.path.exists(HEADER):
        raise FileNotFoundError(HEADER)
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(HEADER)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", SRC, "-o", SO], check=True)
    lib = ctypes.CDLL(SO)
    pu64 = ctypes.POINTER(ctypes.c_uint64)
    lib.pcg64_double_at.restype = ctypes.c_double
    lib.pcg64_double_at.argtypes = [pu64, ctypes.c_uint64]
    lib.pcg64_doubles.restype = None
    lib.pcg64_doubles.argtypes = [pu64, ctypes.c_int64, ctypes.POINTER(ctypes.c_double)]
    lib.pcg64_advance.restype = None
    lib.pcg64_advance.argtypes = [pu64, ctypes.c_uint64, pu64]
    lib.pcg64_stride_walk.restype = None
    lib.pcg64_stride_walk.argtypes = [pu64, ctypes.c_uint64, ctypes.c_int64, pu64]
    lib.pcg64_single_steps.restype = None
    lib.pcg64_single_steps.argtypes = [pu64, ctypes.c_int64, pu64]
    return lib

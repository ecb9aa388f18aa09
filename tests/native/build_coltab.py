"""Builds the host-only (g++) harness of the table look-ups of getdist_amd/csrc/colexpr.hpp on demand; returns a ctypes
handle with prototypes."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libcoltab_harness.so")
SRC = os.path.join(HERE, "coltab_harness.cpp")
HEADERS = [os.path.join(HERE, "..", "..", "getdist_amd", "csrc", "colexpr.hpp"),
           os.path.join(HERE, "..", "..", "include", "gdhip.h")]


def load():
    for h in HEADERS:
        if not os.path.exists(h):
            raise FileNotFoundError(h)
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + HEADERS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", SRC, "-o", SO], check=True)
    lib = ctypes.CDLL(SO)
    pi32, pd, i32, i64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double), ctypes.c_int32, ctypes.c_int64
    pt = ctypes.c_void_p  # gd_expr_table*: _lib.expr_table_structs or a hand-made _lib.GdExprTable array
    lib.coltab_check.restype = ctypes.c_char_p
    lib.coltab_check.argtypes = [pi32, i32, pd, i32, i64, pt, i32]
    lib.coltab_depth.restype = i32
    lib.coltab_depth.argtypes = [pi32, i32, pd, i32, i64, pt, i32]
    lib.coltab_run.restype = i32
    lib.coltab_run.argtypes = [pi32, i32, pd, i32, i64, pd, pd, i64, pd, pt, i32]
    lib.coltab_rows.restype = None
    lib.coltab_rows.argtypes = [pt, pd, pd, i64, pd]
    lib.coltab_upper.restype = i32
    lib.coltab_upper.argtypes = [pd, i32, i32, ctypes.c_double]
    return lib

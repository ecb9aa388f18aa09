"""Builds the host-only (g++) harness of the preparation tail on demand; returns its ctypes handle."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libprepare_harness.so")
SRC = os.path.join(HERE, "prepare_harness.cpp")
DEPS = [os.path.join(HERE, "..", "..", "getdist_amd", "csrc", "batch2d.hpp"), os.path.join(HERE, "..", "..", "include", "gdhip.h")]


def load():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", SRC, "-o", SO, "-pthread"], check=True)
    return ctypes.CDLL(SO)

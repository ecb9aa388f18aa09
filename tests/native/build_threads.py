"""Builds tests/native/batch_threads_main.cpp -- the stand-alone thread test of batch2d.hpp's choreography -- on demand, once
per sanitizer: programs() returns {"thread": path, "address": path} of two plain executables."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "batch_threads_main.cpp")
CSRC = os.path.join(HERE, "..", "..", "getdist_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "batch2d.hpp"), os.path.join(HERE, "..", "..", "include", "gdhip.h")]
KINDS = {"thread": ["-fsanitize=thread"], "address": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def programs():
    out = {}
    for kind, flags in KINDS.items():
        exe = os.path.join(HERE, "batch_threads_" + kind)
        if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in DEPS):
            subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread"] + flags + [SRC, "-o", exe], check=True)
        out[kind] = exe
    return out

"""Builds the host-only (g++) harness of getdist_amd/csrc/parsedouble.hpp on demand: load() returns a ctypes handle with
prototypes, sanitizer_program() the path of the stand-alone AddressSanitizer/UBSan executable (None when g++ has no
sanitizer runtime here), parse_tokens() parses a list of tokens the way the device kernels do."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libparse_harness.so")
EXE = os.path.join(HERE, "parse_harness_asan")
SRC = os.path.join(HERE, "parse_harness.cpp")
CSRC = os.path.join(HERE, "..", "..", "getdist_amd", "csrc")
HEADERS = [os.path.join(CSRC, "parsedouble.hpp"), os.path.join(CSRC, "fmtdouble.hpp"), os.path.join(CSRC, "fmtdouble_pow10.inc")]

DECIDED, UNDECIDED, NOT_A_NUMBER = 0, 1, 2

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
    pc = ctypes.c_void_p
    lib.parse_lines.restype = ctypes.c_int64
    lib.parse_lines.argtypes = [pc, ctypes.c_int64, ctypes.c_int64, pc, pc]
    lib.check_lines.restype = ctypes.c_int64
    lib.check_lines.argtypes = [pc, ctypes.c_int64, ctypes.c_int64, pc]
    _lib = lib
    return lib


def sanitizer_program():
    """Path of the stand-alone sanitizer build of the harness, or None when it cannot be linked here."""
    if _stale(EXE):
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DPARSE_HARNESS_MAIN", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", SRC, "-o", EXE], capture_output=True, text=True)
        if r.returncode != 0:
            if "asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr:
                return None
            raise RuntimeError(r.stderr)
    return EXE


def parse_tokens(tokens):
    """(uint64 bits, uint8 verdicts, grammar-ok flags) of ``tokens``: a list of bytes objects without '\\n', or one bytes
    object holding a token per line (each line ended by '\\n')."""
    lib = load()
    if isinstance(tokens, (bytes, bytearray)):
        text = bytes(tokens)
        n = text.count(b"\n")
    else:
        n = len(tokens)
        text = b"\n".join(tokens) + b"\n" if n else b""
    bits = np.zeros(n, dtype=np.uint64)
    verdict = np.zeros(n, dtype=np.uint8)
    ok = np.zeros(n, dtype=np.uint8)
    buf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
    assert lib.parse_lines(buf.ctypes.data, len(text), n, bits.ctypes.data, verdict.ctypes.data) == n
    assert lib.check_lines(buf.ctypes.data, len(text), n, ok.ctypes.data) == n
    return bits, verdict, ok.astype(bool)

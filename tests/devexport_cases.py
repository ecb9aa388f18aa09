"""Shared by the CPU and GPU tests of device-array output (getDeviceSamples, gd_export_device, csrc/cvtfloat.hpp): the
targeted values of the narrowing conversions, the exact bf16 model they are held to, and the host statement of an export."""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

FLT_MAX = float(np.finfo(np.float32).max)


def targeted_values():
    """float64 values at the edges of the three narrowings: fp16 ties and the double-rounding traps, the fp16 overflow edge,
    the fp16 / fp32 subnormal ranges, the bf16 ties, zeros, infinities and NaNs of both signs"""
    v = [1 + 2.0**-11 + 2.0**-40, 1 + 2.0**-11 - 2.0**-40, 1 + 2.0**-11, 1 + 3 * 2.0**-11, 65519.999, 65520.0, 65504.0,
         2.0**-25, 2.0**-25 * (1 + 2.0**-30), 2.0**-24, 3 * 2.0**-25, 6e-8, 1e-40, 1e-45, 7e-46, FLT_MAX, FLT_MAX * (1 + 2.0**-25),
         FLT_MAX * (1 + 2.0**-24), 0.0, np.inf, 1 + 2.0**-8, 1 + 3 * 2.0**-8, 1 + 2.0**-8 + 2.0**-50, 1 + 2.0**-8 - 2.0**-50,
         2.0**-133, 2.0**-134, 2.0**-134 * (1 + 2.0**-40), 2.0**-126 * (1 - 2.0**-9), 3.3895313892515355e38, 3.4e38, 1e-310, 1e308]
    v = np.array(v, dtype=np.float64)
    nan = np.array([0x7FF8000000000000, 0xFFF8000000000000], dtype=np.uint64).view(np.float64)
    return np.concatenate([v, -v, nan])


def bf16_model_one(b):
    """bf16 bits of the double with bit pattern ``b``, by the exact remainder in Python integers: |x| = M 2^-1074, the
    result's grid is 2^g with g = max(floor(log2 |x|), -126) - 7, the quotient of M by the grid unit is rounded half to
    even and encoded from its VALUE.  (NaN: quiet, sign kept, top payload bits.)"""
    sign = (b >> 63) << 15
    e, frac = (b >> 52) & 0x7FF, b & ((1 << 52) - 1)
    if e == 0x7FF:
        return sign | 0x7F80 | ((0x40 | (frac >> 45)) if frac else 0)
    M = frac if e == 0 else (frac | (1 << 52)) << (e - 1)
    if M == 0:
        return sign
    g = max(M.bit_length() - 1 - 1074, -126) - 7
    unit = 1 << (g + 1074)
    q, r = divmod(M, unit)
    if 2 * r > unit or (2 * r == unit and q & 1):
        q += 1
    if q == 0:
        return sign
    top = q.bit_length() - 1 + g  # floor(log2) of the rounded value
    if top > 127:
        return sign | 0x7F80
    if top < -126:
        return sign | q  # subnormal: g == -133, q < 128
    return sign | ((top + 127) << 7) | (((q << 7) >> (q.bit_length() - 1)) & 0x7F)


def bf16_model(x):
    """uint16 bf16 patterns of the float64 array ``x`` (any shape)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    flat = x.reshape(-1).view(np.uint64)
    return np.array([bf16_model_one(int(b)) for b in flat], dtype=np.uint16).reshape(x.shape)


def narrowed(x, dtype):
    """``x`` in the element type ``dtype`` (a numpy float type or "bfloat16") as the BITS an export must give"""
    if isinstance(dtype, str) and dtype == "bfloat16":
        return bf16_model(x)
    dt = np.dtype(dtype)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        out = np.asarray(x, dtype=np.float64).astype(dt)
    return out.view({8: np.uint64, 4: np.uint32, 2: np.uint16}[dt.itemsize])


def sample_values(N, n, seed=3):
    """(N, n) float64 samples whose rows and columns differ, with the targeted values scattered over them"""
    r = np.random.default_rng(seed)
    x = r.standard_normal((N, n)) * np.exp(r.uniform(-12, 12, (N, n)))
    t = targeted_values()
    t = t[~np.isnan(t)] if N * n < 8 else t
    k = min(t.size, x.size)
    where = r.choice(x.size, size=k, replace=False)
    x.reshape(-1)[where] = t[:k]
    return x

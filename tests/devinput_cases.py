"""Shared by the CPU and GPU tests of device-array input (getdist_amd/devarray.py, gd_upload_device): a buffer that
exposes ``__cuda_array_interface__`` for any numpy view, and the views the kernel's paths are chosen by.

``DevBuf(a, feeder)`` puts the bytes the numpy array ``a`` touches on the device through ``feeder`` -- a SECOND Context,
``alloc`` then the synchronous gd_memcpy_h2d -- and describes them with ``a``'s shape, strides and offset, so the GPU tier
needs no torch.  With ``feeder=None`` the interface points at ``a``'s host memory: the CPU tier's stand-in, read back by
its context double through ctypes."""

import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def byte_span(a):
    """(lowest, one past the highest) byte of ``a``'s elements relative to its first one"""
    if a.size == 0:
        return 0, 0
    lo = hi = 0
    for extent, stride in zip(a.shape, a.strides):
        reach = (extent - 1) * stride
        lo, hi = lo + min(reach, 0), hi + max(reach, 0)
    return lo, hi + a.itemsize


class DevBuf:
    def __init__(self, a, feeder=None, version=3, stream=None, with_strides=None):
        a = np.asarray(a)
        assert a.dtype in (np.float64, np.float32, np.float16)
        self.host = a  # (kept alive: with feeder=None the interface points into it)
        lo, hi = byte_span(a)
        if feeder is None:
            self.block, ptr = None, a.ctypes.data
        else:
            raw = np.frombuffer((ctypes.c_ubyte * max(hi - lo, 1)).from_address(a.ctypes.data + lo), dtype=np.uint8)
            self.block = feeder.alloc(max(hi - lo, 8))
            self.block.from_host(raw[:hi - lo].copy())
            ptr = self.block.ptr - lo
        contiguous = a.flags.c_contiguous if with_strides is None else not with_strides
        self.__cuda_array_interface__ = dict(shape=a.shape, typestr=a.dtype.str, data=(ptr, False), version=version,
                                             strides=None if contiguous else a.strides)
        if version >= 3:
            self.__cuda_array_interface__["stream"] = stream


def block(dtype=np.float64, seed=7):
    """the (600, 52) block the views below are cut from: values exact in fp16, so that every element type holds the same"""
    r = np.random.default_rng(seed)
    return (r.integers(-2048, 2048, (600, 52)) / 8.0).astype(dtype)


def views(x):
    """name -> view of the (600, 52) block ``x`` (none owns its memory)"""
    return {
        "cols_1_51": x[:, 1:51],              # misaligned base for fp32, row_stride > n
        "every_other_row": x[::2],
        "rows_from_5": x[5:, :],
        "transposed": x.T,                    # (52, 600): row_stride 1
        "stride0_column": np.lib.stride_tricks.as_strided(x, shape=(600, 52), strides=(x.strides[0], 0)),
        "stride0_rows": np.lib.stride_tricks.as_strided(x, shape=(40, 52), strides=(0, x.strides[1])),
    }


def values(rows, cols, dtype=np.float64):
    """(rows, cols) values that tell their row and column apart, exact in fp16"""
    r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    return (((r * 37 + c * 101) % 2039) / 8.0 - 100.0).astype(dtype)

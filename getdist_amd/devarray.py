"""
Device arrays as input: what MCSamples needs to know about a ``torch.Tensor`` on the GPU or any object with
``__cuda_array_interface__`` (CuPy, numba) to hand it to gd_upload_device -- pointer, shape, strides in elements, element
type, device and producer stream.  Nothing here imports torch or CuPy: the objects are recognised by their attributes.

Out of scope: handing the resident columns OUT as device arrays (their lifetime across re-uploads needs a design of its
own), device row compaction, integer element types.
"""

import ctypes
import sys

import numpy as np

GD_DT_F64, GD_DT_F32, GD_DT_F16, GD_DT_BF16 = 0, 1, 2, 3
ITEMSIZE = {GD_DT_F64: 8, GD_DT_F32: 4, GD_DT_F16: 2, GD_DT_BF16: 2}
_NUMPY_TYPE = {GD_DT_F64: np.float64, GD_DT_F32: np.float32, GD_DT_F16: np.float16}
_TORCH_TYPES = {"torch.float64": GD_DT_F64, "torch.float32": GD_DT_F32, "torch.float16": GD_DT_F16,
                "torch.bfloat16": GD_DT_BF16}
STREAM_LEGACY, STREAM_PER_THREAD = 1, 2  # the interface's codes for the two default streams; gd_upload_device takes them as is


class DevArray:
    """Descriptor of a device array.  ``strides`` are in elements; ``stream`` is None (no ordering needed), STREAM_LEGACY,
    STREAM_PER_THREAD or a stream handle; ``device`` is None where the container does not say (the library then checks
    the pointer itself); ``owner`` keeps the described object alive."""

    __slots__ = ("ptr", "shape", "strides", "dtype", "device", "stream", "owner")

    def __init__(self, ptr, shape, strides, dtype, device=None, stream=None, owner=None):
        self.ptr, self.shape, self.strides = int(ptr), tuple(int(v) for v in shape), tuple(int(v) for v in strides)
        self.dtype, self.device, self.stream, self.owner = dtype, device, stream, owner

    ndim = property(lambda self: len(self.shape))
    itemsize = property(lambda self: ITEMSIZE[self.dtype])

    def _with(self, ptr, shape, strides):
        return DevArray(ptr, shape, strides, self.dtype, self.device, self.stream, self.owner)

    def as2d(self):
        """(N,) -> (N, 1); 2-D as it is"""
        if self.ndim == 1:
            return self._with(self.ptr, self.shape + (1,), self.strides + (1,))
        if self.ndim != 2:
            raise ValueError("a device sample array must have one or two dimensions, not %d" % self.ndim)
        return self

    def rows_from(self, start):
        """the rows [start:] (the base pointer moves, the row count shrinks)"""
        start = min(max(int(start), 0), self.shape[0])
        return self._with(self.ptr + start * self.strides[0] * self.itemsize, (self.shape[0] - start,) + self.shape[1:],
                          self.strides)

    def row(self, i):
        """row i of a 2-D array, as a 1 x n array"""
        i = i % self.shape[0]
        return self._with(self.ptr + i * self.strides[0] * self.itemsize, (1, self.shape[1]), self.strides)

    def column(self, j):
        """column j of a 2-D array, as an N x 1 array"""
        return self._with(self.ptr + j * self.strides[1] * self.itemsize, (self.shape[0], 1), self.strides)

    def span(self):
        """(lowest, one past the highest) byte the array touches, relative to ``ptr``; (0, 0) for an empty array"""
        if any(v == 0 for v in self.shape):
            return 0, 0
        lo = hi = 0
        for extent, stride in zip(self.shape, self.strides):
            reach = (extent - 1) * stride * self.itemsize
            lo, hi = lo + min(reach, 0), hi + max(reach, 0)
        return lo, hi + self.itemsize

    def forward(self):
        """(array with every negative stride turned round, the axes that were): the same elements, read from the other end"""
        ptr, strides, flipped = self.ptr, list(self.strides), []
        for ax, (extent, stride) in enumerate(zip(self.shape, self.strides)):
            if stride < 0 and extent > 0:
                ptr += (extent - 1) * stride * self.itemsize
                strides[ax] = -stride
                flipped.append(ax)
        return self._with(ptr, self.shape, strides), flipped


def host_view(desc):
    """A numpy view of the described memory, for memory the HOST can address (page-locked or managed memory that
    gd_upload_device declines; the CPU tests' stand-in for device memory)."""
    if desc.dtype not in _NUMPY_TYPE:
        raise TypeError("bfloat16 memory cannot be viewed from numpy: convert with .to(torch.float32)")
    lo, hi = desc.span()
    if hi == lo:
        return np.empty(desc.shape, dtype=_NUMPY_TYPE[desc.dtype])
    raw = (ctypes.c_ubyte * (hi - lo)).from_address(desc.ptr + lo)
    flat = np.frombuffer(raw, dtype=np.uint8)
    byte_strides = tuple(s * desc.itemsize for s in desc.strides)
    return np.ndarray(desc.shape, dtype=_NUMPY_TYPE[desc.dtype], buffer=flat, offset=-lo, strides=byte_strides)


def _unsupported(kind, name):
    return TypeError("%s of element type %s are not taken from the device: convert to a float type first "
                     "(x.astype(numpy.float64) / x.to(torch.float64); float64, float32, float16 and bfloat16 are)" % (kind, name))


def _describe_torch(obj):
    t = obj.detach()
    dtype = _TORCH_TYPES.get(str(t.dtype))
    if dtype is None:
        raise _unsupported("torch tensors", str(t.dtype))
    torch = sys.modules[type(obj).__module__.split(".")[0]]  # the module the tensor's type came from
    index = t.device.index
    if index is None:
        index = torch.cuda.current_device()
    handle = int(torch.cuda.current_stream(t.device).cuda_stream)
    return DevArray(t.data_ptr(), tuple(t.shape), tuple(t.stride()), dtype, int(index), handle or STREAM_LEGACY, t)


def _describe_interface(obj, cai):
    version = int(cai.get("version", 0))
    if version < 2:
        raise TypeError("__cuda_array_interface__ version %d is not supported (2 and 3 are)" % version)
    try:
        dt = np.dtype(cai["typestr"])
    except TypeError:
        raise _unsupported("device arrays", repr(cai["typestr"])) from None
    code = {8: GD_DT_F64, 4: GD_DT_F32, 2: GD_DT_F16}.get(dt.itemsize) if dt.kind == "f" and dt.isnative else None
    if code is None:
        raise _unsupported("device arrays", repr(cai["typestr"]))
    shape = tuple(int(v) for v in cai["shape"])
    strides = cai.get("strides")
    if strides is None:  # C-contiguous
        strides, run = [], 1
        for extent in reversed(shape):
            strides.append(run)
            run *= max(extent, 1)
        strides = tuple(reversed(strides))
    else:
        if any(int(s) % dt.itemsize for s in strides):
            raise TypeError("device array strides %r are not multiples of its %d-byte elements" % (tuple(strides), dt.itemsize))
        strides = tuple(int(s) // dt.itemsize for s in strides)
    stream = cai.get("stream")  # (absent in version 2)
    if stream is not None:
        stream = int(stream)
        if stream == 0:  # not allowed by the interface; ordering behind the default stream is always safe
            stream = STREAM_LEGACY
    return DevArray(cai["data"][0] or 0, shape, strides, code, None, stream, obj)


def describe(obj):
    """The DevArray of a device array, None for anything that is not one (numpy arrays, lists, CPU tensors: those go on
    through np.asarray).  TypeError for a device array of an element type that is not served (integers, complex)."""
    if isinstance(obj, DevArray):
        return obj
    if isinstance(obj, (np.ndarray, list, tuple, str, bytes, int, float)) or obj is None:
        return None
    is_cuda = getattr(obj, "is_cuda", None)
    if isinstance(is_cuda, bool) and all(hasattr(obj, a) for a in ("data_ptr", "stride", "dtype", "device", "detach")):
        return _describe_torch(obj) if is_cuda else None
    cai = getattr(obj, "__cuda_array_interface__", None)
    if isinstance(cai, dict):
        return _describe_interface(obj, cai)
    return None

"""
Device arrays as input and as output.

In: what MCSamples needs to know about a ``torch.Tensor`` on the GPU or any object with ``__cuda_array_interface__`` (CuPy,
numba) to hand it to gd_upload_device -- pointer, shape, strides in elements, element type, device and producer stream.

Out: :class:`DeviceArray`, the owning result of ``getDeviceSamples`` / ``getDeviceWeights`` (gd_export_device).  An export is
a SNAPSHOT, never an alias of the resident columns: the values are copied device to device into memory the sample set does
not own, so every mutator and re-upload stays free to replace the resident set, and the array stays valid after the sample
set and its context are gone.

Nothing here imports torch or CuPy: the objects are recognised by their attributes.  Out of scope: integer element types,
DLPack capsules, zero-copy views of the resident columns.
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


DTYPE_NAMES = {"float64": GD_DT_F64, "float32": GD_DT_F32, "float16": GD_DT_F16, "bfloat16": GD_DT_BF16}
_TYPESTR = {GD_DT_F64: "<f8", GD_DT_F32: "<f4", GD_DT_F16: "<f2", GD_DT_BF16: "<i2"}  # (the interface has no bfloat16)


def dtype_code(dtype):
    """The GD_DT_* code of ``dtype``: a numpy float type (or its name), a torch dtype, or "bfloat16" """
    name = dtype if isinstance(dtype, str) else str(dtype)
    if name in _TORCH_TYPES:
        return _TORCH_TYPES[name]
    if name not in DTYPE_NAMES:
        try:
            name = np.dtype(dtype).name
        except TypeError:
            pass
    if name not in DTYPE_NAMES:
        raise ValueError("dtype must be float64, float32, float16 or \"bfloat16\", not %r" % (dtype,))
    return DTYPE_NAMES[name]


class DeviceArray:
    """A 1-D or 2-D array in device memory that owns its block (``block``: anything with ``ptr``, ``device`` and
    ``fetch(host_array)``, which frees the memory when its last reference goes: _lib.ExportBlock).  ``strides`` are in
    elements; ``dtype`` is a numpy dtype, for bfloat16 the string "bfloat16".  ``stream`` is what the interface dictionary
    announces: None for an array that was complete before it was returned."""

    def __init__(self, block, shape, strides, code, stream=None):
        self.block, self.shape, self.strides = block, tuple(int(v) for v in shape), tuple(int(v) for v in strides)
        self.code, self.stream = code, stream

    @classmethod
    def allocate(cls, ctx, shape, code, order="C"):
        """A new array of ``shape`` in C or Fortran order, in memory from ``ctx.export_block`` (owned by the array alone)"""
        shape = tuple(int(v) for v in shape)
        if order not in ("C", "F"):
            raise ValueError("order must be 'C' or 'F'")
        strides, run = [], 1
        for extent in (reversed(shape) if order == "C" else shape):
            strides.append(run)
            run *= max(extent, 1)
        strides = tuple(reversed(strides)) if order == "C" else tuple(strides)
        size = int(np.prod(shape)) if shape else 1
        return cls(ctx.export_block(size * ITEMSIZE[code]), shape, strides, code)

    ptr = property(lambda self: self.block.ptr)
    device = property(lambda self: self.block.device)
    ndim = property(lambda self: len(self.shape))
    size = property(lambda self: int(np.prod(self.shape)) if self.shape else 1)
    itemsize = property(lambda self: ITEMSIZE[self.code])
    nbytes = property(lambda self: self.size * self.itemsize)
    dtype = property(lambda self: np.dtype(_NUMPY_TYPE[self.code]) if self.code in _NUMPY_TYPE else "bfloat16")

    @property
    def __cuda_array_interface__(self):
        return dict(shape=self.shape, typestr=_TYPESTR[self.code], data=(self.ptr if self.size else 0, False), version=3,
                    strides=tuple(s * self.itemsize for s in self.strides), stream=self.stream)

    def describe(self):
        """the DevArray of this array (it keeps the array, and so the memory, alive)"""
        return DevArray(self.ptr, self.shape, self.strides, self.code, self.device, self.stream, self)

    def numpy(self):
        """A host copy in the array's shape and order; bfloat16 comes back as its uint16 bit patterns."""
        dt = _NUMPY_TYPE.get(self.code, np.uint16)
        flat = np.empty(self.size, dtype=dt)
        if self.size:
            self.block.fetch(flat)
        fortran = self.ndim == 2 and self.strides[0] == 1 and self.shape[1] > 1
        return flat.reshape(self.shape[::-1]).T if fortran else flat.reshape(self.shape)

    def torch(self):
        """The same memory as a torch tensor (no copy; the tensor keeps this array alive).  torch is not imported here: the
        ``torch`` the process has already imported is used."""
        torch = sys.modules.get("torch")
        if torch is None:
            raise RuntimeError("DeviceArray.torch(): import torch first (before the first sample set is made)")
        t = torch.as_tensor(self, device="cuda:%d" % self.device)
        return t.view(torch.bfloat16) if self.code == GD_DT_BF16 else t


def describe(obj):
    """The DevArray of a device array, None for anything that is not one (numpy arrays, lists, CPU tensors: those go on
    through np.asarray).  TypeError for a device array of an element type that is not served (integers, complex)."""
    if isinstance(obj, DevArray):
        return obj
    if isinstance(obj, DeviceArray):
        return obj.describe()
    if isinstance(obj, (np.ndarray, list, tuple, str, bytes, int, float)) or obj is None:
        return None
    is_cuda = getattr(obj, "is_cuda", None)
    if isinstance(is_cuda, bool) and all(hasattr(obj, a) for a in ("data_ptr", "stride", "dtype", "device", "detach")):
        return _describe_torch(obj) if is_cuda else None
    cai = getattr(obj, "__cuda_array_interface__", None)
    if isinstance(cai, dict):
        return _describe_interface(obj, cai)
    return None

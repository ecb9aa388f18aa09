"""Child process of tests/test_gpu_devexport.py: the resident samples handed to torch.  torch is imported FIRST: once
libgdhip.so has loaded the system HIP runtime, a later ``import torch`` reports no GPU."""

import os
import sys

try:
    import torch
except ImportError:
    print("NO_TORCH")
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import devexport_cases as xc  # noqa: E402
from getdist_amd.mcsamples import MCSamples  # noqa: E402


def main():
    assert torch.cuda.is_available(), "torch, imported first, sees no GPU"
    r = np.random.default_rng(6)
    x = r.standard_normal((4099, 7)) * 3.0 + 1.0
    w = r.integers(1, 4, 4099).astype(float)
    s = MCSamples(samples=x, weights=w, names=["p%d" % k for k in range(7)])
    p = s.getDeviceParams()
    keep = x[:, 0] > 1.0
    want64 = np.column_stack([x[:, 2], x[:, 5], x[:, 1] * x[:, 3]])[keep]
    side, done = torch.cuda.Stream(), 0
    for stream in (side, torch.cuda.default_stream()):
        for dtype in (torch.float32, torch.bfloat16):
            with torch.cuda.stream(stream):
                # the tensor is busy on `stream` right up to the call, and read by a torch kernel right after it, no synchronize
                out = torch.empty((int(keep.sum()), 3), device="cuda", dtype=dtype)
                out.fill_(-1.0)
                assert s.getDeviceSamples(["p2", "p5", p.p1 * p.p3], rows=p.p0 > 1.0, out=out) is out
                doubled = out.to(torch.float64) * 2.0
            got = doubled.cpu().numpy()  # (the copy waits for the stream)
            if dtype == torch.float32:
                want = want64.astype(np.float32).astype(np.float64) * 2.0
            else:
                want = (xc.bf16_model(want64).astype(np.uint32) << 16).view(np.float32).astype(np.float64) * 2.0
            assert np.array_equal(got, want), (stream, dtype)
            done += 1

    # DeviceArray.torch() shares the array's memory, and the tensor keeps it alive
    a = s.getDeviceSamples(["p4", "p6"], dtype="bfloat16")
    t = a.torch()
    assert t.dtype == torch.bfloat16 and t.data_ptr() == a.ptr and tuple(t.shape) == (4099, 2)
    full = s.getDeviceSamples()
    tf = full.torch()
    assert tf.dtype == torch.float64 and tf.data_ptr() == full.ptr
    wt = s.getDeviceWeights(dtype=np.float32).torch()
    twin = MCSamples(samples=tf, weights=wt, names=["p%d" % k for k in range(7)])  # the way back in
    assert not twin._host_mirror_ready
    for j in list(range(7)) + [-2]:
        got, ref = np.empty(4099), np.empty(4099)
        for c, o in ((twin.ctx, got), (s.ctx, ref)):
            c._check(c.lib.gd_memcpy_d2h(c.h, o.ctypes.data, c.column_ptr(j), o.nbytes))
        assert np.array_equal(got, ref), j
    done += 1
    twin.ctx.close()
    s.ctx.close()
    del s, a, full, p
    torch.cuda.synchronize()
    assert np.array_equal(t.view(torch.int16).cpu().numpy().view(np.uint16), xc.bf16_model(x[:, [4, 6]]))
    assert np.array_equal(tf.cpu().numpy(), x) and np.array_equal(wt.cpu().numpy(), w.astype(np.float32))
    done += 1
    print("TORCH_EXPORT_OK %d" % done)


if __name__ == "__main__":
    main()

"""Child process of tests/test_gpu_devinput.py: torch tensors on the GPU handed to MCSamples.  torch is imported FIRST: once
libgdhip.so has loaded the system HIP runtime, a later ``import torch`` reports no GPU."""

import os
import sys

try:
    import torch
except ImportError:
    print("NO_TORCH")
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from getdist_amd.mcsamples import MCSamples  # noqa: E402


def same(dev, host, hx):
    assert not dev._host_mirror_ready
    assert (dev.numrows, dev.n) == (host.numrows, host.n) and np.array_equal(dev.weights, host.weights)
    for ctx in (dev.ctx, host.ctx):
        ctx.sync()
    for j in list(range(host.n)) + [-2]:
        got, want = np.empty(host.numrows), np.empty(host.numrows)
        for c, out in ((dev.ctx, got), (host.ctx, want)):
            c._check(c.lib.gd_memcpy_d2h(c.h, out.ctypes.data, c.column_ptr(j), out.nbytes))
        assert np.array_equal(got, want), j
    assert dev.ctx.weights_integral() == host.ctx.weights_integral() and dev.ctx.weight_stats() == host.ctx.weight_stats()
    assert np.array_equal(dev.samples, hx)


def main():
    assert torch.cuda.is_available(), "torch, imported first, sees no GPU"
    side, done = torch.cuda.Stream(), 0
    for stream in (side, torch.cuda.default_stream()):
        for dtype in (torch.bfloat16, torch.float32):
            with torch.cuda.stream(stream):
                g = torch.Generator(device="cuda").manual_seed(4)
                x = (torch.randn(4099, 7, device="cuda", generator=g, dtype=torch.float32) * 3.0 + 1.0).to(dtype)
                w = torch.rand(4099, device="cuda", generator=g, dtype=torch.float32) + 0.5
                dev = MCSamples(samples=x, weights=w)  # straight behind the kernels that produce x and w, no synchronize
            stream.synchronize()
            hx, hw = x.cpu().to(torch.float64).numpy(), w.cpu().to(torch.float64).numpy()
            host = MCSamples(samples=hx, weights=hw)
            same(dev, host, hx)
            dev.ctx.close(), host.ctx.close()
            done += 1
    print("TORCH_CASES_OK %d" % done)


if __name__ == "__main__":
    main()

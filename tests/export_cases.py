"""The inputs and calls of tests/golden/export.npz (saveAsText, saveChainsAsText, saveTextMetadata, writeCovMatrix,
writeCorrelationMatrix).  Inputs are regenerated from seeds on any box, so the golden file holds reference outputs only:
file names and file bytes.  Shared by tests/golden/make_golden_export.py and the CPU / GPU tests."""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "export.npz")


def _rng(stream):
    return np.random.default_rng(np.random.SeedSequence([20261019, stream]))


def fixtures():
    """name -> dict(samples, weights, loglikes, names, ...); ``samples`` is an array or a list of per-chain arrays"""
    out = {}
    r = _rng(1)
    out["unit"] = dict(samples=r.standard_normal((300, 3)) * [1.0, 0.01, 250.0], weights=None, loglikes=None)
    r = _rng(2)
    s = r.standard_normal((400, 4)) * [1.0, 3.0, 1e-4, 1e5] + [0.0, -2.0, 0.0, 1e5]
    out["real"] = dict(samples=s, weights=np.exp(0.5 * s[:, 0]) * r.uniform(0.3, 1.7, 400), loglikes=0.5 * np.sum(s[:, :2] ** 2, axis=1) - 3.0)
    r = _rng(3)
    lens = [150, 200, 97]
    chains = [r.standard_normal((n, 4)) * [1.0, 0.5, 2.0, 10.0] + [0.5, 0.0, -1.0, 100.0] for n in lens]
    out["chains3"] = dict(samples=chains, weights=[r.integers(1, 9, n).astype(float) for n in lens],
                          loglikes=[0.5 * np.sum(c ** 2, axis=1) for c in chains],
                          ranges={"p0": (None, 6.0), "p1": (-4.0, 4.0), "fixedp": (1.5, 1.5)},
                          labels=["\\alpha", "\\beta_1", "x", "H_0"],
                          derived=dict(name="sum01", label="\\alpha+\\beta_1", comment="sum of the first two"))
    r = _rng(4)
    s = r.standard_normal((200, 3))
    s[:, 1] *= 1e120
    s[:, 2] *= 1e-120
    s[::7, 0] = -0.0
    s[::11, 2] = 0.0
    s[5, 1], s[6, 1], s[7, 2], s[8, 2] = 9.999999995e99, 1e100, 9.999999995e-101, 1e-100
    out["extreme"] = dict(samples=[s], weights=[r.uniform(0.5, 2.0, 200)], loglikes=[r.uniform(0, 30, 200) * 1e3])
    r = _rng(5)
    chains = [r.standard_normal((n, 2)) for n in (60, 61)]
    out["labelled"] = dict(samples=chains, weights=[np.ones(60), np.ones(61)], loglikes=[np.sum(c ** 2, axis=1) for c in chains],
                           label="run A, thinned", ranges={"p1": (0.0, None)})
    r = _rng(6)
    s = r.standard_normal((250, 3)) * [1.0, 1e3, 1e-3]
    out["prec5"] = dict(samples=s, weights=r.integers(1, 5, 250).astype(float), loglikes=np.sum(s ** 2, axis=1), precision="%.5e")
    out["prec6f"] = dict(samples=s, weights=r.integers(1, 5, 250).astype(float), loglikes=np.sum(s ** 2, axis=1), precision="%.6f")
    for f in out.values():
        first = f["samples"][0] if isinstance(f["samples"], list) else f["samples"]
        f["names"] = ["p%d" % i for i in range(first.shape[1])]
    return out


PROPS = {"burn_removed": True, "sampler_steps": 12345, "note": "from export_cases"}

# the calls made on each fixture
CALLS_FOR = {
    "unit": ["save", "save_index1", "save_txt_suffix"],
    "real": ["save", "save_index0", "matrices"],
    "chains3": ["chains", "save", "matrices"],
    "extreme": ["chains"],
    "labelled": ["chains_properties", "metadata_steps"],
    "prec5": ["save"],
    "prec6f": ["save"],
}


def all_cases():
    for fx, calls in CALLS_FOR.items():
        for call in calls:
            yield fx, call


def build(cls, fx, **kw):
    """The fixture as an MCSamples of class ``cls`` (the reference's or this package's; kw: e.g. _context_factory)."""
    f = fixtures()[fx]
    for key in ("ranges", "labels", "label"):
        if key in f:
            kw[key] = f[key]
    samples = [np.ascontiguousarray(c) for c in f["samples"]] if isinstance(f["samples"], list) else np.ascontiguousarray(f["samples"])
    mc = cls(samples=samples, weights=f["weights"], loglikes=f["loglikes"], names=f["names"], **kw)
    if "derived" in f:
        d = f["derived"]
        mc.addDerived(mc.samples[:, 0] + mc.samples[:, 1], d["name"], label=d["label"], comment=d["comment"])
    if "precision" in f:
        mc.precision = f["precision"]
    return mc


def _files(folder):
    out = {}
    for dirpath, _, names in os.walk(folder):
        for nm in names:
            full = os.path.join(dirpath, nm)
            with open(full, "rb") as f:
                out[os.path.relpath(full, folder).replace(os.sep, "/")] = f.read()
    return out


def run(mc, call, tmpdir):
    """{relative file name: bytes} of everything CALLS_FOR's ``call`` writes (steps of a call are prefixed step<k>/)."""
    folder = os.path.join(str(tmpdir), "export_%s" % call)
    os.makedirs(folder)
    root = os.path.join(folder, "chain")
    if call == "save":
        mc.saveAsText(root)
    elif call == "save_index0":
        mc.saveAsText(root, chain_index=0)
    elif call == "save_index1":
        mc.saveAsText(root, chain_index=1)
    elif call == "save_txt_suffix":
        mc.saveAsText(root + ".txt")
    elif call == "chains":
        mc.saveChainsAsText(os.path.join(folder, "sub", "dir", "chain"), make_dirs=True)
    elif call == "chains_properties":
        mc.saveChainsAsText(root, properties=PROPS)
    elif call == "matrices":
        mc.writeCovMatrix(os.path.join(folder, "chain.covmat"))
        mc.writeCorrelationMatrix(os.path.join(folder, "chain.corr"))
    elif call == "metadata_steps":
        out = {}
        with open(root + ".properties.ini", "w", encoding="utf-8") as f:
            f.write("# written by an earlier run\nzeta=last\nlabel=old label\n\nalpha = 1\n")
        mc.saveTextMetadata(root, properties={"burn_removed": False})
        out.update({"step1/" + k: v for k, v in _files(folder).items()})
        mc.saveTextMetadata(root, properties=PROPS)
        out.update({"step2/" + k: v for k, v in _files(folder).items()})
        label, mc.label = mc.label, None
        try:
            mc.saveTextMetadata(root)  # nothing to say: the file goes
        finally:
            mc.label = label
        out.update({"step3/" + k: v for k, v in _files(folder).items()})
        return out
    else:
        raise KeyError(call)
    return _files(folder)


def golden_key(fx, call, name):
    return "%s/%s/%s" % (fx, call, name)


def load_golden():
    """{(fixture, call): {file name: bytes}}"""
    out = {}
    with np.load(GOLDEN) as z:
        for key in z.files:
            fx, call, name = key.split("/", 2)
            out.setdefault((fx, call), {})[name] = z[key].tobytes()
    return out

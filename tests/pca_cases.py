"""The inputs and cases of tests/golden/pca.npz (MCSamples.PCA), the text comparison rule, and a vectorised numpy
restatement of the O(N) steps of PCA.  Inputs are regenerated from seeds on any box, so the golden file holds reference
outputs only.  Shared by tests/golden/make_golden_pca.py and the CPU / GPU tests."""

import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pca.npz")
N_ROWS = 20_000


def _rng(stream):
    return np.random.default_rng(np.random.SeedSequence([20261016, stream]))


def fixtures():
    """name -> dict(samples, weights, names, labels, derived): derived = (name, label, vector) added by addDerived"""
    out = {}
    # the classic power law: sigma8 Omega_m^0.5 tightly constrained; all columns positive (default maps: L)
    r = _rng(1)
    lnom = np.log(0.3) + 0.08 * r.standard_normal(N_ROWS)
    lns8 = np.log(0.8) - 0.5 * (lnom - np.log(0.3)) + 0.01 * r.standard_normal(N_ROWS)
    lnh = np.log(0.68) + 0.2 * (lnom - np.log(0.3)) + 0.03 * r.standard_normal(N_ROWS)
    lnns = np.log(0.965) + 0.004 * r.standard_normal(N_ROWS)
    s = np.exp(np.stack([lnom, lns8, lnh, lnns], axis=1))
    out["powerlaw_unit"] = dict(samples=s, weights=None, names=["omegam", "sigma8", "H0", "ns"],
                                labels=[r"\Omega_m", r"\sigma_8", "h", "n_s"], derived=None)
    # positive, negative, zero-crossing columns with integer multiplicities
    r = _rng(2)
    L = np.linalg.cholesky(np.array([[1.0, 0.6, 0.2, 0.1], [0.6, 1.0, -0.3, 0.0], [0.2, -0.3, 1.0, 0.4],
                                     [0.1, 0.0, 0.4, 1.0]]))
    g = _rng(3).standard_normal((N_ROWS, 4)) @ L.T
    s = np.stack([np.exp(0.3 * g[:, 0] + 1.0), -np.exp(0.2 * g[:, 1] + 0.5), 0.7 * g[:, 2] + 0.1, 2.0 + 0.5 * g[:, 3]],
                 axis=1)
    w = r.integers(1, 7, N_ROWS).astype(float)
    out["mixed_int"] = dict(samples=s, weights=w, names=["a", "neg", "x", "b"], labels=["A", "N_{eg}", "x", "B"],
                            derived=None)
    # real weights correlated with the parameters, and a derived column appended by addDerived
    r = _rng(4)
    L = np.linalg.cholesky(np.array([[1.0, 0.5, -0.2], [0.5, 1.0, 0.3], [-0.2, 0.3, 1.0]]))
    g = r.standard_normal((N_ROWS, 3)) @ L.T
    s = np.stack([np.exp(0.1 * g[:, 0] + 0.2), 1.5 + 0.3 * g[:, 1], np.exp(0.25 * g[:, 2] - 1.0)], axis=1)
    w = np.exp(0.4 * g[:, 0] - 0.2 * g[:, 2]) * r.uniform(0.5, 1.5, N_ROWS)
    out["real_derived"] = dict(samples=s, weights=w, names=["p", "q", "r"], labels=["p", "q", "r"],
                               derived=("pr", "p r", s[:, 0] * s[:, 2]))
    return out


# fixture -> list of PCA keyword arguments (every case returns text or a list of texts)
CASES = {
    "powerlaw_unit": [dict(params=["omegam", "sigma8"]),
                      dict(params=["omegam", "sigma8", "H0", "ns"]),
                      dict(params=["omegam", "sigma8", "H0"], n_best_only=1),
                      dict(params=["omegam", "sigma8", "H0"], n_best_only=2),
                      dict(params=["omegam", "sigma8"], normparam="omegam"),
                      dict(params=["omegam", "sigma8"], normparam="H0"),
                      dict(params=["omegam", "nope", "sigma8"]),
                      dict(params=["omegam", "sigma8"], conditional_params=["H0"])],
    "mixed_int": [dict(params=["a", "neg", "x", "b"], param_map="LMNL"),
                  dict(params=["a", "neg", "x"], param_map="NNN"),
                  dict(params=["a", "neg", "b"]),
                  dict(params=["a", "x", "b"], param_map="LNN", normparam="b", conditional_params=["neg"]),
                  dict(params=["neg", "b"], param_map="ML", n_best_only=1)],
    "real_derived": [dict(params=["p", "q", "r"]),
                     dict(params=["q", "pr", "r"], param_map="NLL"),
                     dict(params=["p", "q"], conditional_params=["r"], n_best_only=2)],
}


def case_key(fx, i):
    return "%s/%d" % (fx, i)


def case_spec(fx, i):
    return json.dumps(CASES[fx][i], sort_keys=True)


def all_cases():
    for fx in CASES:
        for i in range(len(CASES[fx])):
            yield fx, i


def load_golden():
    return np.load(GOLDEN)


def build(cls, fx, **kw):
    """The fixture as an MCSamples of class ``cls`` (the reference's or this package's; kw: e.g. _context_factory)."""
    f = fixtures()[fx]
    mc = cls(samples=np.ascontiguousarray(f["samples"]), weights=f["weights"], names=f["names"], labels=f["labels"], **kw)
    if f["derived"] is not None:
        name, label, vec = f["derived"]
        mc.addDerived(vec, name, label=label)
    return mc


def as_text(result):
    """One string for a PCA return value (a text, or a list of mode texts)."""
    return result if isinstance(result, str) else "\x00".join(result)


# ---- text comparison rule ------------------------------------------------------------------------------------------
# Split each line into numeric and non-numeric tokens.  Non-numeric tokens must be equal; a numeric token must agree with
# its counterpart within one unit of its last printed digit; the line structure must be identical.
_NUM = re.compile(r"[-+]?(?:\d+\.\d*|\.\d+|\d+)(?:[eE][-+]?\d+)?|[-+]?(?:nan|inf)")


def _tokens(line):
    out, at = [], 0
    for m in _NUM.finditer(line):
        if m.start() > at:
            out.append(("s", line[at:m.start()]))
        out.append(("n", m.group()))
        at = m.end()
    if at < len(line):
        out.append(("s", line[at:]))
    return out


def _ulp_of(tok):
    if "." not in tok:
        return 1.0
    frac = tok.split(".")[1]
    frac = re.split(r"[eE]", frac)[0]
    return 10.0 ** -len(frac)


def text_mismatches(got, want):
    """Lines where ``got`` breaks the rule against ``want`` (empty list: the texts agree)."""
    gl, wl = got.split("\n"), want.split("\n")
    if len(gl) != len(wl):
        return ["line count %d != %d" % (len(gl), len(wl))]
    bad = []
    for k, (g, w) in enumerate(zip(gl, wl)):
        tg, tw = _tokens(g), _tokens(w)
        ok = len(tg) == len(tw)
        for (kg, vg), (kw, vw) in zip(tg, tw) if ok else []:
            if kg != kw:
                ok = False
            elif kg == "s":
                ok = vg.strip() == vw.strip()  # (field widths move with a sign: padding is not compared)
            else:
                fg, fw = float(vg), float(vw)
                if np.isnan(fw) or np.isinf(fw):
                    ok = ok and vg.lstrip("+") == vw.lstrip("+")
                else:
                    ok = ok and abs(fg - fw) <= 1.0001 * max(_ulp_of(vg), _ulp_of(vw))
            if not ok:
                break
        if not ok:
            bad.append("line %d:\n  got  %r\n  want %r" % (k, g, w))
    return bad


# ---- vectorised numpy restatement of steps 1-2 and 4-5 (row chunks: no N x n temporaries beyond one chunk) -----------
def _map(x, maps):
    y = np.array(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for c, m in enumerate(maps):
            if m == 1:
                y[:, c] = np.log(y[:, c])
            elif m == 2:
                y[:, c] = np.log(-1.0 * y[:, c])
    return y


def _chunks(N, chunk):
    chunk = chunk or N
    return [(a, min(a + chunk, N)) for a in range(0, N, chunk)]


def np_corr(samples, weights, cols, maps, chunk=None):
    """Steps 1-2: (mean, sd, corr) of the mapped columns ``cols`` (weights None = unit)."""
    N = samples.shape[0]
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    norm = np.sum(w)
    s1 = sum(w[a:b] @ _map(samples[a:b][:, cols], maps) for a, b in _chunks(N, chunk))
    mean = s1 / norm
    n = len(cols)
    S = np.zeros((n, n))
    for a, b in _chunks(N, chunk):
        d = _map(samples[a:b][:, cols], maps) - mean
        S += (d * w[a:b, None]).T @ d
    sd = np.sqrt(np.diag(S) / norm)
    sdp = np.where(sd != 0, sd, 1.0)
    corr = S / np.outer(sdp, sdp) / norm
    np.fill_diagonal(corr, 1.0)
    return mean, sd, corr


def np_project(samples, weights, cols, maps, mean, sd, U, doexp, all_means, all_sd, chunk=None):
    """Steps 4-5: (newmean, newsd, pcpc, pcpar) of p = U z (exp'd when ``doexp``) against the first len(all_means)
    columns standardised by all_means / all_sd."""
    N = samples.shape[0]
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    norm = np.sum(w)
    sdp = np.where(sd != 0, sd, 1.0)
    nall = len(all_means)

    def proj(a, b):
        p = ((_map(samples[a:b][:, cols], maps) - mean) / sdp) @ U.T
        if doexp:
            with np.errstate(over="ignore"):
                p = np.exp(p)
        return p

    newmean = sum(w[a:b] @ proj(a, b) for a, b in _chunks(N, chunk)) / norm
    n = len(cols)
    Spp, Spx = np.zeros((n, n)), np.zeros((n, nall))
    for a, b in _chunks(N, chunk):
        d = proj(a, b) - newmean
        dw = d * w[a:b, None]
        Spp += dw.T @ d
        Spx += dw.T @ ((samples[a:b, :nall] - all_means) / all_sd)
    newsd = np.sqrt(np.diag(Spp) / norm)
    pcpc = Spp / np.outer(newsd, newsd) / norm
    pcpar = Spx / newsd[:, None] / norm
    return newmean, newsd, pcpc, pcpar

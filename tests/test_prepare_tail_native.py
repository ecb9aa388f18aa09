"""
The scalar tail of gd_prepare_params (csrc/batch2d.hpp: prepare_tail), built with g++, against the Python tail of
MCSamples._init_params on random records: exactly equal ranges, sigma_range and limit flags.  The Python side is the
method itself, run on a stand-in object whose context has the quantile select only (so the Python tail is what runs).
"""

import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

from getdist_amd._lib import PREPARED_PARAM  # noqa: E402
from getdist_amd.mcsamples import MCSamples  # noqa: E402

NORMAL_DECILES = np.array([-1.2815515655446004, -0.8416212335729143, -0.5244005127080407, -0.2533471031357997, 0.0,
                           0.2533471031357997, 0.5244005127080407, 0.8416212335729143, 1.2815515655446004])


def make_records(m, seed):
    """q (m x 11), minmax (m x 2), err (m), limits (m x 2, NaN = none), prior flags: every combination of
    {no / lower / upper / both limits} x {far from / near / at the limit} x {flat / peaked deciles} x {err below / above scale}."""
    rng = np.random.default_rng(seed)
    q, mm, err, lim = np.zeros((m, 11)), np.zeros((m, 2)), np.zeros(m), np.full((m, 2), np.nan)
    for r in range(m):
        kind_lim, kind_dist, flat, err_above = r % 4, (r // 4) % 3, (r // 12) % 2, (r // 24) % 2
        mu = rng.normal() * 10.0 ** rng.integers(-3, 4)
        s = 10.0 ** rng.uniform(-4, 3)
        if flat:
            dec = mu + s * (np.linspace(0.1, 0.9, 9) - 0.5) * (1 + 0.02 * rng.normal(size=9))
            lo, hi = mu - 0.5 * s * rng.uniform(1.0, 1.02), mu + 0.5 * s * rng.uniform(1.0, 1.02)
        else:
            dec = mu + s * NORMAL_DECILES * (1 + 0.05 * rng.normal(size=9))
            lo, hi = mu - s * rng.uniform(3, 5), mu + s * rng.uniform(3, 5)
        dec = np.sort(dec)
        q[r, 2:] = dec
        q[r, 0] = lo + (dec[0] - lo) * rng.uniform(0.0, 0.5)
        q[r, 1] = hi - (hi - dec[-1]) * rng.uniform(0.0, 0.5)
        mm[r] = lo, hi
        conf = np.concatenate([[lo], dec, [hi]])
        scale = np.min(conf[4:] - conf[:-4]) / 1.049
        err[r] = scale * (rng.uniform(1.05, 3.0) if err_above else rng.uniform(0.2, 0.95))
        gap = [rng.uniform(2, 20) * s, rng.uniform(0, 1.0) * 0.4 * min(err[r], scale), 0.0][kind_dist]
        if kind_lim in (1, 3):
            lim[r, 0] = lo - gap
        if kind_lim in (2, 3):
            lim[r, 1] = hi + gap
    return q, mm, err, lim


def python_tail(q, mm, err, lim):
    """MCSamples._init_params itself on a stand-in object: its quantile select returns ``q``."""
    m = len(q)
    names = []
    for r in range(m):
        p = types.SimpleNamespace(name="p%d" % r, _ranges_done=False)
        p.limmin = None if np.isnan(lim[r, 0]) else float(lim[r, 0])
        p.limmax = None if np.isnan(lim[r, 1]) else float(lim[r, 1])
        p.has_limits_bot, p.has_limits_top = p.limmin is not None, p.limmax is not None
        names.append(p)
    me = types.SimpleNamespace(
        paramNames=types.SimpleNamespace(names=names), range_confidence=0.001, norm=1.0, sddev=err, means=np.zeros(m),
        _col_min=mm[:, 0].copy(), _col_max=mm[:, 1].copy(), range_ND_contour=-1, loglikes=None,
        ctx=types.SimpleNamespace(quantiles=lambda cols, targets, minmax=None: q[np.asarray(cols)]),
        _minmax_of=lambda js: mm[np.asarray(js)])
    MCSamples._init_params(me, list(range(m)))
    return names


def test_native_tail_equals_python_tail():
    import build_prepare

    lib = build_prepare.load()
    m = 4320  # 90 of each of the 48 kinds
    q, mm, err, lim = make_records(m, 20240611)
    recs = np.zeros(m, dtype=PREPARED_PARAM)
    recs["has_limits_bot"], recs["has_limits_top"] = ~np.isnan(lim[:, 0]), ~np.isnan(lim[:, 1])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    lib.gdt_prepare_tail(C.c_int32(m), dp(q), dp(mm), dp(err), dp(lim), C.c_void_p(recs.ctypes.data))
    names = python_tail(q, mm, err, lim)
    want = np.zeros(m, dtype=PREPARED_PARAM)
    for r, p in enumerate(names):
        want[r] = (p.range_min, p.range_max, p.sigma_range, p.has_limits_bot, p.has_limits_top)
        assert p.has_limits == bool(recs["has_limits_bot"][r] or recs["has_limits_top"][r])
    for f in PREPARED_PARAM.names:
        assert np.array_equal(recs[f], want[f]), f
    # the records exercise every branch: limits kept and dropped on both sides, flat and peaked, either sigma_range
    kept_b, prior_b = recs["has_limits_bot"] == 1, ~np.isnan(lim[:, 0])
    kept_t, prior_t = recs["has_limits_top"] == 1, ~np.isnan(lim[:, 1])
    assert 200 < np.count_nonzero(kept_b) < np.count_nonzero(prior_b) - 200
    assert 200 < np.count_nonzero(kept_t) < np.count_nonzero(prior_t) - 200
    conf = np.concatenate([mm[:, :1], q[:, 2:], mm[:, 1:]], axis=1)
    scale = np.min(conf[:, 4:] - conf[:, :-4], axis=1) / 1.049
    assert 200 < np.count_nonzero(recs["sigma_range"] == scale) and 200 < np.count_nonzero(recs["sigma_range"] == err)
    assert 200 < np.count_nonzero((recs["sigma_range"] == scale) & (err < scale))  # the flat branch


def test_native_tail_propagates_nan_like_numpy():
    """A NaN decile: np.min gives NaN, every comparison is false -- sigma_range = err, limits kept, ranges NaN-free where
    the quantiles are."""
    import build_prepare

    lib = build_prepare.load()
    q, mm, err, lim = make_records(48, 7)
    q[:, 5] = np.nan
    recs = np.zeros(48, dtype=PREPARED_PARAM)
    recs["has_limits_bot"], recs["has_limits_top"] = ~np.isnan(lim[:, 0]), ~np.isnan(lim[:, 1])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    lib.gdt_prepare_tail(C.c_int32(48), dp(q), dp(mm), dp(err), dp(lim), C.c_void_p(recs.ctypes.data))
    with np.errstate(invalid="ignore"):
        names = python_tail(q, mm, err, lim)
    for r, p in enumerate(names):
        got = (recs["range_min"][r], recs["range_max"][r], recs["sigma_range"][r], recs["has_limits_bot"][r], recs["has_limits_top"][r])
        assert np.array_equal(np.array(got, dtype=np.float64),
                              np.array((p.range_min, p.range_max, p.sigma_range, p.has_limits_bot, p.has_limits_top), dtype=np.float64),
                              equal_nan=True)

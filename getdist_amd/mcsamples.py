"""
``MCSamples``: the host-side mirror of GetDist's analysis object for the KDE / weighted-statistics hot
path, driving libgdhip.so (HIP kernels on one MI355X) through the ctypes C ABI.

Same method names, keyword arguments, defaults (analysis_defaults.ini) and result types as
getdist/mcsamples.py + getdist/chains.py for that path; every O(N) step and every O(F^2) grid step runs
on the GPU, including the root finders of the bandwidth selection (MINPACK hybrd as scipy's fsolve runs it for the
1D Botev fixed point, Brent's method for the 2D one: csrc/solvers.hpp).  What stays in Python is the reference's
*scalar* logic (ranges and limits, bin edges, bandwidth branch selection, fallbacks), evaluated in the reference's
expression order so that bin edges are bit-identical.  ``MCSamples`` holds the constructor, the settings, ranges and
limits, the densities and PCA; the sample statistics it inherits (``WeightedSamples`` -> ``Chains``) are in chains.py.

Additive API (not in the reference): ``get1DDensities``, ``get2DDensities`` and ``triangleDensities``
compute many densities in batched kernel launches; the per-name/per-pair methods are thin views over
them.  There is no CPU fallback: without the library or a GPU, construction raises.
"""

import copy as _copy
import logging
import os
import time

import numpy as np

from ._lib import Context
from .chains import Chains, MCSamplesError
from .densities import Density1D, Density2D, DensitiesError
from .paramnames import ParamNames
from .parampriors import ParamBounds
from .types import LikeStats, MargeStats, NoLineTableFormatter, ParamLimit, ResultTable

# Re-exported: tests, scripts and callers written against getdist_amd.mcsamples import these names from this module; they
# are defined in chains.py and paramnames.py (the same objects).
import threading  # noqa: F401

from ._lib import GdhipError  # noqa: F401
from .chains import (ChainView, ParamConfidenceData, ParamError, WeightedSampleError, WeightedSamples,  # noqa: F401
                     _g2_independence_vs_markov, _g2_markov_vs_second_order, _where_rows, covToCorr)
from .paramnames import ParamInfo, _PlotParamInfo  # noqa: F401

# analysis_defaults.ini:1-76 (the ini always overrides the class literals, mcsamples.py:491-492)
DEFAULT_SETTINGS = dict(
    ignore_rows=0.0, min_weight_ratio=1e-30, contours=[0.68, 0.95, 0.99], credible_interval_threshold=0.05,
    range_ND_contour=-1, range_confidence=0.001, corr_length_thin=0, corr_length_steps=15, converge_test_limit=0.95, fine_bins=1024, smooth_scale_1D=-1.0,
    boundary_correction_order=1, mult_bias_correction_order=1, smooth_scale_2D=-1.0, max_corr_2D=0.99,
    fine_bins_2D=256, use_effective_samples_2D=False, max_scatter_points=2000, num_bins=100, num_bins_2D=40,
    num_bins_ND=12)  # (num_bins_ND: the class default of mcsamples.py:224, read from an ini too, :407)


class SettingError(MCSamplesError):
    pass


class BandwidthError(MCSamplesError):
    pass


# keys of a reference analysis .ini that are settings of this path although they are not in analysis_defaults.ini by
# that name: the contour list in its numbered form and the limit-type overrides (mcsamples.py:417-433)
_INI_EXTRA = ("num_contours", "force_twotail")


def _read_ini_settings(ini):
    """
    The analysis settings of a GetDist .ini file (``key = value`` lines, ``#`` comments; inifile.py:100-180) that this
    path knows; other keys (plot options, file lists) are ignored like the reference ignores what it does not read.
    ``num_contours`` + ``contour1..N`` become ``contours`` (unless ``contours`` itself is given, mcsamples.py:420-424),
    ``force_twotail`` and ``max_frac_twotailN`` are kept (mcsamples.py:417,426-431).  A dict is passed through.
    """
    if isinstance(ini, dict):
        raw = {str(k): v for k, v in ini.items()}
    else:
        raw = {}
        with open(ini, encoding="utf-8-sig") as f:
            for line in f:
                line = line.split("#", 1)[0].strip()
                if "=" not in line:
                    continue
                key, value = (t.strip() for t in line.split("=", 1))
                if value != "":
                    raw[key] = value
    out = {}
    for key, value in raw.items():
        if key in DEFAULT_SETTINGS:
            out[key] = [float(v) for v in value.split()] if (key == "contours" and isinstance(value, str)) else value
        elif key == "force_twotail" or key.startswith("max_frac_twotail"):
            out[key] = value
    if "contours" not in out and "num_contours" in raw:
        n = int(raw["num_contours"])
        missing = [i + 1 for i in range(n) if "contour%d" % (i + 1) not in raw]
        if missing:
            raise SettingError("num_contours = %d but contour%d is not set" % (n, missing[0]))
        out["contours"] = [float(raw["contour%d" % (i + 1)]) for i in range(n)]
    return out


def _stack_rows(parts):
    """
    np.vstack / np.hstack of per-chain arrays.  Chains that are consecutive row ranges of one column-major block (the
    binary chain cache, chainfiles.read_soa_cache) are returned as a view of that block -- no host copy, and the
    page-locked columns go to the device as they are; anything else is copied into a new column-major array.
    """
    first = parts[0]
    if len(parts) == 1:
        return first
    adjacent = all(p.dtype == np.float64 and p.strides == first.strides and p.shape[1:] == first.shape[1:] for p in parts)
    if adjacent:
        addr = first.ctypes.data
        for p in parts:
            if p.ctypes.data != addr:
                adjacent = False
                break
            addr += p.shape[0] * p.strides[0]
        adjacent = adjacent and first.strides[0] == 8
    total = sum(p.shape[0] for p in parts)
    if adjacent:
        shape = (total,) + first.shape[1:]
        return np.lib.stride_tricks.as_strided(first, shape=shape, strides=first.strides, writeable=False)
    out = np.empty((total,) + first.shape[1:], dtype=np.float64, order="F")
    a = 0
    for p in parts:
        out[a:a + p.shape[0]] = p
        a += p.shape[0]
    return out


_HOSTLOG = [] if os.environ.get("GETDIST_AMD_HOSTLOG") else None


def _hostlog(what):
    """Host-side timeline of a batched call (GETDIST_AMD_HOSTLOG=1; read by scripts and tests only)."""
    if _HOSTLOG is not None:
        import time

        _HOSTLOG.append((time.perf_counter(), what))


class _Plan(list):
    """The per-pair bandwidth records (dicts) of _bandwidth_plan plus the same fields as arrays over the pairs
    (``arr``: branch code 0/1/2 = A/B/C, has_limits, corr, rangex, rangey and -- once the effective sample numbers are
    known -- neff, fallback_t): what sits between two kernels of a batched call is evaluated on the arrays."""

    arr = None


class _Done:
    """A finished future (the lag probe that came back with the quantile select)."""

    def __init__(self, value):
        self._value = value

    def result(self):
        return self._value


class _FastThreadSwitch:
    """While a helper thread drives a second stream, a thread returning from a C call would wait for the GIL up to the
    interpreter's switch interval (5 ms by default) whenever the other thread is in Python scalar code -- longer than
    most kernels here.  100 us for the duration of a batched call; restored on exit."""

    def __init__(self, active=True):
        self.active = active

    def __enter__(self):
        if self.active:
            import sys

            self.old = sys.getswitchinterval()
            sys.setswitchinterval(float(os.environ.get("GETDIST_AMD_SWITCH_INTERVAL", 1e-4)))
        return self

    def __exit__(self, *exc):
        if self.active:
            import sys

            sys.setswitchinterval(self.old)
        return False


class _Phase:
    """Wall-clock phase accounting (enabled by GETDIST_AMD_TIMING=1; syncs the stream at phase edges)."""

    def __init__(self, mc, name):
        self.mc, self.name = mc, name

    def __enter__(self):
        if self.mc._timing:
            self.mc.ctx.sync()
            self.t0 = time.perf_counter()

    def __exit__(self, *a):
        if self.mc._timing:
            self.mc.ctx.sync()
            self.mc.timings[self.name] = self.mc.timings.get(self.name, 0.0) + time.perf_counter() - self.t0


def _set_raw_edge_mask_nd(parv, prior_mask):
    """mcsamples.py:2012-2033: halve the faces of the raw N-D grid on the bounded sides.  Axis i of the mask (C order,
    the last parameter first) belongs to parv[::-1][i]."""
    vrap = parv[::-1]
    if prior_mask.ndim != len(parv):
        raise ValueError("parv and prior_mask or different sizes!")
    for i, par in enumerate(vrap):
        sl = [slice(None)] * prior_mask.ndim
        if par.has_limits_bot:
            sl[i] = 0
            prior_mask[tuple(sl)] /= 2
        if par.has_limits_top:
            sl[i] = prior_mask.shape[i] - 1
            prior_mask[tuple(sl)] /= 2


def _set_edge_mask_2d(parx, pary, prior_mask, winw):
    """mcsamples.py:1688-1703: half weight on a limit's edge bins, zero beyond -- on non-periodic axes only"""
    if not parx.periodic:
        if parx.has_limits_bot:
            prior_mask[:, winw] /= 2
            prior_mask[:, :winw] = 0
        if parx.has_limits_top:
            prior_mask[:, -(winw + 1)] /= 2
            prior_mask[:, -winw:] = 0
    if not pary.periodic:
        if pary.has_limits_bot:
            prior_mask[winw, :] /= 2
            prior_mask[:winw] = 0
        if pary.has_limits_top:
            prior_mask[-(winw + 1), :] /= 2
            prior_mask[-winw:, :] = 0


def _set_all_edge_mask_2d(prior_mask, winw, periodic_x=False, periodic_y=False):
    """mcsamples.py:1705-1712: zero the padding margins along non-periodic axes"""
    if not periodic_x:
        prior_mask[:, :winw] = 0
        prior_mask[:, -winw:] = 0
    if not periodic_y:
        prior_mask[:winw] = 0
        prior_mask[-winw:, :] = 0


class MCSamples(Chains):
    """
    Weighted samples resident in HBM + the KDE hot path.  Constructor arguments follow
    mcsamples.py:149-161 (``samples`` may be an (N, n) array or a list of per-chain arrays;
    ``ranges`` maps name -> (lower, upper[, True|'periodic'])).  ``device`` selects the GPU.  ``renames`` maps names to
    alternative name(s) (chains.py:1139-1140); a name given as ``"x*"`` is the derived parameter ``x``.  With ``root`` of a
    Cobaya run (chainfiles.read_root) the run's yaml also gives label, sampler and temperature where none was passed
    (_cobaya_properties); unlike the reference, a sampler that comes out as "nested" this way refuses ``ignore_rows`` too.
    """

    def __init__(self, root=None, ini=None, settings=None, ranges=None, samples=None, weights=None, loglikes=None,
                 temperature=None, names=None, labels=None, label=None, name_tag=None, sampler=None, device=0,
                 _context_factory=None, renames=None, **kwargs):
        self.sampler = sampler or "mcmc"
        self.temperature, self.cooled = temperature, 1
        self._likeStats = None
        self._loglikes_col = None
        self.label, self.name_tag = label, name_tag
        self.properties = None  # mcsamples.py:243: {key: value} (or an object with .params) saved to root.properties.ini
        self.root = root
        self.rootdirname = ""  # mcsamples.py:244: the output root of writeDataToFile (PCA writes rootdirname + ".PCA")
        self.raise_on_bandwidth_errors = False
        self.no_warning_params = []          # mcsamples.py:259-260,438-439: parameters whose 1D bandwidth fallback is silent
        self.no_warning_chi2_params = True
        self.chain_offsets = None
        self.chains = None
        self.indep_thin = 0  # mcsamples.py:245: set by getCorrLengths / getConvergeTests
        self.ctx = None
        for k, v in DEFAULT_SETTINGS.items():
            setattr(self, k, v)
        if "ignore_rows" in kwargs:  # mcsamples.py:246-250: the keyword is a setting
            settings = dict(settings or {})
            settings["ignore_rows"] = kwargs.pop("ignore_rows")
        chain_exclude, no_cache = kwargs.pop("_chain_exclude", None), kwargs.pop("_no_cache", False)
        # multi-rank jobs: a parallel.ColumnShare -- this rank uploads only its block of columns over PCIe and the ranks
        # broadcast their blocks to one another over xGMI (gd_upload_shard / gd_comm_share_columns); additive keyword
        self._column_share = kwargs.pop("column_share", None)
        if kwargs:
            raise TypeError("unexpected keyword arguments: %s" % ", ".join(kwargs))
        if ini is not None:
            settings = dict(_read_ini_settings(ini), **(settings or {}))  # the dict takes preference (:472-499)
        if settings:
            self.updateSettings(settings, doUpdate=False)
        if self.sampler == "nested" and not np.isclose(self.ignore_rows, 0):
            raise ValueError("Should not remove burn-in from Nested Sampler samples.")
        self.ranges = ParamBounds()
        derived = comments = info_dict = file_renames = None
        if root is not None and samples is None:
            # mcsamples.py:47-146, chains.py:1368-1405: the chain files, side files and (when fresh) the binary cache
            from . import chainfiles

            self.ctx = (_context_factory or Context)(device)  # page-locked landing buffer for the binary cache
            loaded = chainfiles.read_root(root, chain_exclude, no_cache,
                                          alloc=getattr(self.ctx, "pinned_block", None), ctx=self.ctx)
            samples, weights, loglikes = loaded["samples"], loaded["weights"], loaded["loglikes"]
            names = names or loaded["names"]
            labels = labels or loaded["labels"]
            derived, comments = loaded["derived"], loaded.get("comments")
            for nm, rng in loaded["ranges"].items():
                self.ranges.setRange(nm, rng)
            self.name_tag = self.name_tag or os.path.basename(root)
            info_dict = loaded.get("info_dict")
            if info_dict is not None:
                file_renames = loaded["renames"]
                if not os.path.exists(root + ".properties.ini"):
                    self._cobaya_properties(info_dict, sampler is None)
        elif names is not None and any(isinstance(nm, str) and nm.endswith("*") for nm in names):
            # paramnames.py:97-111 through chains.py:1170-1172: a name given as "x*" is the derived parameter x
            derived = [nm.endswith("*") for nm in names]
            names = [nm[:-1] if d else nm for nm, d in zip(names, derived)]
        ignore_lines = int(self.ignore_rows)
        if samples is None:
            raise MCSamplesError("samples are required")
        if isinstance(ranges, ParamBounds):  # mcsamples.py:342-343: taken over as a copy
            self.ranges = _copy.deepcopy(ranges)
        else:
            for nm, rng in (ranges or {}).items():
                self.ranges.setRange(nm, rng)
        self._device_installed = False
        on_device = self._read_device_chains(samples, weights, loglikes, ignore_lines, device, _context_factory or Context)
        if isinstance(on_device, dict):  # the columns are resident already; the host mirror is made when first read
            weights, loglikes, fixed = on_device["weights"], on_device["loglikes"], on_device["fixed"]
            self._samples, self._samples_on_device = None, True
            self.numrows, n_kept = on_device["numrows"], on_device["n"]
        else:
            if on_device is not None:  # device arrays the device route does not serve, as host arrays
                samples, weights, loglikes = on_device
            samples, weights, loglikes, fixed = self._read_chains(samples, weights, loglikes, ignore_lines)
            self.samples = samples
            self.numrows, n_kept = samples.shape
        self.loglikes = loglikes
        n_all = n_kept + len(fixed)
        self._user_weights = weights is not None
        self.weights = weights
        if names is None:
            names = ["param%d" % (i + 1) for i in range(n_all)]
        if len(names) != n_all:
            raise MCSamplesError("names do not match the number of sample columns")
        self.paramNames = ParamNames(list(names), labels)
        self.paramNames.info_dict = info_dict
        for more in (file_renames, renames):  # those of a Cobaya run's yaml, then the keyword's (chains.py:1139-1140)
            if more:
                self.paramNames.updateRenames(more)
        if derived is not None:
            for par, d in zip(self.paramNames.names, derived):
                par.isDerived = bool(d)
        if comments is not None:
            for par, c in zip(self.paramNames.names, comments):
                par.comment = c
        for ix, value in fixed:  # chains.py:1555-1559: a parameter that never moves becomes a zero-width range
            self.ranges.setFixed(self.paramNames.names[ix].name, value)
        self.paramNames.deleteIndices([ix for ix, _ in fixed])
        self.n = n_kept
        self.index = {p.name: i for i, p in enumerate(self.paramNames.names)}
        # _context_factory is a TEST hook (tests/fake_ctx.py drives the host logic on CPU); the product always uses
        # the HIP library and raises if it or a GPU is missing
        if getattr(self, "ctx", None) is None:
            self.ctx = (_context_factory or Context)(device)
        self._timing = os.environ.get("GETDIST_AMD_TIMING", "0") == "1"
        self.timings = {}
        self.density1D = {}
        self._idx_cols = {}
        self.shade_likes_is_mean_loglikes = False  # mcsamples.py:233
        self._context_factory = _context_factory or Context
        self._device = device
        self._lane, self._nlanes = 0, 1
        # set up front: helper threads assign these while another thread may be iterating this object's __dict__
        self._lag_prefetch = self._pending_results = self._parked = None
        self._helper_exec = None
        self._lane_exec = None
        self._twin = None
        self._chain_stats_cache = {}
        self.needs_update = True
        self._upload(filter_weights=False)  # the per-chain filter already ran (makeSingle passes min_weight_ratio=-1)
        self.updateBaseStatistics()

    def _cobaya_properties(self, info, want_sampler):
        """mcsamples.py:285-303: what a Cobaya run's yaml says about the chain, for a root without a .properties.ini.  Rows
        the run reports as removed already (cobaya_interface.get_burn_removed) are not removed again; the run's label is
        taken if none was given, its sampler if none was passed (``want_sampler``; setSampler, chains.py:1147-1152: an
        unknown one warns and counts as mcmc) and its temperature if none was passed.  ``self.properties`` records all of it
        -- the temperature only when it is not 1 -- and that a burn-in is (or was) removed."""
        from . import cobaya_interface as ci

        self.properties = {}
        if ci.get_burn_removed(info):
            self.properties["burn_removed"] = True
            self.ignore_rows = 0.0
        if not self.label:
            self.label = ci.get_sample_label(info)
            if self.label:
                self.properties["label"] = self.label
        if want_sampler:
            sampler = ci.get_sampler_type(info).lower()
            if sampler not in ("mcmc", "nested", "uncorrelated"):
                import warnings

                warnings.warn("Unknown sampler type %s. Assuming MCMC." % sampler)
                sampler = "mcmc"
            self.sampler = sampler
            if sampler == "nested" and not np.isclose(self.ignore_rows, 0):  # (the check of the constructor, for this sampler)
                raise ValueError("Should not remove burn-in from Nested Sampler samples.")
        self.properties["sampler"] = self.sampler
        if self.temperature is None:
            self.temperature = ci.get_sampler_temperature(info)
        if self.temperature is not None and self.temperature != 1:
            self.properties["temperature"] = self.temperature
        if self.ignore_rows:
            self.properties["burn_removed"] = True

    def _read_chains(self, samples, weights, loglikes, ignore_lines):
        """
        loadChains + readChains for array input (chains.py:1405-1443, mcsamples.py:501-528): per chain, drop
        ``ignore_lines`` leading rows, drop rows below min_weight_ratio of THAT chain's maximum weight
        (chains.py:1017-1027), drop the burn-in fraction (chains.py:1047-1061); delete the parameters that do not move
        (decided on the first chain, chains.py:1029-1045,1548-1555); stack the chains and record their offsets
        (makeSingle, chains.py:1488-1503).  Returns (samples, weights, loglikes, [(fixed column, value)]).
        """
        is_list = isinstance(samples, (list, tuple)) and len(samples) and np.ndim(samples[0]) == 2
        if is_list:
            chains = [[np.asarray(c), None if weights is None else np.asarray(weights[i], dtype=np.float64),
                       None if loglikes is None else np.asarray(loglikes[i], dtype=np.float64)]
                      for i, c in enumerate(samples)]
        else:
            if isinstance(samples, (list, tuple)):  # a list of parameter vectors (chains.py:287-288)
                samples = np.hstack([np.asarray(x).reshape(-1, 1) for x in samples])
            samples = np.asarray(samples)
            if samples.ndim == 1:
                samples = samples.reshape(-1, 1)
            chains = [[samples, None if weights is None else np.asarray(weights, dtype=np.float64),
                       None if loglikes is None else np.asarray(loglikes, dtype=np.float64)]]
        ignore_frac = 0 if int(self.ignore_rows) else self.ignore_rows
        mwr = self.min_weight_ratio
        for ch in chains:
            if ignore_lines:
                ch[:] = [None if v is None else v[ignore_lines:] for v in ch]
            w = ch[1]
            if w is not None and mwr is not None and mwr >= 0 and w.size:
                mx = np.max(w)
                if np.min(w) < mx * mwr:
                    keep = w > mx * mwr
                    ch[:] = [None if v is None else v[keep] for v in ch]
            if ignore_frac:
                ix = int(ignore_frac) if ignore_frac >= 1 else int(round(ch[0].shape[0] * ignore_frac))
                ch[:] = [None if v is None else v[ix:] for v in ch]
        first = chains[0][0]
        fixed = self._fixed_columns(first[[0, -1]], lambda i: first[:, i]) if first.shape[0] else []
        if fixed:
            gone = [i for i, _ in fixed]
            for ch in chains:
                ch[0] = np.delete(ch[0], gone, 1)
        if is_list:
            self.chain_offsets = np.cumsum(np.array([0] + [ch[0].shape[0] for ch in chains]))
            samples = _stack_rows([ch[0] for ch in chains])
            weights = None if chains[0][1] is None else _stack_rows([ch[1] for ch in chains])
            loglikes = None if chains[0][2] is None else _stack_rows([ch[2] for ch in chains])
        else:
            samples, weights, loglikes = chains[0]
        weights = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        return samples, weights, loglikes, fixed

    @staticmethod
    def _fixed_columns(first_last, column):
        """chains.py:1029-1045 on the first chain: ``first_last`` its first and last row, ``column(i)`` its column i (asked
        for the candidates only).  Returns [(column, value)]."""
        fixed = []
        for i in range(first_last.shape[1]):
            if np.isclose(first_last[0, i], first_last[-1, i], equal_nan=True):
                col = column(i)
                mean = np.average(col)
                if np.allclose(col, mean, rtol=1e-12, atol=0, equal_nan=True):
                    fixed.append((i, mean))
        return fixed

    def _read_device_chains(self, samples, weights, loglikes, ignore_lines, device, factory):
        """
        _read_chains for samples that live in DEVICE memory (a torch tensor on the GPU, anything with
        __cuda_array_interface__: devarray.describe): one 2-D array, a 1-D one (a single parameter) or a list of per-chain
        2-D arrays; ``weights`` and ``loglikes`` device or host vectors independently.  The N x n matrix never exists on
        the host: ``ignore_rows`` moves each part's base pointer, the fixed parameters are decided from the first chain's
        first and last row and the candidate columns (the only sample values downloaded) and left out through the kept-column
        list, and gd_upload_device builds the resident columns and weights device to device.  Device weights and loglikes
        are copied to the host once, as float64 vectors, for their existing host consumers.

        Returns None when no device array is involved; a dict (numrows, n, weights, loglikes, fixed) when the set is
        resident; (samples, weights, loglikes) as host arrays when the device route does not serve the input: if
        ``min_weight_ratio`` would remove rows (the constructor keeps the host route for that, as the per-chain filter runs
        before the chains are stacked: the result is the same, only slower -- everything is downloaded and the host code
        runs), or if the library declines the memory (page-locked, managed, negative strides).
        """
        from . import devarray

        is_list = False
        if isinstance(samples, (list, tuple)) and len(samples):
            d0 = devarray.describe(samples[0])
            is_list = (np.ndim(samples[0]) if d0 is None else len(d0.shape)) == 2
            if not is_list and any(devarray.describe(v) is not None for v in samples):
                raise TypeError("a list of 1-D device vectors (one per parameter) is not taken: stack them into one (N, n) "
                                "device array, or pass a list of per-chain (N_k, n) arrays")
        chain_arrays = list(samples) if is_list else [samples]
        per_chain = (lambda v: [None] * len(chain_arrays) if v is None else (list(v) if is_list else [v]))
        descs = [[devarray.describe(a) for a in chain_arrays]] + [[None if a is None else devarray.describe(a) for a in per_chain(v)]
                                                                   for v in (weights, loglikes)]
        if not any(d is not None for row in descs for d in row):
            return None
        if self._column_share is not None:
            raise MCSamplesError("column_share needs host samples: a device array is resident on one device, each rank "
                                 "uploads its own share of the columns")
        for d in (d for row in descs for d in row if d is not None):
            if d.device is not None and d.device != device:
                raise ValueError("the array lives on device %d: pass device=%d" % (d.device, d.device))
        if self.ctx is None:
            self.ctx = factory(device)
        ctx = self.ctx

        def to_host(obj, d, dtype=None):
            if d is None:
                return None if obj is None else np.asarray(obj, dtype=dtype)
            out = ctx.fetch_device_array(d)  # (ValueError for another device's memory, an error for an unknown pointer)
            if out is None:  # declined: memory the host can address as well -- and only that is read from here
                from ._lib import GD_PTR_MANAGED, GD_PTR_PINNED

                if ctx.pointer_info(d.ptr)[0] not in (GD_PTR_PINNED, GD_PTR_MANAGED):
                    raise MCSamplesError("the device array is neither device memory of this device nor host-readable memory")
                out = np.asarray(devarray.host_view(d), dtype=np.float64)
            return out

        def host_route():
            back = [[to_host(o, d) for o, d in zip(chain_arrays, descs[0])]] + \
                [None if v is None else [to_host(o, d, np.float64) for o, d in zip(per_chain(v), row)]
                 for v, row in zip((weights, loglikes), descs[1:])]
            return tuple(v if is_list or v is None else v[0] for v in back)

        if any(d is None for d in descs[0]) or len({d.dtype for d in descs[0]}) != 1:
            return host_route()  # host and device chains mixed, or chains of different element types
        parts = [d.as2d() for d in descs[0]]
        if any(p.shape[1] != parts[0].shape[1] for p in parts) or not parts[0].shape[1]:
            return host_route()  # (the host code raises what it raises for such input)
        # host copies of the weight and loglike vectors (N values each); the device descriptors of the weights stay for the
        # resident weight column
        host = [[None if o is None else to_host(o, d, np.float64).reshape(-1) for o, d in zip(per_chain(v), row)]
                for v, row in zip((weights, loglikes), descs[1:])]
        wdesc = list(descs[1])
        for k, p in enumerate(parts):
            for v in (host[0][k], host[1][k]):
                if v is not None and v.shape[0] != p.shape[0]:
                    return host_route()
        ignore_frac = 0 if int(self.ignore_rows) else self.ignore_rows
        mwr = self.min_weight_ratio

        def drop(k, count):
            parts[k] = parts[k].rows_from(count)
            host[0][k], host[1][k] = (None if v is None else v[count:] for v in (host[0][k], host[1][k]))
            if wdesc[k] is not None:
                wdesc[k] = wdesc[k].rows_from(count)

        for k in range(len(parts)):
            if ignore_lines:
                drop(k, ignore_lines)
            w = host[0][k]
            if w is not None and mwr is not None and mwr >= 0 and w.size and np.min(w) < np.max(w) * mwr:
                return host_route()
            if ignore_frac:
                drop(k, int(ignore_frac) if ignore_frac >= 1 else int(round(parts[k].shape[0] * ignore_frac)))
        numrows = sum(p.shape[0] for p in parts)
        if numrows == 0:
            return host_route()
        fixed = []
        first = parts[0]
        if first.shape[0]:
            ends = [ctx.fetch_device_array(first.row(i)) for i in (0, -1)]
            if ends[0] is None:
                return host_route()
            fixed = self._fixed_columns(np.vstack(ends), lambda i: ctx.fetch_device_array(first.column(i)).reshape(-1))
        gone = {i for i, _ in fixed}
        keep = [i for i in range(first.shape[1]) if i not in gone]
        if not keep:
            return host_route()
        wparts = temp = None
        if weights is not None:
            # a host weight vector reaches the device through a block of its own and is then described like the others
            wparts, temp = [], []
            for k, w in enumerate(host[0]):
                if wdesc[k] is None:
                    buf = ctx.alloc(max(w.nbytes, 8))
                    buf.from_host(np.ascontiguousarray(w))
                    temp.append(buf)
                    wdesc[k] = devarray.DevArray(buf.ptr, w.shape, (1,), devarray.GD_DT_F64, None, None, buf)
                wparts.append(wdesc[k])
            if len({d.dtype for d in wparts}) != 1:  # one element type per call: the odd ones out go through their fp64 copy
                for k, w in enumerate(host[0]):
                    if wparts[k].dtype != devarray.GD_DT_F64:
                        buf = ctx.alloc(max(w.nbytes, 8))
                        buf.from_host(np.ascontiguousarray(w))
                        temp.append(buf)
                        wparts[k] = devarray.DevArray(buf.ptr, w.shape, (1,), devarray.GD_DT_F64, None, None, buf)
        try:
            if not ctx.upload_device(parts, wparts, keep if fixed else None):
                return host_route()
        finally:
            for buf in temp or ():
                buf.free()
        if is_list:
            self.chain_offsets = np.cumsum(np.array([0] + [p.shape[0] for p in parts]))
        self._device_installed = True
        stack = (lambda vs: None if vs[0] is None else np.ascontiguousarray(np.concatenate(vs), dtype=np.float64))
        return dict(numrows=numrows, n=len(keep), weights=stack(host[0]), loglikes=stack(host[1]), fixed=fixed)

    # ---- state -----------------------------------------------------------------------------------------
    def _second_lane(self):
        """
        A shallow twin of this object on a second context (= second stream) that borrows the resident sample set:
        independent pairs dealt to the two lanes overlap one lane's host-side scalar work, launch gaps and result
        copies with the other lane's kernels.  Parameter state is shared (read-only while densities are made).
        """
        own = ("ctx", "_idx_cols", "density1D", "timings", "_helper_exec", "_lane_exec", "_twin", "_lane")
        if self._twin is None:
            import copy

            twin = copy.copy(self)
            twin.ctx = self._context_factory(self._device)
            twin.ctx.attach(self.ctx)
            twin._idx_cols, twin.density1D, twin.timings = {}, {}, {}
            twin._helper_exec = twin._lane_exec = twin._twin = None
            twin._lane = 1
            self._twin = twin
        self._nlanes = 2
        # settings and statistics may have changed since the twin was made: everything but the lane's own state follows
        # (a snapshot: a helper thread may be adding attributes to this object at the same time)
        self._twin.__dict__.update({k: v for k, v in list(self.__dict__.items()) if k not in own})
        return self._twin

    def _twin_context(self):
        """The second lane's context (made on first use) for work that only needs its STREAM: unlike _second_lane this
        neither deals this object's pairs to two lanes (``_nlanes`` stays) nor refreshes the twin's copy of the settings."""
        if self._twin is None:
            nlanes = self._nlanes
            self._second_lane()
            self._nlanes = nlanes
        return self._twin.ctx

    def _lane_thread(self, twin):
        """The thread that drives the second lane (its own helper thread stays free for the lane's inner overlap)."""
        if self._lane_exec is None:
            from concurrent.futures import ThreadPoolExecutor

            self._lane_exec = ThreadPoolExecutor(max_workers=1, thread_name_prefix="gdhip-lane",
                                                 initializer=twin.ctx.bind_thread)
        return self._lane_exec

    def _finish_pending(self):
        """Complete a lazily delivered batched call (its grids view page-locked memory of this object's contexts)."""
        pend, self._pending_results = getattr(self, "_pending_results", None), None
        if pend is not None:
            pend.wait()
        if getattr(self.ctx, "h", None) is not None and hasattr(self.ctx, "batch2d_finish"):
            self.ctx.batch2d_finish()  # the library hands the call's device blocks back (before a second context goes away)
        twin = getattr(self, "_twin", None)
        if twin is not None and getattr(twin, "_pending_results", None) is not None:
            pend, twin._pending_results = twin._pending_results, None
            pend.wait()

    def _drop_second_lane(self):
        self._finish_pending()
        if getattr(self, "_lane_exec", None) is not None:
            self._lane_exec.shutdown(wait=True)
        self._lane_exec = None
        if self._twin is not None:
            if self._twin._helper_exec is not None:
                self._twin._helper_exec.shutdown(wait=True)
            self._twin.ctx.close()
            self._twin = None
        self._nlanes = 1

    def _sample_set_changing(self):
        """The bookkeeping every replacement of the resident samples or weights shares (a re-upload, and the device-to-device
        edits of chains.py): the second lane borrows the set, and everything cached about it is stale."""
        self._drop_second_lane()
        self._chain_stats_cache = {}
        self._loglikes_col = None  # (an extra-column slot of the old sample set)
        self.indep_thin = 0  # (a correlation length of the old sample set)
        self._idx_cols = {}
        self.mean_loglike = None  # chains.py:317; recomputed on the device when a mean-likelihood is asked for
        self._like_mode = None

    def _upload(self, filter_weights=True):
        """(Re)build the device mirror of samples/weights (chains.py:276-323 funnel).  The min-weight filter of
        setSamples applies to a single sample array only: chain lists are filtered per chain before they are stacked."""
        self._sample_set_changing()
        self.__dict__["_mirror_assigned"] = False  # (whatever ``samples`` holds is what is resident when this returns)
        w = self.weights
        if self._device_installed:
            # the constructor's device route (gd_upload_device) has installed this very set, its weight filter settled
            # (_read_device_chains declines when the filter would remove a row): nothing to filter, nothing to upload
            self._device_installed = False
            return
        if (filter_weights and self.chain_offsets is None and w is not None and self.min_weight_ratio is not None
                and self.min_weight_ratio >= 0):
            mx, mn = np.max(w), np.min(w)  # chains.py:1017-1027
            if mn < mx * self.min_weight_ratio:
                thr = mx * self.min_weight_ratio
                keep = w > thr
                on_device = self._device_edit_applies() and np.any(keep)
                if on_device:
                    # the whole array goes up as it is and the rows are dropped there (GD_SEL_WEIGHT_GT, the same comparison
                    # on the resident weights): no fancy-indexed copy of the matrix on the host
                    self.ctx.upload(self.samples, w)
                    on_device = self._select_on_device(rows=("weight_gt", thr))
                if not on_device:
                    self.samples = self.samples[keep]
                self.weights = w = w[keep]
                if self.loglikes is not None:
                    self.loglikes = self.loglikes[keep]
                self.numrows = len(w)
                if on_device:
                    return
        share = getattr(self, "_column_share", None)
        if share is not None:
            share.upload(self.ctx, self.samples, w)  # (collective: every rank of the job uploads at the same point)
        else:
            self.ctx.upload(self.samples, w)

    def parName(self, i, starDerived=False):
        """mcsamples.py:348-356: the name of parameter ``i``, with a trailing * for a derived one when ``starDerived``"""
        par = self.paramNames.names[i]
        return par.name + "*" if starDerived and par.isDerived else par.name

    def parLabel(self, i):
        """mcsamples.py:358-368: the label of parameter ``i`` (an index or a name)"""
        if isinstance(i, str):
            return self.paramNames.parWithName(i).label
        return self.paramNames.names[i].label

    def getUpper(self, name):
        """mcsamples.py:2311-2321: the hard upper bound in force for the parameter (None: unbounded / unknown name)"""
        par = self.paramNames.parWithName(name)
        return getattr(par, "limmax", None) if par else None

    def getLower(self, name):
        par = self.paramNames.parWithName(name)
        return getattr(par, "limmin", None) if par else None

    # ---- copies and combined sample sets (mcsamples.py:308-322, 2620-2660) ---------------------------------------
    # what belongs to this object's contexts, threads and ranks: a copy starts without it (the values it starts with instead;
    # the two caches of device results get dicts of their own)
    _NOT_COPIED = dict(ctx=None, _twin=None, _helper_exec=None, _lane_exec=None, _lag_prefetch=None, _pending_results=None,
                       _parked=None, _neff_share=None, _loglikes_col=None, _like_mode=None, _lane=0, _nlanes=1,
                       _idx_cols=None, _chain_stats_cache=None)

    def __deepcopy__(self, memo):
        """copy.deepcopy(samples): host state equal-valued and independent; the resident sample set duplicated device to
        device into a context of the copy's own (gd_clone_samples) -- the columns do not cross PCIe a second time."""
        if getattr(self, "_column_share", None) is not None:
            raise MCSamplesError("copy needs every column resident on one device: this context holds only its rank's "
                                 "share of the columns (copies of a multi-GPU sample set are not supported)")
        self._finish_pending()
        new = object.__new__(type(self))
        memo[id(self)] = new
        for k, v in list(self.__dict__.items()):
            if k not in self._NOT_COPIED:
                new.__dict__[k] = _copy.deepcopy(v, memo)
        new.__dict__.update(self._NOT_COPIED)
        new._idx_cols, new._chain_stats_cache = {}, {}
        new.ctx = self._context_factory(self._device)
        if hasattr(new.ctx, "clone_samples"):
            new.ctx.clone_samples(self.ctx)
        else:  # (a context double of the CPU tests)
            new.ctx.upload(new.samples, new.weights)
        return new

    def copy(self, label=None, settings=None):
        """mcsamples.py:308-322: an independent copy, optionally with another label and / or modified settings"""
        new = _copy.deepcopy(self)
        if label:
            new.label = label
        if settings is not None:
            new.needs_update = True
            new.updateSettings(settings)
        return new

    def _current_settings(self):
        """The settings in force, as a dict the constructor / updateSettings takes (an independent copy)."""
        out = {k: getattr(self, k) for k in DEFAULT_SETTINGS}
        out.update(no_warning_params=self.no_warning_params, no_warning_chi2_params=self.no_warning_chi2_params)
        if hasattr(self, "force_twotail"):
            out["force_twotail"] = self.force_twotail
        for i, v in getattr(self, "_max_frac_overrides", {}).items():
            out["max_frac_twotail%d" % (i + 1)] = v
        return _copy.deepcopy(out)

    def getCombinedSamplesWithSamples(self, samps2, sample_weights=(1, 1)):
        """
        mcsamples.py:2620-2660: a new MCSamples of this set's rows followed by ``samps2``'s, over the parameters of
        ``samps2`` that this set has too (``samps2``'s order, labels and derived flags).  By default the two sets carry the
        same total weight, times ``sample_weights``; ``sample_weights=None`` appends the weights as they are.  The new
        object goes through the constructor (ranges and settings of this set, nothing ignored), which uploads it.
        """
        mine = self.paramNames.list()
        pars = [p for p in samps2.paramNames.names if p.name in mine]
        loglikes = None
        if self.loglikes is not None and samps2.loglikes is not None:
            loglikes = np.concatenate([self.loglikes, samps2.loglikes])
        w1, w2 = self._host_weights(), samps2._host_weights()
        if sample_weights is None:
            fac, sample_weights = 1, (1, 1)
        else:
            fac = np.sum(w1) / np.sum(w2)
        weights = np.concatenate([w1 * sample_weights[0], w2 * sample_weights[1] * fac])
        samples = np.empty((self.numrows + samps2.numrows, len(pars)), order="F")  # the device layout: no transpose
        for k, p in enumerate(pars):
            samples[:self.numrows, k] = self.samples[:, self.index[p.name]]
            samples[self.numrows:, k] = samps2.samples[:, samps2.index[p.name]]
        new = MCSamples(samples=samples, weights=weights, loglikes=loglikes, names=[p.name for p in pars],
                        labels=[p.label if getattr(p, "_label_given", True) else None for p in pars], ignore_rows=0,
                        ranges=self.ranges, settings=self._current_settings(), device=self._device,
                        _context_factory=self._context_factory)
        derived = {p.name: p.isDerived for p in pars}
        for par in new.paramNames.names:  # (those the constructor kept: a parameter that never moves is a fixed range now)
            par.isDerived = derived[par.name]
        return new

    # ---- look-ups and small queries ----------------------------------------------------------------------------
    def getParamSampleDict(self, ix, want_derived=True, want_fixed=True):
        """mcsamples.py:2606-2618: the values of sample row ``ix`` by name, with those of the fixed parameters"""
        res = super().getParamSampleDict(ix, want_derived=want_derived)
        if want_fixed:
            res.update(self.ranges.fixedValueDict())
        return res

    def getParamBestFitDict(self, best_sample=False, want_derived=True, want_fixed=True, max_posterior=True):
        """mcsamples.py:2578-2604: the best-fit SAMPLE (``best_sample=True``: the row of the smallest loglike, as
        getParamSampleDict gives it); the best fit of a minimiser's files is outside this package."""
        if not best_sample:
            raise NotImplementedError("best-fit files are outside the accelerated path")
        if not max_posterior:
            raise ValueError("best_fit_sample is only maximum posterior")
        if self.loglikes is None:
            raise ValueError("No likelihoods in samples")
        return self.getParamSampleDict(np.argmin(self.loglikes))

    def getBounds(self):
        """mcsamples.py:2293-2309: the hard bounds the samples actually come near (a ParamBounds; a range the samples stay
        far from is no bound).  The reference reads the flags whatever density call last left them; here the range logic is
        run for every parameter first, as getMargeStats does."""
        if self.needs_update:
            self.updateBaseStatistics()
        self._init_params(list(range(self.n)))
        bounds = ParamBounds()
        bounds.names = self.paramNames.list()
        for par in self.paramNames.names:
            if par.has_limits_bot:
                bounds.lower[par.name] = par.limmin
            if par.has_limits_top:
                bounds.upper[par.name] = par.limmax
        return bounds

    def getCorrelatedVariable2DPlots(self, num_plots=12, nparam=None):
        """mcsamples.py:2533-2558: [x, y] names of the most correlated pairs among the first ``nparam`` parameters (default:
        the non-derived ones), strongest first.  The reference's scan: each pick is the largest |correlation| strictly
        below the previous pick, the first such pair in row order -- so of pairs that tie exactly only one is listed."""
        if self.needs_update:
            self.updateBaseStatistics()
        nparam = nparam or self.paramNames.numNonDerived()
        ix1, ix2 = np.triu_indices(nparam, 1)
        vals = np.abs(np.asarray(self.getCorrelationMatrix())[ix1, ix2])
        pairs, below = [], np.inf
        for _ in range(num_plots):
            left = vals < below  # (a NaN correlation never qualifies)
            if not left.any():
                break
            below = vals[left].max()
            k = int(np.nonzero(vals == below)[0][0])
            pairs.append([self.parName(int(ix1[k])), self.parName(int(ix2[k]))])
        return pairs

    def getNumSampleSummaryText(self):
        """mcsamples.py:887-901: rows, parameters and the measures of the effective number of samples, as text"""
        if self.needs_update:
            self.updateBaseStatistics()
        lines = "using %s rows, %s parameters; mean weight %s, tot weight %s\n" % (
            self.numrows, self.paramNames.numParams(), self.mean_mult, self.norm)
        if self.indep_thin != 0:
            lines += "Approx indep samples (N/corr length): %s\n" % (round(self.norm / self.indep_thin))
        lines += "Equiv number of single samples (sum w)/max(w): %s\n" % (round(self.norm / self.max_mult))
        lines += "Effective number of weighted samples (sum w)^2/sum(w^2): %s\n" % (int(self.norm**2 / self._sum_w2))
        return lines

    # ---- likelihood statistics (mcsamples.py:2216-2261, 2369-2378) ----------------------------------------------
    def _setLikeStats(self):
        """Best-fit sample, posterior likelihood statistics and the N-D confidence-region limits.  Two passes over the
        loglikes column on the device (gd_like_stats) give every weighted mean the reference forms from exp / square
        of that vector; the N-D limits come from _setNDLimits (weighted quantile + conditional min / max)."""
        if self.loglikes is None:
            self._likeStats = None
            return None
        ctx = self.ctx
        col = ctx.set_extra_column(ctx.EXTRA_COLS - 1, self.loglikes)
        self._loglikes_col = col  # (_setNDLimits below reads the same resident copy instead of uploading it again)
        try:  # whatever happens below, the column id must not outlive this call: the slot is rewritten by later uploads
            st = ctx.like_stats(col)
            norm = self.norm
            maxlike = st["min"]
            m = LikeStats()
            m.logLike_sample = maxlike
            m.logMeanInvLike = (np.log(st["sum_w_exp_plus"] / norm) + maxlike) if st["max"] - maxlike < 30 else None
            self.mean_loglike = st["sum_wl"] / norm  # chains.py:380-383
            m.meanLogLike = self.mean_loglike
            m.logMeanLike = -np.log(st["sum_w_exp_minus"] / norm) + maxlike
            m.complexity = 2 * (self.mean_loglike - maxlike)
            m.varLogLike = st["sum_wl2"] / norm - self.mean_loglike**2
            m.names = self.paramNames.names
            self._setNDLimits()
        finally:
            self._loglikes_col = None
        best = self._sample_row(st["argmin"])
        for j, par in enumerate(self.paramNames.names):
            par.bestfit_sample = best[j]
        self._likeStats = m
        return m

    @property
    def likeStats(self):
        """The reference sets this attribute inside updateBaseStatistics (mcsamples.py:552-576); here it is computed when first
        read after a change of the samples (three passes over the sample set) -- reading the attribute and calling
        getLikeStats() are the same thing, as are the parameters' ``bestfit_sample`` values it leaves."""
        return self._likeStats if self._likeStats is not None else self._setLikeStats()

    @likeStats.setter
    def likeStats(self, value):
        self._likeStats = value

    def getLikeStats(self):
        """mcsamples.py:2369-2378 (computed on first use after a change of the samples, not inside every
        updateBaseStatistics: it costs three passes over the sample set)"""
        return self.likeStats

    def _use_like_weights(self, mode):
        """
        Make the mean-likelihood weights resident on the device: mode 0 = weights*exp(mean_loglike - loglikes)
        (mcsamples.py:1560,1830), mode 1 = weights*loglikes (:1558).  mean_loglike (chains.py:380-383) falls out of
        the mode-1 pass as sum/norm.
        """
        if self.loglikes is None:
            raise MCSamplesError("mean likelihoods need the loglikes column")
        if self.mean_loglike is None:
            self.mean_loglike = self.ctx.like_weights(self.loglikes, 1, 0.0) / self.norm
            self._like_mode = 1
        if self._like_mode != mode:
            self.ctx.like_weights(self.loglikes, mode, self.mean_loglike)
            self._like_mode = mode

    def _like_histograms(self, mode, fn):
        """Run the histogram call ``fn`` with the like weights selected (np.bincount(..., weights=w) of :1561,1831)."""
        self._use_like_weights(mode)
        self.ctx.select_weights(1)
        try:
            return fn()
        finally:
            self.ctx.select_weights(0)

    def makeSingleSamples(self, filename="", single_thin=None, random_state=None):
        """
        mcsamples.py:578-606: unit-weight samples, each row chosen with probability weight / (max weight * single_thin);
        the same rows as the reference for the same ``random_state``.  ``single_thin`` defaults to what leaves about
        max_scatter_points rows.  Without ``filename`` the kept rows are gathered on the device (gd_gather_rows) and
        returned as a (K, n) array; with it they are formatted on the device (gd_format_rows) and written as text
        (weight 1, loglike, parameters), and nothing is returned -- that branch divides in the reference's other order, (weight / max weight) / single_thin.
        """
        if single_thin is None:
            single_thin = max(1, self.norm / self.max_mult / self.max_scatter_points)
        if not filename:
            buf, K = self._draw_single_rows(random_state, self.max_mult, single_thin, 0)
            try:
                return self.ctx.gather_rows(buf, K, np.arange(self.n))
            finally:
                buf.free()
        if self.loglikes is None:
            raise MCSamplesError("writing single samples needs the loglikes column")
        buf, K = self._draw_single_rows(random_state, self.max_mult, single_thin, 1)
        try:
            # weight 1, loglike, parameters as "%16.7E" with nothing between the fields (mcsamples.py:596-601), formatted
            # on the device from the row list the draw left there
            from . import chainfiles
            from ._lib import GD_FMT_SRC_ONE

            srcs = [GD_FMT_SRC_ONE, self.ctx.set_extra_column(self.ctx.EXTRA_COLS - 1, self.loglikes)] + list(range(self.n))

            def host_rows(index):
                return np.hstack((np.ones((len(index), 1)), self.loglikes[index].reshape(-1, 1), self.samples[index]))

            with open(filename, "wb") as f:
                chainfiles.write_text_rows(f, self.ctx, srcs, (buf, K), fmt="%16.7E", delimiter="", host_rows=host_rows)
        finally:
            buf.free()

    # ---- text export (mcsamples.py:637-666, 2662-2693) -------------------------------------------------------
    def saveTextMetadata(self, root, properties=None):
        """mcsamples.py:2662-2684: ``root.paramnames``, ``root.ranges`` and ``root.properties.ini`` -- the keys of an existing
        file, then ``self.properties``, the label and ``properties``; the file is removed when there is nothing to say."""
        from . import chainfiles

        super().saveTextMetadata(root)
        self.ranges.saveToFile(root + ".ranges")
        ini_name = root + ".properties.ini"
        own = getattr(self.properties, "params", self.properties)
        if properties or own or self.label:
            params = chainfiles.read_properties(ini_name) if os.path.exists(ini_name) else {}
            read_order = list(params)
            params.update(own or {})
            if self.label:
                params["label"] = self.label
            params.update(properties or {})
            chainfiles.write_properties(ini_name, params, read_order)
        elif os.path.exists(ini_name):
            os.remove(ini_name)

    def saveChainsAsText(self, root, make_dirs=False, properties=None):
        """mcsamples.py:2686-2693: ``root_1.txt, root_2.txt, ...``, one per chain of getSeparateChains (row ranges of the
        resident set: what thin / filter / reweighting left there is what is saved), then the metadata files."""
        sources = self._text_sources()
        for i, chain in enumerate(self.getSeparateChains()):
            chain.saveAsText(root, i, make_dirs, _sources=sources)
        self.saveTextMetadata(root, properties)

    def writeCovMatrix(self, filename=None):
        """mcsamples.py:637-657, covmat.py:41-49: ``# name1 name2 ...`` of the non-derived parameters, then their covariance
        as "%15.7E" rows; default ``rootdirname + ".covmat"``.  An n x n matrix: np.savetxt on the host, as the reference."""
        n = self.paramNames.numNonDerived()
        with open(filename or self.rootdirname + ".covmat", "wb") as f:
            f.write(("# " + " ".join(self.paramNames.list()[:n]) + "\n").encode("UTF-8"))
            np.savetxt(f, self.fullcov[:n, :n], "%15.7E")

    def writeCorrelationMatrix(self, filename=None):
        """mcsamples.py:659-666: the correlation matrix as "%15.7E" rows (np.savetxt on the host: n x n); default
        ``rootdirname + ".corr"``"""
        np.savetxt(filename or self.rootdirname + ".corr", self.getCorrelationMatrix(), fmt="%15.7E")

    def getFractionIndices(self, weights, n):
        """mcsamples.py:668-680: row indices splitting the total weight into n equal parts"""
        if weights is None:
            weights = np.ones(self.numrows)
        cumsum = np.cumsum(weights)
        return np.append(np.searchsorted(cumsum, np.linspace(0, 1, n, endpoint=False) * self.norm), self.numrows)

    def getConvergeTests(self, test_confidence=0.95, writeDataToFile=False,
                         what=("MeanVar", "GelmanRubin", "SplitTest", "RafteryLewis", "CorrLengths"), filename=None,
                         feedback=False):
        """
        mcsamples.py:904-1221: the report text of the convergence tests (same defaults as the reference; "CorrSteps" is
        opt-in there too).  Sets self.GelmanRubin, self.indep_thin, self.RL_indep_thin like the reference.  Every
        N-sized pass behind the numbers (chain covariances, quantiles on row sub-ranges, lag sums, thinning, transition
        counts) runs on the GPU; this function only formats.
        """
        if writeDataToFile or filename:
            raise NotImplementedError("file output is outside the accelerated path")
        for w in what:
            if w not in ("MeanVar", "GelmanRubin", "SplitTest", "CorrLengths", "RafteryLewis", "CorrSteps"):
                raise NotImplementedError("convergence test %s is outside the accelerated path" % w)
        lines = ""
        nchains = 0 if self.chain_offsets is None else len(self.chain_offsets) - 1
        if "CorrLengths" in what:
            lines += ("Parameter autocorrelation lengths (effective number of samples N_eff = tot weight/weight length)\n\n"
                      + "%-20s%15s %15s %15s\n" % ("", "Weight Length", "Sample length", "N_eff"))
            for nm, Nw in zip(self.paramNames.list(), self.getCorrLengths()):
                form = "%15.2f" if self.mean_mult > 1 else "%15.2E"
                lines += "%-20s" % nm + form % Nw + " %15.2f %15i\n" % (Nw / self.mean_mult, self.norm / Nw)
            lines += "\n"
        if nchains > 1 and "MeanVar" in what:
            lines += "\nmean convergence stats using remaining chains\nparam sqrt(var(chain mean)/mean(chain var))\n\n"
            for nm, v in zip(self.paramNames.list(), self.getMeanVarTest()):
                lines += "%-20s%10.4f\n" % (nm, v)
            lines += "\n"
        if nchains > 1 and "GelmanRubin" in what:
            D = self.getGelmanRubinEigenvalues()
            if D is not None:
                self.GelmanRubin = np.max(D)
                lines += "var(mean)/mean(var) for eigenvalues of covariance of y of orthonormalized parameters\n"
                for jj, Di in enumerate(D):
                    lines += "%3i%13.5f\n" % (jj + 1, Di)
                summary = " var(mean)/mean(var), remaining chains, worst e-value: R-1 = %13.5F" % self.GelmanRubin
            else:
                self.GelmanRubin = None
                summary = "Gelman-Rubin covariance not invertible (parameter not moved?)"
                logging.warning(summary)
            if feedback:
                print(summary)
            lines += "\n"
        if "SplitTest" in what:
            lines += "Split tests: rms_n([delta(upper/lower quantile)]/sd) n={2,3,4}, limit=%.0f%%:\n" % (
                100 * self.converge_test_limit)
            lines += "i.e. mean sample splitting change in the quantiles in units of the st. dev.\n\n"
            st = self.getSplitTests(test_confidence)
            for j, nm in enumerate(self.paramNames.list()):
                for endb, typestr in enumerate(["upper", "lower"]):
                    lines += "%-20s" % nm + "".join("%9.4f" % st[j, ix, endb] for ix in range(st.shape[1])) + " %s\n" % typestr
            lines += "\n"
        # mcsamples.py:1039: the remaining two tests need integer weights (raw MCMC multiplicities)
        if ("RafteryLewis" in what or "CorrSteps" in what) and self.ctx.weights_integral():
            if "RafteryLewis" in what:
                rl = self.getRafteryLewis(test_confidence)
                if rl is None:
                    print("Raftery and Lewis estimator had problems")
                    return None
                lines += "Raftery&Lewis statistics\n\nchain  markov_thin  indep_thin    nburn\n"
                for ix in range(len(rl["thin_fac"])):
                    if rl["thin_fac"][ix] == 0:
                        lines += "%4i      Failed/not enough samples\n" % ix
                    else:
                        lines += "%4i%12i%12i%12i\n" % (ix, rl["markov_thin"][ix], rl["thin_fac"][ix], rl["nburn"][ix])
                if feedback:
                    if not np.all(rl["thin_fac"] != 0):
                        print("RL: Not enough samples to estimate convergence stats")
                    else:
                        print("RL: Thin for Markov: ", np.max(rl["markov_thin"]))
                        print("RL: Thin for indep samples:  ", str(self.RL_indep_thin))
                        print("RL: Estimated burn in steps: ", np.max(rl["nburn"]), " (",
                              int(round(np.max(rl["nburn"]) / self.mean_mult)), " rows)")
                lines += "\n"
            if "CorrSteps" in what:
                lines += "Parameter auto-correlations as function of step separation\n\n"
                thin, corrs = self.getCorrSteps()
                if corrs is not None:
                    lines += "%-20s" % "" + "".join("%8i" % ((i + 1) * thin) for i in range(corrs.shape[0])) + "\n"
                    for j, nm in enumerate(self.paramNames.list()):
                        lines += "%-20s" % nm + "".join("%8.3f" % corrs[i][j] for i in range(corrs.shape[0])) + " \n"
        return lines

    def updateSettings(self, settings=None, ini=None, doUpdate=True):
        """mcsamples.py:472-499: analysis settings from a dict and / or a .ini file (the dict takes preference)"""
        if ini is not None:
            settings = dict(_read_ini_settings(ini), **(settings or {}))
        for k, v in (settings or {}).items():
            if k == "force_twotail":
                self.force_twotail = v in (True, "T", "t", "True", "true", 1)
                if self.force_twotail:
                    logging.warning("Computing two tail limits")
                continue
            if k.startswith("max_frac_twotail") and k[len("max_frac_twotail"):].isdigit():
                self._max_frac_overrides = dict(getattr(self, "_max_frac_overrides", {}))
                self._max_frac_overrides[int(k[len("max_frac_twotail"):]) - 1] = float(v)
                continue
            if k == "no_warning_params":  # (ini: a space-separated list, mcsamples.py:438)
                self.no_warning_params = v.split() if isinstance(v, str) else list(v)
                continue
            if k == "no_warning_chi2_params":
                self.no_warning_chi2_params = v in (True, "T", "t", "True", "true", 1)
                continue
            if k not in DEFAULT_SETTINGS:
                raise SettingError("unknown setting: %s" % k)
            cur = DEFAULT_SETTINGS[k]
            if isinstance(cur, bool):
                v = v in (True, "T", "t", "True", "true", 1)
            elif isinstance(cur, int) and not isinstance(v, bool):
                v = int(v)
            elif isinstance(cur, float):
                v = float(v)
            setattr(self, k, v)
        if doUpdate:
            self.needs_update = True

    def setRanges(self, ranges):
        """mcsamples.py:324-346"""
        if isinstance(ranges, dict):
            for nm, rng in ranges.items():
                self.ranges.setRange(nm, rng)
        else:
            for nm, rng in zip(self.paramNames.list(), ranges):
                self.ranges.setRange(nm, rng)
        self.needs_update = True

    def _after_base_statistics(self):
        self.density1D = {}
        self._initLimits()
        for par in self.paramNames.names:
            par.N_eff_kde = None
            par._ranges_done = False
        self._nd_limits_done = False
        self._marge_done = None
        self.likeStats = None
        self.needs_update = False

    def _initLimits(self):
        """mcsamples.py:442-470"""
        for par in self.paramNames.names:
            par.limmin = self.ranges.getLower(par.name)
            par.limmax = self.ranges.getUpper(par.name)
            par.has_limits_bot = par.limmin is not None
            par.has_limits_top = par.limmax is not None
            par.periodic = par.name in self.ranges.periodic

    # batched 2D calls of this many pairs convolve their batches on two streams (below: not worth a second context's
    # plans and scratch; above: one batch fills the chip)
    CONV_TWO_STREAMS_PAIRS = (64, 400)
    # large calls: the share of the base grid's pairs whose bandwidths are optimised first, so that their convolution
    # (second stream) runs beside the optimisation of the rest
    KOPT_FIRST_FRACTION = 0.5
    KOPT_SPLIT_MIN = 256  # ... when the launch has at least this many pairs

    def _get1DNeff(self, par, param):
        """mcsamples.py:1230-1235"""
        if par.N_eff_kde is None:
            par.N_eff_kde = self.getEffectiveSamplesGaussianKDE(param, scale=par.sigma_range)
        return par.N_eff_kde

    # ---- ranges and limits (mcsamples.py:1421-1498) --------------------------------------------------------
    def _initParamRanges(self, j, paramConfid=None):
        self._init_params([self._col(j)])
        return self.paramNames.names[self._col(j)]

    def _setNDLimits(self):
        """
        The N-dimensional confidence-region limits of _setLikeStats (mcsamples.py:2263-2274): per contour, min / max of
        every parameter over the best-likelihood samples holding that fraction of the weight.  The reference argsorts
        loglikes; here the weighted quantile of the loglikes column (gd_quantiles) is the likelihood of the first
        sample outside the region, and one conditional min/max pass per contour (gd_col_minmax) does the rest.  Rows
        tied with that threshold are all excluded (the reference keeps an arbitrary subset of them).
        """
        if self._nd_limits_done:
            return
        ctx = self.ctx
        col = getattr(self, "_loglikes_col", None)  # (resident already when _setLikeStats is the caller)
        if col is None:
            col = ctx.set_extra_column(ctx.EXTRA_COLS - 1, self.loglikes)
        contours = np.asarray(self.contours, dtype=np.float64)
        thr = ctx.quantiles([col], (self.norm * contours)[None, :])[0]
        lims = np.empty((len(contours), self.n, 2))
        for i, (c, t) in enumerate(zip(contours, thr)):
            lims[i] = ctx.col_minmax(list(range(self.n)), cond_col=-1 if c >= 1 else col, cond_below=t)
        for j, par in enumerate(self.paramNames.names):
            par.ND_limit_bot = lims[:, j, 0].copy()
            par.ND_limit_top = lims[:, j, 1].copy()
        self._nd_limits_done = True

    def _init_params(self, js, lag_probe=False, ahead=0):
        """_initParam for several parameters with ONE batched quantile-select launch.  ``lag_probe``: the select's counting
        pass also delivers the autocovariance probe of the N_eff estimate for the same columns (one read of the samples
        serves both; kept in ``_lag_prefetch`` for _probe_lags / the batched 2D entry).  ``ahead``: what the library may
        enqueue for the next batched 2D call once the quantiles are known (gd_prepare_params)."""
        todo = [j for j in dict.fromkeys(js) if not getattr(self.paramNames.names[j], "_ranges_done", False)]
        if not todo:
            return
        rc = self.range_confidence
        fracs = np.array([rc, 1 - rc] + list(np.linspace(0.1, 0.9, 9)))
        targets = np.tile(self.norm * fracs, (len(todo), 1))
        if (lag_probe and hasattr(self.ctx, "prepare_params") and getattr(self, "_col_min", None) is not None
                and not (self.range_ND_contour >= 0 and self.loglikes is not None)):
            return self._init_params_native(todo, targets, ahead)
        if lag_probe:
            q, lags = self.ctx.quantiles_probe(todo, targets, self._minmax_of(todo), self.means[todo])
            q = np.asarray(q)
            if lags is not None:
                self._lag_prefetch = (todo, 8, _Done(lags))
        else:
            q = np.asarray(self.ctx.quantiles(todo, targets, minmax=self._minmax_of(todo)))
        # mcsamples.py:1440-1452 for all parameters at once: [param_min, deciles 0.1..0.9, param_max], spans of four
        err_v = np.asarray(self.sddev)[todo]
        confids = np.empty_like(q)
        confids[:, 0] = np.asarray(self._col_min)[todo]
        confids[:, 1:-1] = q[:, 2:]
        confids[:, -1] = np.asarray(self._col_max)[todo]
        diffs = confids[:, 4:] - confids[:, :-4]
        scale_v = np.min(diffs, axis=1) / 1.049
        flat_v = (np.all(diffs > (err_v * 1.049)[:, None], axis=1) & np.all(diffs < (scale_v * 1.5)[:, None], axis=1)).tolist()
        for row, j in enumerate(todo):
            par = self.paramNames.names[j]
            par.err = self.sddev[j]
            par.mean = self.means[j]
            par.param_min = self._col_min[j]
            par.param_max = self._col_max[j]
            par.range_min, par.range_max = q[row, 0], q[row, 1]
            scale = scale_v[row]
            if flat_v[row]:
                par.sigma_range = scale  # very flat
            else:
                par.sigma_range = min(par.err, scale)
            if self.range_ND_contour >= 0 and self.loglikes is not None:  # mcsamples.py:1455-1459
                self._setNDLimits()
                if self.range_ND_contour >= par.ND_limit_bot.size:
                    raise SettingError("range_ND_contour should be -1 (off), or an index into the computed contour levels")
                par.range_min = min(max(par.range_min - par.err, par.ND_limit_bot[self.range_ND_contour]), par.range_min)
                par.range_max = max(max(par.range_max + par.err, par.ND_limit_top[self.range_ND_contour]), par.range_max)
            smooth_1D = par.sigma_range * 0.4
            if par.has_limits_bot:
                if par.range_min - par.limmin > 2 * smooth_1D and par.param_min - par.limmin > smooth_1D:
                    par.has_limits_bot = False  # long way from limit
                else:
                    par.range_min = par.limmin
            if par.has_limits_top:
                if par.limmax - par.range_max > 2 * smooth_1D and par.limmax - par.param_max > smooth_1D:
                    par.has_limits_top = False
                else:
                    par.range_max = par.limmax
            if not par.has_limits_bot:
                par.range_min -= smooth_1D * 2
            if not par.has_limits_top:
                par.range_max += smooth_1D * 2
            par.has_limits = par.has_limits_top or par.has_limits_bot
            par._ranges_done = True

    def _init_params_native(self, todo, targets, ahead):
        """_init_params through gd_prepare_params: the select, the probe and the scalar tail in one native call (the same fp64
        operations in the same order, csrc/batch2d.hpp prepare_tail); only the attributes are stored here."""
        names = self.paramNames.names
        pars = [names[j] for j in todo]
        nan = np.nan
        limits = np.array([[nan if p.limmin is None else p.limmin, nan if p.limmax is None else p.limmax] for p in pars])
        twin = None
        if (ahead & 2 and self._lane == 0 and self._context_factory is not None and self.weights is None
                and len(todo) * (len(todo) - 1) // 2 >= min(64, self.CONV_TWO_STREAMS_PAIRS[0])):
            twin = self._twin_context()  # (the batched call's second stream: the index columns are made on it)
        q, lags, recs = self.ctx.prepare_params(
            todo, targets, self._minmax_of(todo), self.means[todo], np.asarray(self.vars)[todo], np.asarray(self.sddev)[todo],
            limits, [bool(p.has_limits_bot) for p in pars], [bool(p.has_limits_top) for p in pars], twin=twin,
            fine_bins_2D=self.fine_bins_2D, auto_bandwidth=self.smooth_scale_2D < 0 and not self.use_effective_samples_2D,
            uncorrelated_sampler=self.sampler in ("nested", "uncorrelated"), ahead=ahead if twin is not None else ahead & 1)
        if lags is not None:
            self._lag_prefetch = (todo, 8, _Done(lags))
        for row, (j, par) in enumerate(zip(todo, pars)):
            par.err = self.sddev[j]
            par.mean = self.means[j]
            par.param_min = self._col_min[j]
            par.param_max = self._col_max[j]
            par.range_min, par.range_max = recs["range_min"][row], recs["range_max"][row]
            par.sigma_range = recs["sigma_range"][row]
            par.has_limits_bot, par.has_limits_top = bool(recs["has_limits_bot"][row]), bool(recs["has_limits_top"][row])
            par.has_limits = par.has_limits_top or par.has_limits_bot
            par._ranges_done = True

    def prepareParams(self, params=None, neff=True):
        """
        Additive API: compute the per-parameter state every density needs (ranges, limits, sigma_range and, if
        ``neff``, the KDE effective sample number) for ``params`` (default all).  The reference recomputes this inside
        every density call (mcsamples.py:1786-1787); it is a pure function of the column, so doing it once is
        result-preserving.
        """
        if self.needs_update:
            self.updateBaseStatistics()
        js = list(range(self.n)) if params is None else [self._col(p) for p in params]
        todo = [j for j in js if self.paramNames.names[j].N_eff_kde is None]
        # the autocovariance probe of the N_eff estimate needs the means only.  Round 6: it rides on the counting pass of the
        # quantile select (gd_quantiles_mm_probe: one read of the columns for both) when every parameter that needs it is
        # about to go through that select; else, as before, it runs on the second context beside the select
        fused = (bool(todo) and self.sampler not in ("nested", "uncorrelated") and self.numrows // 10 + 1 >= 8
                 and hasattr(self.ctx, "quantiles_probe") and os.environ.get("GETDIST_AMD_FUSED_PROBE", "1") == "1"
                 and all(not getattr(self.paramNames.names[j], "_ranges_done", False) for j in todo))
        if fused:
            # neff=False: the caller does not wait for N_eff here -- the library may start its lag sums (and the index columns
            # of the base grid) behind the select, for the batched 2D call to pick up (GDHIP_PREPARE_AHEAD=0: it does not)
            ahead = 3 if (not neff and getattr(self, "_neff_share", None) is None
                          and os.environ.get("GDHIP_PREPARE_AHEAD", "1") != "0") else 0
            with _Phase(self, "prep.ranges"):
                self._init_params(js, lag_probe=True, ahead=ahead)
        elif (todo and self._lane == 0 and not self._timing and self.sampler not in ("nested", "uncorrelated")
                and len(todo) >= 2 and os.environ.get("GETDIST_AMD_OVERLAP_NEFF", "1") == "1"):
            # the autocovariance probe of the N_eff estimate depends on the means only: start it on the second context
            # (own stream) while this one runs the quantile select
            twin = self._second_lane()
            self._nlanes = 1
            nl = min(8, self.numrows // 10 + 1)
            self._lag_prefetch = (todo, nl, self._lane_thread(twin).submit(
                twin.ctx.autocov_lags_batch, todo, self.means[todo], 0, nl))
        with _Phase(self, "prep.ranges"), _FastThreadSwitch(getattr(self, "_lag_prefetch", None) is not None):
            self._init_params(js)
        _hostlog("prep: ranges done")
        if neff:
            with _Phase(self, "prep.neff"):
                self._neff_batch(js)
            _hostlog("prep: N_eff done")
        return js

    def _bin_edge_arrays(self, js, borderfrac=0.1):
        """binmin, binmax of _bin_edges for the parameters ``js``, as arrays indexed by parameter number (the same
        fp64 operations, element by element)."""
        names = self.paramNames.names
        n = max(js) + 1
        rmin, rmax, pmin, pmax = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
        lim_b, lim_t = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        for j in js:
            p = names[j]
            rmin[j], rmax[j], pmin[j], pmax[j] = p.range_min, p.range_max, p.param_min, p.param_max
            lim_b[j], lim_t[j] = bool(p.has_limits_bot), bool(p.has_limits_top)
        border = (rmax - rmin) * borderfrac
        binmin = np.minimum(pmin, rmin)
        binmin = np.where(lim_b, binmin, binmin - border)
        binmax = np.maximum(pmax, rmax)
        binmax = np.where(lim_t, binmax, binmax + border)
        return binmin, binmax

    @staticmethod
    def _bin_edges(par, num_fine_bins, borderfrac=0.1):
        """The scalar half of _binSamples (mcsamples.py:1486-1496); the index half runs fused in the kernels."""
        border = (par.range_max - par.range_min) * borderfrac
        binmin = min(par.param_min, par.range_min)
        if not par.has_limits_bot:
            binmin -= border
        binmax = max(par.param_max, par.range_max)
        if not par.has_limits_top:
            binmax += border
        fine_width = (binmax - binmin) / (num_fine_bins - 1)
        return fine_width, binmin, binmax

    # ---- 1D densities (mcsamples.py:1237-1283, 1500-1686) ---------------------------------------------------
    def getAutoBandwidth1D(self, bins, par, param, mult_bias_correction_order=None, kernel_order=1, N_eff=None):
        if N_eff is None:
            N_eff = self._get1DNeff(par, param)
        h, status = self.ctx.isj1d(np.asarray(bins, dtype=np.float64)[None, :], [N_eff])
        return self._bandwidth_1d(None if status[0] else h[0], par, N_eff, mult_bias_correction_order, kernel_order)

    def _no_bandwidth_warning(self, par):
        """mcsamples.py:1259-1261: parameters for which a failed / very small 1D bandwidth neither warns nor raises."""
        return par.name in self.no_warning_params or (
            bool(self.no_warning_chi2_params) and ("chi2_" in par.name or "minuslog" in par.name))

    def _bandwidth_1d(self, h, par, N_eff, mult_bias_correction_order, kernel_order):
        """The scalar tail of getAutoBandwidth1D (mcsamples.py:1256-1283) given the device's ISJ solution ``h`` (None
        where the solver failed): rule-of-thumb fallback when it failed or is very small, higher-order rescaling."""
        if h is None:
            logging.warning("1D auto bandwidth failed. Using fallback: zero f in _bandwidth_fixed_point (non-convergence)")
        bin_range = max(par.param_max, par.range_max) - min(par.param_min, par.range_min)
        if h is None or h < 0.01 * N_eff ** (-1.0 / 5) * (par.range_max - par.range_min) / bin_range:
            hnew = 1.06 * par.sigma_range * N_eff ** (-1.0 / 5) / bin_range
            if not self._no_bandwidth_warning(par):
                msg = f"auto bandwidth for {par.name} very small or failed (h={h},N_eff={N_eff}). Using fallback (h={hnew})"
                if self.raise_on_bandwidth_errors:
                    raise BandwidthError(msg)
                logging.warning(msg)
            h = hnew
        par.kde_h = h
        m = self.mult_bias_correction_order if mult_bias_correction_order is None else mult_bias_correction_order
        if kernel_order > 1:
            m = max(m, 1)
        if m:
            return h * N_eff ** (1.0 / 5 - 1.0 / (4 * m + 5))
        return h

    def get1DDensity(self, name, **kwargs):
        if self.needs_update:
            self.updateBaseStatistics()
        if not kwargs:
            j, par = self._parAndNumber(name)
            if par is not None and par.name in self.density1D:
                return self.density1D[par.name]
        return self.get1DDensityGridData(name, **kwargs)

    def get1DDensityGridData(self, j, paramConfid=None, meanlikes=False, **kwargs):
        if self.needs_update:
            self.updateBaseStatistics()
        j = self._parAndNumber(j)[0]
        if j is None:
            return None
        return self.get1DDensities([j], meanlikes=meanlikes, **kwargs)[0]

    def get1DDensities(self, params=None, meanlikes=False, **kwargs):
        """
        Batched 1D KDEs (additive API): a list of Density1D, one per entry of ``params`` (default: all); with
        ``meanlikes`` each carries the mean-likelihood profile ``likes`` (mcsamples.py:1556-1561,1672-1682).
        """
        if self.needs_update:
            self.updateBaseStatistics()
        for k in kwargs:
            if k not in ("smooth_scale_1D", "boundary_correction_order", "mult_bias_correction_order", "fine_bins",
                         "num_bins"):
                raise SettingError("unknown 1D density argument %s" % k)
        js = list(range(self.n)) if params is None else [self._col(p) for p in params]
        num_bins = kwargs.get("num_bins", self.num_bins)
        smooth_scale_1D = kwargs.get("smooth_scale_1D", self.smooth_scale_1D)
        bco = kwargs.get("boundary_correction_order", self.boundary_correction_order)
        mbc = kwargs.get("mult_bias_correction_order", self.mult_bias_correction_order)
        fine_bins = kwargs.get("fine_bins", self.fine_bins)
        if bco > 2:
            raise SettingError("Unknown boundary_correction_order (expected 0, 1, 2)")
        self._init_params(js)
        pars = [self.paramNames.names[j] for j in js]
        if hasattr(self.ctx, "density1d_batch") and os.environ.get("GETDIST_AMD_NATIVE_BATCH", "1") == "1":
            # ONE native call (csrc/batch1d.hpp) for every case: in a multi-rank job this rank's share of the N_eff values and
            # the exchange happen first (the call then finds every value), a parameter listed twice is computed once
            from . import batch1d

            if getattr(self, "_neff_share", None) is not None and smooth_scale_1D <= 0:
                self._neff_batch(js)
            uniq = list(dict.fromkeys(js))
            P, hist, meta = batch1d.run(self, uniq, fine_bins, num_bins, smooth_scale_1D, bco, mbc, want_hist=meanlikes)
            if len(uniq) != len(js):
                at = {j: b for b, j in enumerate(uniq)}
                rows = [at[j] for j in js]
                P, meta = P[rows], meta[rows]
                hist = None if hist is None else hist[rows]
            edges = [((meta[b, 1] - meta[b, 0]) / (fine_bins - 1), meta[b, 0], meta[b, 1]) for b in range(len(js))]
            smooth, winw = meta[:, 3].tolist(), meta[:, 4].astype(np.int64).tolist()
            flags = [(1 if par.has_limits_bot else 0) | (2 if par.has_limits_top else 0) | (4 if par.periodic else 0)
                     for par in pars]
            return self._finish_1d(js, pars, edges, P, hist, smooth, winw, flags, fine_bins, meanlikes, kwargs)
        # (no native entry on this context: the Python-planned sequence is tests/planned_route.py, as for the 2D path)
        route = getattr(MCSamples, "_planned_route_1d", None)
        if route is None:
            raise MCSamplesError("get1DDensities needs a device context with gd_density1d_batch (libgdhip)")
        return route(self, js, pars, fine_bins, num_bins, smooth_scale_1D, bco, mbc, meanlikes, kwargs)

    def _finish_1d(self, js, pars, edges, P, hist, smooth, winw, flags, fine_bins, meanlikes, kwargs):
        """Mean-likelihood profiles (mcsamples.py:1556-1561,1672-1682) and the Density1D objects of get1DDensities."""
        likes = None
        if meanlikes:
            shade = bool(self.shade_likes_is_mean_loglikes)
            likehist = self._like_histograms(1 if shade else 0, lambda: self.ctx.hist1d(
                js, [e[1] for e in edges], [e[0] for e in edges], fine_bins))
            likes, _ = self.ctx.likes1d(hist, likehist, P, smooth, winw, flags, shade)
        out = []
        for b, (j, par) in enumerate(zip(js, pars)):
            fine_width, binmin, binmax = edges[b]
            d = Density1D(np.linspace(binmin, binmax, fine_bins), P=P[b].copy(), view_ranges=[par.range_min, par.range_max])
            d.likes = None if likes is None else likes[b].copy()
            if not kwargs:
                self.density1D[par.name] = d
            out.append(d)
        return out

    # ---- raw N-D densities (mcsamples.py:2012-2235) ---------------------------------------------------------------
    def getRawNDDensity(self, xs, normalized=False, **kwargs):
        """DensityND of the unsmoothed histogram of the parameters ``xs`` (mcsamples.py:2094-2108): maximum 1, or with
        ``normalized`` divided by DensityND.integrate.  kwargs as getRawNDDensityGridData."""
        if self.needs_update:
            self.updateBaseStatistics()
        density = self.getRawNDDensityGridData(xs, get_density=True, **kwargs)
        if density is not None and normalized:
            density.normalize(in_place=True)
        return density

    def getRawNDDensityGridData(self, js, writeDataToFile=False, num_plot_contours=None, get_density=False,
                                meanlikes=False, maxlikes=False, **kwargs):
        """
        Unsmoothed N-D marginalised density of the parameters ``js`` (mcsamples.py:2111-2235): a DensityND with maximum 1,
        ``contours`` (unless ``get_density``), ``likes`` (mean likelihoods, maximum 1) with ``meanlikes``, and ``maxlikes``
        (profile likelihood exp(min L - L_bin)) with ``maxcontours`` with ``maxlikes``.  None when a parameter is unknown.
        kwargs: ``num_bins_ND`` and ``boundary_correction_order``.  ``writeDataToFile`` is not supported (this package
        writes no plot-data files, for 1D and 2D densities neither) and raises NotImplementedError.
        """
        if writeDataToFile:
            raise NotImplementedError("writeDataToFile: this package writes no plot-data files")
        if self.needs_update:
            self.updateBaseStatistics()
        return self.getRawNDDensities([js], num_plot_contours=num_plot_contours, get_density=get_density,
                                      meanlikes=meanlikes, maxlikes=maxlikes, **kwargs)[0]

    def getRawNDDensities(self, param_lists, num_plot_contours=None, get_density=False, meanlikes=False, maxlikes=False,
                          **kwargs):
        """
        Batched getRawNDDensityGridData (additive API): one DensityND (or None where a parameter is unknown) per list of
        parameters in ``param_lists``; the lists may differ in length.  Every histogram of a batch comes from ONE native
        call (gd_histnd_batch): each parameter's index column is made once and shared by the densities that use it.
        """
        if self.needs_update:
            self.updateBaseStatistics()
        for k in kwargs:
            if k not in ("num_bins_ND", "boundary_correction_order"):
                raise SettingError("unknown N-D density argument %s" % k)
        if (meanlikes or maxlikes) and self.loglikes is None:
            raise MCSamplesError("mean / profile likelihoods need the loglikes column")
        nb = int(kwargs.get("num_bins_ND", self.num_bins_ND))
        bco = kwargs.get("boundary_correction_order", self.boundary_correction_order)
        jlists = []
        for js in param_lists:
            jv = [self._parAndNumber(j)[0] for j in js]
            jlists.append(None if None in jv else jv)
        todo = [b for b, jv in enumerate(jlists) if jv is not None]
        out = [None] * len(jlists)
        if not todo:
            return out
        if nb < 2:
            raise SettingError("num_bins_ND must be at least 2")
        from ._lib import GD_HISTND_MAX_BINS, GD_HISTND_MAXD

        for b in todo:
            if len(jlists[b]) > GD_HISTND_MAXD or nb ** len(jlists[b]) > GD_HISTND_MAX_BINS:
                raise SettingError("raw N-D grid of %d^%d bins is above the limit of %d" % (nb, len(jlists[b]),
                                                                                          GD_HISTND_MAX_BINS))
        self._init_params([j for b in todo for j in jlists[b]])
        names = self.paramNames.names
        edges = {j: self._bin_edges(names[j], nb) for b in todo for j in jlists[b]}
        want_likes = meanlikes and not get_density
        want_max = maxlikes and not get_density
        if want_likes:
            self._use_like_weights(0)
        ll_col = self.ctx.set_extra_column(self.ctx.EXTRA_COLS - 1, self.loglikes) if want_max else -1
        if want_max:
            bestfit = np.max(-self.loglikes)
        # batches of at most _ND_BATCH_BINS grid entries (one native call each)
        batches, cur, bins = [], [], 0
        for b in todo:
            M = nb ** len(jlists[b])
            if cur and bins + M > self._ND_BATCH_BINS:
                batches.append(cur)
                cur, bins = [], 0
            cur.append(b)
            bins += M
        batches.append(cur)
        for batch in batches:
            dims = [len(jlists[b]) for b in batch]
            cols = [j for b in batch for j in jlists[b]]
            H, HL, Lmin = self.ctx.histnd_batch(dims, cols, [edges[j][1] for j in cols], [edges[j][0] for j in cols], nb,
                                                want_h=True, want_likes=want_likes, want_lmin=want_max, loglike_col=ll_col)
            at = 0
            for b, d in zip(batch, dims):
                M = nb ** d
                grids = [None if g is None else g[at:at + M].reshape((nb,) * d) for g in (H, HL, Lmin)]
                at += M
                out[b] = self._finish_nd(jlists[b], nb, bco, grids, num_plot_contours, get_density,
                                         bestfit if want_max else None)
        return out

    _ND_BATCH_BINS = 1 << 24  # grid entries per native call (8 bytes per entry and output on the device and the host)

    def _finish_nd(self, jv, nb, bco, grids, num_plot_contours, get_density, bestfit):
        """The host tail of getRawNDDensityGridData (mcsamples.py:2150-2197) for one density from its device grids."""
        from .densities import DensityND, getContourLevels

        binsND, likes, Lmin = grids
        parv = [self.paramNames.names[j] for j in jv]
        ndim = len(parv)
        if any(p.has_limits for p in parv) and bco >= 0:
            prior_mask = np.ones((nb,) * ndim)
            _set_raw_edge_mask_nd(parv, prior_mask)
            binsND /= prior_mask
        xv = []
        for p in parv:
            _, binmin, binmax = self._bin_edges(p, nb)
            xv.append(np.linspace(binmin, binmax, nb))
        views = [(p.range_min, p.range_max) for p in parv]
        density = DensityND(xv, binsND, view_ranges=views)
        density.normalize("max", in_place=True)
        if get_density:
            return density
        ncontours = len(self.contours)
        if num_plot_contours:
            ncontours = min(num_plot_contours, ncontours)
        contours = self.contours[:ncontours]
        density.contours = density.getContourLevels(contours)
        if likes is not None:
            likes /= np.max(likes)
            density.likes = likes
        if Lmin is not None:
            # max over a bin of exp(-bestfit - L) (the reference's loop, :2165-2171) = exp(-bestfit - min L): the
            # subtraction and exp are monotone; an empty bin (+inf) gives 0, the loop's starting value
            density.maxlikes = np.exp(-bestfit - Lmin)
            density.maxcontours = getContourLevels(density.maxlikes, contours, half_edge=False)
        return density

    # ---- principal components (mcsamples.py:682-885) -----------------------------------------------------------
    def PCA(self, params, param_map=None, normparam=None, writeDataToFile=False, filename=None, conditional_params=(),
            n_best_only=None):
        """
        Principal component analysis of the parameters ``params`` (names not in the sample set are dropped), optionally
        mapped (``param_map``: one of N, L (log), M (log of the negation) per parameter; by default L unless a parameter's
        maximum is negative or its minimum is below a tenth of its range) and conditional on fixed values of
        ``conditional_params``.  ``normparam`` gives that parameter unit power in every component (default: the largest).
        Returns the text of mcsamples.py:682-885, or with ``n_best_only`` the tightest component's summary (1) or a list of
        the ``n_best_only`` tightest; ``writeDataToFile`` writes the text to ``filename`` or ``rootdirname + ".PCA"``.
        The O(N) passes run on the device (gd_pca_corr: means, standard deviations and the correlation matrix of the
        mapped columns; gd_pca_project: the projected components' means, standard deviations and correlations); the
        eigen-decomposition and the text stay on the host.
        """
        if self.needs_update:
            self.updateBaseStatistics()
        if getattr(self, "_column_share", None) is not None:
            raise NotImplementedError("PCA needs every column resident on one device: this context holds only its rank's "
                                      "share of the columns (multi-GPU PCA is not supported)")
        logging.info("Doing PCA for %s parameters", len(params))
        if len(conditional_params):
            logging.info("conditional %u fixed parameters", len(conditional_params))
        text = "PCA for parameters:\n"
        params = [name for name in params if self.paramNames.parWithName(name)]
        nparams = len(params)
        indices = [self.index[p] for p in params] + [self.index[p] for p in conditional_params]
        normparam = params.index(normparam) if normparam and normparam in params else -1
        n = len(indices)
        if param_map is None:
            # param_min / param_max of _initParamRanges are the base statistics' column extrema
            param_map = ""
            for j in indices[:nparams]:
                mn, mx = self._col_min[j], self._col_max[j]
                param_map += "N" if mx < 0 or mn < (mx - mn) / 10 else "L"
        maps = np.zeros(n, dtype=np.int32)
        labels = []
        for i in range(nparams):
            label = self.parLabel(indices[i])
            if param_map[i] == "L":
                maps[i] = 1
                labels.append("ln(" + label + ")")
            elif param_map[i] == "M":
                maps[i] = 2
                labels.append("ln(-" + label + ")")
            else:
                labels.append(label)
            text += "%10s :%s\n" % (str(indices[i] + 1), str(labels[i]))
        doexp = bool(np.any(maps[:nparams] != 0))
        PCmean, sd, corr = self.ctx.pca_corr(indices, maps)

        text += "\nCorrelation matrix for reduced parameters\n"
        for i in range(nparams):
            text += "%12s :" % params[i] + "".join("%8.4f" % corr[j][i] for j in range(n)) + "\n"
        if len(conditional_params):
            u = np.linalg.inv(corr)
            u = np.linalg.inv(u[np.ix_(range(nparams), range(nparams))])
            n = nparams
        else:
            u = corr
        evals, evects = np.linalg.eig(u)
        isorted = evals.argsort()
        u = np.transpose(evects[:, isorted])

        text += "\ne-values of correlation matrix\n"
        for i in range(n):
            text += "PC%2i: %8.4f\n" % (i + 1, evals[isorted[i]])
        text += "\ne-vectors\n"
        for j in range(n):
            text += "%3i:" % (indices[j] + 1) + "".join("%8.4f" % evects[j][isorted[i]] for i in range(n)) + "\n"
        for i in range(n):
            k = normparam if normparam != -1 else np.abs(u[i, :]).argmax()
            u[i, :] = u[i, :] / u[i, k] * sd[k]

        newmean, newsd, pcpc, pcpar = self.ctx.pca_project(indices[:n], maps[:n], PCmean[:n], sd[:n], u, doexp,
                                                           self.means, self.sddev)
        text += "\nPrincipal components\n"
        mode_texts = []
        for i in range(n):
            summary = "PC%i (e-value: %f)\n" % (i + 1, evals[isorted[i]])
            for j in range(n):
                label = self.parLabel(indices[j])
                if param_map[j] in ["L", "M"]:
                    expo = "%f" % (1.0 / sd[j] * u[i][j])
                    div = "%f" % (-np.exp(PCmean[j]) if param_map[j] == "M" else np.exp(PCmean[j]))
                    summary += "[%f]  (%s/%s)^{%s}\n" % (u[i][j], label, div, expo)
                else:
                    expo = "%f" % (sd[j] / u[i][j])
                    if doexp:
                        summary += "[%f]   exp((%s-%f)/%s)\n" % (u[i][j], label, PCmean[j], expo)
                    else:
                        summary += "[%f]   (%s-%f)/%s\n" % (u[i][j], label, PCmean[j], expo)
            summary += "          = %f +- %f\n\n" % (newmean[i], newsd[i])
            mode_texts.append(summary)
            text += summary

        text += "Correlations of principal components\n"
        text += "".join("%8i" % i for i in range(1, n + 1)) + "\n"
        for j in range(n):
            text += "PC%2i" % (j + 1) + "".join("%8.3f" % pcpc[i][j] for i in range(n)) + "\n"
        for j in range(self.n):
            text += "%4i" % (j + 1) + "".join("%8.3f" % pcpar[i][j] for i in range(n))
            text += "   (%s)\n" % self.parLabel(j)

        if writeDataToFile:
            with open(filename or self.rootdirname + ".PCA", "w", encoding="utf-8") as f:
                f.write(text)
        if n_best_only:
            if n_best_only == 1:
                return mode_texts[0]
            return mode_texts[:n_best_only]
        return text

    # ---- marginalised limits (mcsamples.py:2353-2367, 2442-2531) -----------------------------------------------
    def _max_frac_twotail(self):
        """mcsamples.py:427-433: how small the end bin must be relative to the maximum to use a two-tail limit"""
        from scipy.stats import norm
        import math

        over = getattr(self, "_max_frac_overrides", {})  # max_frac_twotailN of the .ini (mcsamples.py:429-430)
        return [over.get(i, np.exp(-1.0 * math.pow(norm.ppf((1 - c) / 2), 2) / 2)) for i, c in enumerate(self.contours)]

    def _marge_limit_inputs(self, js, densities):
        """
        Everything the marginalised limits of parameters ``js`` need from the device, in three batched calls:
        equal-density credible intervals of every (density, contour) (gd_limits1d), and the one- and two-tail sample
        quantiles of every (column, contour) (gd_quantiles; targets per contour: f, 1-f, f/2, 1-f/2 with f = 1-contour).
        Returns (credible[len(js), nc, 4], tails[len(js), nc, 4]).
        """
        contours = np.asarray(self.contours, dtype=np.float64)
        nc = len(contours)
        credible = np.zeros((len(js), nc, 4))
        by_F = {}
        for b, d in enumerate(densities):
            by_F.setdefault(d.P.size, []).append(b)
        for F, members in by_F.items():
            for c0 in range(0, nc, 8):
                lims, status = self.ctx.limits1d(np.stack([densities[b].P for b in members]),
                                                 [densities[b].x[0] for b in members],
                                                 [densities[b].spacing for b in members], contours[c0:c0 + 8])
                if np.any(status != 0):
                    raise DensitiesError("credible limit outside the refined density grid")
                credible[members, c0:c0 + 8] = lims
        tails = np.zeros((len(js), nc, 4))
        f = 1 - contours
        for c0 in range(0, nc, 4):
            fr = f[c0:c0 + 4]
            fracs = np.stack([fr, 1 - fr, fr / 2, 1 - fr / 2], axis=1).reshape(-1)
            q = self.ctx.quantiles(js, np.tile(self.norm * fracs, (len(js), 1)), minmax=self._minmax_of(js))
            tails[:, c0:c0 + 4] = q.reshape(len(js), -1, 4)
        return credible, tails

    def _assign_marge_limits(self, par, density, credible, tails, max_frac_twotail):
        """
        The limit type and values per contour (contract of mcsamples.py:2460-2531).  A hard prior edge where the
        density is still high (above max_frac_twotail of the peak) makes that side unconstrained; otherwise the
        equal-density interval of the smoothed density decides which sides are open, open sides take the prior range,
        a single closed side takes the one-tail sample quantile, and two closed sides take the equal-density interval
        -- or the two-tail quantiles when the density is nearly equal at them (credible_interval_threshold).
        """
        force_twotail = getattr(self, "force_twotail", False)
        par.limits = []
        for c in range(len(self.contours)):
            open_bot = bool(par.has_limits_bot and not force_twotail and density.P[0] > max_frac_twotail[c])
            open_top = bool(par.has_limits_top and not force_twotail and density.P[-1] > max_frac_twotail[c])
            lower, upper = par.range_min, par.range_max
            if not (open_bot and open_top):
                cred_lo, cred_hi, open_bot, open_top = credible[c]
                open_bot, open_top = bool(open_bot), bool(open_top)
                one_lo, one_hi, two_lo, two_hi = tails[c]
                if not open_bot and not open_top:
                    lower, upper = cred_lo, cred_hi
                    if abs(density.Prob(two_hi) - density.Prob(two_lo)) < self.credible_interval_threshold:
                        lower, upper = two_lo, two_hi
                elif not open_bot:
                    lower = one_lo
                elif not open_top:
                    upper = one_hi
            tag = {(True, True): "none", (True, False): ">", (False, True): "<", (False, False): "two"}[(open_bot, open_top)]
            par.limits.append(ParamLimit([lower, upper], tag))

    def _setMargeLimits(self, par, paramConfid=None, max_frac_twotail=None, density1D=None):
        """Marginalised limits of ONE parameter (the reference's per-parameter entry point, mcsamples.py:2460)."""
        j = self._col(par.name)
        density1D = density1D or self.get1DDensity(par.name)
        credible, tails = self._marge_limit_inputs([j], [density1D])
        self._assign_marge_limits(par, density1D, credible[0], tails[0], max_frac_twotail or self._max_frac_twotail())

    def getMargeStats(self, include_bestfit=False):
        """mcsamples.py:2353-2367: marginalised 1D constraints.  All densities, all equal-density intervals and all tail
        quantiles come from batched device calls; the MargeStats returned turns them into text (str(), saveAsText) and
        LaTeX (texValues; see getTable / getLatex / getInlineLatex) on the host.  Best-fit files are not read."""
        if include_bestfit:
            raise NotImplementedError("best-fit files are outside the accelerated path")
        if self.needs_update:
            self.updateBaseStatistics()
        # the limits stay on the parameters until the statistics are recomputed (the reference's done_1Dbins,
        # mcsamples.py:2449): a table or a plot title per parameter asks for them again and again
        asked = (tuple(self.contours), self.credible_interval_threshold, bool(getattr(self, "force_twotail", False)),
                 tuple(sorted(getattr(self, "_max_frac_overrides", {}).items())))
        if getattr(self, "_marge_done", None) != asked:
            dens = self.get1DDensities()  # one batched launch, cached per name
            mft = self._max_frac_twotail()
            js = list(range(self.n))
            credible, tails = self._marge_limit_inputs(js, dens)
            for j, par in enumerate(self.paramNames.names):
                self._assign_marge_limits(par, dens[j], credible[j], tails[j], mft)
            self._marge_done = asked
        return MargeStats(self.paramNames.names, self.contours)

    # ---- result text (mcsamples.py:2379-2440): formatting of what getMargeStats brought back, no device call of its own
    def getTable(self, columns=1, include_bestfit=False, **kwargs):
        """mcsamples.py:2379-2388: a types.ResultTable of the marginalised constraints in ``columns`` parameter columns;
        ``kwargs`` go to ResultTable (limit, paramList, titles, formatter, refResults, ...)."""
        return ResultTable(columns, [self.getMargeStats(include_bestfit)], **kwargs)

    def getLatex(self, params=None, limit=1, err_sig_figs=None):
        """mcsamples.py:2390-2422: (labels, LaTeX snippets) of the constraints on ``params`` (names or ParamInfo objects;
        default all) at limit number ``limit``; None entries for names not present.  A single name as a string gives
        what getInlineLatex gives.  ``err_sig_figs``: significant figures of the errors."""
        if isinstance(params, str):
            return self.getInlineLatex(params, limit, err_sig_figs)
        marge = self.getMargeStats()
        formatter = NoLineTableFormatter()
        if err_sig_figs:
            formatter.numberFormatter.err_sf = err_sig_figs
        labels, texs = [], []
        for par in marge.list() if params is None else params:
            tex = marge.texValues(formatter, par, limit=limit)
            texs.append(None if tex is None else tex[0])
            labels.append(None if tex is None else marge.parWithName(par if isinstance(par, str) else par.name).getLabel())
        return labels, texs

    def getInlineLatex(self, param, limit=1, err_sig_figs=None):
        """mcsamples.py:2424-2440: ``label = value +- error`` of one parameter, or ``label < value`` for a one-tail limit"""
        labels, texs = self.getLatex([param], limit, err_sig_figs)
        if texs[0] is None:
            raise ValueError("parameter %s not found" % param)
        return labels[0] + (" " if texs[0][0] in "<>" else " = ") + texs[0]

    # ---- 2D densities (mcsamples.py:1285-1419, 1730-2010) ---------------------------------------------------
    def get2DDensity(self, x, y, normalized=False, **kwargs):
        if self.needs_update:
            self.updateBaseStatistics()
        density = self.get2DDensityGridData(x, y, get_density=True, **kwargs)
        if density is not None and normalized:
            density.normalize(in_place=True)
        return density

    def get2DDensityGridData(self, j, j2, num_plot_contours=None, get_density=False, meanlikes=False,
                             mask_function=None, **kwargs):
        if self.needs_update:
            self.updateBaseStatistics()
        j = self._parAndNumber(j)[0]
        j2 = self._parAndNumber(j2)[0]
        if j is None or j2 is None:
            return None
        density = self.get2DDensities([(j, j2)], num_plot_contours=num_plot_contours, get_density=get_density,
                                      meanlikes=meanlikes, mask_function=mask_function, **kwargs)[0]
        density.P  # a single-pair call delivers (and raises "no samples in bin") here, like the reference
        return density

    def triangleDensities(self, params=None, **kwargs):
        """All lower-triangle pairs (x=params[i], y=params[i2>i]) in triangle-plot order; returns (pairs, densities)."""
        names = list(range(self.n)) if params is None else [self._col(p) for p in params]
        pairs = [(names[i], names[i2]) for i in range(len(names)) for i2 in range(i + 1, len(names))]
        return pairs, self.get2DDensities(pairs, **kwargs)

    # ---- per-pair bandwidth selection planned in Python (getAutoBandwidth2D) -----------------------------------------
    # getAutoBandwidth2D takes the caller's own histogram, which the native entry cannot, so it still plans in Python:
    # _bandwidth_plan, _fallback_widths, _shear_histograms, _bandwidth_2d and the module's _Plan.  The product's batched
    # route (get2DDensities -> gd_density2d_batch) does not use any of them; the comparison route of
    # tests/planned_route.py does.
    def getAutoBandwidth2D(self, bins, parx, pary, paramx, paramy, corr, rangex, rangey, base_fine_bins_2D,
                           mult_bias_correction_order=None, min_corr=0.2, N_eff=None, use_2D_Neff=False):
        """Per-pair entry point with the reference's signature (mcsamples.py:1285-1419); ``bins`` is a host F x F grid."""
        bins = np.ascontiguousarray(bins, dtype=np.float64)
        F = bins.shape[0]
        d = self.ctx.alloc(bins.nbytes)
        d.from_host(bins)
        plan = self._bandwidth_plan([(paramx, paramy)], [corr], [(rangex, rangey)], base_fine_bins_2D, N_eff=N_eff)
        res = self._bandwidth_2d(plan, {F: (d, [0])}, [F], base_fine_bins_2D, mult_bias_correction_order)
        return tuple(res[0].tolist())

    def _bandwidth_plan(self, pairs, corrs, ranges_xy, base_F, min_corr=0.2, N_eff=None, defer_neff=False):
        """Branch selection per pair (mcsamples.py:1325-1409), scalars only.  The classification is evaluated on arrays
        over the pairs (a triangle has thousands); powers stay Python-float operations so that every scalar is the one the
        reference computes.  With ``defer_neff`` the effective sample numbers are not touched yet (their kernels may
        still be running on a helper thread): returns (plan, fill) and ``fill()`` completes the entries later."""
        names = self.paramNames.names
        npairs = len(pairs)
        if npairs == 0:
            return (_Plan(), lambda: None) if defer_neff else _Plan()
        if N_eff is None and not defer_neff:
            self._neff_batch(list(dict.fromkeys([j for p in pairs for j in p])))
        jx = [p[0] for p in pairs]
        jy = [p[1] for p in pairs]
        used = sorted(set(jx) | set(jy))
        at = np.full(max(used) + 1, -1, dtype=np.int64)
        at[used] = np.arange(len(used))
        ix, iy = at[jx], at[jy]
        upar = [names[j] for j in used]
        lim_u = np.array([bool(p.has_limits) for p in upar])
        sig_u = np.array([np.nan if p.sigma_range is None else p.sigma_range for p in upar], dtype=np.float64)
        corr_v = np.asarray(corrs, dtype=np.float64)

        def effective_samples():
            if N_eff is not None:
                return np.full(npairs, float(N_eff))
            if self.use_effective_samples_2D:
                return np.array([self.getEffectiveSamplesGaussianKDE_2d(a, b) if abs(c) < 0.999  # mcsamples.py:1326-1328
                                 else min(self._get1DNeff(names[a], a), self._get1DNeff(names[b], b))
                                 for a, b, c in zip(jx, jy, corr_v.tolist())], dtype=np.float64)
            neff_u = np.array([self._get1DNeff(p, j) for p, j in zip(upar, used)], dtype=np.float64)
            return np.minimum(neff_u[ix], neff_u[iy])

        limx, limy = lim_u[ix], lim_u[iy]
        has_limits = limx | limy
        do_correlated = ~limx | ~limy
        absc = np.abs(corr_v)
        is_A = (min_corr < absc) & (absc <= self.max_corr_2D) & do_correlated
        is_B = ~is_A & ((absc > self.max_corr_2D) | (~do_correlated & (corr_v > 0.8)))
        rng = np.asarray(ranges_xy, dtype=np.float64).reshape(npairs, 2)
        with np.errstate(all="ignore"):
            ratio = np.minimum(sig_u[iy] / rng[:, 1], sig_u[ix] / rng[:, 0]).tolist()
        branch = np.where(is_A, "A", np.where(is_B, "B", "C")).tolist()
        plan = _Plan(dict(jx=a, jy=b, parx=names[a], pary=names[b], corr=c, neff=None, has_limits=hl, rangex=rx_, rangey=ry_,
                          branch=br)
                     for a, b, c, hl, rx_, ry_, br in zip(jx, jy, corr_v.tolist(), has_limits.tolist(),
                                                          rng[:, 0].tolist(), rng[:, 1].tolist(), branch))
        plan.arr = dict(branch=np.where(is_A, 0, np.where(is_B, 1, 2)).astype(np.int8), has_limits=has_limits, corr=corr_v,
                        rangex=rng[:, 0].copy(), rangey=rng[:, 1].copy(), neff=None, fallback_t=None)
        is_C = np.nonzero(~is_A & ~is_B)[0].tolist()

        def fill():
            neff_v = effective_samples()
            neff_l = neff_v.tolist()
            for e, ne in zip(plan, neff_l):
                e["neff"] = ne
            fb = np.full(npairs, np.nan)
            for k in is_C:
                fb[k] = plan[k]["fallback_t"] = (ratio[k] / neff_l[k] ** (1.0 / 6)) ** 2
            plan.arr["neff"], plan.arr["fallback_t"] = neff_v, fb

        if not defer_neff:
            fill()
        for k in np.nonzero(is_A)[0].tolist():
            e = plan[k]
            parx, pary = e["parx"], e["pary"]
            i, j = e["jx"], e["jy"]
            imax, imin = None, None
            if parx.has_limits_bot:
                imin = parx.range_min
            if parx.has_limits_top:
                imax = parx.range_max
            if pary.has_limits:
                i, j = j, i
                if pary.has_limits_bot:
                    imin = pary.range_min
                if pary.has_limits_top:
                    imax = pary.range_max
            cov = self.getCov(pars=[i, j])
            S = np.linalg.cholesky(cov)
            ichol = np.linalg.inv(S)
            S *= ichol[0, 0]
            r = ichol[1, :] / ichol[0, 0]
            e.update(i=i, j=j, imin=imin, imax=imax, S=S, r=r)
        return (plan, fill) if defer_neff else plan

    def _fallback_widths(self, e, ex):
        parx, pary, corr, neff = e["parx"], e["pary"], e["corr"], e["neff"]
        msg = f"2D kernel density bandwidth optimizer failed for {parx.name}, {pary.name}. Using fallback width: {ex}"
        if self.raise_on_bandwidth_errors:
            raise BandwidthError(msg)
        logging.warning(msg)
        _hx = parx.sigma_range / neff ** (1.0 / 6)
        _hy = pary.sigma_range / neff ** (1.0 / 6)
        return _hx, _hy, max(min(corr, self.max_corr_2D), -self.max_corr_2D)

    def _shear_histograms(self, plan, base_F):
        """Branch A of getAutoBandwidth2D (mcsamples.py:1347-1378): min/max of the sheared coordinate and the re-binned
        base_F x base_F histograms of every sheared pair, two batched launches.  Independent of the pairs' own histograms,
        so the caller may run it while those are still being made on the second stream.  None if there is no such pair."""
        A = [k for k, e in enumerate(plan) if e["branch"] == "A"]
        if not A:
            return None
        ctx = self.ctx
        mm = ctx.minmax_affine([plan[k]["i"] for k in A], [plan[k]["j"] for k in A], [plan[k]["r"][0] for k in A],
                               [plan[k]["r"][1] for k in A])
        xmin, dx, ymin, dy, r1s, r2s = [], [], [], [], [], []
        for row, k in enumerate(A):
            e = plan[k]
            # kde.bin_samples(p1, nbins, range_min=imin, range_max=imax) (kde_bandwidth.py:76-87)
            mn, mx = self._col_min[e["i"]], self._col_max[e["i"]]
            delta = mx - mn
            rmin = e["imin"] if e["imin"] is not None else mn - delta * 0.1
            rmax = e["imax"] if e["imax"] is not None else mx + delta * 0.1
            R1 = rmax - rmin
            mn2, mx2 = mm[row]
            delta2 = mx2 - mn2
            rmin2 = mn2 - delta2 * 0.1
            R2 = (mx2 + delta2 * 0.1) - rmin2
            xmin.append(rmin), dx.append(R1 / (base_F - 1)), ymin.append(rmin2), dy.append(R2 / (base_F - 1))
            r1s.append(R1), r2s.append(R2)
        d_rot = ctx.hist2d_sheared([plan[k]["i"] for k in A], [plan[k]["j"] for k in A],
                                   [plan[k]["r"][0] for k in A], [plan[k]["r"][1] for k in A], xmin, dx, ymin, dy,
                                   base_F)
        return dict(d_rot=d_rot, r1s=r1s, r2s=r2s)

    def _bandwidth_2d(self, plan, hists_by_F, pair_F, base_F, mult_bias_correction_order, shear=None, deferred=None,
                      on_chunk=None, first_fraction=None, more_deferred=None):
        """
        getAutoBandwidth2D for a batch (mcsamples.py:1325-1419).  ``hists_by_F``: F -> (device buffer of that class's
        histograms, list of plan indices in buffer order); ``pair_F[k]`` the fine grid size of plan entry k.  Returns the
        (hx, hy, corr) triples in parameter units as an (npair, 3) array.  The whole KernelOptimizer2D -- fixed point,
        functionals, get_h with its TNC minimisations -- runs on the device (gd_kopt2d); here only branch bookkeeping and
        unit conversions, on arrays over the pairs: this code sits between the optimiser's kernels and the convolution's.
        The per-pair records (``plan[k]["kopt"]``) are written by a callable appended to ``deferred`` (the caller runs it
        once the next kernels are enqueued), or at once when ``deferred`` is None.

        ``on_chunk(ks, last, W)`` is called after every optimiser launch with the plan indices whose triples are final
        (rule-of-thumb pairs ride with the first launch); with ``first_fraction`` the base grid's launch is cut in two at
        that fraction of its pairs, so that the caller can convolve the first part (on another stream) while the second
        part is being optimised.
        """
        npair = len(plan)
        ctx = self.ctx
        arr = plan.arr
        W = np.full((npair, 3), np.nan)
        kopt_rows = []  # (plan indices, optimiser output rows) per launch
        m = self.mult_bias_correction_order if mult_bias_correction_order is None else mult_bias_correction_order
        branch = arr["branch"]
        if m:  # higher-order bias correction widens the kernel (mcsamples.py:1412-1416); few distinct N_eff values, each
            # scale a Python-float power as before
            uniq, inv = np.unique(arr["neff"], return_inverse=True)
            widen = np.array([1.1 * ne ** (1.0 / 6 - 1.0 / (2 + 4 * (1 + m))) for ne in uniq.tolist()])[inv]
        else:
            widen = None

        # -- branch A: sheared re-binning at base_F, optimiser with corr=0 and no fallback_t
        A = np.nonzero(branch == 0)[0]
        if shear is None:
            shear = self._shear_histograms(plan, base_F)
        # -- branch B: rule of thumb
        kB = np.nonzero(branch == 1)[0]
        for k in kB.tolist():
            e = plan[k]
            c = max(min(e["corr"], self.max_corr_2D), -self.max_corr_2D)
            W[k] = (e["parx"].sigma_range / e["neff"] ** (1.0 / 6), e["pary"].sigma_range / e["neff"] ** (1.0 / 6), c)
        waiting = [kB]  # final triples not yet reported to on_chunk

        def report(ks, last):
            ks = np.concatenate(waiting + [ks]) if waiting else ks
            waiting.clear()
            if widen is not None:
                W[ks, 0] *= widen[ks]
                W[ks, 1] *= widen[ks]
            if on_chunk is not None and (len(ks) or last):
                on_chunk(ks, last, W)

        def optimise(F, d_batch, ks, row_A, r1, r2):
            """One device-optimiser launch over plan entries ``ks`` (batch order); ``row_A`` marks the sheared rows,
            whose sheared ranges are r1, r2."""
            fb = np.where(row_A, -1.0, arr["fallback_t"][ks])
            corr_in = np.where(row_A, 0.0, arr["corr"][ks])
            out = ctx.kopt2d(d_batch, len(ks), F, arr["neff"][ks], (~arr["has_limits"][ks]).astype(np.int32), fb, corr_in)
            no_root = out[:, 7] != 0
            if np.any(~no_root & (out[:, 11] != 0)):
                raise Exception("bias not positive definite")  # kde_bandwidth.py:229-230, raised out of get_h
            # branch C (the bulk): parameter units = the fractions times the ranges, evaluated on the whole batch
            hx = out[:, 8] * arr["rangex"][ks]
            hy = out[:, 9] * arr["rangey"][ks]
            c = out[:, 10].copy()
            # branch A: de-rotate the sheared kernels (mcsamples.py:1379-1390), kernelC = S K S^T written out for the
            # 2x2 case and evaluated on all sheared pairs at once
            if np.any(row_A):
                ra = np.nonzero(row_A)[0]
                hxa = out[ra, 8] * r1
                hya = out[ra, 9] * r2
                ca = out[ra, 10]
                S = np.array([plan[k]["S"] for k in ks[ra].tolist()])  # (nA, 2, 2)
                k00, k01, k11 = hxa**2, hxa * hya * ca, hya**2
                t00 = S[:, 0, 0] * k00 + S[:, 0, 1] * k01
                t01 = S[:, 0, 0] * k01 + S[:, 0, 1] * k11
                t10 = S[:, 1, 0] * k00 + S[:, 1, 1] * k01
                t11 = S[:, 1, 0] * k01 + S[:, 1, 1] * k11
                c00 = t00 * S[:, 0, 0] + t01 * S[:, 0, 1]
                c01 = t00 * S[:, 1, 0] + t01 * S[:, 1, 1]
                c11 = t10 * S[:, 1, 0] + t11 * S[:, 1, 1]
                sx, sy = np.sqrt(c00), np.sqrt(c11)
                swap = np.array([bool(plan[k]["pary"].has_limits) for k in ks[ra].tolist()])
                hx[ra], hy[ra], c[ra] = np.where(swap, sy, sx), np.where(swap, sx, sy), c01 / np.sqrt(c00 * c11)
            W[ks, 0], W[ks, 1], W[ks, 2] = hx, hy, c
            for row in np.nonzero(no_root)[0].tolist():
                k = int(ks[row])
                plan[k]["kopt"] = out[row]
                W[k] = self._fallback_widths(plan[k], "2D fixed point: no root in [0, 0.1]")
            kopt_rows.append((ks, out))

        # -- branches A and C share the device optimiser: the sheared histograms ride in the same launch as the
        #    base-grid pairs' own histograms (one block per pair; a short extra launch would cost a full block latency)
        item = base_F * base_F * 8
        nA = len(A)
        r1s = np.asarray(shear["r1s"], dtype=np.float64) if nA else None
        r2s = np.asarray(shear["r2s"], dtype=np.float64) if nA else None
        launches = []  # callables (last) -> None, in launch order

        def book():
            for e in plan:
                e["kopt"] = None
            for ks, out in kopt_rows:
                for k, row in zip(ks.tolist(), out):
                    plan[k]["kopt"] = row

        if deferred is not None:  # queued before on_chunk enqueues anything: it runs when the caller drains the list
            deferred.append(book)
            if more_deferred is not None:
                deferred.append(more_deferred)

        def add_launch(F, build, ks, row_A, r1, r2):
            def go(last):
                d_batch, own = build()
                try:
                    optimise(F, d_batch, ks, row_A, r1, r2)
                finally:
                    if own:
                        d_batch.free()
                report(ks, last)

            launches.append(go)

        merged = False
        for F, (d_hist, members) in hists_by_F.items():
            mem = np.asarray(members, dtype=np.int64)
            pos_C = np.nonzero(branch[mem] == 2)[0]
            if F == base_F and len(pos_C):
                cuts = [0, len(pos_C)]
                if first_fraction and len(pos_C) >= self.KOPT_SPLIT_MIN:
                    cuts = [0, int(len(pos_C) * first_fraction), len(pos_C)]
                for part in range(len(cuts) - 1):
                    pc = pos_C[cuts[part]:cuts[part + 1]]
                    na = nA if part == 0 else 0  # the sheared pairs ride with the first part

                    def build(pc=pc, na=na, d_hist=d_hist, whole=len(mem)):
                        if na == 0 and len(pc) == whole:
                            return d_hist, False  # the class's buffer as it is
                        d_all = ctx.alloc((na + len(pc)) * item)
                        if na:
                            ctx.gather_items(d_all, shear["d_rot"], np.arange(na, dtype=np.int32), item)
                        ctx.gather_items(d_all, d_hist, pc, item, dst_offset=na)
                        return d_all, True

                    add_launch(F, build, np.concatenate([A[:na], mem[pc]]), np.arange(na + len(pc)) < na, r1s if na else None,
                               r2s if na else None)
                merged = True
                continue
            if not len(pos_C):
                continue

            def build(pos_C=pos_C, mem=mem, d_hist=d_hist, F=F):
                if len(pos_C) == len(mem):
                    return d_hist, False
                d_sub = ctx.alloc(len(pos_C) * F * F * 8)
                self._gather_device(d_hist, d_sub, pos_C, F * F * 8)
                return d_sub, True

            add_launch(F, build, mem[pos_C], np.zeros(len(pos_C), dtype=bool), None, None)
        if nA and not merged:
            add_launch(base_F, lambda: (shear["d_rot"], False), A, np.ones(nA, dtype=bool), r1s, r2s)
        try:
            for q, go in enumerate(launches):
                go(q == len(launches) - 1)
            if not launches:
                report(np.zeros(0, dtype=np.int64), True)
        finally:
            if shear is not None:
                shear["d_rot"].free()
        if deferred is None:
            book()
        return W

    # ---- batched 2D densities ----------------------------------------------------------------------------------------
    def _gather_device(self, d_src, d_dst, positions, item_bytes, ctx=None):
        """Copy selected fixed-size items of one device buffer into another (one gather kernel)."""
        (ctx or self.ctx).gather_items(d_dst, d_src, positions, item_bytes)

    def _index_columns8(self, wanted):
        """Byte index columns of the 256-bin grid (wanted: j -> (binmin, width)) in ONE launch; False if any sample of
        any column falls outside the grid (then the u16 path, which marks such samples, must be used)."""
        todo = [j for j, bw in wanted.items() if self._idx_cols.get((j, 256, "u8"), (None, None))[1] != bw]
        if todo:
            bufs = []
            for j in todo:
                hit = self._idx_cols.get((j, 256, "u8"))
                bufs.append(hit[0] if hit is not None else self.ctx.alloc(self.numrows + 64))
            bad = self.ctx.prebin8_batch(todo, [wanted[j][0] for j in todo], [wanted[j][1] for j in todo], 256, bufs)
            for j, buf, nb in zip(todo, bufs, bad):
                self._idx_cols[(j, 256, "u8")] = (buf, wanted[j] if nb == 0 else None)
        return all(self._idx_cols[(j, 256, "u8")][1] == bw for j, bw in wanted.items())

    def _index_column(self, j, F, binmin, width):
        key = (j, F)
        hit = self._idx_cols.get(key)
        if hit is None or hit[1] != (binmin, width):
            buf = hit[0] if hit is not None else None
            buf = self.ctx.prebin(j, binmin, width, F, buf)
            self._idx_cols[key] = (buf, (binmin, width))
        return self._idx_cols[key][0]

    def get2DDensities(self, pairs, num_plot_contours=None, get_density=True, _bandwidths=None, meanlikes=False,
                       mask_function=None, **kwargs):
        """
        Batched 2D KDEs (additive API): a list of Density2D, one per (x, y) entry of ``pairs``.
        ``mask_function(minx, miny, stepx, stepy, mask)`` may zero parts of each pair's prior mask in place
        (mcsamples.py:1767-1770); those pairs take the explicit-mask entry point one at a time.
        With ``meanlikes`` each result carries the mean-likelihood grid ``likes`` (mcsamples.py:1829-1831,1886-1903).
        Each result carries ``bandwidth`` = (hx, hy, corr) in parameter units, ``bandwidth_branch`` and
        ``kopt`` (the device optimiser's {t*, psi_02, psi_20, psi_11, psi_00, psi_13, psi_31, status}).
        ``_bandwidths`` (tests only) injects the (hx, hy, corr) triples instead of optimising.

        One implementation: every branch goes through gd_density2d_batch (getdist_amd/batch2d.py, csrc/batch2d.hpp).
        """
        if self.needs_update:
            self.updateBaseStatistics()
        for k in kwargs:
            if k not in ("fine_bins_2D", "boundary_correction_order", "mult_bias_correction_order", "smooth_scale_2D"):
                raise SettingError("unknown 2D density argument %s" % k)
        pa = None
        if len(pairs) > 8:
            try:  # a triangle's worth of integer indices: one conversion instead of a name lookup per entry
                pa = np.asarray(pairs)
                if pa.ndim != 2 or pa.shape[1] != 2 or pa.dtype.kind != "i" or pa.min() < 0 or pa.max() >= self.n:
                    pa = None
            except (ValueError, TypeError):
                pa = None
        pairs = pa.astype(np.int64, copy=False) if pa is not None else [(self._col(a), self._col(b)) for a, b in pairs]
        if hasattr(self.ctx, "density2d_batch") and os.environ.get("GETDIST_AMD_NATIVE_BATCH", "1") == "1":
            # ONE native call: every decision between the kernels is taken inside the library (csrc/batch2d.hpp), for the
            # optional branches too -- injected bandwidths and the 2D effective sample numbers are inputs of the call, the
            # mean-likelihood grids are a pass of their own over its per-pair table, and a mask callback gets the call's
            # bandwidths (bandwidths_only) and then the explicit-mask entry point pair by pair.
            from . import batch2d

            base_F = kwargs.get("fine_bins_2D", self.fine_bins_2D)
            bco = kwargs.get("boundary_correction_order", self.boundary_correction_order)
            mbc = kwargs.get("mult_bias_correction_order", self.mult_bias_correction_order)
            ss = float(kwargs.get("smooth_scale_2D", self.smooth_scale_2D))
            if abs(self.max_corr_2D) > 1:
                raise SettingError("max_corr_2D cannot be >=1")
            if bco > 1:
                raise SettingError("unknown boundary_correction_order (expected 0 or 1)")
            pa64 = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
            pair_neff = None
            if self.use_effective_samples_2D and ss < 0 and _bandwidths is None and len(pa64):
                pair_neff = self._pair_neff_2d(pa64)
            if mask_function is not None and len(pa64):
                return self._densities_with_mask_callback(pa64, base_F, bco, mbc, ss, num_plot_contours, get_density, _bandwidths,
                                                          pair_neff, meanlikes, mask_function)
            out = batch2d.run(self, pa64, base_F, bco, mbc, ss, num_plot_contours, get_density, bandwidths=_bandwidths,
                              pair_neff=pair_neff)
            if meanlikes and len(pa64):
                self._attach_mean_likelihoods(out, pa64, mbc)
            return out
        # No native entry on this context: the product has no second orchestration of the kernels.  The Python-planned
        # pipeline of rounds 2-5 lives in tests/planned_route.py as the comparison the native route is held bit-equal to;
        # it registers itself here for the numpy context double of the CPU tests (and for GETDIST_AMD_NATIVE_BATCH=0).
        route = getattr(MCSamples, "_planned_route", None)
        if route is None:
            raise MCSamplesError("get2DDensities needs a device context with gd_density2d_batch (libgdhip)")
        with _FastThreadSwitch(len(pairs) >= 64):
            return route(self, pairs, num_plot_contours, get_density, _bandwidths, meanlikes, mask_function=mask_function,
                         **kwargs)

    def get2DContourPaths(self, pairs, num_plot_contours=None, meanlikes=False, **kwargs):
        """
        Batched 2D contour geometry (additive API): one contourpaths.ContourPaths per (x, y) entry of ``pairs``, at the
        contour levels of ``self.contours`` (the first ``num_plot_contours`` of them).  The densities come from
        ``get2DDensities(..., get_density=False)`` with the same keyword arguments and stay attached as ``.density``; their
        grids are traced on this sample set's device in one native call (gd_contour_paths).
        """
        from .contourpaths import contour_paths

        densities = self.get2DDensities(pairs, num_plot_contours=num_plot_contours, get_density=False, meanlikes=meanlikes,
                                        **kwargs)
        return contour_paths(densities, ctx=self.ctx)

    # ---- the optional branches of the native route -------------------------------------------------------------------
    def _pair_neff_2d(self, pa):
        """use_effective_samples_2D (mcsamples.py:1322-1328): the 2D estimate per pair, the smaller 1D one for a pair that is
        correlated to 0.999."""
        used = list(dict.fromkeys(pa.ravel().tolist()))
        self._init_params(used)
        names = self.paramNames.names
        corr = np.asarray(self.getCorrelationMatrix())[pa[:, 1], pa[:, 0]]
        return np.array([self.getEffectiveSamplesGaussianKDE_2d(a, b) if abs(c) < 0.999
                         else min(self._get1DNeff(names[a], a), self._get1DNeff(names[b], b))
                         for (a, b), c in zip(pa.tolist(), corr.tolist())], dtype=np.float64)

    def _pair_flags(self, pa, with_prior_mask=False):
        """Flag bits per pair (mcsamples.py:1688-1703, 1794): 0/1 = x bot/top, 2/3 = y bot/top, 4/5 = x/y periodic, 6 = has_prior."""
        names = self.paramNames.names
        lim_bits, per_bit, has_lim = np.zeros(self.n, np.int64), np.zeros(self.n, np.int64), np.zeros(self.n, bool)
        for j in np.unique(pa).tolist():
            p_ = names[j]
            lim_bits[j] = 0 if p_.periodic else (1 if p_.has_limits_bot else 0) | (2 if p_.has_limits_top else 0)
            per_bit[j] = 1 if p_.periodic else 0
            has_lim[j] = bool(p_.has_limits)
        jx, jy = pa[:, 0], pa[:, 1]
        has_prior = has_lim[jx] | has_lim[jy] | bool(with_prior_mask)
        return lim_bits[jx] | (per_bit[jx] << 4) | (lim_bits[jy] << 2) | (per_bit[jy] << 5) | (has_prior.astype(np.int64) << 6)

    def _class_histograms(self, pa, members, F, meta, likes=False):
        """Histograms (and, with ``likes``, the like-weighted ones: mcsamples.py:1829-1831) of the pairs ``members`` of one
        grid-size class from the bin edges the native call used (meta[23..26])."""
        ctx = self.ctx
        ix = [self._index_column(int(pa[k, 0]), F, meta[k, 23], (meta[k, 24] - meta[k, 23]) / (F - 1)) for k in members]
        iy = [self._index_column(int(pa[k, 1]), F, meta[k, 25], (meta[k, 26] - meta[k, 25]) / (F - 1)) for k in members]
        d_hist = ctx.hist2d_prebinned(ix, iy, F)
        d_like = self._like_histograms(0, lambda: ctx.hist2d_prebinned(ix, iy, F)) if likes else None
        return d_hist, d_like

    def _attach_mean_likelihoods(self, out, pa, mbc):
        """``likes`` of every result of a native call (mcsamples.py:1829-1831, 1886-1903): the like-weighted histogram of
        each pair convolved with the pair's own window (the call's per-pair table holds its scales), grid class by grid
        class."""
        ctx = self.ctx
        meta, F_v = out._meta, np.asarray(out._F)
        flags = self._pair_flags(pa)
        for F, periodic_bits in sorted(set(zip(F_v.tolist(), (flags & 48).tolist()))):  # (a launch holds one kind of axes)
            members = np.nonzero((F_v == F) & ((flags & 48) == periodic_bits))[0]
            step = max(1, min(int(24e9 // (F * F * 8 * 30)), 320))
            for s0 in range(0, len(members), step):
                mem = members[s0:s0 + step]
                d_hist, d_like = self._class_histograms(pa, mem.tolist(), F, meta, likes=True)
                d_L, lstatus = ctx.likes2d(d_hist, d_like, len(mem), F, meta[mem, 18], meta[mem, 19], meta[mem, 20],
                                           meta[mem, 21].astype(np.int64), flags[mem], mbc)
                d_hist.free()
                d_like.free()
                if np.any(lstatus != 0):
                    d_L.free()
                    raise DensitiesError("no likelihood weight in any bin")
                L = d_L.to_host((len(mem), F, F))
                d_L.free()
                for row, k in enumerate(mem.tolist()):
                    out[k].likes = L[row]

    def _densities_with_mask_callback(self, pa, base_F, bco, mbc, ss, num_plot_contours, get_density, bandwidths, pair_neff,
                                      meanlikes, mask_function):
        """get2DDensities with ``mask_function`` (mcsamples.py:1767-1770, 1905-1919, 1973-1979): the callback edits each pair's
        prior mask on the padded frame, whose size follows from the pair's window -- so the native call runs up to the
        bandwidths (bandwidths_only) and every pair then goes through the explicit-mask entry point."""
        from . import batch2d

        ctx = self.ctx
        names = self.paramNames.names
        meta, F_v = batch2d.run(self, pa, base_F, bco, mbc, ss, None, True, bandwidths=bandwidths, pair_neff=pair_neff,
                                bandwidths_only=True)
        F_v = np.asarray(F_v)
        flags = self._pair_flags(pa, with_prior_mask=True)
        ncontours = len(self.contours)
        if num_plot_contours:
            ncontours = min(num_plot_contours, ncontours)
        out = [None] * len(pa)
        for F in np.unique(F_v).tolist():
            members = np.nonzero(F_v == F)[0].tolist()
            d_hist, d_like = self._class_histograms(pa, members, F, meta, likes=meanlikes)
            try:
                for pos, k in enumerate(members):
                    j, j2 = int(pa[k, 0]), int(pa[k, 1])
                    parx, pary = names[j], names[j2]
                    w_ = int(meta[k, 21])
                    fwx, fwy = (meta[k, 24] - meta[k, 23]) / (F - 1), (meta[k, 26] - meta[k, 25]) / (F - 1)
                    prior_mask = np.ones((F + 2 * w_, F + 2 * w_))
                    mask_function(meta[k, 23] - w_ * fwx, meta[k, 25] - w_ * fwy, fwx, fwy, prior_mask)
                    bool_mask = prior_mask[w_:-w_, w_:-w_] < 1e-8
                    mask_bc = mask_mbc = None
                    if bco >= 0:
                        _set_edge_mask_2d(parx, pary, prior_mask, w_)
                        mask_bc = prior_mask.copy()
                    if mbc:
                        _set_all_edge_mask_2d(prior_mask, w_, parx.periodic, pary.periodic)
                        mask_mbc = prior_mask
                    d_P, status = ctx.density2d_masked(d_hist, pos, F, float(meta[k, 18]), float(meta[k, 19]), float(meta[k, 20]),
                                                       w_, int(flags[k]), bco, mbc, mask_bc, mask_mbc, bool_mask)
                    contours = None
                    if not get_density:
                        lev, lev_state = ctx.contour_levels(d_P, 1, F, self.contours[:ncontours])
                        state = int(np.asarray(lev_state)[0])
                        if state == -4:
                            raise DensitiesError("Contour level outside plotted ranges")
                        contours = lev[0].copy() if state == 0 else None
                    L = None
                    if meanlikes:
                        # the mean-likelihood grid does not see the mask (mcsamples.py:1886-1903 precede it)
                        d_one, d_lone = ctx.alloc(F * F * 8), ctx.alloc(F * F * 8)
                        self._gather_device(d_hist, d_one, [pos], F * F * 8)
                        self._gather_device(d_like, d_lone, [pos], F * F * 8)
                        d_L, lstatus = ctx.likes2d(d_one, d_lone, 1, F, meta[[k], 18], meta[[k], 19], meta[[k], 20],
                                                   meta[[k], 21].astype(np.int64), flags[[k]], mbc)
                        d_one.free()
                        d_lone.free()
                        if np.any(lstatus != 0):
                            raise DensitiesError("no likelihood weight in any bin")
                        L = d_L.to_host((1, F, F))[0]
                        d_L.free()
                    P = d_P.to_host((1, F, F))[0]
                    d_P.free()
                    if np.any(np.asarray(status) != 0):
                        raise DensitiesError("no samples in bin")
                    ax = np.arange(F, dtype=np.float64) * fwx + meta[k, 23]
                    ay = np.arange(F, dtype=np.float64) * fwy + meta[k, 25]
                    ax[-1], ay[-1] = meta[k, 24], meta[k, 26]
                    auto = ss < 0
                    dens = Density2D._from_fields(dict(
                        x=ax, y=ay, axes=[ay, ax], spacing=(ax[1] - ax[0]) * (ay[1] - ay[0]),
                        view_ranges=[(parx.range_min, parx.range_max), (pary.range_min, pary.range_max)], mask=bool_mask, likes=L,
                        contours=contours, spl=None, _P=P, _wait=None,
                        bandwidth=tuple(meta[k, 2:5].tolist()) if auto else None,
                        bandwidth_branch="ABC"[int(meta[k, 5])] if auto and meta[k, 5] >= 0 else None,
                        kopt=None if np.isnan(meta[k, 13]) else meta[k, 6:18].copy()))
                    if contours is None and not get_density:
                        dens.contours = dens.getContourLevels(self.contours[:ncontours])
                    out[k] = dens
            finally:
                d_hist.free()
                if d_like is not None:
                    d_like.free()
        return out


_FFT_SIZE_CACHE = {}


def next_fft_size(n):
    """Smallest 2^a * {1,3,5,9,15} (a >= 4) >= n: the FFT frame ladder density2d.hip plans for."""
    if n in _FFT_SIZE_CACHE:
        return _FFT_SIZE_CACHE[n]
    _FFT_SIZE_CACHE[n] = v = _next_fft_size(n)
    return v


def _next_fft_size(n):
    best = None
    for a in range(4, 28):
        for odd in (1, 3, 5, 9, 15):
            v = (1 << a) * odd
            if v >= n and (best is None or v < best):
                best = v
    return best

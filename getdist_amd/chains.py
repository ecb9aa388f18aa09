"""
The sample-statistics layers under ``MCSamples``, named as in getdist/chains.py: ``WeightedSamples`` (moments, covariance,
weighted quantiles, autocorrelation and effective sample numbers, thinning, the mutators of the sample set) and
``Chains(WeightedSamples)`` (parameter names, derived parameters, the base statistics, per-chain statistics and the
convergence diagnostics), plus ``ChainView``, one chain of a combined sample set as a row range of the resident columns.

Neither class has a constructor of its own: ``mcsamples.MCSamples`` builds the object (host arrays, the device context
``ctx`` and the upload funnel ``_upload``); the methods here run their O(N) passes through that context.
"""

import logging
import os
import threading

import numpy as np

from .paramnames import ParamInfo


class WeightedSampleError(Exception):
    pass


class MCSamplesError(WeightedSampleError):  # (raised by mcsamples.py; defined here because ParamError derives from it)
    pass


class ParamError(MCSamplesError):
    pass


def _is_expr(x):
    """A colexpr.ColumnExpr?  Tested before any ``==`` / ``in`` on a parameter argument: on an expression those build nodes."""
    from .colexpr import ColumnExpr

    return isinstance(x, ColumnExpr)


def _where_rows(where, numrows):
    """Row indices of a ``where=`` index array with numpy's semantics of x[where]: negative indices count from the end,
    anything outside [-numrows, numrows) raises IndexError (it used to wrap around silently)."""
    ix = np.asarray(where).astype(np.int64).ravel()
    if ix.size and (ix.min() < -numrows or ix.max() >= numrows):
        bad = ix[(ix < -numrows) | (ix >= numrows)][0]
        raise IndexError("index %d is out of bounds for axis 0 with size %d" % (int(bad), int(numrows)))
    return np.where(ix < 0, ix + numrows, ix)


def covToCorr(cov, copy=True):
    """chains.py:155-169: for i in order, row i and then column i are divided by sqrt(cov[i, i]) -- so element (a, b) is
    divided by the standard deviation of min(a, b) FIRST and by that of max(a, b) second (zero deviations are skipped).
    The same two divisions per element, on the whole matrix at once."""
    cov = np.array(cov, dtype=np.float64) if copy else cov
    d = np.sqrt(cov.diagonal())
    d = np.where(d != 0, d, 1.0)
    idx = np.arange(len(d))
    first, second = np.minimum(idx[:, None], idx[None, :]), np.maximum(idx[:, None], idx[None, :])
    cov[...] = (cov / d[first]) / d[second]
    return cov


def getSignalToNoise(C, noise=None, R=None, eigs_only=False):
    """chains.py:131-153: eigenvalues w (ascending; small = well constrained against the noise) of M = R C R^T, where R
    defaults to the inverse Cholesky root of ``noise``, and unless ``eigs_only`` also the matrix whose rows are the
    eigenvectors of M mapped back through R."""
    if R is None:
        if noise is None:
            raise WeightedSampleError("Must give noise or rotation R")
        R = np.linalg.inv(np.linalg.cholesky(noise))
    M = np.dot(R, C).dot(R.T)
    if eigs_only:
        return np.linalg.eigvalsh(M)
    w, U = np.linalg.eigh(M)
    return w, np.dot(U.T, R)


class ParSamples:
    """chains.py:172-175: the attribute bag of getParams / setParams (one sample vector per parameter name)"""


class ParamConfidenceData:
    """Handle returned by initParamConfidenceData (chains.py:176-178 namedtuple in the reference)."""

    def __init__(self, col, start, end, weights=None, vec=None):
        self.col, self.start, self.end = col, start, end
        self.weights = weights  # alternative weights (host, full length) or None
        self.vec = vec          # host vector the handle refers to when it is not a resident column


def _g2_markov_vs_second_order(tran):
    """
    Likelihood-ratio statistic G^2 of the first-order Markov model against the second-order one for the transition
    counts tran[a, b, c] of a binary chain (mcsamples.py:1072-1089): the Markov fit of cell (a, b, c) is
    n(a,b,.) n(.,b,c) / n(.,b,.); empty cells drop out.  Terms are added in C order, like the reference's loops.
    """
    import math

    n_ab = tran.sum(axis=2)
    n_bc = tran.sum(axis=0)
    n_b = tran.sum(axis=(0, 2))
    g2 = 0.0
    for (a, b, c), focus in np.ndenumerate(tran):
        if focus != 0:
            fitted = float(n_ab[a, b] * n_bc[b, c]) / float(n_b[b])
            g2 += math.log(float(focus) / fitted) * float(focus)
    return 2 * g2


def _g2_independence_vs_markov(tran2, thin_rows):
    """G^2 of independence against first-order Markov for pair counts tran2[a, b] (mcsamples.py:1124-1139); None where the
    reference gives up ("Raftery and Lewis estimator had problems")."""
    rows, cols = tran2.sum(axis=1), tran2.sum(axis=0)
    g2 = 0
    for (a, b), focus in np.ndenumerate(tran2):
        if focus != 0:
            fitted = float(rows[a] * cols[b]) / float(thin_rows - 1)
            if fitted <= 0 or focus <= 0:
                return None
            g2 += np.log(float(focus) / fitted) * float(focus)
    return 2 * g2


class WeightedSamples:
    """
    The methods getdist's WeightedSamples defines (chains.py:179-1089), over the sample set resident on the device, and the
    private helpers they share.
    """

    # ---- the host mirror of the samples ----------------------------------------------------------------------
    # ``samples`` is the reference's (N, n) fp64 host array.  A set built from host data stores it at construction and never
    # downloads anything; a set built from a device array (MCSamples._read_device_chains) has none until it is first read:
    # then the resident columns are downloaded once (gd_download_samples) and kept.
    @property
    def samples(self):
        s = self.__dict__.get("_samples")
        if s is None and self.__dict__.get("_samples_on_device"):
            s = self.__dict__["_samples"] = self.ctx.download_samples()
        return s

    @samples.setter
    def samples(self, value):
        self.__dict__["_samples"] = value
        self.__dict__["_samples_on_device"] = False
        self.__dict__["_mirror_assigned"] = True  # until the next upload the resident set is not known to equal it

    @property
    def _host_mirror_ready(self):
        """False while the samples of a set built from a device array exist on the device only"""
        return self.__dict__.get("_samples") is not None

    def _sample_row(self, i):
        """samples[i] without forming the host mirror for it"""
        return self.samples[i] if self._host_mirror_ready else self.ctx.read_row(i)

    # ---- replacing the sample set (chains.py:276-323) --------------------------------------------------------
    def setSamples(self, samples, weights=None, loglikes=None, min_weight_ratio=None):
        """chains.py:276-300: replace samples / weights; drops the device mirror and every derived cache."""
        samples = np.asarray(samples)
        if samples.ndim == 1:
            samples = samples.reshape(-1, 1)
        if samples.shape[1] != self.n:
            raise WeightedSampleError("setSamples: number of parameters changed")
        self.samples = samples
        self.numrows = samples.shape[0]
        self.weights = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        self.loglikes = None if loglikes is None else np.asarray(loglikes, dtype=np.float64)
        if min_weight_ratio is not None:
            self.min_weight_ratio = min_weight_ratio
        self.chain_offsets = None
        self._weightsChanged()

    def changeSamples(self, samples):
        """chains.py:302-308"""
        self.setSamples(samples, self.weights, self.loglikes)

    def _weightsChanged(self, filter_weights=True, resident=False):
        """chains.py:310-323: everything derived from samples/weights is stale; re-upload (unless an edit on the device has
        left the ``resident`` set what the host state says) and recompute.  The min-weight filter belongs to setSamples
        (chains.py:296-299), not to the reference's _weightsChanged: mutators that call that directly
        (reweightAddingLogLikes, cool) pass filter_weights=False."""
        self.means = self.vars = self.sddev = self.fullcov = self.correlationMatrix = None
        if not resident:
            self._upload(filter_weights=filter_weights)
        self.needs_update = True
        self.updateBaseStatistics()

    # ---- mutators of the sample set (state invalidation): every one states its edit once, to _edit_samples ----
    # Where it can, the resident set is replaced by a selection of itself, device to device (gd_select_samples): no
    # fancy-indexed copy of the matrix on the host, no re-upload, and a set built from device arrays keeps doing without its
    # host mirror.  Otherwise the same edit is made on the host array with numpy and uploaded.
    def _device_edit_applies(self):
        """The resident set can be edited in place of the host array: a real context (the CPU tests' doubles without
        ``select_samples`` keep the host route), every column on this device, and a host mirror that is absent or float64 (and
        was uploaded as it is) -- then ``samples``, made again on first read (gd_download_samples), is bit for bit what numpy
        indexing gives."""
        if not hasattr(self.ctx, "select_samples") or getattr(self, "_column_share", None) is not None:
            return False
        if self.__dict__.get("_mirror_assigned"):  # ``samples`` was assigned since the last upload: the host array is the truth
            return False
        mirror = self.__dict__.get("_samples")
        if mirror is None:
            return bool(self.__dict__.get("_samples_on_device"))
        return isinstance(mirror, np.ndarray) and mirror.dtype == np.float64 and mirror.ndim == 2

    def _select_on_device(self, **selection):
        """ctx.select_samples(**selection); afterwards the samples exist on the device only.  False when the second set does
        not fit beside the first (the caller takes the host route); any other refusal raises with the object unchanged."""
        from ._lib import GD_ERR_NOMEM, GdhipError

        try:
            self.ctx.select_samples(**selection)
        except GdhipError as e:
            if e.code != GD_ERR_NOMEM:
                raise
            return False
        self.__dict__["_samples"], self.__dict__["_samples_on_device"] = None, True
        return True

    def _edit_samples(self, rows=None, keep_cols=None, append=None, weights="keep", chain_offsets=None, index=None, device=True):
        """The sample set becomes a selection of itself.  ``rows`` / ``keep_cols`` / ``weights`` as Context.select_samples takes
        them; ``append`` too, a host vector or ``("slot", s, expr)`` with the expression that spare column s was evaluated
        from (the host route fetches its values); ``chain_offsets`` are those of the result.  ``index`` is what numpy indexes
        the rows with, where ``rows`` does not say it (a device row list) or only numpy can judge it; ``device`` is the
        caller's own condition for the device route, which is taken when _device_edit_applies and the second set fits beside
        the first, else the same edit is made on the host array and uploaded.  The new host weights and loglikes are the old
        ones at ``index``, so a selection numpy refuses raises numpy's error before anything has changed."""
        if index is None:
            index = slice(None) if rows is None else slice(rows[1], rows[2]) if rows[0] == "range" else rows[1]
        if isinstance(weights, str):
            weights_new = None if weights == "unit" or self.weights is None else self.weights[index]
        else:
            weights_new = weights
        loglikes = None if self.loglikes is None else self.loglikes[index]
        on_device = device and self._device_edit_applies()
        if on_device:
            self._sample_set_changing()
            on_device = self._select_on_device(rows=rows, keep_cols=keep_cols, append=append, weights=weights)
        if on_device:
            numrows, n = self.ctx.N, self.ctx.n
        else:
            samples = self.samples[index, :]
            if keep_cols is not None:
                samples = np.delete(samples, np.setdiff1d(np.arange(self.n), keep_cols), 1)
            if append is not None:
                old = samples
                samples = np.empty((old.shape[0], old.shape[1] + 1), dtype=np.float64, order="F")  # the device layout: no transpose
                samples[:, :-1] = old
                samples[:, -1] = append[2].eval(self) if isinstance(append, tuple) else append
            numrows, n = samples.shape
        if n != len(self.paramNames.names):
            raise WeightedSampleError("number of sample columns does not match the parameter names")
        if not on_device:
            self.samples = samples
        self.numrows, self.n = numrows, n
        self.weights = None if weights_new is None else np.ascontiguousarray(weights_new, dtype=np.float64)
        self.loglikes = None if loglikes is None else np.ascontiguousarray(loglikes, dtype=np.float64)
        self.chain_offsets = None if chain_offsets is None else np.asarray(chain_offsets, dtype=np.int64)
        self.index = {p.name: i for i, p in enumerate(self.paramNames.names)}
        self._weightsChanged(filter_weights=False, resident=on_device)

    def _weights_replaced(self):
        """_weightsChanged(filter_weights=False) for mutators that change ``self.weights`` only: the resident weight column
        is replaced (gd_set_weights), the sample columns stay where they are."""
        resident = (hasattr(self.ctx, "set_weights") and getattr(self, "_column_share", None) is None
                    and not self.__dict__.get("_mirror_assigned"))
        if resident:
            self._sample_set_changing()
            self.ctx.set_weights(self.weights)
        self._weightsChanged(filter_weights=False, resident=resident)

    def _host_weights(self):
        return self.weights if self.weights is not None else np.ones(self.numrows)

    def thin(self, factor):
        """chains.py:941-952: thin by ``factor`` to unit-weight samples (integer weights).  The thinned row list comes
        from the device (gd_thin_rows); chain boundaries follow the rows that survive."""
        if not self.ctx.weights_integral():
            raise WeightedSampleError("Can only thin with integer weights")
        buf, K = self._thin_rows(factor)  # (the list goes into the selection as it lies in device memory)
        try:
            thin_ix = buf.to_host((K,), dtype=np.int32).astype(np.int64) if K else np.zeros(0, dtype=np.int64)
            offsets = None if self.chain_offsets is None else np.searchsorted(thin_ix, self.chain_offsets)
            self._edit_samples(rows=("rows", buf, K), index=thin_ix, weights="unit", chain_offsets=offsets, device=K > 0)
        finally:
            buf.free()

    def weighted_thin(self, factor):
        """chains.py:954-966,1188-1206: thin by ``factor`` keeping integer multiplicities; separate chains are thinned
        one by one (the cumulative weight restarts with every chain), as the reference does."""
        if not self.ctx.weights_integral():
            raise WeightedSampleError("Can only thin with integer weights")
        ranges = [(0, self.numrows)] if self.chain_offsets is None else self._chain_ranges()
        rows, counts, lens = [], [], [0]
        for lo, hi in ranges:
            buf, K = self._thin_rows(factor, lo, hi)
            ix = buf.to_host((K,), dtype=np.int32).astype(np.int64) if K else np.zeros(0, dtype=np.int64)
            buf.free()
            u, c = np.unique(ix, return_counts=True)
            rows.append(u), counts.append(c), lens.append(len(u))
        rows, counts = np.concatenate(rows), np.concatenate(counts)
        offsets = None if self.chain_offsets is None else np.cumsum(lens)
        self._edit_samples(rows=("rows", rows), weights=counts.astype(np.float64), chain_offsets=offsets, device=rows.size > 0)

    def filter(self, where):
        """chains.py:968-979,1174-1186: keep the rows ``where`` (boolean mask, row indices, or a boolean column expression,
        whose mask is fetched from the device as bytes)"""
        if _is_expr(where):
            if not where.is_bool:
                raise WeightedSampleError("filter takes a boolean expression (a comparison), not a float one")
            where = where.eval(self)
        where = np.asarray(where)
        offsets = None
        if self.chain_offsets is not None:
            if where.dtype == bool:
                offsets = np.cumsum([0] + [int(np.count_nonzero(where[a:b])) for a, b in self._chain_ranges()])
            elif where.size == 0 or np.all(np.diff(where) > 0):
                offsets = np.searchsorted(where, self.chain_offsets)
        # the device route serves what numpy would accept without a doubt: a mask of one entry per row, or in-range integer
        # indices (negative ones counted from the end); anything else goes to numpy, whose error it then is
        rows = None
        if where.dtype == bool and where.shape == (self.numrows,):
            rows = ("mask", where)
        elif (where.ndim == 1 and where.size and where.dtype.kind in "iu" and where.min() >= -self.numrows
              and where.max() < self.numrows):
            rows = ("rows", np.where(where < 0, where + self.numrows, where))
        self._edit_samples(rows=rows, index=where, chain_offsets=offsets, device=rows is not None)

    def deleteZeros(self):
        """chains.py:1010-1015"""
        self.filter(self._host_weights() > 0)

    def setMinWeightRatio(self, min_weight_ratio=1e-30):
        """chains.py:1017-1027"""
        if self.weights is not None and min_weight_ratio >= 0:
            mx, mn = np.max(self.weights), np.min(self.weights)
            if mn < mx * min_weight_ratio:
                self.filter(self.weights > mx * min_weight_ratio)

    def reweightAddingLogLikes(self, logLikes):
        """chains.py:981-993: importance-sample by adding ``logLikes`` (-log likelihood per sample; a host vector or a column
        expression, which is evaluated on the device and fetched)"""
        if _is_expr(logLikes):
            logLikes = logLikes.eval(self)
        logLikes = np.asarray(logLikes, dtype=np.float64)
        if logLikes.shape != (self.numrows,):
            raise WeightedSampleError("logLikes must have one entry per sample")
        scale = np.min(logLikes)
        if self.loglikes is not None:
            self.loglikes = self.loglikes + logLikes
        self.weights = self._host_weights() * np.exp(-(logLikes - scale))
        self._weights_replaced()

    def cool(self, cool=None):
        """mcsamples.py:533-550 + chains.py:995-1008: multiply the log-likelihoods by ``cool`` and re-weight"""
        if cool is None:
            if self.temperature is None:
                raise ValueError("Pass a cooling temperature, since the sample does not have one specified")
            cool = float(self.temperature)
        if cool == 1:
            return
        if self.cooled != 1:
            logging.warning("Chain has already been cooled by %s", self.cooled)
        if self.loglikes is None:
            raise WeightedSampleError("Samples have no likelihood values, required to cool")
        MaxL = np.min(self.loglikes)
        newL = self.loglikes * cool
        self.weights = self._host_weights() * np.exp(-(newL - self.loglikes) - (MaxL * (1 - cool)))
        self.loglikes = newL
        self._weights_replaced()
        self.cooled = cool
        if self.temperature is not None:
            self.temperature = float(self.temperature) / cool

    def removeBurn(self, remove=0.3):
        """chains.py:1047-1061: drop the first ``remove`` fraction of the rows (or that many rows if >= 1)"""
        ix = int(remove) if remove >= 1 else int(round(self.numrows * remove))
        offsets = None
        if self.chain_offsets is not None:
            # the rows go from the front of the stacked array (the reference, chains.py:1047-1061, knows no chains here);
            # chains that lose all their rows are dropped from the chain list instead of staying behind with zero length
            offsets = np.unique(np.maximum(self.chain_offsets - ix, 0))
            if len(offsets) < 2:
                offsets = None
        self._edit_samples(rows=("range", ix, self.numrows), chain_offsets=offsets, device=0 <= ix < self.numrows)

    def removeBurnFraction(self, ignore_frac):
        """chains.py:1529-1543: remove the burn-in fraction (or number of rows) from every chain.  The chains of this library
        are always combined into one stacked set, for which the reference removes the rows from the front of it."""
        self.removeBurn(ignore_frac)
        self.needs_update = True

    def deleteFixedParams(self):
        """chains.py:1029-1045,1544-1559: remove the parameters that do not vary (they become zero-width ranges).
        Returns (indices removed, their values)."""
        fixed, values = [], []
        on_device = self._device_edit_applies()
        if on_device and not self._host_mirror_ready:
            # fixedness without the host mirror, by the probe of the constructor's device route: the first and the last row,
            # then the candidate columns only
            first, last = self.ctx.read_row(0), self.ctx.read_row(self.numrows - 1)
            column = self.ctx.read_column
        else:
            first, last = self.samples[0], self.samples[-1]
            column = (lambda i: self.samples[:, i])
        for i in range(self.n):
            if np.isclose(first[i], last[i], equal_nan=True):
                col = column(i)
                mean = np.average(col)
                if np.allclose(col, mean, rtol=1e-12, atol=0, equal_nan=True):
                    fixed.append(i)
                    values.append(mean)
        if fixed:
            keep = [i for i in range(self.n) if i not in fixed]
            for ix, value in zip(fixed, values):
                self.ranges.setFixed(self.paramNames.names[ix].name, value)
            self.paramNames.deleteIndices(fixed)
            self._edit_samples(keep_cols=keep, chain_offsets=self.chain_offsets, device=bool(keep))
        return fixed, values

    # ---- name and label (chains.py:260-273) ------------------------------------------------------------------
    def getName(self):
        return self.name_tag

    def getLabel(self):
        """chains.py:260-266: the samples' label for legends (the name tag with LaTeX specials escaped when there is none)"""
        if self.label:
            return self.label
        name = self.getName()
        return None if name is None else "".join("\\" + ch if ch in "_&%$#{}" else ch for ch in name)

    # ---- text export (chains.py:227, 1063-1085) --------------------------------------------------------------
    precision = "%.8e"  # chains.py:227: the format of saveAsText

    def _text_sources(self):
        """(field sources of gd_format_rows, host_rows) for the rows of a chain file: weight, -log(posterior) (zeros when
        there are no loglikes, chains.py:1072-1075), parameters.  The loglikes go into a spare device column; ``host_rows``
        is the same table from the host arrays, for a ``precision`` the device does not format."""
        from ._lib import GD_FMT_SRC_WEIGHT, GD_FMT_SRC_ZERO

        ll = GD_FMT_SRC_ZERO if self.loglikes is None else self.ctx.set_extra_column(self.ctx.EXTRA_COLS - 1, self.loglikes)

        def host_rows(index):
            w = self._host_weights()[index]
            loglikes = np.zeros(len(w)) if self.loglikes is None else self.loglikes[index]
            return np.hstack((w.reshape(-1, 1), loglikes.reshape(-1, 1), self.samples[index]))

        return [GD_FMT_SRC_WEIGHT, ll] + list(range(self.n)), host_rows

    def _save_rows_as_text(self, root, chain_index, make_dirs, lo, hi, precision, sources=None):
        """chains.py:1076-1085 for rows [lo, hi) of the resident set, formatted on the device (chainfiles.write_text_rows)"""
        from . import chainfiles

        if make_dirs and not os.path.exists(os.path.dirname(root)):
            os.makedirs(os.path.dirname(root))
        if root.endswith(".txt"):
            root = root[:-3]  # (the reference's slice: the dot stays)
        srcs, host_rows = sources or self._text_sources()
        chainfiles.write_text_rows(root + ("" if chain_index is None else "_" + str(chain_index + 1)) + ".txt", self.ctx, srcs,
                                   (int(lo), int(hi)), fmt=precision, host_rows=host_rows)

    def saveAsText(self, root, chain_index=None, make_dirs=False):
        """chains.py:1063-1085: the samples as ``root[_<chain_index + 1>].txt`` with columns weight, -log(posterior),
        parameters in the format ``self.precision`` -- the bytes np.savetxt writes, formatted on the device."""
        self._save_rows_as_text(root, chain_index, make_dirs, 0, self.numrows, self.precision)

    # ---- moments (chains.py:339-412, 636-780) ------------------------------------------------------------
    # Vectors, row filters and alternative weights (chains.py:325-337, 636-780): a host vector goes into one of the
    # device's spare columns; `where=` / `weights=` become an auxiliary weight vector (weights*mask) that is swapped in
    # for the duration of the call, which gives exactly the reference's x[where], w[where] sums.
    def _host_vector(self, par):
        """The host vector behind a non-column argument of _makeParamvec (chains.py:325-337), else None."""
        if isinstance(par, np.ndarray):
            if par.shape != (self.numrows,):
                raise WeightedSampleError("parameter vector must have one entry per sample")
            return par
        if isinstance(par, (int, np.integer)) and not isinstance(par, bool):
            if par == -1:
                if self.loglikes is None:
                    raise WeightedSampleError("Samples do not have logLikes (par=-1)")
                return self.loglikes
            if par == -2:
                return self.weights if self.weights is not None else np.ones(self.numrows)
            if not 0 <= par < self.n:
                raise WeightedSampleError("Parameter %i does not exist" % par)
        return None

    def _vec_col(self, par, slot=0):
        """Device column index for a parameter reference, a host vector (uploaded into spare column ``slot``) or a column
        expression (evaluated into that slot on the device, colexpr.py).  An expression that reads the loglikes has them
        made resident in their usual slot, the last one, first: such a call has one slot fewer."""
        vec = par.vec if isinstance(par, ParamConfidenceData) else (par if _is_expr(par) else self._host_vector(par))
        if _is_expr(vec):
            if slot >= self.ctx.EXTRA_COLS - (1 if vec.uses_loglikes() else 0):
                raise WeightedSampleError("at most %d vector arguments per call" % self.ctx.EXTRA_COLS)
            return vec.to_column(self, slot)
        if vec is not None:
            if slot >= self.ctx.EXTRA_COLS:
                raise WeightedSampleError("at most %d vector arguments per call" % self.ctx.EXTRA_COLS)
            return self.ctx.set_extra_column(slot, vec)
        return par.col if isinstance(par, ParamConfidenceData) else self._col(par)

    def _where_weights(self, where):
        """weights*mask for a boolean mask or an index array (numpy semantics of x[where])."""
        where = np.asarray(where)
        w = self.weights if self.weights is not None else np.ones(self.numrows)
        if where.dtype == bool:
            if where.shape != (self.numrows,):
                raise WeightedSampleError("where must have one entry per sample")
            return w * where
        return w * np.bincount(_where_rows(where, self.numrows), minlength=self.numrows)

    def _with_weights(self, w_host, fn):
        """Run ``fn`` with the auxiliary weight vector ``w_host`` selected on the device."""
        self.ctx.aux_weights(w_host)
        return self._with_aux_selected(fn)

    def _with_aux_selected(self, fn):
        self._like_mode = None  # the auxiliary buffer is shared with the like weights
        self.ctx.select_weights(1)
        try:
            return fn()
        finally:
            self.ctx.select_weights(0)

    def _where_expr_weights(self, where):
        """weights*mask of a boolean column expression, formed in the auxiliary weight buffer on the device."""
        if not where.is_bool:
            raise WeightedSampleError("where= takes a boolean expression (a comparison), not a float one")
        self._like_mode = None  # the auxiliary buffer is shared with the like weights: forget them BEFORE it is overwritten,
        where.to_aux_weights(self)  # so that an error raised between here and the selection leaves no stale claim on it

    def _with_where(self, where, fn):
        """Run ``fn`` over the rows ``where`` selects: a boolean column expression, a boolean mask or an index array."""
        if _is_expr(where):
            self._where_expr_weights(where)
            return self._with_aux_selected(fn)
        return self._with_weights(self._where_weights(where), fn)

    def get_norm(self, where=None):
        if where is None:
            return self.norm
        return self._with_where(where, lambda: self.ctx.weight_stats()["norm"])

    def weighted_sum(self, paramVec, where=None):
        """chains.py:636-649"""
        return self.mean(paramVec, where) * self.get_norm(where)

    def getMeans(self, pars=None):
        return self.means if pars is None else np.array([self.means[i] for i in pars])

    def getVars(self):
        return self.vars

    def _setCov(self):
        _, cov, _ = self.ctx.cov()
        self.fullcov = cov
        return cov

    def getCov(self, nparam=None, pars=None):
        if self.fullcov is None:
            self._setCov()
        if pars is not None:
            return self.fullcov[np.ix_(pars, pars)]
        return self.fullcov[:nparam, :nparam]

    def _moments(self, pars, where):
        """(means, cov, norm) of parameter references / vectors, optionally over a row filter: one gd_cov call."""
        if _is_expr(where):  # first: a mask that reads the loglikes borrows the last spare column while it is evaluated
            self._where_expr_weights(where)
        slot = 0
        cols = []
        for p in pars:
            if _is_expr(p) or self._host_vector(p) is not None:
                cols.append(self._vec_col(p, slot))
                slot += 1
            else:
                cols.append(self._col(p))
        if where is None:
            return self.ctx.cov(cols)
        if _is_expr(where):
            return self._with_aux_selected(lambda: self.ctx.cov(cols))
        return self._with_weights(self._where_weights(where), lambda: self.ctx.cov(cols))

    def cov(self, pars=None, where=None):
        """chains.py:709-733"""
        if isinstance(pars, (int, np.integer)):
            pars = range(pars)
        return self._moments(list(range(self.n)) if pars is None else list(pars), where)[1]

    def corr(self, pars=None):
        return covToCorr(self.cov(pars))

    def getSignalToNoise(self, params, noise=None, R=None, eigs_only=False):
        """chains.py:840-851: getSignalToNoise of the covariance of ``params`` (one device pass; the rest is m x m host algebra)"""
        return getSignalToNoise(self.cov(params), noise, R, eigs_only)

    def getCorrelationMatrix(self):
        if self.correlationMatrix is None:
            self.correlationMatrix = covToCorr(self.getCov())
        return self.correlationMatrix

    def _col(self, par):
        if type(par) is int and 0 <= par < self.n:
            return par
        j = self._parAndNumber(par)[0]
        if j is None:
            raise ParamError("unknown parameter %s" % par)
        return j

    def _is_plain_column(self, par):
        return not _is_expr(par) and self._host_vector(par) is None

    def mean(self, paramVec, where=None):
        """chains.py:665-677"""
        if isinstance(paramVec, (list, tuple)):
            if where is None and all(self._is_plain_column(p) for p in paramVec):
                return np.array([self.means[self._col(p)] for p in paramVec])
            if _is_expr(where):  # the mask is evaluated once for the whole list
                self._where_expr_weights(where)
                return self._with_aux_selected(lambda: np.array([self._moments([p], None)[0][0] for p in paramVec]))
            return np.array([self.mean(p, where) for p in paramVec])
        if where is None and self._is_plain_column(paramVec):
            return self.means[self._col(paramVec)]
        return self._moments([paramVec], where)[0][0]

    def var(self, paramVec, where=None):
        """chains.py:679-693 (like the reference, a list ignores ``where``)"""
        if isinstance(paramVec, (list, tuple)):
            return np.array([self.var(p) for p in paramVec])
        if where is None and self._is_plain_column(paramVec):
            return self.vars[self._col(paramVec)]
        return self._moments([paramVec], where)[1][0, 0]

    def std(self, paramVec, where=None):
        return np.sqrt(self.var(paramVec, where))

    def mean_diff(self, paramVec, where=None):
        """chains.py:744-761 (host vector p_i - mean; the device path never materialises it)"""
        vec = paramVec.eval(self) if _is_expr(paramVec) else self._host_vector(paramVec)
        if vec is None:
            vec = self.samples[:, self._col(paramVec)]
        if where is None:
            return vec - self.mean(paramVec)
        return vec[where.eval(self) if _is_expr(where) else where] - self.mean(paramVec, where)

    def mean_diffs(self, pars=None, where=None):
        """chains.py:763-780"""
        cols = range(self.n) if pars is None else (range(pars) if isinstance(pars, (int, np.integer)) else pars)
        return [self.mean_diff(j, where) for j in cols]

    # ---- weighted quantiles (chains.py:782-838) ----------------------------------------------------------
    def confidence(self, paramVec, limfrac, upper=False, start=0, end=None, weights=None):
        """chains.py:814-838: sort-free weighted quantile selection on the device (gd_quantiles)."""
        if isinstance(paramVec, ParamConfidenceData):
            start, end = paramVec.start, paramVec.end
            weights = paramVec.weights if weights is None else weights
        vec_arg = paramVec.vec if isinstance(paramVec, ParamConfidenceData) else (
            paramVec if _is_expr(paramVec) else self._host_vector(paramVec))
        j = self._vec_col(paramVec)
        limfrac = np.atleast_1d(np.asarray(limfrac, dtype=np.float64))
        end = self.numrows if end is None else end

        def select():
            full = start == 0 and end == self.numrows and weights is None
            norm = self.norm if full else self.ctx.weight_stats(start, end)["norm"]
            targets = norm * limfrac if not upper else norm * (1 - limfrac)
            mm = self._minmax_of([j]) if (vec_arg is None and j < self.n) else None
            return self.ctx.quantiles([j], targets[None, :], lo=start, hi=end, minmax=mm)[0]

        if weights is None:
            out = select()
        else:
            weights = np.asarray(weights, dtype=np.float64)
            if weights.shape != (self.numrows,):
                raise WeightedSampleError("weights must have one entry per sample")
            out = self._with_weights(weights, select)
        return out if out.size > 1 else out[0]

    def twoTailLimits(self, paramVec, confidence):
        limits = np.array([(1 - confidence) / 2, 1 - (1 - confidence) / 2])
        return self.confidence(paramVec, limits)

    def initParamConfidenceData(self, paramVec, start=0, end=None, weights=None):
        """
        chains.py:793-812.  The reference caches argsort + cumulative weights here; the device path selects
        quantiles without sorting, so the "cache" is just the (column, row range) handle confidence() accepts.
        """
        vec = paramVec if _is_expr(paramVec) else self._host_vector(paramVec)  # (an expression is kept as the handle's vec)
        return ParamConfidenceData(None if vec is not None else self._col(paramVec), start,
                                   self.numrows if end is None else end, weights=weights, vec=vec)

    def _minmax_of(self, js):
        """(len(js), 2) minima / maxima of resident columns from the base statistics: with them the quantile select
        needs two reads of a column instead of four (gd_quantiles_mm)."""
        if getattr(self, "_col_min", None) is None:
            return None
        js = np.asarray(js, dtype=np.int64)
        return np.stack([np.asarray(self._col_min)[js], np.asarray(self._col_max)[js]], axis=1)

    # ---- thinned-chain diagnostics (mcsamples.py:1039-1221; chains.py:853-916) ---------------------------------
    def _chain_ranges(self):
        if self.chain_offsets is None:
            raise WeightedSampleError("Samples were not combined from separate chains")
        return [(int(a), int(b)) for a, b in zip(self.chain_offsets[:-1], self.chain_offsets[1:])]

    def _thin_rows(self, factor, lo=0, hi=None):
        """
        Device row list of the weight-one thinning of rows [lo,hi) (chains.py:878-916): (buffer, count).  Which of the
        reference's two branches applies is decided by factor >= max weight of that chain, as there.
        """
        hi = self.numrows if hi is None else hi
        return self._thin_rows_on(self.ctx, factor, lo, hi)

    @staticmethod
    def _thin_rows_on(ctx, factor, lo, hi):
        if factor != int(factor):
            raise WeightedSampleError("Thin factor must be integer")
        ws = ctx.weight_stats(lo, hi)
        unique_mode = int(factor) >= ws["max_w"]
        capacity = int(ws["norm"]) // int(factor) + 2
        return ctx.thin_rows(lo, hi, int(factor), unique_mode, capacity)

    def thin_indices(self, factor, weights=None):
        """chains.py:853-863: indices that make single-weight samples (the device list copied to the host).  ``weights``:
        thin THAT weight vector instead of the resident one (any length, as the reference's static
        thin_indices_single_samples does): it is uploaded to a short-lived context of its own -- the cached prefix sum and the
        thinning kernels belong to a context's sample weights -- and thinned by the same kernels."""
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64).ravel()
            if w.size == 0:
                return np.zeros(0, dtype=np.int64)
            tmp = self._context_factory(self._device)
            try:
                tmp.upload(np.zeros((w.size, 1)), w)
                if not tmp.weights_integral():
                    raise WeightedSampleError("Can only thin with integer weights")
                buf, K = self._thin_rows_on(tmp, factor, 0, w.size)
                out = buf.to_host((K,), dtype=np.int32).astype(np.int64) if K else np.zeros(0, dtype=np.int64)
                buf.free()
            finally:
                tmp.close()
            return out
        if not self.ctx.weights_integral():
            raise WeightedSampleError("Can only thin with integer weights")
        buf, K = self._thin_rows(factor)
        out = buf.to_host((K,), dtype=np.int32).astype(np.int64) if K else np.zeros(0, dtype=np.int64)
        buf.free()
        return out

    # ---- weight-one random draws (chains.py:918-939; mcsamples.py:578-606) --------------------------------------
    def _draw_single_rows(self, random_state, a, b, mode):
        """
        Device row list (buffer, count) of the rows a weight-one draw keeps: rand <= w / (a * b) (mode 0) or (w / a) / b
        (mode 1), rand = np.random.default_rng(random_state).random(numrows) -- the reference's rows, bit for bit.  A PCG64
        bit generator (numpy's default) hands its (state, inc) to the device, where every thread regenerates its rows'
        variates (gd_draw_single_rows), and is moved numrows steps on; any other bit generator draws on the host and the
        vector is uploaded.  Either way a Generator the caller passed in ends where the reference leaves it.
        """
        rng = np.random.default_rng(random_state)
        bg = rng.bit_generator
        if type(bg) is np.random.PCG64:
            before = bg.state
            source = dict(pcg=(before["state"]["state"], before["state"]["inc"]))
            bg.advance(self.numrows)
            if before["has_uint32"]:  # random() keeps a buffered 32-bit half, advance() drops it
                after = bg.state
                after["has_uint32"], after["uinteger"] = before["has_uint32"], before["uinteger"]
                bg.state = after
        else:
            source = dict(rand=rng.random(self.numrows))
        # room for the expected number of rows and eight standard deviations (Poisson-binomial: variance <= mean); the rare
        # draw that keeps more reports its count and is repeated with exactly that room
        with np.errstate(all="ignore"):
            mean = float(self.norm) / (float(a) * float(b))
        capacity = self.numrows
        if np.isfinite(mean) and mean >= 0:
            capacity = min(self.numrows, int(mean + 8 * np.sqrt(mean)) + 64)
        buf, K = self.ctx.draw_single_rows(a, b, mode, capacity=capacity, **source)
        if buf is None:
            buf, K = self.ctx.draw_single_rows(a, b, mode, capacity=K, **source)
        return buf, K

    def random_single_samples_indices(self, random_state=None, thin=None, max_samples=None):
        """chains.py:918-939: indices of a weight-one subset, each row kept with probability weight / (max weight * thin);
        the same rows as the reference for the same ``random_state`` (seed, Generator or bit generator).  ``max_samples``
        thins to that mean number of rows instead.  The draw and the ordered compaction run on the device."""
        if max_samples is None:
            thin = thin or 1
        else:
            if thin is not None:
                raise WeightedSampleError("Cannot set thin and max_samples")
            thin = max(1, self.norm / self.max_mult / max_samples)
        buf, K = self._draw_single_rows(random_state, self.max_mult, thin, 0)
        out = buf.to_host((K,), dtype=np.int32).astype(np.int64) if K else np.zeros(0, dtype=np.int64)
        buf.free()
        return out

    # ---- autocorrelation / effective samples (chains.py:423-574) -------------------------------------------
    DIRECT_LAGS_MAX = 512  # beyond this many lags the length-2N FFT (gd_autoconvolve) is cheaper than lag sums

    def _autocov(self, col, mean, k0, nlags):
        """Un-normalised autocovariance lag sums sum_i d_i d_{i+k}, d = (x - mean) w, for k0 <= k < k0 + nlags: direct
        lag sums for a few lags, the reference's FFT route (convolve.py:458-478 on the device) for many."""
        if nlags <= self.DIRECT_LAGS_MAX:
            return self.ctx.autocov_lags(col, mean, k0, nlags)
        from .convolve import nearestFFTnumber

        s = int(nearestFFTnumber(2 * self.numrows))
        return self.ctx.autoconvolve(s, k0 + nlags, False, col=col, mean=mean, use_weights=self.weights is not None)[k0:]

    def _mean_var_of(self, par, col, want_var=True):
        """(mean, variance) of ``par``, which _vec_col has just placed in device column ``col``.  An expression is not
        evaluated again for them: one gd_cov over the column it sits in, the call mean() and var() would each end in."""
        if _is_expr(par):
            means, cov, _ = self.ctx.cov([col])
            return means[0], cov[0, 0]
        return self.mean(par), (self.var(par) if want_var else None)

    def getAutocorrelation(self, paramVec, maxOff=None, weight_units=True, normalized=True):
        """chains.py:423-447; ``paramVec`` may be a parameter or a vector of one value per sample"""
        j = self._vec_col(paramVec)
        if maxOff is None:
            maxOff = self.n - 1
        mean, var = self._mean_var_of(paramVec, j, normalized)
        lags = self._autocov(j, mean, 0, maxOff + 1)
        corr = lags / np.arange(self.numrows, self.numrows - (maxOff + 1), -1)
        if normalized:
            corr /= var
        if weight_units:
            return corr * self.numrows / self.norm
        return corr

    def getCorrelationLength(self, j, weight_units=True, min_corr=0.05, corr=None):
        """chains.py:449-466.  Without ``corr``: direct lag sums in growing chunks with early exit; a
        chain whose correlation has not dropped below ``min_corr`` within DIRECT_LAGS_MAX lags takes the FFT route for
        all N/10 lags at once."""
        if corr is not None:
            corr = np.asarray(corr)
            ix = int(np.argmin(corr > min_corr * corr[0]))
            return corr[0] + 2 * np.sum(corr[1:ix])
        col = self._vec_col(j)
        mean, var = self._mean_var_of(j, col)
        max_off = self.numrows // 10
        scale = (self.numrows / self.norm) if weight_units else 1.0
        vals = np.zeros(0)
        k0, chunk = 0, 32
        while k0 <= max_off:
            nl = min(chunk, max_off + 1 - k0)
            if k0 + nl > self.DIRECT_LAGS_MAX:
                nl = max_off + 1 - k0  # everything that is left, in one transform
            lags = self._autocov(col, mean, k0, nl)
            c = lags / (self.numrows - np.arange(k0, k0 + nl)) / var * scale
            vals = np.concatenate([vals, c])
            below = np.nonzero(~(vals > min_corr * vals[0]))[0]
            if below.size:
                return vals[0] + 2 * float(np.sum(vals[1:int(below[0])]))
            k0 += nl
            chunk *= 2
        return vals[0]  # argmin of an all-True mask is 0 (chains.py:464-465)

    def getEffectiveSamples(self, j=0, min_corr=0.05):
        return self.norm / self.getCorrelationLength(j, min_corr=min_corr)

    def getEffectiveSamplesGaussianKDE(self, paramVec, h=0.2, scale=None, maxoff=None, min_corr=0.05):
        """chains.py:477-574; the lag sums with the Gaussian kernel run on the GPU."""
        if self.sampler in ("nested", "uncorrelated"):
            return self.norm**2 / self._sum_w2
        j = self._col(paramVec)
        kernel_std = (scale or self.sddev[j]) * h
        if maxoff is None:
            maxoff = int(self.getCorrelationLength(j, weight_units=False) * 1.5) + 4
        return self._neff_from_lags(j, kernel_std, maxoff, min_corr, None)

    def _neff_lag_list(self, tail=2):
        """The lags of the batched kernel-sum launch: the five of the uncorrelated term (chains.py:514-519) and the first
        ``tail`` of the scan (corr_k(1), corr_k(2): :541-545).  corr_k(2) is needed only by a chain that is still correlated
        at lag 1; _neff_batch asks for it up front (tail = 2) unless the autocorrelation probe shows every column of the
        batch below the threshold already at lag 1 -- then the launch carries six exponentials per sample instead of seven,
        and a column the probe misjudged fetches its lag 2 by itself (same value, one more launch)."""
        uncorr_len = self.numrows // 2
        return list(range(uncorr_len, uncorr_len + 5)) + [k for k in (1, 2)[:tail] if k <= self.numrows // 10]

    def _neff_from_lags(self, j, kernel_std, maxoff, min_corr, seed_sums):
        """The scalar part of chains.py:509-574 given (optionally pre-computed) Gaussian-kernel lag sums."""
        maxoff = min(maxoff, self.numrows // 10)
        uncorr_len = self.numrows // 2
        inv4s2 = 1.0 / (4 * kernel_std**2)
        lags = self._neff_lag_list() if seed_sums is None else self._neff_lag_list(len(seed_sums) - 5)
        sums = self.ctx.kde_lag_sums(j, inv4s2, lags) if seed_sums is None else seed_sums
        nav = sum(self.numrows - k for k in range(uncorr_len, uncorr_len + 5))
        uncorr_term = float(np.sum(sums[:5])) / nav
        n = float(self.numrows)
        cache = {k: sums[5 + i] for i, k in enumerate(lags[5:])}

        def corr_k(k):
            if k not in cache:
                cache[k] = self.ctx.kde_lag_sums(j, inv4s2, [k])[0]
            return cache[k] - (n - k) * uncorr_term

        corr0 = self._sum_w2
        threshold = min_corr * corr0
        c1 = corr_k(1)
        if c1 < threshold:
            N = corr0
        else:
            c2 = corr_k(2)
            if c2 > threshold:
                max_k = maxoff
                while max_k > 10:
                    if corr_k(max_k // 3) >= threshold:
                        break
                    max_k //= 3
                step_size = 1 if max_k < 20 else max_k // 10
                cum_sum = c1 + c2
                for k in range(3, maxoff + 1, step_size):
                    test_val = corr_k(k)
                    if test_val < threshold:
                        break
                    cum_sum += test_val * step_size if k > 3 else (test_val * step_size) / 2
                N = corr0 + 2 * cum_sum
            else:
                N = corr0 + 2 * c1
        return self.norm**2 / N

    def _probe_lags(self, todo, nl):
        """The first ``nl`` autocovariance lag sums of columns ``todo``: taken from the prefetch started by
        prepareParams on the second context (they need the means only, so they ran beside the quantile select), else
        computed now."""
        pre = getattr(self, "_lag_prefetch", None)
        self._lag_prefetch = None
        if pre is not None:
            cols, pnl, fut = pre
            try:
                lags = fut.result()
            except Exception:
                lags = None
            if lags is not None and pnl == nl and set(todo) <= set(cols):
                row = {c: k for k, c in enumerate(cols)}
                return lags[[row[c] for c in todo]]
        return self.ctx.autocov_lags_batch(todo, self.means[todo], 0, nl)

    def _neff_batch(self, js, min_corr=0.05):
        """_get1DNeff for many parameters with two batched launches (32 autocovariance lags, 7 kernel lag sums)."""
        todo = [j for j in js if self.paramNames.names[j].N_eff_kde is None]
        if not todo:
            return
        share = getattr(self, "_neff_share", None)
        if share is not None:
            # multi-rank runs (parallel.NeffShare): this rank computes the parameters it owns; the others arrive by an
            # exchange that is always issued from the main thread (collectives of a process stay on one thread), i.e.
            # here, or -- when this runs on the helper thread beside the binning -- by the caller's _neff_complete
            self._neff_share = None
            try:
                self._neff_batch([j for j in todo if j in share.params], min_corr)
            finally:
                self._neff_share = share
            if threading.current_thread() is threading.main_thread():
                self._neff_complete(js, min_corr)
            return
        if self.sampler in ("nested", "uncorrelated"):
            for j in todo:
                self.paramNames.names[j].N_eff_kde = self.norm**2 / self._sum_w2
            return
        max_off = self.numrows // 10
        nl = min(8, max_off + 1)  # short probe first; correlated chains continue in getCorrelationLength
        lag0 = self._probe_lags(todo, nl)
        kstd, maxoffs = [], []
        # the probe of all columns at once: c[row, k] = autocovariance at lag k over the variance (chains.py:449-466)
        C_all = np.asarray(lag0) / (self.numrows - np.arange(nl)) / np.asarray(self.vars)[todo][:, None]
        below_all = ~(C_all > min_corr * C_all[:, :1])
        first_below = np.where(below_all.any(axis=1), below_all.argmax(axis=1), -1).tolist()
        for row, j in enumerate(todo):
            par = self.paramNames.names[j]
            c = C_all[row]
            if first_below[row] >= 0:
                corrlen = c[0] + 2 * float(np.sum(c[1:first_below[row]]))
            elif nl == max_off + 1:
                corrlen = c[0]
            else:
                corrlen = self.getCorrelationLength(j, weight_units=False, min_corr=min_corr)
            kstd.append((par.sigma_range or self.sddev[j]) * 0.2)
            maxoffs.append(int(corrlen * 1.5) + 4)
        # (the rule of csrc/batch2d.hpp neff_batch: lag 2 rides along unless every column is uncorrelated at lag 1 by the probe)
        tail = 1 if all(fb == 1 for fb in first_below) else 2
        sums = self.ctx.kde_lag_sums_batch(todo, [1.0 / (4 * k**2) for k in kstd], self._neff_lag_list(tail))
        for row, j in enumerate(todo):
            self.paramNames.names[j].N_eff_kde = self._neff_from_lags(j, kstd[row], maxoffs[row], min_corr, sums[row])

    def _neff_complete(self, js, min_corr=0.05):
        """Multi-rank runs: fetch the N_eff values of the parameters other ranks own (parallel.NeffShare.exchange), then
        compute whatever nobody owned.  Main thread only."""
        share = getattr(self, "_neff_share", None)
        if share is None:
            return
        if not getattr(share, "exchanged", False):
            # unconditional, once per step on every rank: a rank whose own parameters cover its pairs must still enter
            # the collective the other ranks are waiting in
            share.exchanged = True
            share.exchange(self)
        self._neff_share = None
        try:
            self._neff_batch(js, min_corr)  # owned by nobody: computed here
        finally:
            self._neff_share = share

    def getEffectiveSamplesGaussianKDE_2d(self, i, j, h=0.3, maxoff=None, min_corr=0.05):
        """chains.py:576-635 (used when use_effective_samples_2D is set); lag sums on the GPU, 8 lags per launch."""
        if self.sampler in ("nested", "uncorrelated"):
            return self.norm**2 / self._sum_w2
        i, j = self._col(i), self._col(j)
        cov = self.getCov(pars=[i, j])
        if abs(cov[0, 1]) > np.sqrt(cov[0, 0] * cov[1, 1]) * 0.999:
            return self.getEffectiveSamplesGaussianKDE(i, h=h, min_corr=min_corr)  # totally correlated: 1D estimate
        kernel_inv = np.linalg.inv(cov) / h**2
        kinv3 = [kernel_inv[0, 0], kernel_inv[0, 1] + kernel_inv[1, 0], kernel_inv[1, 1]]
        if maxoff is None:
            maxoff = int(max(self.getCorrelationLength(i, weight_units=False),
                             self.getCorrelationLength(j, weight_units=False)) * 1.5) + 4
        maxoff = min(maxoff, self.numrows // 10)
        uncorr_len = self.numrows // 2
        sums = self.ctx.kde_lag_sums_2d(i, j, kinv3, list(range(uncorr_len, uncorr_len + 5)))
        nav = sum(self.numrows - k for k in range(uncorr_len, uncorr_len + 5))
        uncorr_term = float(np.sum(sums)) / nav
        corr0 = self._sum_w2
        n = float(self.numrows)
        total = 0.0
        k = 1
        done = False
        while k <= maxoff and not done:
            lags = list(range(k, min(k + 8, maxoff + 1)))
            vals = self.ctx.kde_lag_sums_2d(i, j, kinv3, lags)
            for kk, v in zip(lags, vals):
                c = v - (n - kk) * uncorr_term
                if c < min_corr * corr0:
                    done = True
                    break
                total += c
            k += len(lags)
        N = corr0 + 2 * total
        return self.norm**2 / N


class Chains(WeightedSamples):
    """Named parameters, the base statistics and the per-chain convergence statistics (chains.py:1092-1563, Chains)."""

    # ---- parameters (chains.py:1210-1304, 1354-1366) ---------------------------------------------------------
    def _parAndNumber(self, name):
        """chains.py:1235-1250"""
        if isinstance(name, ParamInfo):
            name = name.name
        if isinstance(name, str):
            name = self.index.get(name, None)
            if name is None:
                return None, None
        if isinstance(name, (int, np.integer)):
            return int(name), self.paramNames.names[int(name)]
        raise ParamError("Unknown parameter type %s" % name)

    def addDerived(self, paramVec, name, label="", comment="", range=None):
        """mcsamples.py:2560-2575 + chains.py:1354-1366: append a derived parameter column (a host vector, or a column
        expression evaluated on the device and fetched).  Returns its ParamInfo."""
        if self.paramNames.parWithName(name):
            raise ValueError("Parameter with name %s already exists" % name)
        par = ParamInfo(name, label or None)
        par.isDerived, par.comment = True, comment
        if _is_expr(paramVec) and self._device_edit_applies():
            # the expression is evaluated into a spare column and appended from there: its values never cross PCIe
            paramVec.to_column(self, 0)
            append = ("slot", 0, paramVec)
        else:
            if _is_expr(paramVec):
                paramVec = paramVec.eval(self)
            append = np.asarray(paramVec, dtype=np.float64).reshape(-1)
            if append.shape != (self.numrows,):
                raise WeightedSampleError("derived parameter vector must have one entry per sample")
        if range is not None:
            self.ranges.setRange(name, range)
        self.paramNames.names.append(par)
        self._edit_samples(append=append, chain_offsets=self.chain_offsets)
        return par

    # ---- text export (chains.py:1562-1581) -------------------------------------------------------------------
    def saveAsText(self, root, chain_index=None, make_dirs=False):
        """chains.py:1562-1573: the chain file, and the metadata files unless a chain index above 0 is given"""
        super().saveAsText(root, chain_index, make_dirs)
        if not chain_index:
            self.saveTextMetadata(root)

    def saveTextMetadata(self, root):
        """chains.py:1575-1581"""
        self.paramNames.saveAsText(root + ".paramnames")

    # ---- what GetDist's plotting layer asks a sample set for besides densities (plots.py:655-690,933-955,2262-2290) ------
    def getParamNames(self):
        """chains.py:1221-1225"""
        return self.paramNames

    def getRenames(self):
        return self.paramNames.getRenames()

    def updateRenames(self, renames):
        """chains.py:1258-1262"""
        self.paramNames.updateRenames(renames)

    def setParams(self, obj):
        """chains.py:1264-1289: give ``obj`` one attribute per parameter name holding its sample vector.  A dotted name
        aa.bb.cc becomes obj.aa.bb.cc through ParSamples sub-objects; a parameter aa whose name is also the head of a dotted
        one is reached as obj.aa.value.  Returns ``obj``."""
        return self._set_param_attrs(obj, lambda j, par: self.samples[:, j])

    def _set_param_attrs(self, obj, value_of):
        """The attribute layout of setParams with ``value_of(j, par)`` as the value of parameter j"""
        holders = []
        for par in self.paramNames.names:  # every sub-object first: whether a name holds one does not depend on the order
            *heads, leaf = par.name.split(".")
            holder = obj
            for head in heads:
                if not hasattr(holder, head):
                    setattr(holder, head, ParSamples())
                holder = getattr(holder, head)
            holders.append((holder, leaf))
        for j, (holder, leaf) in enumerate(holders):
            if isinstance(getattr(holder, leaf, None), ParSamples):
                getattr(holder, leaf).value = value_of(j, self.paramNames.names[j])
            else:
                setattr(holder, leaf, value_of(j, self.paramNames.names[j]))
        return obj

    def getParams(self):
        """chains.py:1291-1301: a ParSamples with one attribute per parameter name holding its sample vector"""
        return self.setParams(ParSamples())

    def getDeviceParams(self):
        """getParams() with a column-expression leaf (colexpr.col(name)) in place of every host vector, same attribute
        layout: arithmetic on the attributes builds expressions that mean / confidence / addDerived / ``where=`` evaluate
        on the device.  The leaves hold names, not data: they stay valid across mutators and for other sample sets with
        the same parameter names.  Not in the reference."""
        from .colexpr import col

        return self._set_param_attrs(ParSamples(), lambda j, par: col(par.name))

    # ---- the resident samples as device arrays (gd_export_device; not in the reference, which has no device) ---------------
    _EXPORT_ROWS = ("rows= takes None, a slice with step 1, a boolean mask with one entry per sample, a 1-D integer index array "
                    "(negative indices count from the end) or a boolean column expression")

    def _export_rows(self, rows):
        """``rows=`` of getDeviceSamples as (what Context.export_device selects by, the row count K or None where only the
        device will know it, the boolean expression to evaluate on the device or None)"""
        N = self.numrows
        if rows is None:
            return None, N, None
        if _is_expr(rows):
            if not rows.is_bool:
                raise ValueError("rows= takes a boolean expression (a comparison), not a float one")
            return None, None, rows
        if isinstance(rows, slice):
            lo, hi, step = rows.indices(N)
            if step != 1:
                raise ValueError("%s; not a slice with step %d" % (self._EXPORT_ROWS, step))
            return ("range", lo, max(hi, lo)), max(hi - lo, 0), None
        if isinstance(rows, (np.ndarray, list, tuple)):
            a = np.asarray(rows)
            if a.dtype == bool and a.shape == (N,):
                return ("mask", a), int(np.count_nonzero(a)), None
            if a.ndim == 1 and (a.dtype.kind in "iu" or a.size == 0):
                ix = _where_rows(a, N)  # (numpy's IndexError for an index outside [-N, N))
                return ("rows", ix), int(ix.size), None
        what = "%s array of shape %s" % (np.asarray(rows).dtype, np.shape(rows)) if isinstance(rows, (np.ndarray, list, tuple)) \
            else type(rows).__name__
        raise ValueError("%s; not a %s" % (self._EXPORT_ROWS, what))

    def _export(self, items, single, rows, dtype, order, out, stream):
        """getDeviceSamples / getDeviceWeights: ``items`` are resident column indices and column expressions (None: the sample
        weights).  Expressions go through the spare columns, a group of as many as there are free slots per export call,
        each group into its column sub-view of the destination."""
        from . import devarray

        ctx = self.ctx
        if not hasattr(ctx, "export_device"):
            raise NotImplementedError("%s has no export_device: the resident samples cannot be handed out as device arrays "
                                      "by this context" % type(ctx).__name__)
        if getattr(self, "_column_share", None) is not None:
            raise MCSamplesError("device arrays need every column resident on one device: this context holds only its rank's "
                                 "share of the columns")
        selection, K, mask_expr = self._export_rows(rows)
        m = 1 if items is None else len(items)
        exprs = [it for it in (items or []) if _is_expr(it)] + ([] if mask_expr is None else [mask_expr])
        slots = list(range(ctx.EXTRA_COLS - (1 if any(e.uses_loglikes() for e in exprs) else 0)))
        dest = None
        if out is None:
            code, stream = devarray.dtype_code(dtype), None  # (a result of the library's own is complete on return)
            if order not in ("C", "F"):
                raise ValueError("order must be 'C' or 'F'")
        else:
            dest = devarray.describe(out)
            if dest is None:
                raise TypeError("out= must be a device array: a torch tensor on the GPU or an object with "
                                "__cuda_array_interface__")
            if dest.ndim != (1 if single else 2) or (not single and dest.shape[1] != m):
                raise ValueError("out= must have shape %s, not %s" % ("(K,)" if single else "(K, %d)" % m, dest.shape))
            if any(s < 0 for s in dest.strides):
                raise ValueError("out= must be plain device memory with non-negative strides (strides %s)" % (dest.strides,))
            if K is not None and dest.shape[0] != K:
                raise ValueError("out= must have %d rows (the rows selected), not %d" % (K, dest.shape[0]))
            if stream is None:
                stream = dest.stream
        if stream is not None:  # (a handle or a torch stream object; handle 0 is the legacy default stream)
            stream = int(getattr(stream, "cuda_stream", stream)) or devarray.STREAM_LEGACY
        if mask_expr is not None:
            selection = ("nonzero", mask_expr.to_column(self, slots.pop(0)))  # 0.0 / 1.0 per row; never fetched
            K = ctx.export_device(rows=selection, cols=None if items is None else [0])  # a count: nothing is written
            if dest is not None and dest.shape[0] != K:
                raise ValueError("out= must have %d rows (the rows selected), not %d" % (K, dest.shape[0]))
        if dest is None:
            result = devarray.DeviceArray.allocate(ctx, (K,) if single else (K, m), code, order)
            dest = result.describe()
        else:
            result = out
        dest = dest.as2d()
        if K == 0 or m == 0:
            return result
        if items is None:
            ctx.export_device(rows=selection, cols=None, dest=dest, stream=stream)
            return result
        start = 0
        while start < m:
            free, cols, end = list(slots), [], start
            while end < m and not (_is_expr(items[end]) and not free):
                cols.append(items[end].to_column(self, free.pop(0)) if _is_expr(items[end]) else items[end])
                end += 1
            part = devarray.DevArray(dest.ptr + start * dest.strides[1] * dest.itemsize, (K, end - start), dest.strides, dest.dtype,
                                     dest.device, dest.stream, dest.owner)
            ctx.export_device(rows=selection, cols=cols, dest=part, stream=stream)
            start = end
        return result

    def getDeviceSamples(self, params=None, rows=None, dtype=np.float64, order="C", out=None, stream=None):
        """Rows of parameters (or of expressions of them) as an array in DEVICE memory, without crossing the host: what
        ``torch.as_tensor(samples.samples[rows][:, cols].astype(dtype)).cuda()`` gives, made on the device.  The result is a
        snapshot: the sample set may be mutated, re-uploaded or deleted afterwards.  Not in the reference.

        :param params: None (every parameter, in paramNames order) or a list of names, indices, ParamInfo objects and column
            expressions (getDeviceParams); a single item that is not in a list gives a 1-D result
        :param rows: None, a slice with step 1, a boolean mask, an integer index array with numpy's semantics, or a boolean
            column expression (evaluated on the device, never fetched)
        :param dtype: np.float64, np.float32, np.float16 or "bfloat16": rounded to nearest even in one step from the double
        :param order: "C" or "F", the layout of a result this call allocates
        :param out: a device array to write into instead (a torch tensor on the GPU, anything with
            ``__cuda_array_interface__``): shape (K, m), or (K,) for a single item; any non-negative strides; ITS element type
            decides the conversion.  Only its elements are written.
        :param stream: the stream that uses ``out`` (default: the one ``out`` announces); the copy is ordered behind that
            stream's earlier work and the stream behind the copy, by events.  Without ``out`` it is ignored: the call is
            complete on return.
        :return: ``out``, or a :class:`devarray.DeviceArray` that owns its memory (``.torch()``, ``.numpy()``,
            ``__cuda_array_interface__``)
        """
        single = params is not None and not isinstance(params, (list, tuple))
        wanted = list(range(self.n)) if params is None else [params] if single else list(params)
        items = []
        for par in wanted:
            if _is_expr(par):
                items.append(par)
            else:
                items.append(self._col(int(par) if isinstance(par, np.integer) else par))
        return self._export(items, single, rows, dtype, order, out, stream)

    def getDeviceWeights(self, rows=None, dtype=np.float64, out=None, stream=None):
        """The sample weights of the same rows as a 1-D device array (ones for a unit-weight set); arguments as
        :meth:`getDeviceSamples`."""
        return self._export(None, True, rows, dtype, "C", out, stream)

    def getParamSampleDict(self, ix, want_derived=True):
        """chains.py:1303-1317: {"weight", "loglike", parameter name: value} of sample row ``ix`` (the weight of a unit-weight
        set is 1.0; without loglikes this raises TypeError, as indexing None does in the reference)"""
        res = {"weight": 1.0 if self.weights is None else self.weights[ix], "loglike": self.loglikes[ix]}
        for j, par in enumerate(self.paramNames.names):
            if want_derived or not par.isDerived:
                res[par.name] = self.samples[ix, j]
        return res

    # ---- base statistics (chains.py:1340-1352) ---------------------------------------------------------------
    def _partial_moments(self, lo, hi):
        """One packed vector of the base statistics of rows [lo, hi): [norm, max_w, sum_w2, min(n), max(n), mean(n),
        cov(n x n)] -- what a rank contributes when the rows are split over ranks (three launches over its share)."""
        ws = self.ctx.weight_stats(lo, hi)
        means, cov, norm, mm = self.ctx.cov(list(range(self.n)), lo=lo, hi=hi, minmax=True)
        nrm = norm if self.weights is not None else float(hi - lo)
        return np.concatenate([[nrm, ws["max_w"], ws["sum_w2"]], mm[:, 0], mm[:, 1], means, cov.reshape(-1)])

    def _combine_moments(self, parts):
        """Pool per-share moments: means by weight, covariance as the weighted mean of the shares' covariances plus the
        spread of their means (the identity behind chains.py:1456-1466), minima / maxima / sums directly."""
        n = self.n
        parts = np.asarray(parts, dtype=np.float64)
        norms = parts[:, 0]
        norm = float(np.sum(norms))
        means = norms @ parts[:, 3 + 2 * n:3 + 3 * n] / norm
        cov = np.zeros((n, n))
        for p in parts:
            d = p[3 + 2 * n:3 + 3 * n] - means
            cov += p[0] * (p[3 + 3 * n:].reshape(n, n) + np.outer(d, d))
        cov /= norm
        return dict(norm=norm, max_w=float(np.max(parts[:, 1])), sum_w2=float(np.sum(parts[:, 2])),
                    col_min=np.min(parts[:, 3:3 + n], axis=0), col_max=np.max(parts[:, 3 + n:3 + 2 * n], axis=0),
                    means=means, cov=cov)

    def updateBaseStatistics(self, row_share=None, exchange=None):
        """
        chains.py:1340-1352 + mcsamples.py:552-576, with the column scans on the GPU.

        Multi-GPU (samples replicated): ``row_share=(rank, world)`` makes this process reduce only its
        contiguous share of the rows; ``exchange(vector) -> (world, len)`` (an all-gather of n^2 + 3n + 3 doubles over
        RCCL) pools the shares, so the O(N n^2) covariance pass costs 1/world per rank instead of being repeated.
        """
        if row_share is not None:
            rank, world = row_share
            per = (self.numrows + world - 1) // world
            lo, hi = min(rank * per, self.numrows), min((rank + 1) * per, self.numrows)
            if hi > lo:
                mine = self._partial_moments(lo, hi)
            else:
                # a rank without rows (N < world, or the last rank after the ceiling division) still contributes a
                # vector of the full length, so the all-gather's shapes agree: zero norm, +inf / -inf extrema
                n = self.n
                mine = np.zeros(3 + 3 * n + n * n)
                mine[3:3 + n], mine[3 + n:3 + 2 * n] = np.inf, -np.inf
            parts = exchange(mine)
            pooled = self._combine_moments([p for p in parts if p is not None and p[0] > 0])
            self.norm = np.float64(pooled["norm"]) if self.weights is not None else np.float64(self.numrows)
            self._col_min, self._col_max = pooled["col_min"], pooled["col_max"]
            self.means = pooled["means"]
            self.fullcov = pooled["cov"]
            self.vars = np.diag(self.fullcov).copy()
            self.sddev = np.sqrt(self.vars)
            self.mean_mult = self.norm / self.numrows
            self.max_mult = pooled["max_w"]
            self._sum_w2 = pooled["sum_w2"]
            if self.weights is not None:  # mcsamples.py:559-562, from the pooled sums (each rank counts its own rows)
                mult_max = (self.mean_mult * self.numrows) / min(self.numrows // 2, 500)
                if self.max_mult > mult_max:
                    outliers = self.ctx.weight_stats(thresh=mult_max)["n_above"]
                    if outliers != 0:
                        logging.warning("outlier fraction %s ", float(outliers) / self.numrows)
            self.correlationMatrix = None
            self._after_base_statistics()
            return self
        ws = self.ctx.weight_stats()
        if self.weights is not None:
            self.norm = ws["norm"]
        else:
            self.norm = np.float64(self.numrows)  # chains.py:315
        # one statistics pass (min, max, weighted mean) + one covariance pass; the variances are its diagonal
        # (chains.py:409-410 and :729 are the same sum)
        means, cov, _, mm = self.ctx.cov(list(range(self.n)), minmax=True)
        self._col_min, self._col_max = mm[:, 0].copy(), mm[:, 1].copy()
        self.means = means
        self.vars = np.diag(cov).copy()
        self.sddev = np.sqrt(self.vars)
        self.mean_mult = self.norm / self.numrows
        self.max_mult = ws["max_w"]
        self._sum_w2 = ws["sum_w2"]
        mult_max = (self.mean_mult * self.numrows) / min(self.numrows // 2, 500)
        if self.weights is not None:
            outliers = self.ctx.weight_stats(thresh=mult_max)["n_above"]
            if outliers != 0:
                logging.warning("outlier fraction %s ", float(outliers) / self.numrows)
        self.fullcov = cov
        self.correlationMatrix = None
        self._after_base_statistics()
        return self

    # ---- convergence (chains.py:1446-1527; mcsamples.py:964-1003) ------------------------------------------
    def getSeparateChainStats(self, nparam=None):
        """Per-chain (means, cov, norm) over the first nparam parameters: one covariance launch per chain over ALL
        columns, cached until the samples change, so Gelman-Rubin, MeanVar, CorrLengths and CorrSteps share one pass."""
        if self.chain_offsets is None:
            raise WeightedSampleError("Samples were not combined from separate chains")
        nparam = nparam or self.paramNames.numNonDerived()
        if "all" not in self._chain_stats_cache:
            cols = list(range(self.n))
            self._chain_stats_cache["all"] = [self.ctx.cov(cols, lo=int(a), hi=int(b))
                                              for a, b in zip(self.chain_offsets[:-1], self.chain_offsets[1:])]
        return [(m[:nparam], c[:nparam, :nparam], nrm) for m, c, nrm in self._chain_stats_cache["all"]]

    def getSeparateChains(self):
        """
        chains.py:1505-1527: one object per chain.  The reference slices the host arrays into WeightedSamples; here each
        is a ChainView -- a row range [lo, hi) of the resident device columns with the WeightedSamples statistics API
        (getMeans / getVars / getCov / mean / var / std / cov / corr / confidence / twoTailLimits / norm), no copy.
        """
        if self.chain_offsets is None:
            raise WeightedSampleError("Samples were not combined from separate chains")
        return [ChainView(self, int(a), int(b)) for a, b in zip(self.chain_offsets[:-1], self.chain_offsets[1:])]

    def makeSingle(self):
        """chains.py:1488-1503.  The constructor already stacks a list of chains into one resident array (recording
        chain_offsets), after which the reference's ``chains`` attribute is None and this call raises there too."""
        if not self.chains:
            raise ValueError("There are no separated chains for makeSingle()")
        return self

    def getGelmanRubinEigenvalues(self, nparam=None, chainlist=None):
        """chains.py:1446-1474: var(mean)/mean(var) in the orthogonalised parameters; ``chainlist`` may be any
        sub-list of getSeparateChains() (or objects with getMeans() / getCov(nparam))."""
        from .parallel import gelman_rubin_from_chain_stats

        nparam = nparam or self.paramNames.numNonDerived()
        if chainlist is None:
            stats = self.getSeparateChainStats(nparam)
        else:
            stats = [(np.asarray(ch.getMeans())[:nparam], np.asarray(ch.getCov(nparam)), None) for ch in chainlist]
        return gelman_rubin_from_chain_stats(stats, self.getMeans())

    def getGelmanRubin(self, nparam=None, chainlist=None):
        return np.max(self.getGelmanRubinEigenvalues(nparam, chainlist))

    def getMeanVarTest(self, nparam=None):
        """The MeanVar block of getConvergeTests (mcsamples.py:964-985): sqrt(var(chain mean)/mean(chain var))."""
        nparam = nparam or self.n
        stats = self.getSeparateChainStats(nparam)
        between = np.zeros(nparam)
        within = np.zeros(nparam)
        for cmeans, ccov, cnorm in stats:
            between += (cmeans - self.means[:nparam]) ** 2
            within += np.diag(ccov) * cnorm
        between /= len(stats) - 1
        within /= self.norm
        return np.sqrt(between / within)

    # ---- the numbers behind the blocks of MCSamples.getConvergeTests (mcsamples.py:941-1210) -----------------
    def getCorrLengths(self, min_corr=0.05):
        """
        The numbers of the CorrLengths block of getConvergeTests (mcsamples.py:941-962): per parameter, the weight-unit
        autocorrelation length from the chain-averaged autocovariance (each chain about its own mean), summed up to the
        first lag at or below 5 %.  Lag sums per chain run on the GPU in 32-lag chunks with early exit.
        """
        if self.chain_offsets is None:
            raise WeightedSampleError("Samples were not combined from separate chains")
        if self.needs_update:
            self.updateBaseStatistics()
        ranges = list(zip(self.chain_offsets[:-1], self.chain_offsets[1:]))
        stats = self.getSeparateChainStats(self.n)
        maxoff = int(min((b - a) // 10 for a, b in ranges))
        cols = list(range(self.n))
        corr_rows = [[] for _ in cols]
        result = [None] * self.n
        k0 = 0
        while k0 <= maxoff and any(r is None for r in result):
            nl = min(32, maxoff + 1 - k0)
            chunk = np.zeros((self.n, nl))
            for (a, b), (cmeans, _, _) in zip(ranges, stats):
                nc = int(b - a)
                lags = self.ctx.autocov_lags_range_batch(cols, cmeans, int(a), int(b), k0, nl)
                chunk += lags / (nc - np.arange(k0, k0 + nl)) * nc  # normalize=True, weight_units, times chain.norm
            chunk /= (self.norm * self.vars)[:, None]
            for j in cols:
                if result[j] is not None:
                    continue
                corr_rows[j].extend(chunk[j].tolist())
                c = np.array(corr_rows[j])
                below = np.nonzero(~(c > min_corr * c[0]))[0]
                if below.size:
                    result[j] = c[0] + 2 * float(np.sum(c[1:int(below[0])]))
            k0 += nl
        for j in cols:
            if result[j] is None:
                result[j] = corr_rows[j][0]  # argmin of an all-True mask is 0
        self.indep_thin = max(result)
        return np.array(result)

    def getSplitTests(self, test_confidence=0.95, max_split_tests=4):
        """
        The numbers of the SplitTest block of getConvergeTests (mcsamples.py:1005-1034): for n = 2..max_split_tests
        splits of the rows, rms over the splits of the change in the upper / lower quantile, in units of the standard
        deviation.  Returns an array (nparam, max_split_tests-1, 2) ordered [upper, lower] like the reference's table.
        Every (row range) needs one batched quantile-select launch over all parameters.
        """
        if self.needs_update:
            self.updateBaseStatistics()
        limits = np.array([1 - (1 - test_confidence) / 2, (1 - test_confidence) / 2])
        cols = list(range(self.n))

        def conf(lo, hi):
            norm = self.norm if (lo == 0 and hi == self.numrows) else self.ctx.weight_stats(int(lo), int(hi))["norm"]
            return self.ctx.quantiles(cols, np.tile(norm * limits, (self.n, 1)), lo=int(lo), hi=int(hi))

        confids = conf(0, self.numrows)
        out = np.zeros((self.n, max_split_tests - 1, 2))
        for ix in range(max_split_tests - 1):
            split_n = 2 + ix
            frac = self.getFractionIndices(self.weights, split_n)
            for f1, f2 in zip(frac[:-1], frac[1:]):
                out[:, ix, :] += (conf(f1, f2) - confids) ** 2
            out[:, ix, :] = np.sqrt(out[:, ix, :] / split_n) / self.sddev[:, None]
        return out

    def getRafteryLewis(self, test_confidence=0.95, nparam=None):
        """
        The Raftery-Lewis block of getConvergeTests (mcsamples.py:1039-1165): per chain the thinning needed for the
        thinned binary chains (parameter above/below a tail quantile) to be first-order Markov, then independent, and
        the burn-in estimate.  Returns dict(markov_thin, thin_fac, nburn) (arrays over chains; thin_fac = indep_thin,
        0 = failed) or None where the reference gives up.  The quantiles, the thinning and the transition counts of
        every (parameter, tail) at the current thin factor come from the GPU in one launch each; only the BIC logic
        on 8 / 4 integers runs here.
        """
        import math

        if not self.ctx.weights_integral():
            raise WeightedSampleError("Raftery-Lewis needs integer weights")
        ctx = self.ctx
        ranges = self._chain_ranges()
        nparamMC = nparam or self.paramNames.numNonDerived()
        cols = list(range(nparamMC))
        limits = np.array([1 - (1 - test_confidence) / 2, (1 - test_confidence) / 2])
        nc = len(ranges)
        thin_fac = np.zeros(nc, dtype=int)
        nburn = np.zeros(nc, dtype=int)
        markov_thin = np.zeros(nc, dtype=int)
        epsilon = 0.001
        hardest, hardestend = -1, 0  # carried over from chain to chain, as in the reference

        class Failed(Exception):
            pass

        for ix, (lo, hi) in enumerate(ranges):
            ws = ctx.weight_stats(lo, hi)
            thin_fac[ix] = int(round(ws["max_w"]))
            targets = np.tile(ws["norm"] * limits, (nparamMC, 1))
            confids = ctx.quantiles(cols, targets, lo=lo, hi=hi)  # (param, upper/lower)
            cache = {}

            def counts(f, columns=cols, thr=confids, key="all"):
                """(thin_rows, transition counts of every column/threshold) at thin factor f, cached per factor."""
                if (key, f) not in cache:
                    rows, K = self._thin_rows(f, lo, hi)
                    cache[(key, f)] = (K, ctx.binary_transitions(columns, rows, K, thr) if K >= 2 else None)
                    rows.free()
                return cache[(key, f)]

            thin_rows = None
            try:
                for j in range(nparamMC):
                    for endb in (0, 1):
                        tran = None
                        while True:
                            thin_rows, c = counts(int(thin_fac[ix]))
                            if thin_rows < 2:
                                break
                            tran = c[j, endb, :8].reshape(2, 2, 2)
                            g2 = _g2_markov_vs_second_order(tran)
                            if g2 - math.log(float(thin_rows - 2)) * 2 < 0:
                                break
                            thin_fac[ix] += 1
                        if tran is None:
                            raise ValueError("not enough thinned samples")  # the reference's NameError -> bare except
                        if np.sum(tran[:, 0, 1]) == 0 or np.sum(tran[:, 1, 0]) == 0:
                            thin_fac[ix] = 0
                            raise Failed()
                        alpha = np.sum(tran[:, 0, 1]) / float(np.sum(tran[:, 0, 0]) + np.sum(tran[:, 0, 1]))
                        beta = np.sum(tran[:, 1, 0]) / float(np.sum(tran[:, 1, 0]) + np.sum(tran[:, 1, 1]))
                        probsum = alpha + beta
                        tmp1 = math.log(probsum * epsilon / max(alpha, beta)) / math.log(abs(1.0 - probsum))
                        if int(tmp1 + 1) * thin_fac[ix] > nburn[ix]:
                            nburn[ix] = int(tmp1 + 1) * thin_fac[ix]
                            hardest, hardestend = j, endb
                markov_thin[ix] = thin_fac[ix]
                hardest = max(hardest, 0)
                u = self.confidence(hardest, (1 - test_confidence) / 2, hardestend == 0)  # over ALL samples (:1113)
                while True:
                    thin_rows, c = counts(int(thin_fac[ix]), [hardest], [[u]], key=("indep", hardest, hardestend))
                    if thin_rows < 2:
                        break
                    tran2 = c[0, 0, 8:].reshape(2, 2)
                    g2 = _g2_independence_vs_markov(tran2, thin_rows)
                    if g2 is None:
                        return None
                    if g2 - np.log(float(thin_rows - 1)) < 0:
                        break
                    thin_fac[ix] += 1
            except Failed:
                pass
            except (ValueError, ZeroDivisionError, OverflowError, FloatingPointError):
                thin_fac[ix] = 0  # the arithmetic failures the reference's bare `except:` swallows (:1146-1147)
            if thin_fac[ix] and thin_rows is not None and thin_rows < 2:
                thin_fac[ix] = 0
        self.RL_indep_thin = np.max(thin_fac)
        return dict(markov_thin=markov_thin, thin_fac=thin_fac, nburn=nburn)

    def getCorrSteps(self):
        """
        The CorrSteps block (mcsamples.py:1183-1210): auto-correlation of every parameter in the thinned chains
        (each about its own mean) at step separations 1..maxoff thinned rows.  Returns (autocorr_thin, corrs[maxoff, n])
        or (autocorr_thin, None).  Thinning and the gathered lag sums run on the GPU.
        """
        if self.needs_update:
            self.updateBaseStatistics()
        ranges = self._chain_ranges()
        if self.corr_length_thin != 0:
            autocorr_thin = self.corr_length_thin
        else:
            indep_thin = getattr(self, "indep_thin", 0)
            if indep_thin == 0:
                autocorr_thin = 20
            elif indep_thin <= 30:
                autocorr_thin = 5
            else:
                autocorr_thin = int(5 * (indep_thin / 30))
        rows, K = self._thin_rows(autocorr_thin)
        rows.free()
        maxoff = int(min(self.corr_length_steps, K // (2 * len(ranges))))
        if maxoff <= 0:
            return autocorr_thin, None
        cols = list(range(self.n))
        corrs = np.zeros((maxoff, self.n))
        for (lo, hi), (cmeans, _, _) in zip(ranges, self.getSeparateChainStats(self.n)):
            rows, K = self._thin_rows(autocorr_thin, lo, hi)
            maxoff = min(maxoff, K // autocorr_thin)
            if maxoff > 0:
                lags = self.ctx.thinned_lag_sums(cols, cmeans, rows, K, maxoff)  # (n, maxoff)
                corrs[:maxoff] += (lags / (K - np.arange(1, maxoff + 1))).T / self.vars
            rows.free()
        corrs /= len(ranges)
        return autocorr_thin, corrs[:maxoff]


class ChainView:
    """
    One chain of a combined sample set: rows [lo, hi) of the parent's device-resident columns, with the statistics
    interface of chains.WeightedSamples (chains.py:339-412, 636-838) evaluated on that row range by the same kernels
    (every entry point of the C ABI takes a row range).  ``samples`` / ``weights`` / ``loglikes`` are host views.
    """

    def __init__(self, parent, lo, hi):
        self.parent, self.lo, self.hi = parent, lo, hi
        self.numrows = hi - lo
        self.n = parent.n
        self.paramNames = parent.paramNames
        self._stats = self._cov = self._ws = None

    samples = property(lambda self: self.parent.samples[self.lo:self.hi])
    weights = property(lambda self: (np.ones(self.numrows) if self.parent.weights is None
                                     else self.parent.weights[self.lo:self.hi]))
    loglikes = property(lambda self: None if self.parent.loglikes is None else self.parent.loglikes[self.lo:self.hi])

    precision = "%.8e"  # a separate chain is a plain WeightedSamples in the reference: the class default (chains.py:227)

    def saveAsText(self, root, chain_index=None, make_dirs=False, _sources=None):
        """chains.py:1063-1085 over this chain's rows of the resident set: no copy of the chain, no metadata files"""
        self.parent._save_rows_as_text(root, chain_index, make_dirs, self.lo, self.hi, self.precision, _sources)

    def _weight_stats(self):
        if self._ws is None:
            self._ws = self.parent.ctx.weight_stats(self.lo, self.hi)
        return self._ws

    @property
    def norm(self):
        return self._weight_stats()["norm"] if self.parent.weights is not None else np.float64(self.numrows)

    def _where_global(self, where):
        """A chain-relative ``where`` (boolean mask or row indices of THIS chain) as full-length weights*mask of the
        parent: the kernels then see x[where], w[where] of the chain inside its row range."""
        where = np.asarray(where)
        p = self.parent
        w = np.zeros(p.numrows)
        base = p.weights[self.lo:self.hi] if p.weights is not None else np.ones(self.numrows)
        if where.dtype == bool:
            if where.shape != (self.numrows,):
                raise WeightedSampleError("where must have one entry per sample of the chain")
            w[self.lo:self.hi] = base * where
        else:
            w[self.lo:self.hi] = base * np.bincount(_where_rows(where, self.numrows), minlength=self.numrows)
        return w

    def _moments(self, pars, where):
        p = self.parent
        cols = [p._col(q) for q in pars]
        return p._with_weights(self._where_global(where), lambda: p.ctx.cov(cols, lo=self.lo, hi=self.hi))

    def get_norm(self, where=None):
        if where is not None:
            p = self.parent
            return p._with_weights(self._where_global(where), lambda: p.ctx.weight_stats(self.lo, self.hi)["norm"])
        return self.norm

    def _col_stats(self):
        if self._stats is None:
            self._stats = self.parent.ctx.col_stats(self.lo, self.hi)
        return self._stats

    def getMeans(self, pars=None):
        means = self._col_stats()[:, 2]
        return means.copy() if pars is None else np.array([means[self.parent._col(p)] for p in pars])

    def getVars(self):
        return self._col_stats()[:, 3].copy()

    def getCov(self, nparam=None, pars=None):
        if self._cov is None:
            self._cov = self.parent.ctx.cov(list(range(self.n)), lo=self.lo, hi=self.hi)[1]
        if pars is not None:
            return self._cov[np.ix_(pars, pars)]
        return self._cov[:nparam, :nparam]

    def getCorrelationMatrix(self):
        return covToCorr(self.getCov())

    def cov(self, pars=None, where=None):
        if isinstance(pars, (int, np.integer)):
            pars = range(pars)
        cols = list(range(self.n)) if pars is None else [self.parent._col(p) for p in pars]
        if where is not None:
            return self._moments(cols, where)[1]
        return self.parent.ctx.cov(cols, lo=self.lo, hi=self.hi)[1]

    def corr(self, pars=None):
        return covToCorr(self.cov(pars))

    def mean(self, paramVec, where=None):
        if isinstance(paramVec, (list, tuple)):
            return np.array([self.mean(p, where) for p in paramVec])
        if where is not None:
            return self._moments([paramVec], where)[0][0]
        return self._col_stats()[self.parent._col(paramVec), 2]

    def var(self, paramVec, where=None):
        if isinstance(paramVec, (list, tuple)):
            return np.array([self.var(p) for p in paramVec])  # like the reference, a list ignores ``where``
        if where is not None:
            return self._moments([paramVec], where)[1][0, 0]
        return self._col_stats()[self.parent._col(paramVec), 3]

    def std(self, paramVec, where=None):
        return np.sqrt(self.var(paramVec, where))

    def confidence(self, paramVec, limfrac, upper=False):
        return self.parent.confidence(paramVec, limfrac, upper, start=self.lo, end=self.hi)

    def twoTailLimits(self, paramVec, confidence):
        limits = np.array([(1 - confidence) / 2, 1 - (1 - confidence) / 2])
        return self.confidence(paramVec, limits)

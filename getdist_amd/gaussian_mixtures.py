"""
Gaussian mixture models with optional hard parameter limits: the surface of getdist/gaussian_mixtures.py
(``MixtureND``, ``Mixture2D``, ``Gaussian2D``, ``GaussianND``, ``Mixture1D``, ``Gaussian1D``, ``RandomTestMixtureND``,
``randomTestMCSamples``, ``make_2D_Cov``).

Use them to draw test sample sets with a known density (``mix.MCSamples(size, logLikes=True)``), to overlay an analytic
forecast on a triangle plot (``density1D`` / ``density2D``), to marginalise or condition a Gaussian model, and to
re-weight a chain by a Gaussian prior or likelihood (``samples.reweightAddingLogLikes(prior.logLikes(samples))``).

Where the work happens: sampling (``sim``) and the densities on caller-supplied points or grids are host numpy, as in the
reference -- ``sim`` consumes the numpy Generator in the reference's order, so a seed gives the same rows.  The one O(N)
evaluation, the mixture's -log pdf at every row of a device-resident sample set, runs in the library (gd_mixture_nll):
``MixtureND.logLikes`` (an extension, not in the reference) and ``MCSamples(..., logLikes=True)``.  Importing this module
does not load the native library.
"""

import numpy as np

from .densities import Density1D, Density2D
from .paramnames import ParamNames


def make_2D_Cov(sigmax, sigmay, corr):
    """The 2 x 2 covariance of two standard deviations and their correlation coefficient."""
    off = sigmax * sigmay * corr
    return np.array([[sigmax ** 2, off], [off, sigmay ** 2]])


def _param_names(names, dim, labels):
    """names param1.. / labels p_{1}.. when no names are given (paramnames.py:186-188); ``labels`` override"""
    if names is None:
        pn = ParamNames(["param%d" % (i + 1) for i in range(dim)], ["p_{%d}" % (i + 1) for i in range(dim)])
    else:
        pn = ParamNames(list(names))
    if labels is not None:
        for par, lab in zip(pn.names, labels):
            par.label = lab
    return pn


def _inherit_labels(pn, parent):
    """labels and derived flags of the parent's parameters of the same name (setLabelsAndDerivedFromParamNames)"""
    for src in parent.names:
        par = pn.parWithName(src.name)
        if par is not None:
            par.label = src.label
            par.isDerived = src.isDerived


class MixtureND:
    """
    A Gaussian mixture in ``dim`` dimensions, optionally cut off at hard limits.  An instance can stand in for a sample set
    where smooth theoretical contours are wanted (Fisher forecasts): it offers ``density1D`` / ``density2D`` and the names.
    ``GaussianND`` is the one-component special case.
    """

    def __init__(self, means, covs, weights=None, lims=None, names=None, label="", labels=None):
        """
        :param means: one mean vector per component
        :param covs: one covariance matrix per component
        :param weights: relative weight of each component (default: equal); normalised to sum to one
        :param lims: hard limits per parameter, [[x1min, x1max], [x2min, x2max], ...], None for an open side
        :param names: parameter names (default param1, param2, ...)
        :param label: a label for the mixture
        :param labels: latex labels of the parameters (default p_{1}, p_{2}, ... when no names are given)
        """
        self.means = np.asarray(means)
        self.dim = self.means.shape[1]
        self.covs = [np.array(c) for c in covs]
        self.invcovs = [np.linalg.inv(c) for c in self.covs]
        ncomp = len(means)
        if weights is None:
            weights = [1.0 / ncomp] * ncomp
        self.weights = np.array(weights, dtype=np.float64)
        if np.sum(self.weights) <= 0:
            raise ValueError("Weight <= 0 in MixtureND")
        self.weights /= np.sum(weights)
        self.norms = (2 * np.pi) ** (0.5 * self.dim) * np.array([np.sqrt(np.linalg.det(c)) for c in self.covs])
        self.lims = lims
        self.paramNames = _param_names(names, self.dim, labels)
        self.names = self.paramNames.list()
        self.label = label
        self.total_mean = np.atleast_1d(np.dot(self.weights, self.means))
        self.total_cov = np.zeros((self.dim, self.dim))
        # (the reference zips the components with the ENTRIES of total_mean, so component k is offset by total_mean[k] in
        #  every direction and components beyond dim are dropped; kept, since total_cov is compared with it)
        for mean, cov, weight, tm in zip(self.means, self.covs, self.weights, self.total_mean):
            self.total_cov += weight * (cov + np.outer(mean - tm, mean - tm))

    # ---- sampling ----------------------------------------------------------------------------------------------
    def sim(self, size, random_state=None):
        """
        ``size`` independent samples as a (size, dim) array.  ``random_state`` is a numpy Generator or a seed.  The
        Generator is consumed exactly as in the reference (a multinomial over the components, one multivariate_normal per
        populated component, rejection at the limits, further blocks while rows are missing, one permutation when more
        than one batch was drawn, surplus rows cut from the end), so a seed reproduces the reference's rows.
        """
        rng = np.random.default_rng(random_state)
        batches, have, block = [], 0, None
        while True:
            per_component = rng.multinomial(block or size, self.weights)
            for count, mean, cov in zip(per_component, self.means, self.covs):
                if count <= 0:
                    continue
                rows = rng.multivariate_normal(mean, cov, size=count)
                if self.lims is not None:
                    for i, (lower, upper) in enumerate(self.lims):
                        if lower is not None:
                            rows = rows[rows[:, i] >= lower]
                        if upper is not None:
                            rows = rows[rows[:, i] <= upper]
                have += rows.shape[0]
                batches.append(rows)
            if have >= size:
                break
            if block is None:  # the size of every further draw is fixed by the first shortfall
                block = min(max(size, 100000), int(1.1 * (size * (size - have))) // max(have, 1) + 1)
        samples = np.vstack(batches)
        if len(batches) > 1:
            samples = rng.permutation(samples)
        if have != size:
            samples = samples[:size - have, :]
        return samples

    def MCSamples(self, size, names=None, logLikes=False, random_state=None, **kwargs):
        """
        ``size`` independent samples as a :class:`getdist_amd.MCSamples` (ranges = the mixture's limits, names and labels
        from ``paramNames`` unless ``names`` / ``labels`` override them; other keywords, e.g. ``device`` or ``settings``,
        go to the MCSamples constructor).  With ``logLikes`` the -log(pdf) of every sample is stored as its loglike,
        evaluated on the device over the uploaded columns (gd_mixture_nll): finite also where the pdf underflows.
        """
        from .mcsamples import MCSamples

        if logLikes:
            self._whitened()  # (a covariance that is not positive definite fails here, before anything is drawn or uploaded)
        samples = self.sim(size, random_state=random_state)
        own = self.paramNames
        names = list(names) if names is not None else own.list()
        labels = kwargs.pop("labels", None) or own.labels()
        ranges = None
        if self.lims is not None:
            ranges = {nm: tuple(lim) for nm, lim in zip(names, self.lims)}
        mc = MCSamples(samples=samples, names=names, labels=labels, ranges=ranges, **kwargs)
        if logLikes:
            # the constructor keeps every column unless one never moves (a zero-variance direction): evaluate by name
            mc.loglikes = self.logLikes(mc, params=names)
            mc.likeStats = None
        return mc

    # ---- device log-pdf (an extension: not in the reference) --------------------------------------------------------
    def _whitened(self):
        """(whiten, logcoef): per component the inverse W = L^-1 of the Cholesky factor of its covariance (cov = L L^T,
        W lower-triangular, chi^2 = |W (x - mean)|^2) and log(weight) - log(norm) with log(norm) taken from the factor's
        diagonal.  ValueError for a covariance that is not positive definite."""
        from scipy.linalg import solve_triangular

        d = self.dim
        whiten = np.zeros((len(self.covs), d, d))
        logcoef = np.zeros(len(self.covs))
        for k, cov in enumerate(self.covs):
            cov = np.asarray(cov, dtype=np.float64)
            try:
                if not np.all(np.isfinite(cov)) or not np.allclose(cov, cov.T, rtol=1e-8, atol=0):
                    raise np.linalg.LinAlgError("not symmetric")
                L = np.linalg.cholesky(cov)
            except np.linalg.LinAlgError:
                raise ValueError("covariance of mixture component %d is not positive definite" % k) from None
            whiten[k] = np.tril(solve_triangular(L, np.eye(d), lower=True))
            with np.errstate(divide="ignore"):
                logcoef[k] = np.log(self.weights[k]) - (0.5 * d * np.log(2 * np.pi) + np.sum(np.log(np.diag(L))))
        return whiten, logcoef

    def logLikes(self, samples, params=None):
        """
        -log(pdf) of this mixture at every row of ``samples``, a device-resident :class:`getdist_amd.MCSamples`; a host
        float64 vector with one entry per row.  ``params`` (names or column indices, default: this mixture's names looked
        up in the sample set) selects the ``dim`` columns.  Not in the reference, which offers ``-log(mix.pdf(rows))``
        on host rows only; here nothing of size N x dim is formed and the result stays finite far out in the tails.
        Intended use: ``samples.reweightAddingLogLikes(prior.logLikes(samples))`` -- on ``samples.copy()`` to keep the
        original set as well.
        """
        from .chains import MCSamplesError

        if getattr(samples, "_column_share", None) is not None:
            raise MCSamplesError("logLikes needs every column resident on one device: this context holds only its rank's "
                                 "share of the columns (multi-GPU logLikes is not supported)")
        if params is None:
            params = self.names
        if len(params) != self.dim:
            raise ValueError("logLikes needs %d parameters, got %d" % (self.dim, len(params)))
        cols = []
        for p in params:
            name = p if isinstance(p, str) else getattr(p, "name", None)
            if name is not None:
                if name not in samples.index:
                    raise MCSamplesError("parameter %s is not in the sample set" % name)
                cols.append(samples.index[name])
            else:
                j = int(p)
                if not 0 <= j < samples.n:
                    raise MCSamplesError("column index %d is not in the sample set" % j)
                cols.append(j)
        whiten, logcoef = self._whitened()  # (raises before anything is launched)
        nll = samples.ctx.mixture_nll(cols, np.asarray(self.means, dtype=np.float64), whiten, logcoef)
        return np.array(nll, dtype=np.float64)  # an owned copy: the context recycles its page-locked block

    # ---- ranges ------------------------------------------------------------------------------------------------------
    def autoRanges(self, sigma_max=4, lims=None):
        """Per parameter (lower, upper): the hard limit where there is one, else the outermost ``mean -+ sigma_max sigma`` of
        the components (moved, for a one-sided limit, so that ``sigma_max`` sigma beyond the limit are covered)."""
        if lims is None:
            lims = self.lims
        if lims is None:
            lims = [(None, None)] * self.dim
        out = []
        for i, (lower, upper) in enumerate(lims):
            lo = hi = None
            if lower is None or upper is None:
                for mean, cov in zip(self.means, self.covs):
                    reach = sigma_max * np.sqrt(cov[i, i])
                    a, b = mean[i] - reach, mean[i] + reach
                    if lower is not None:
                        b = max(b, lower + reach)
                    if upper is not None:
                        a = min(a, upper - reach)
                    lo = a if lo is None else min(a, lo)
                    hi = b if hi is None else max(b, hi)
            out.append((lo if lower is None else lower, hi if upper is None else upper))
        return out

    # ---- densities on host points ---------------------------------------------------------------------------------
    def pdf(self, x):
        """The density at ``x`` (one point, or an array of points by row).  Limits are not applied: the value is not set
        to zero outside them and is normalised only for a mixture without limits."""
        x = np.asarray(x)
        total = None
        for mean, icov, weight, norm in zip(self.means, self.invcovs, self.weights, self.norms):
            dx = x - mean
            chi2 = icov.dot(dx).dot(dx) if x.ndim == 1 else np.einsum("ik,km,im->i", dx, icov, dx)
            part = np.exp(-chi2 / 2) / norm * weight
            total = part if total is None else total + part
        return total

    def pdf_marged(self, index, x, no_limit_marge=False):
        """The 1D marginalised density of parameter ``index`` (a number or a name) at ``x``.  Analytic, so it needs the other
        parameters to be unlimited unless ``no_limit_marge``."""
        if isinstance(index, str):
            index = self.names.index(index)
        if not no_limit_marge:
            self.checkNoLimits([index])
        total = None
        for mean, cov, weight in zip(self.means, self.covs, self.weights):
            var = cov[index, index]
            dx = x - mean[index]
            part = np.exp(-(dx ** 2) / var / 2) / np.sqrt(2 * np.pi * var) * weight
            total = part if total is None else total + part
        return total

    def density1D(self, index=0, num_points=1024, sigma_max=4, no_limit_marge=False):
        """The 1D marginalised density of a parameter on ``num_points`` grid points over autoRanges(sigma_max), as a
        :class:`getdist_amd.Density1D`."""
        if isinstance(index, str):
            index = self.names.index(index)
        if not no_limit_marge:
            self.checkNoLimits([index])
        lower, upper = self.autoRanges(sigma_max)[index]
        x = np.linspace(lower, upper, num_points)
        return Density1D(x, self.pdf_marged(index, x))

    def density2D(self, params=None, num_points=1024, xmin=None, xmax=None, ymin=None, ymax=None, sigma_max=5):
        """The 2D marginalised density of a pair of parameters (names or indices; None for a 2D mixture) on a
        ``num_points`` x ``num_points`` grid, as a :class:`getdist_amd.Density2D`.  ``xmin`` .. ``ymax`` override the
        grid's bounds."""
        if self.dim > 2 or params is not None or not isinstance(self, Mixture2D):
            target = self.marginalizedMixture(params=params)
        elif self.dim != 2:
            raise Exception("density2D requires at least two dimensions")
        else:
            target = self
        return target._density2D(num_points=num_points, xmin=xmin, xmax=xmax, ymin=ymin, ymax=ymax, sigma_max=sigma_max)

    # ---- derived mixtures ------------------------------------------------------------------------------------------------
    def _params_to_indices(self, params):
        if params is None:
            params = self.names
        out = []
        for p in params:
            if isinstance(p, str):
                out.append(self.names.index(p))
            elif hasattr(p, "name"):
                out.append(self.names.index(p.name))
            else:
                out.append(p)
        return out

    def marginalizedMixture(self, params, label=None, no_limit_marge=False):
        """The mixture of the parameters ``params`` (names or indices; None: all) with the others integrated out: a
        :class:`Mixture2D` for two parameters, else a :class:`MixtureND`."""
        keep = self._params_to_indices(params)
        if not no_limit_marge:
            self.checkNoLimits(keep)
        keep = np.array(keep)
        names = [self.names[i] for i in keep] if self.names is not None else None
        lims = [self.lims[i] for i in keep] if self.lims is not None else None
        cls = Mixture2D if len(keep) == 2 else MixtureND
        out = cls([m[keep] for m in self.means], [c[np.ix_(keep, keep)] for c in self.covs], self.weights, lims=lims,
                  names=names, label=self.label if label is None else label)
        _inherit_labels(out.paramNames, self.paramNames)
        return out

    def conditionalMixture(self, fixed_params, fixed_param_values, label=None):
        """The mixture of the remaining parameters when ``fixed_params`` (names or indices) are held at
        ``fixed_param_values``: per component cov' = (block of cov^-1 over the kept parameters)^-1, the mean shifted
        accordingly, and the component weights multiplied by the component's marginal density at the fixed values."""
        fixed = self._params_to_indices(fixed_params)
        self.checkNoLimits(fixed)
        keep = [i for i in range(self.dim) if i not in fixed]
        if not keep:
            raise ValueError("conditionalMixture must leave at least one non-fixed parameter")
        kk, kf, ff, fk = np.ix_(keep, keep), np.ix_(keep, fixed), np.ix_(fixed, fixed), np.ix_(fixed, keep)
        means, covs, minus2logw = [], [], []
        for mean, cov, icov in zip(self.means, self.covs, self.invcovs):
            delta = np.asarray(fixed_param_values) - mean[fixed]
            cov_new = np.linalg.inv(icov[kk])
            means.append(mean[keep] - cov_new.dot(icov[kf].dot(delta)))
            covs.append(cov_new)
            schur = cov[ff] - cov[fk].dot(np.linalg.inv(cov[kk]).dot(cov[kf]))
            minus2logw.append(icov[ff].dot(delta).dot(delta) + np.log(np.linalg.det(schur)))
        # (as the reference: the prior component weights do not enter)
        weights = np.exp(-(np.asarray(minus2logw) - min(minus2logw)) / 2)
        names = [self.names[i] for i in keep] if self.names is not None else None
        out = MixtureND(means, covs, weights, names=names, label=label)
        _inherit_labels(out.paramNames, self.paramNames)
        return out

    def checkNoLimits(self, keep_params):
        """Raise unless every parameter outside ``keep_params`` is free of hard limits."""
        if self.lims is None:
            return
        for i, lim in enumerate(self.lims):
            if i not in keep_params and (lim[0] is not None or lim[1] is not None):
                raise Exception("In general can only marginalize analytically if no hard boundary limits: " + self.label)

    def getUpper(self, name):
        """The hard upper limit of parameter ``name`` (None: open)."""
        if self.lims is None:
            return None
        return self.lims[self.names.index(name)][1]

    def getLower(self, name):
        """The hard LOWER limit of parameter ``name`` (None: open).  The reference returns the upper limit from both
        getUpper and getLower (gaussian_mixtures.py:335-338 reads ``[1]``): a slip there, deliberately not reproduced."""
        if self.lims is None:
            return None
        return self.lims[self.names.index(name)][0]


class Mixture2D(MixtureND):
    """A Gaussian mixture in two dimensions with optional hard bounds on x and y."""

    def __init__(self, means, covs, weights=None, lims=None, names=("x", "y"), xmin=None, xmax=None, ymin=None, ymax=None,
                 **kwargs):
        """
        :param means: one (x, y) mean per component
        :param covs: per component a 2 x 2 covariance, or [sigma_x, sigma_y, correlation]
        :param weights: relative weight of each component (default: equal)
        :param lims: [[xmin, xmax], [ymin, ymax]], None for an open side; the keywords below take preference
        :param names: the two parameter names (default x, y)
        :param xmin, xmax, ymin, ymax: hard bounds
        :param kwargs: passed to :class:`MixtureND`
        """
        limits = self._updateLimits(lims, xmin, xmax, ymin, ymax) if lims is not None else [(xmin, xmax), (ymin, ymax)]
        full = []
        for cov in covs:
            if isinstance(cov, (list, tuple)) and len(cov) == 3 and not isinstance(cov[0], (list, tuple)):
                cov = make_2D_Cov(*cov)
            full.append(cov)
        super().__init__(means, full, weights, limits, names=names, **kwargs)

    def _updateLimits(self, lims, xmin=None, xmax=None, ymin=None, ymax=None):
        (x0, x1), (y0, y1) = lims
        return [(x0 if xmin is None else xmin, x1 if xmax is None else xmax),
                (y0 if ymin is None else ymin, y1 if ymax is None else ymax)]

    def _density2D(self, num_points=1024, xmin=None, xmax=None, ymin=None, ymax=None, sigma_max=5):
        lims = self._updateLimits(self.lims, xmin, xmax, ymin, ymax)
        (xmin, xmax), (ymin, ymax) = self.autoRanges(sigma_max, lims=lims)
        x = np.linspace(xmin, xmax, num_points)
        y = np.linspace(ymin, ymax, num_points)
        xx, yy = np.meshgrid(x, y)
        return Density2D(x, y, self.pdf(xx, yy))

    def pdf(self, x, y=None):
        """The density at (x, y) (arrays of equal shape broadcast).  With one argument: as :meth:`MixtureND.pdf`, ``x``
        being a point or an array of points by row.  Limits are not applied."""
        if y is None:
            return super().pdf(x)
        total = None
        for mean, icov, weight, norm in zip(self.means, self.invcovs, self.weights, self.norms):
            dx, dy = x - mean[0], y - mean[1]
            chi2 = dx ** 2 * icov[0, 0] + 2 * dx * dy * icov[0, 1] + dy ** 2 * icov[1, 1]
            part = np.exp(-chi2 / 2) / norm * weight
            total = part if total is None else total + part
        return total


class Gaussian2D(Mixture2D):
    """One Gaussian in two dimensions."""

    def __init__(self, mean, cov, **kwargs):
        """
        :param mean: the (x, y) mean
        :param cov: 2 x 2 covariance, or [sigma_x, sigma_y, correlation]
        :param kwargs: passed to :class:`Mixture2D`
        """
        super().__init__([mean], [cov], **kwargs)


class GaussianND(MixtureND):
    """One Gaussian in any number of dimensions."""

    def __init__(self, mean, cov, is_inv_cov=False, **kwargs):
        """
        :param mean: the mean vector, or the name of a text file holding it
        :param cov: the covariance matrix, or the name of a text file holding it
        :param is_inv_cov: ``cov`` is the inverse covariance
        :param kwargs: passed to :class:`MixtureND`
        """
        if isinstance(mean, str):
            mean = np.loadtxt(mean)
        if isinstance(cov, str):
            cov = np.loadtxt(cov)
        if is_inv_cov:
            cov = np.linalg.inv(cov)
        super().__init__([mean], [cov], **kwargs)


class Mixture1D(MixtureND):
    """A Gaussian mixture in one dimension with optional hard bounds."""

    def __init__(self, means, sigmas, weights=None, lims=None, name="x", xmin=None, xmax=None, **kwargs):
        """
        :param means: the mean of each component
        :param sigmas: the standard deviation of each component
        :param weights: relative weight of each component (default: equal)
        :param lims: (lower, upper), None for an open side; ``xmin`` / ``xmax`` take preference
        :param name: the parameter name (default x)
        :param kwargs: passed to :class:`MixtureND`
        """
        if lims is not None:
            limits = [(lims[0] if xmin is None else xmin, lims[1] if xmax is None else xmax)]
        else:
            limits = [(xmin, xmax)]
        super().__init__([[m] for m in means], [np.atleast_2d(s ** 2) for s in sigmas], weights, limits, names=[name],
                         **kwargs)

    def pdf(self, x):
        return self.pdf_marged(0, x)


class Gaussian1D(Mixture1D):
    """One Gaussian in one dimension."""

    def __init__(self, mean, sigma, **kwargs):
        super().__init__([mean], [sigma], **kwargs)


class RandomTestMixtureND(MixtureND):
    """A mixture with RANDOM PARAMETERS (covariances A A^T of uniform matrices, uniform means) for tests -- not random
    samples of a mixture."""

    def __init__(self, ndim=4, ncomponent=1, names=None, weights=None, seed=None, label="RandomMixture"):
        """
        :param ndim: number of dimensions
        :param ncomponent: number of components
        :param names: parameter names
        :param weights: component weights
        :param seed: seed or numpy Generator (consumed: ncomponent matrices, then the means)
        :param label: label of the mixture
        """
        rng = np.random.default_rng(seed)
        covs = []
        for _ in range(ncomponent):
            A = rng.random((ndim, ndim))
            covs.append(np.dot(A, A.T))
        super().__init__(rng.random((ncomponent, ndim)), covs, weights=weights, lims=None, names=names, label=label)


def randomTestMCSamples(ndim=4, ncomponent=1, nsamp=10009, nMCSamples=1, seed=10, names=None, labels=None, **kwargs):
    """One :class:`getdist_amd.MCSamples` (or a list of ``nMCSamples``) of ``nsamp`` samples from random mixtures; one
    Generator made from ``seed`` feeds the mixtures' parameters and their samples in turn.  Further keywords (``device``)
    go to the MCSamples constructor."""
    if names is None:
        names = ["x%s" % i for i in range(ndim)]
    if labels is None:
        labels = ["x_{%s}" % i for i in range(ndim)]
    rng = np.random.default_rng(seed)
    out = [RandomTestMixtureND(ndim, ncomponent, names, seed=rng).MCSamples(nsamp, labels=labels, name_tag="Sim %s" % (i + 1),
                                                                         random_state=rng, **kwargs)
           for i in range(nMCSamples)]
    return out if nMCSamples > 1 else out[0]

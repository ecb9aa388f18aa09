"""
What a Cobaya run says about its samples (getdist/cobaya_interface.py): the parameters with their labels, renames and hard
prior ranges, the sampler, its temperature and the label, read from the run's ``updated.yaml`` (or from the info dictionary
``cobaya.run`` returns), and ``MCSamplesFromCobaya`` for sample collections that are still in memory.

All of this is host work on a small dictionary.  The O(N) part of loading a run -- the chain text ``root.1.txt, ...`` -- goes
through chainfiles.loadNumpyTxt like any other chain file (on the device: gd_parse_scan / gd_parse_rows).
"""

import logging
import os
from collections.abc import Mapping, Sequence
from copy import deepcopy
from numbers import Number

import numpy as np

# the keys of an info dictionary and of a parameter's entry (cobaya_interface.py:12-29)
_label = "label"
_prior = "prior"
_params = "params"
_likelihood = "likelihood"
_sampler = "sampler"
_p_label = "latex"
_p_dist = "dist"
_p_value = "value"
_p_derived = "derived"
_p_renames = "renames"
_separator = "__"
_minuslogprior = "minuslogprior"
_prior_1d_name = "0"
_chi2 = "chi2"
_weight = "weight"
_minuslogpost = "minuslogpost"
_post = "post"


def cobaya_params_file(root):
    """cobaya_interface.py:32-40: ``root.updated.yaml`` if it exists, else ``root__full.yaml`` (the older name), else None.
    A root that ends in a path separator names a folder: the two files are then ``updated.yaml`` / ``full.yaml`` inside it."""
    is_folder = root.endswith((os.sep, "/"))
    for joint, tail in ((".", "updated.yaml"), ("__", "full.yaml")):
        file = root + ("" if is_folder else joint) + tail
        if os.path.exists(file):
            return file
    return None


def yaml_file_or_dict(file_or_dict):
    """cobaya_interface.py:43-51: the info dictionary itself, or the one a yaml file of that name holds"""
    if isinstance(file_or_dict, str):
        from .yaml_tools import yaml_load_file

        return yaml_load_file(file_or_dict)
    if isinstance(file_or_dict, Mapping):
        return file_or_dict
    raise ValueError("Cobya parameter input must be a dictionary or filename")


def _as_list(x):
    return [x] if isinstance(x, str) else x


def _text_label(name):
    return name.replace("_", r"\ ")


def get_info_params(info):
    """cobaya_interface.py:143-181: {name: entry} of everything a chain of this run can hold, in the order the reference
    gives: the ``params`` block as written -- fixed parameters included -- without those ``post: remove: params`` names and
    with the entries of ``post: add: params`` merged in (a new name goes to the end); then ``minuslogprior``,
    ``minuslogprior__0`` (the product of the 1D priors) and one ``minuslogprior__<name>`` per named prior; then ``chi2`` and
    one ``chi2__<name>`` per likelihood.  Priors and likelihoods follow ``post: remove / add`` too.  The synthetic entries
    hold a LaTeX label only, so they count as derived."""
    info = yaml_file_or_dict(info)
    params = dict(info.get(_params))
    priors = [_prior_1d_name] + list(info.get(_prior) or [])
    likes = list(info.get(_likelihood))
    post = info.get(_post, {})
    remove, add = post.get("remove", {}), post.get("add", {})
    for name in remove.get(_params, []) or []:
        params.pop(name, None)
    for like in _as_list(remove.get(_likelihood) or []):
        likes.remove(like)
    for prior in _as_list(remove.get(_prior)) or []:
        priors.remove(prior)
    for name, entry in add.get(_params, {}).items():
        merged = dict(params.get(name, {}))  # (the reference updates the entry of the info dictionary in place)
        merged.update(entry)
        params[name] = merged
    likes += list(add.get(_likelihood, []))
    priors += list(add.get(_prior, []))
    params[_minuslogprior] = {_p_label: r"-\log\pi"}
    for prior in priors:
        params[_minuslogprior + _separator + prior] = {_p_label: r"-\log\pi_\mathrm{" + _text_label(prior) + "}"}
    params[_chi2] = {_p_label: r"\chi^2"}
    for like in likes:
        params[_chi2 + _separator + like] = {_p_label: r"\chi^2_\mathrm{" + _text_label(like) + "}"}
    return params


def expand_info_param(info_param):
    """cobaya_interface.py:227-245: a parameter's entry as a dictionary of its own (a deep copy).  A bare value becomes
    ``{"value": v}`` and nothing becomes ``{}``; an entry with neither ``prior``, ``value`` nor ``derived`` is derived, and so
    is -- unless it says otherwise -- one whose value is a string or a callable (computed from other parameters)."""
    if isinstance(info_param, Mapping):
        out = deepcopy(info_param)
    else:
        out = {} if info_param is None else {_p_value: info_param}
    if not any(key in out for key in (_prior, _p_value, _p_derived)):
        out[_p_derived] = True
    value = out.get(_p_value)
    if isinstance(value, str) or callable(value):
        out.setdefault(_p_derived, True)
    return out


def is_sampled_param(info_param):
    """cobaya_interface.py:213-217: the parameter has a prior"""
    return _prior in expand_info_param(info_param)


def is_derived_param(info_param):
    """cobaya_interface.py:220-224: the parameter is saved as a derived one (the ``derived`` entry itself, False if none)"""
    return expand_info_param(info_param).get(_p_derived, False)


def get_range(param_info):
    """cobaya_interface.py:185-210: (lower, upper, periodic) of a parameter's entry; None is an open side.

    - sampled: the prior is ``[min, max]`` or a dictionary.  ``min`` / ``max`` win if either is there; otherwise ``loc`` /
      ``scale`` (and whatever else but ``dist`` and ``periodic`` the dictionary holds) go to
      ``scipy.stats.<dist, default "uniform">.interval(1, ...)``, whose infinite ends are open sides.  Any other prior
      raises ValueError.  ``periodic`` may stand in the entry or inside the prior.
    - a fixed number: ``(v, v, False)``.
    - anything else (derived, or a value computed from other parameters): the entry's own ``min`` / ``max`` and ``periodic``.

    A prior dictionary with none of min / max / loc / scale has no bounds to report: ValueError here (in the reference the
    function then fails on an unset variable)."""
    entry = expand_info_param(param_info or {})
    periodic = entry.get("periodic", False)
    if is_sampled_param(entry):
        prior = entry[_prior]
        if isinstance(prior, Sequence) and len(prior) == 2:
            prior = dict(zip(("min", "max"), prior))
        elif not isinstance(prior, Mapping):
            raise ValueError("Format of prior not recognised: %r. " % (prior,)
                             + "Use '[min, max]' or a dictionary following Cobaya's documentation.")
        periodic = periodic or prior.pop("periodic", False)
        if prior.get("min") is not None or prior.get("max") is not None:
            lims = [prior.get("min"), prior.get("max")]
        elif prior.get("loc") is not None or prior.get("scale") is not None:
            import scipy.stats

            args = dict(prior)
            dist = args.pop(_p_dist, "uniform")
            lims = getattr(scipy.stats, dist).interval(1, **args)
        else:
            raise ValueError("Prior has neither min / max nor loc / scale: %r" % (prior,))
        return lims[0] if lims[0] != -np.inf else None, lims[1] if lims[1] != np.inf else None, periodic
    value = entry.get(_p_value)
    if isinstance(value, Number):
        return float(value), float(value), False
    return entry.get("min"), entry.get("max"), periodic


def get_sampler_key(filename_or_info, default_sampler_for_chain_type="mcmc"):
    """cobaya_interface.py:248-249: the first key of the ``sampler`` block"""
    return list(yaml_file_or_dict(filename_or_info).get(_sampler, [default_sampler_for_chain_type]))[0]


def get_sampler_type(filename_or_info, default_sampler_for_chain_type="mcmc"):
    """cobaya_interface.py:252-257: what MCSamples takes as ``sampler``: the ``sampler_type`` the sampler's own options give
    if there is one, else "nested" for polychord, else the sampler's key.  A sampler written without options
    (``polychord: null``, as in a hand-written input) has no ``sampler_type``; the reference fails on it with AttributeError,
    while Cobaya's own updated.yaml always spells the options out."""
    info = yaml_file_or_dict(filename_or_info)
    sampler = get_sampler_key(info, default_sampler_for_chain_type)
    sampler_type = ((info.get(_sampler) or {}).get(sampler) or {}).get("sampler_type", None)
    if sampler_type is None:
        return "nested" if sampler == "polychord" else sampler
    return sampler_type


def get_sampler_temperature(filename_or_info):
    """cobaya_interface.py:260-267: None without a ``sampler`` block; 1 for a post-processed run (always cooled already);
    else the sampler's ``temperature`` option (None if it has none)"""
    info = yaml_file_or_dict(filename_or_info)
    if _sampler not in info:
        return None
    if _post in info:
        return 1
    return (info[_sampler][get_sampler_key(info)] or {}).get("temperature")


def get_sample_label(filename_or_info):
    """cobaya_interface.py:270-271: the run's ``label`` (None if it has none)"""
    return yaml_file_or_dict(filename_or_info).get(_label)


def get_burn_removed(filename_or_info):
    """cobaya_interface.py:274-277, as the reference computes it: the ``skip`` entry of ``post`` looked up in the dictionary
    of get_info_params -- that is, among the PARAMETER entries, not in the run's ``post`` block.  So the answer is 0 for every
    run but one that has a parameter called ``post`` whose entry holds ``skip``; in particular a run whose ``post: skip`` did
    remove rows still reports 0, and the burn-in asked for is removed from it again."""
    return get_info_params(filename_or_info).get(_post, {}).get("skip", 0)


def MCSamplesFromCobaya(info, collections, name_tag=None, ignore_rows=0, ini=None, settings=None, **kwargs):
    """
    cobaya_interface.py:54-136: an MCSamples from the sample collection(s) of a Cobaya run held in memory and the run's
    updated info dictionary.  A collection is anything with ``.data`` (a DataFrame whose first two columns are the weight
    and minus log posterior) that indexes by column name(s): ``c[cols]``, ``c["weight"]``, ``c["minuslogpost"]``.

    The parameters are the collection's columns in the COLLECTION's order; the info supplies the derived flags, labels,
    renames, the ranges (those of the fixed parameters too, which have no column), the sampler, its temperature and the
    label.  Sampled plus derived parameters of the info must be the collection's columns (AssertionError otherwise).  Asking
    for ``ignore_rows`` of a run whose ``post: skip`` removed rows already, and a temperature other than 1, are warned about.
    Further keywords (``device``, ``_context_factory``) go to MCSamples.
    """
    if hasattr(collections, "data"):
        collections = [collections]
    try:  # (the columns of a DataFrame: a bare array has a ``.data`` too, but that has none)
        columns = list(collections[0].data.columns)
    except (AttributeError, TypeError, IndexError, KeyError):
        raise TypeError("The second argument does not appear to be a (list of) samples `Collection`.") from None
    if not all(list(c.data.columns) == columns for c in collections[1:]):
        raise ValueError("The given collections don't have the same columns.")
    info = yaml_file_or_dict(info)
    info_params = get_info_params(info)
    skip = info.get(_post, {}).get("skip", 0)
    if ignore_rows != 0 and skip != 0:
        logging.warning("You are asking for rows to be ignored (%r), but some (%r) were already ignored in the original chain.",
                        ignore_rows, skip)
    var_params = [p for p, entry in info_params.items() if is_sampled_param(entry) or is_derived_param(entry)]
    assert set(columns[2:]) == set(var_params), (
        "Info and collection(s) are not compatible, because their parameters differ: the collection(s) have %r and the info "
        "has %r. " % (columns[2:], var_params)
        + "Are you sure that you are using an *updated* info dictionary (i.e. the output of `cobaya.run`)?")
    pars = columns[2:]
    derived = [bool(is_derived_param(info_params[p])) for p in pars]
    labels = [(info_params[p] or {}).get(_p_label, p) for p in pars]
    ranges = {p: get_range(entry) for p, entry in info_params.items()}  # the fixed parameters too
    renames = {p: (info_params[p] or {}).get(_p_renames, []) for p in pars}
    samples = [c[c.data.columns[2:]].values.astype(np.float64) for c in collections]
    weights = [c[_weight].values.astype(np.float64) for c in collections]
    loglikes = [c[_minuslogpost].values.astype(np.float64) for c in collections]
    temperature = get_sampler_temperature(info)
    if temperature is not None and temperature != 1:
        logging.warning("You have loaded a sample with non-unit temperature. Use the 'MCSamples.cool()' method to turn it "
                        "into a sample from the original posterior before performing statistical analyses, but maybe after "
                        "thinning the sample with method 'MCSamples.thin_indices()'.")
    from .mcsamples import MCSamples

    return MCSamples(samples=samples, weights=weights, loglikes=loglikes, sampler=get_sampler_type(info),
                     names=[p + "*" * d for p, d in zip(pars, derived)], labels=labels, ranges=ranges, renames=renames,
                     ignore_rows=ignore_rows, name_tag=name_tag, label=get_sample_label(info), ini=ini, temperature=temperature,
                     settings=settings, **kwargs)

"""CPU tests of loading Cobaya runs: yaml_tools, the cobaya_interface functions, the yaml branches of ParamNames / ParamBounds,
chainfiles.read_root / MCSamples(root=...) / loadMCSamples on run folders, the binary cache's freshness rule,
MCSamplesFromCobaya and the save / reload round trip -- against tests/golden/cobaya.json (the reference's results for the
same files: tests/golden/make_golden_cobaya.py).  The device context is the numpy double of tests/fake_ctx.py."""

import copy
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cobaya_cases as cc  # noqa: E402
import fake_ctx  # noqa: E402
from getdist_amd import chainfiles, yaml_tools  # noqa: E402
from getdist_amd import cobaya_interface as ci  # noqa: E402
from getdist_amd.chains import WeightedSampleError  # noqa: E402
from getdist_amd.mcsamples import MCSamples  # noqa: E402
from getdist_amd.paramnames import ParamNames  # noqa: E402
from getdist_amd.parampriors import ParamBounds  # noqa: E402

FAKE = dict(_context_factory=fake_ctx.FakeContext)
MEANS_RTOL = 1e-12  # the gate for host-visible statistics


@pytest.fixture(scope="module")
def golden():
    return cc.load_golden()


def load(root, **kw):
    return MCSamples(root=root, _no_cache=True, **FAKE, **kw)


def check_numbers(numbers, want):
    for key in want:
        assert np.allclose(numbers[key], want[key], rtol=MEANS_RTOL, atol=0), key


# ---- 1. the pure functions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.RUNS))
def test_interface_functions(golden, tmp_path, name):
    got, want = cc.interface_results(ci, name, str(tmp_path)), golden["interface"][name]
    assert [k for k, _ in got["info_params"]] == [k for k, _ in want["info_params"]]  # the order, as a list
    if name == "runB":
        # `polychord: null`: the reference's get_sampler_type fails on the missing options; here they count as empty
        assert want["get_sampler_type"] == {"error": "AttributeError"}
        assert got.pop("get_sampler_type") == golden["interface"]["runB2"]["get_sampler_type"] == "nested"
        want = {k: v for k, v in want.items() if k != "get_sampler_type"}
    assert got == want


def test_get_range_cases(golden):
    got = cc.range_results(ci)
    assert len(got) == len(cc.RANGE_CASES) == len(golden["get_range"]) >= 15
    for case, g, w in zip(cc.RANGE_CASES, got, golden["get_range"]):
        assert g == w, case
    assert sum("error" in w for w in golden["get_range"] if isinstance(w, dict)) == 3
    with pytest.raises(ValueError, match="Format of prior not recognised: 'flat'"):
        ci.get_range({"prior": "flat"})


def test_get_range_leaves_the_entry_alone():
    entry = {"prior": {"min": 0, "max": 1, "periodic": True}}
    before = copy.deepcopy(entry)
    assert ci.get_range(entry) == (0, 1, True) and entry == before


def test_params_file_and_file_or_dict(tmp_path):
    root = str(tmp_path / "run")
    assert ci.cobaya_params_file(root) is None
    (tmp_path / "run__full.yaml").write_text("params: {}\n")
    assert ci.cobaya_params_file(root) == root + "__full.yaml"
    (tmp_path / "run.updated.yaml").write_text("params: {}\n")
    assert ci.cobaya_params_file(root) == root + ".updated.yaml"
    folder = str(tmp_path / "out") + "/"  # a root that names a folder: the files have no prefix
    os.makedirs(folder)
    open(folder + "full.yaml", "w").close()
    assert ci.cobaya_params_file(folder) == folder + "full.yaml"
    open(folder + "updated.yaml", "w").close()
    assert ci.cobaya_params_file(folder) == folder + "updated.yaml"
    info = {"params": {}}
    assert ci.yaml_file_or_dict(info) is info and ci.yaml_file_or_dict(root + ".updated.yaml") == info
    with pytest.raises(ValueError):
        ci.yaml_file_or_dict(3)


def test_burn_removed_looks_among_the_parameters():
    info = {"params": {"x": {"prior": [0, 1]}}, "likelihood": {"one": None}, "post": {"skip": 0.3}}
    assert ci.get_burn_removed(info) == 0  # the run's post block is not where it looks
    info["params"]["post"] = {"skip": 0.3, "derived": True}
    assert ci.get_burn_removed(info) == 0.3


# ---- 2. yaml_load -----------------------------------------------------------------------------------------------------------
def test_yaml_load():
    got = yaml_tools.yaml_load("a: 1e2\nb: 1E-3\nc: 12\nd: 1.5e+3\ne: !!python/name:builtins.len ''\nf: 1e\n")
    assert got == dict(a=100.0, b=0.001, c=12, d=1500.0, e=None, f="1e")
    assert isinstance(got["a"], float) and isinstance(got["b"], float) and isinstance(got["c"], int)


def test_yaml_syntax_error_names_file_line_and_column(tmp_path):
    path = str(tmp_path / "broken.yaml")
    with open(path, "w", encoding="utf-8") as f:
        f.write("params:\n  a:\n    prior: [0, 1]\n   latex: x\n")
    with pytest.raises(yaml_tools.InputSyntaxError) as e:
        yaml_tools.yaml_load_file(path)
    text = str(e.value)
    assert path in text and "at line 4, column 4." in text and " --> |   latex: x" in text
    with pytest.raises(yaml_tools.InputSyntaxError):
        yaml_tools.yaml_load("a: [1, 2\nb: 3\n")
    with open(path, "w", encoding="utf-8-sig") as f:  # a byte-order mark is dropped
        f.write("a: 1e2\n")
    assert yaml_tools.yaml_load_file(path) == {"a": 100.0}


def test_yaml_is_imported_when_a_file_is_read(monkeypatch):
    import importlib

    monkeypatch.setitem(sys.modules, "yaml", None)  # what a missing PyYAML looks like to an import statement
    importlib.reload(yaml_tools)
    try:
        with pytest.raises(ModuleNotFoundError, match="PyYAML"):
            yaml_tools.yaml_load("a: 1\n")
    finally:
        monkeypatch.undo()
        importlib.reload(yaml_tools)


# ---- the side-file readers -----------------------------------------------------------------------------------------------------
def test_param_names_from_yaml():
    pars = ParamNames.fromFile(cc.yaml_path("runA"))
    assert pars.list() == cc.RUNS["runA"]["columns"]  # sampled first, then derived: the order of the chain's columns
    assert [p.isDerived for p in pars.names] == [False] * 3 + [True] * 7
    assert pars.parWithName("a").label == "\\alpha_{\\rm s}" and pars.parWithName("d").label == "d"
    assert pars.getRenames() == {"a": ["alpha", "a_s"]} and pars.parWithName("a_s") is pars.names[0]
    assert pars.filenameLoadedFrom == "runA.updated.yaml"
    assert pars.info_dict["sampler"] == {"mcmc": {"temperature": 1, "burn_in": 0, "max_tries": 1000.0}}
    assert pars.info_dict["params"]["fixedp"] == 0.06 and not pars.hasParam("fixedp")
    with pytest.raises(ValueError, match="ParanNames must be loaded from .paramnames or .yaml/.yml file, found run.txt"):
        ParamNames.fromFile("run.txt")
    assert ParamNames(["x"]).info_dict is None


def test_param_names_from_paramnames_file(tmp_path):
    path = str(tmp_path / "r.paramnames")
    with open(path, "w") as f:
        f.write("x\tx_1\ny*\t\\gamma\t#a comment\n")
    pars = ParamNames.fromFile(path)
    assert str(pars) == "x\tx_1\ny*\t\\gamma\t#a comment\n" and pars.filenameLoadedFrom == "r.paramnames"


def test_param_bounds_from_files(tmp_path):
    b = ParamBounds(cc.yaml_path("runA"))
    assert b.names == ["a", "th", "fixedp", "d"] and b.periodic == {"th"}
    assert (b.getLower("a"), b.getUpper("a")) == (0.0, 3.0) and b.fixedValue("fixedp") == 0.06
    assert b.getLower("b") is None and b.getUpper("b") is None and (b.getLower("d"), b.getUpper("d")) == (0.0, None)
    path = str(tmp_path / "r.ranges")
    b.saveToFile(path)
    again = ParamBounds(path)
    assert str(again) == str(b) and again.periodic == {"th"}
    assert ParamBounds().names == []
    with pytest.raises(ValueError, match="ParamBounds must be loaded from .bounds, .ranges or .yaml/.yml file, not r.txt"):
        ParamBounds("r.txt")


# ---- 3. / 4. loading the runs ------------------------------------------------------------------------------------------------
def test_run_a_has_the_names_and_bounds_of_its_yaml(tmp_path):
    """On a tree that reads no updated.yaml the parameters are param1 ... and nothing bounds them."""
    mc = load(cc.build_run("runA", tmp_path), ignore_rows=0.3)
    assert mc.paramNames.list() == ["a", "b", "th", "c", "d", "chi2", "chi2__gauss_like"]
    assert not any(nm.startswith("param") for nm in mc.paramNames.list())
    assert mc.getUpper("a") == 3.0 and mc.getLower("a") == 0.0 and mc.getUpper("alpha") == 3.0
    assert mc.numrows == 280 and list(mc.chain_offsets) == [0, 140, 280]
    assert mc.ranges.fixedValueDict() == {"fixedp": 0.06, "minuslogprior": 1.5, "minuslogprior__0": 1.0, "minuslogprior__ab_prior": 0.5}
    assert mc.getParamSampleDict(0)["fixedp"] == 0.06 and "fixedp" not in mc.getParamSampleDict(0, want_fixed=False)
    assert mc.ranges.getLower("b") is None and mc.ranges.getUpper("b") is None and "b" not in mc.ranges.names
    assert mc.paramNames.parWithName("th").periodic and mc.paramNames.parWithName("a").has_limits_top
    assert mc.paramNames.info_dict["label"] == mc.label


@pytest.mark.parametrize("name", cc.LOADED_RUNS)
@pytest.mark.parametrize("through", ["MCSamples", "loadMCSamples"])
def test_loaded_runs_against_the_reference(golden, tmp_path, name, through):
    root = cc.build_run(name, tmp_path)
    rows = cc.RUNS[name]["ignore_rows"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # none of these samplers is unknown
        if through == "MCSamples":
            mc = load(root, ignore_rows=rows)
        else:
            mc = chainfiles.loadMCSamples(root, no_cache=True, settings={"ignore_rows": rows}, **FAKE)
    exact, numbers = cc.summarize(mc)
    want = golden["runs"][name]
    for key in want["exact"]:
        assert exact[key] == want["exact"][key], key
    assert set(exact) == set(want["exact"])
    check_numbers(numbers, want["numbers"])
    assert mc.temperature == golden["interface"][name]["get_sampler_temperature"]
    assert mc.name_tag == name


def test_run_b_is_nested_and_keeps_its_rows(golden, tmp_path):
    root = cc.build_run("runB", tmp_path)
    mc = load(root)
    assert mc.sampler == "nested" and mc.properties == {"sampler": "nested"} and mc.numrows == 150
    twin = load(cc.build_run("runB2", tmp_path))  # the same chain under the yaml the reference can read
    exact, numbers = cc.summarize(mc)
    assert exact == cc.summarize(twin)[0] == golden["runs"]["runB2"]["exact"]
    check_numbers(numbers, golden["runs"]["runB2"]["numbers"])
    for kw in (dict(ignore_rows=0.3), dict(ignore_rows=10), dict(settings={"ignore_rows": 0.2})):
        with pytest.raises(ValueError, match="Should not remove burn-in from Nested Sampler samples."):
            load(root, **kw)
    with pytest.raises(ValueError, match="Nested Sampler"):
        chainfiles.loadMCSamples(root, no_cache=True, ignore_rows=0.3, **FAKE)
    assert load(root, sampler="mcmc", ignore_rows=0.2).numrows == 120  # a sampler that was passed wins


def test_keywords_win_over_the_yaml(tmp_path):
    root = cc.build_run("runC", tmp_path)
    mc = load(root, label="mine", sampler="uncorrelated", temperature=3.0)
    assert (mc.label, mc.sampler, mc.temperature) == ("mine", "uncorrelated", 3.0)
    assert mc.properties == {"sampler": "uncorrelated", "temperature": 3.0}
    mc = load(root, renames={"x": "ex", "z": ["zed"]})
    assert mc.getRenames() == {"x": ["ex"], "z": ["zed"]} and mc.paramNames.parWithName("zed").name == "z"


def test_unknown_sampler_and_count_mismatch(tmp_path):
    root = cc.build_run("runD", tmp_path, with_yaml=False)
    text = open(cc.yaml_path("runD")).read()
    with open(root + ".updated.yaml", "w") as f:
        f.write(text.replace("sampler_type: uncorrelated", "sampler_type: Slice"))
    with pytest.warns(UserWarning, match="Unknown sampler type slice. Assuming MCMC."):
        mc = load(root)
    assert mc.sampler == "mcmc" and mc.properties["sampler"] == "mcmc"
    with open(root + ".updated.yaml", "w") as f:
        f.write(text.replace("  r:\n    derived: true\n    min: 0\n    latex: r_{xy}\n", ""))
    with pytest.raises(WeightedSampleError):
        load(root)


def test_a_ranges_file_wins_over_the_yaml(tmp_path):
    root = cc.build_run("runA", tmp_path)
    with open(root + ".ranges", "w") as f:
        f.write("a 0.5 N\nfixedp 0.07 0.07\nth 0 6.5 periodic\n")
    mc = load(root)
    assert (mc.getLower("a"), mc.getUpper("a"), mc.getLower("d")) == (0.5, None, None)
    assert mc.ranges.fixedValue("fixedp") == 0.07 and mc.ranges.periodic == {"th"}


def test_a_properties_file_keeps_the_yaml_out(tmp_path):
    root = cc.build_run("runB", tmp_path)
    open(root + ".properties.ini", "w").close()
    mc = load(root, ignore_rows=0.2)  # (reading the file itself is not part of loading yet)
    assert mc.sampler == "mcmc" and mc.properties is None and mc.label is None and mc.numrows == 120
    assert mc.paramNames.list()[:3] == ["x", "y", "r"]  # names and ranges still come from the yaml


# ---- 5. the binary cache -----------------------------------------------------------------------------------------------------
def test_cache_is_older_than_a_rewritten_yaml(tmp_path):
    root = cc.build_run("runA", tmp_path)
    yaml_file, cache = root + ".updated.yaml", chainfiles.cache_path(root)
    for k, f in enumerate([root + ".1.txt", root + ".2.txt", yaml_file]):
        os.utime(f, (1000 + k, 1000 + k))
    first = MCSamples(root=root, **FAKE)
    assert os.path.isfile(cache) and first.label == "Run A \\ (mcmc)"
    os.utime(cache, (2000, 2000))
    assert chainfiles.read_root(root)["from_cache"]
    text = open(yaml_file).read()
    with open(yaml_file, "w") as f:
        f.write(text.replace("label: Run A \\ (mcmc)", "label: Run A again"))
    os.utime(yaml_file, (3000, 3000))  # newer than the cache: a rewritten yaml
    loaded = chainfiles.read_root(root)
    assert not loaded["from_cache"] and loaded["info_dict"]["label"] == "Run A again"
    assert os.path.getmtime(cache) > 3000  # written again
    third = chainfiles.read_root(root)
    assert third["from_cache"]
    again = MCSamples(root=root, **FAKE)
    assert again.label == "Run A again" and np.array_equal(again.samples, first.samples)
    # only yamls that carry the root's prefix count, and only for a root without .paramnames
    other = str(tmp_path / "other.updated.yaml")
    open(other, "w").close()
    os.utime(other, (4e9, 4e9))
    assert chainfiles.read_root(root)["from_cache"]
    post = root + ".post.rerun.updated.yaml"  # (the output of a post-processing of this run)
    open(post, "w").close()
    os.utime(post, (4e9, 4e9))
    assert not chainfiles.read_root(root)["from_cache"]


def test_full_yaml_only_root(golden, tmp_path):
    root = cc.build_run("runD", tmp_path)
    assert ci.cobaya_params_file(root) == root + "__full.yaml" and not os.path.exists(root + ".updated.yaml")
    assert load(root).sampler == "uncorrelated"


# ---- 6. MCSamplesFromCobaya -------------------------------------------------------------------------------------------------
def test_from_cobaya_collections(tmp_path, caplog):
    root = cc.build_run("runA", tmp_path)
    info = yaml_tools.yaml_load_file(root + ".updated.yaml")
    before = copy.deepcopy(info)
    from_root = load(root)
    mc = ci.MCSamplesFromCobaya(info, cc.collections_of("runA", root), name_tag="tag", **FAKE)
    assert info == before
    a, b = cc.summarize(mc), cc.summarize(from_root)
    for key in ("names", "labels", "derived", "renames", "ranges", "periodic", "sampler", "label", "numrows", "chain_offsets",
                "upper", "lower", "ranges_upper", "ranges_lower"):
        assert a[0][key] == b[0][key], key
    assert a[1] == b[1] and mc.name_tag == "tag" and mc.temperature == 1
    single = ci.MCSamplesFromCobaya(info, cc.collections_of("runA", root)[0], ignore_rows=0.5, **FAKE)
    assert single.numrows == 100 and single.chains is None
    # column order comes from the collection
    cols = cc.collections_of("runA", root)
    order = list(cols[0].data.columns[:2]) + list(cols[0].data.columns[:1:-1])
    swapped = ci.MCSamplesFromCobaya(info, [cc.Collection(c.data[order]) for c in cols], **FAKE)
    assert swapped.paramNames.list() == ["chi2__gauss_like", "chi2", "d", "c", "th", "b", "a"]
    assert [p.isDerived for p in swapped.paramNames.names] == [True] * 4 + [False] * 3
    assert np.array_equal(swapped.samples[:, 6], mc.samples[:, 0])
    # the failures
    short = [cc.Collection(c.data.drop(columns=["d"])) for c in cols]
    with pytest.raises(AssertionError) as e:
        ci.MCSamplesFromCobaya(info, short, **FAKE)
    assert repr(list(short[0].data.columns[2:])) in str(e.value) and repr(cc.RUNS["runA"]["columns"]) in str(e.value)
    assert "*updated* info dictionary" in str(e.value)
    with pytest.raises(TypeError, match="does not appear to be a"):
        ci.MCSamplesFromCobaya(info, np.zeros((3, 12)), **FAKE)
    with pytest.raises(ValueError, match="don't have the same columns"):
        ci.MCSamplesFromCobaya(info, [cols[0], short[1]], **FAKE)
    # the two warnings
    hot = copy.deepcopy(info)
    hot["sampler"]["mcmc"]["temperature"] = 2
    with caplog.at_level("WARNING"):
        assert ci.MCSamplesFromCobaya(hot, cols, **FAKE).temperature == 2
    assert "non-unit temperature" in caplog.text
    caplog.clear()
    hot["post"] = {"skip": 0.1}
    with caplog.at_level("WARNING"):
        assert ci.MCSamplesFromCobaya(hot, cols, ignore_rows=0.1, **FAKE).temperature == 1
    assert "were already ignored in the original chain" in caplog.text and "non-unit" not in caplog.text


def test_starred_names_are_derived():
    x = np.random.default_rng(1).standard_normal((50, 2))
    mc = MCSamples(samples=x, names=["u", "v*"], **FAKE)
    assert mc.paramNames.list() == ["u", "v"] and [p.isDerived for p in mc.paramNames.names] == [False, True]


# ---- 7. / 8. GetDist-format roots -----------------------------------------------------------------------------------------
def test_save_as_text_round_trip(tmp_path):
    mc = load(cc.build_run("runA", tmp_path / "in"), ignore_rows=0.3)
    os.makedirs(tmp_path / "out")
    root2 = str(tmp_path / "out" / "saved")
    mc.saveAsText(root2)
    assert os.path.isfile(root2 + ".paramnames") and os.path.isfile(root2 + ".ranges") and os.path.isfile(root2 + ".txt")
    back = load(root2)
    assert back.paramNames.list() == mc.paramNames.list() and back.paramNames.labels() == mc.paramNames.labels()
    assert [p.isDerived for p in back.paramNames.names] == [p.isDerived for p in mc.paramNames.names]
    for nm in mc.paramNames.list():
        for got, want in ((back.getLower(nm), mc.getLower(nm)), (back.getUpper(nm), mc.getUpper(nm))):
            assert got == (None if want is None else float("%15.7E" % want)), nm  # the figures a .ranges file holds
        assert back.paramNames.parWithName(nm).periodic == mc.paramNames.parWithName(nm).periodic
    assert back.ranges.periodic == {"th"} and back.paramNames.info_dict is None
    assert back.getRenames() == {}  # a .paramnames file has no place for them
    assert back.numrows == mc.numrows and np.allclose(back.getMeans(), mc.getMeans(), rtol=1e-7)  # "%.8e" text


def test_getdist_root_ignores_a_stray_yaml(tmp_path):
    rng = np.random.default_rng(5)
    root = str(tmp_path / "chain")
    for k in (1, 2):
        x = np.column_stack([rng.integers(1, 4, 60), rng.random(60) * 10, rng.standard_normal((60, 3))])
        np.savetxt("%s_%d.txt" % (root, k), x, fmt="%.8e")
    with open(root + ".paramnames", "w") as f:
        f.write("p\tp_1\nq\nr*\tr\n")
    with open(root + ".ranges", "w") as f:
        f.write("p -10 N\nelsewhere 0 1\n")
    plain = load(root, ignore_rows=0.1)
    with open(root + ".updated.yaml", "w") as f:
        f.write(open(cc.yaml_path("runB2")).read())
    os.utime(root + ".updated.yaml", (4e9, 4e9))
    mc = load(root, ignore_rows=0.1)
    assert cc.summarize(mc) == cc.summarize(plain)
    assert mc.paramNames.list() == ["p", "q", "r"] and mc.sampler == "mcmc" and mc.properties is None
    assert mc.ranges.names == ["p"] and mc.paramNames.info_dict is None and mc.label is None
    MCSamples(root=root, **FAKE)
    assert chainfiles.read_root(root)["from_cache"]  # the yaml's date is nothing to a root with .paramnames

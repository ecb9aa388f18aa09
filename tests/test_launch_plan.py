"""
The optimiser's launch list of gd_density2d_batch (plan_launches in getdist_amd/csrc/batch2d.hpp: a pure function of the
branch plan, the grid-size classes and the part sizes) on the CPU: its properties over random plans, and the layouts of
four calls whose part sizes were read off the host timeline (GDHIP_BATCH_LOG=1, "kopt: stage A enqueue (q, B)" /
"kopt: launch (B, F)") of the commit before the function was split out of bandwidth_2d.
"""

import ctypes as C

import numpy as np
import pytest

import native_batch_util as nb

A, B_, C_ = 0, 1, 2  # bandwidth branches: sheared / rule of thumb / the optimiser's own


def plan(branch, F, base_F=256, staged=True, deferred=False, split_min=8):
    lib = nb.harness()
    branch = np.ascontiguousarray(branch, dtype=np.int8)
    F = np.ascontiguousarray(F, dtype=np.int32)
    P = len(branch)
    head, ks, pos = np.zeros(4 * (P + 1), dtype=np.int32), np.full(P, -1, dtype=np.int32), np.full(P, -1, dtype=np.int32)
    fn = lib.gdt_plan_launches
    fn.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p] * 3
    n = fn(branch.ctypes.data, F.ctypes.data, P, base_F, int(staged), int(deferred), split_min, P + 1, head.ctypes.data,
           ks.ctypes.data, pos.ctypes.data)
    assert n >= 0, n
    out, k0, p0 = [], 0, 0
    for q in range(n):
        Fq, na, whole, rows = (int(v) for v in head[4 * q:4 * q + 4])
        out.append(dict(F=Fq, na=na, whole=bool(whole), ks=ks[k0:k0 + rows].tolist(), pos=pos[p0:p0 + rows - na].tolist()))
        k0, p0 = k0 + rows, p0 + rows - na
    assert k0 == int(np.sum(branch != B_)) or not out, "every sheared and optimiser pair is in a launch"
    return out


def classes_of(F):
    order, members = [], {}
    for k, f in enumerate(F):
        if f not in members:
            order.append(f)
            members[f] = []
        members[f].append(k)
    return order, members


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("deferred", [False, True])
def test_launch_list_properties(staged, deferred):
    rng = np.random.default_rng(11)
    for trial in range(300):
        P = int(rng.integers(1, 90))
        weights = rng.dirichlet([1, 1, 1]) if trial % 5 else np.array([0.5, 0.5, 0.0])  # (every fifth: no optimiser pair)
        branch = rng.choice([A, B_, C_], size=P, p=weights)
        F = rng.choice([256, 576, 960], size=P, p=[0.8, 0.15, 0.05])
        split_min = int(rng.choice([4, 8, 20, 256]))
        launches = plan(branch, F, staged=staged, deferred=deferred, split_min=split_min)
        order, members = classes_of(F.tolist())
        sheared = [k for k in range(P) if branch[k] == A]
        # every optimiser pair of every class in exactly one launch, in class order
        got = [(L["F"], p) for L in launches for p in L["pos"]]
        want = [(f, q) for f in order for q, k in enumerate(members[f]) if branch[k] == C_]
        assert got == want, (trial, got, want)
        for L in launches:
            assert L["ks"] == sheared[:L["na"]] + [members[L["F"]][p] for p in L["pos"]], trial
            assert L["na"] in (0, len(sheared)) and L["ks"], trial
        # the sheared rows lead exactly one launch of the base class: the first, or with the deferred chain the last
        carriers = [q for q, L in enumerate(launches) if L["na"]]
        base = [q for q, L in enumerate(launches) if L["F"] == 256]
        if sheared:
            assert len(carriers) == 1 and carriers[0] == (base[-1] if deferred else base[0]), (trial, carriers, base)
        else:
            assert not carriers
        # `whole` only when the launch is a buffer as it lies: a class's, or the sheared histograms alone
        for L in launches:
            lies = (L["na"] == 0 and L["pos"] == list(range(len(members[L["F"]])))) or (L["na"] > 0 and not L["pos"])
            assert L["whole"] == lies, (trial, L)
        # without staging, one launch per class (the sheared pairs alone make one where the base class has no optimiser pair)
        if not staged:
            with_c = [f for f in order if any(branch[k] == C_ for k in members[f])]
            alone = bool(sheared) and 256 not in with_c
            assert [L["F"] for L in launches] == with_c + ([256] if alone else []), trial


def letters(s):
    return [{"A": A, "B": B_, "C": C_}[c] for c in s]


# (pairs of a triangle of the block50 fixture, all on the base grid; KOPT_SPLIT_MIN as given; the rows of every launch as
# the timeline of the commit before the split printed them)
TRI13 = "AAAACCCCCCCCAAACCCCCCCCAACCCCCCCCACCCCCCCCCCCCCCCCAAAACCCAAACCCAACCCACCCCCCAAA"
TRI12 = "AAAACCCCCCCAAACCCCCCCAACCCCCCCACCCCCCCCCCCCCCAAAACCAAACCAACCACCCCA"
TRI11 = "AAAACCCCCCAAACCCCCCAACCCCCCACCCCCCCCCCCCAAAACAAACAACACC"
LAYOUTS = [
    ("13 parameters, staged, deferred chain", TRI13, True, True, 8, [39, 39]),
    ("13 parameters, staged, chain joined first", TRI13, True, False, 8, [39, 39]),
    ("12 parameters, staged, deferred chain", TRI12, True, True, 20, [33, 33]),
    ("11 parameters, one blocking launch", TRI11, False, False, 8, [55]),
]


@pytest.mark.parametrize("name,branches,staged,deferred,split_min,rows", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_launch_list_layouts_of_the_previous_commit(name, branches, staged, deferred, split_min, rows):
    branch = letters(branches)
    launches = plan(branch, [256] * len(branch), staged=staged, deferred=deferred, split_min=split_min)
    assert [len(L["ks"]) for L in launches] == rows
    nA = branches.count("A")
    assert [L["na"] for L in launches] == ([0] * (len(rows) - 1) + [nA] if deferred else [nA] + [0] * (len(rows) - 1))

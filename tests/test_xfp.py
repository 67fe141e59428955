"""The exact best-response table and full-width fictitious play (XFP) without a GPU: the ABI
of nfsp_best_response_table / nfsp_xfp_* and its host-side validation, and the numpy
restatements of the two kernels (tests/xfp_ref.py) against the brute-force oracle
(oracle/exploit_oracle.py), which plays full histories and knows nothing of the tree.  The GPU
side holds the kernels to these restatements: tests/test_gpu_xfp.py."""
import ctypes as C

import numpy as np
import pytest

import policy_ref as pr
import xfp_ref as xr

GAMES = {"leduc": 0, "kuhn": 1}
UNIFORM_GAP = {"leduc": 2.31111, "kuhn": 7.0 / 6.0}
_TREES = {}
_RUNS = {}


@pytest.fixture(scope="module")
def trees(pkg):
    import __graft_entry__
    __graft_entry__.build()
    for name, g in GAMES.items():
        if name not in _TREES:
            _TREES[name] = pkg.evaluation.GameTree(g)
    return _TREES


def xfp_run(trees, game, weight, iters):
    """One restated run per (game, weight), computed once and left unchanged."""
    key = (game, weight, iters)
    if key not in _RUNS:
        _RUNS[key] = xr.XfpRef(trees[game], 0.0, weight).run(iters)
    return _RUNS[key]


# ---- ABI ------------------------------------------------------------------------------------
NEW = ["nfsp_best_response_table", "nfsp_xfp_create", "nfsp_xfp_run", "nfsp_xfp_iterations", "nfsp_xfp_average",
       "nfsp_xfp_state", "nfsp_xfp_destroy"]


def test_new_symbols_exported_and_bound(pkg):
    import __graft_entry__
    __graft_entry__.build()
    nat = pkg.native
    L = nat.load()
    for name in NEW:
        assert name in nat.SIGNATURES and hasattr(L, name), name
    assert C.sizeof(nat.XfpCfg) == 16
    assert (nat.XFP_WEIGHT_UNIFORM, nat.XFP_WEIGHT_LINEAR) == (0, 1)
    assert nat.XFP_LAUNCH_ITERS == 1024 and nat.XFP_MAX_RUNS == 1024
    hdr = open(__graft_entry__.REPO + "/include/nfsp.h").read()
    for name, v in (("NFSP_XFP_WEIGHT_UNIFORM", 0), ("NFSP_XFP_WEIGHT_LINEAR", 1), ("NFSP_XFP_LAUNCH_ITERS", 1024),
                    ("NFSP_XFP_MAX_RUNS", 1024)):
        assert f"#define {name} {v}" in " ".join(hdr.split()), name


def test_validation_names_the_field(pkg):
    import __graft_entry__
    __graft_entry__.build()
    nat = pkg.native
    L = nat.load()

    def einval(rc, word):
        assert rc == nat.EINVAL
        assert word.encode() in L.nfsp_last_error(), (word, L.nfsp_last_error())

    h = nat.P()
    cfg = lambda eta=0.0, weight=0, reserved=0, n=1: (nat.XfpCfg * n)(*[nat.XfpCfg(eta, weight, reserved)] * n)  # noqa: E731
    # no rule needs a context, a handle or a device to answer
    einval(L.nfsp_best_response_table(None, None, None, None, None, None), "null")
    einval(L.nfsp_xfp_create(None, None, 1, None), "null")
    einval(L.nfsp_xfp_create(None, cfg(), 1, None), "null")
    einval(L.nfsp_xfp_create(None, cfg(), 1, C.byref(h)), "null")            # the context
    einval(L.nfsp_xfp_create(None, cfg(), 0, C.byref(h)), "n must")
    einval(L.nfsp_xfp_create(None, cfg(), -1, C.byref(h)), "n must")
    einval(L.nfsp_xfp_create(None, cfg(n=2), nat.XFP_MAX_RUNS + 1, C.byref(h)), "n must")
    for eta in (-0.1, 1.0, 1.5, float("nan")):
        einval(L.nfsp_xfp_create(None, cfg(eta=eta), 1, C.byref(h)), "eta")
    for weight in (-1, 2):
        einval(L.nfsp_xfp_create(None, cfg(weight=weight), 1, C.byref(h)), "weight")
    einval(L.nfsp_xfp_create(None, cfg(reserved=1), 1, C.byref(h)), "reserved")
    # the second of two: every cfg is checked
    two = (nat.XfpCfg * 2)(nat.XfpCfg(0.0, 0, 0), nat.XfpCfg(0.0, 0, 7))
    einval(L.nfsp_xfp_create(None, two, 2, C.byref(h)), "reserved")
    assert not h.value
    einval(L.nfsp_xfp_run(None, 1, None), "null")
    einval(L.nfsp_xfp_run(None, -1, None), "iters")
    einval(L.nfsp_xfp_iterations(None, None), "null")
    einval(L.nfsp_xfp_average(None, 0, None), "null")
    einval(L.nfsp_xfp_average(None, -1, None), "run")
    w = nat.F64(0)
    einval(L.nfsp_xfp_state(None, 0, None, None, C.byref(w)), "null")
    einval(L.nfsp_xfp_state(None, -1, None, None, C.byref(w)), "run")
    einval(L.nfsp_xfp_destroy(None), "null")


# ---- the best response restated, against the brute force ---------------------------------------
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
@pytest.mark.parametrize("case", ["seed0", "seed1", "uniform"])
def test_best_response_restatement_attains_the_br_values(trees, game, case):
    t = trees[game]
    p = t.uniform() if case == "uniform" else pr.random_table(t, int(case[-1]))
    beta, q, reach = xr.best_response(t, p, p)
    assert np.array_equal(beta.sum(-1), np.ones((t.ndec, 3))) and set(np.unique(beta)) == {0.0, 1.0}
    assert np.all(beta[~t.legal][:, :, 2] == 0) and np.all(q[~t.legal][:, :, 2] == 0)
    assert np.all(reach >= 0) and reach.max() <= 1.0
    want = pr.walk(t, p, p)
    v0 = pr.walk(t, beta, p)["value0"]
    v1 = -pr.walk(t, p, beta)["value0"]
    print(game, case, "br0", v0 - want["br0"], "br1", v1 - want["br1"])
    assert abs(v0 - want["br0"]) <= 1e-12 and abs(v1 - want["br1"]) <= 1e-12
    assert abs(pr.oracle_table_scores(t, beta, p, keys=("value0",))["value0"] - v0) <= 1e-9
    assert abs(-pr.oracle_table_scores(t, p, beta, keys=("value0",))["value0"] - v1) <= 1e-9
    # the chosen action is the first maximum of the legal action values
    qm =np.where(np.arange(3)[None, None, :] < np.where(t.legal, 3, 2)[:, None, None], q, -np.inf)
    assert np.array_equal(beta.argmax(-1), qm.argmax(-1))


def test_best_response_ties_and_unreached_rows_fold(trees):
    """An opponent that always folds: below its fold nothing is reached, every value there is 0
    and the first maximum is fold; where it has not acted yet the responder's values tie too."""
    t = trees["leduc"]
    fold = np.zeros((t.ndec, 3, 3))
    fold[:, :, 0] = 1.0
    beta, q, reach = xr.best_response(t, fold, fold)
    dead = reach == 0
    assert dead.any() and np.all(beta[dead][:, 0] == 1.0) and np.all(q[dead] == 0.0)
    ties = (q[:, :, 0] == q[:, :, 1]) & (q[:, :, 0] >= np.where(t.legal[:, None], q[:, :, 2], -np.inf))
    assert np.all(beta[ties][:, 0] == 1.0)


# ---- XFP restated, scored by the brute force ------------------------------------------------------
@pytest.mark.parametrize("game,weight,iters,bound", [("kuhn", xr.WEIGHT_UNIFORM, 256, 0.04),
                                                     ("leduc", xr.WEIGHT_UNIFORM, 64, 0.37),
                                                     ("leduc", xr.WEIGHT_LINEAR, 64, 0.24)])
def test_xfp_restatement_converges(trees, game, weight, iters, bound):
    """Measured: kuhn uniform 256 0.02669, leduc uniform 64 0.24427, leduc linear 64 0.15630;
    the bounds are 1.5 x those."""
    t = trees[game]
    ref = xfp_run(trees, game, weight, iters)
    avg = ref.average()
    assert np.abs(avg.sum(-1) - 1.0).max() <= 1e-12 and np.all(avg[~t.legal][:, :, 2] == 0)
    s = pr.oracle_table_scores(t, avg, avg, keys=("br0", "br1"))
    print(game, weight, iters, "exploitability", s["exploitability"])
    assert 0 <= s["exploitability"] < bound
    assert abs(ref.gaps[0] - UNIFORM_GAP[game]) <= 1e-5
    # S is a sum of 0 / 1 plans with integer weights; W is the weights' sum
    assert np.array_equal(ref.S, np.round(ref.S)) and set(np.unique(ref.B)) <= {0.0, 1.0}
    assert ref.W == (iters if weight == xr.WEIGHT_UNIFORM else iters * (iters + 1) // 2)


@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_xfp_gap_is_the_exploitability_of_the_average_before(trees, game):
    """eta = 0: gap_t is the walk's exploitability of the average after t - 1 iterations."""
    t = trees[game]
    ref = xr.XfpRef(t)
    assert np.array_equal(ref.average(), t.uniform())
    for k in range(4):
        a = ref.average()
        ref.run(1)
        assert abs(ref.gaps[k] - pr.walk(t, a, a)["exploitability"]) <= 1e-12, k


def test_xfp_restatement_split_runs_and_anticipation(trees):
    t = trees["kuhn"]
    a, b = xr.XfpRef(t, 0.25, xr.WEIGHT_LINEAR).run(12), xr.XfpRef(t, 0.25, xr.WEIGHT_LINEAR).run(5).run(7)
    assert np.array_equal(a.S, b.S) and np.array_equal(a.B, b.B) and a.gaps == b.gaps and a.W == b.W == 78.0
    plain = xr.XfpRef(t, 0.0, xr.WEIGHT_LINEAR).run(12)
    assert not np.array_equal(a.S, plain.S)          # eta changes the path
    # B is a realisation plan: each seat's root rows put mass 1 on one action
    for d in range(2):
        assert np.array_equal(a.B[int(t.nodes["row"][t.root[d]])].sum(-1), np.ones(3))

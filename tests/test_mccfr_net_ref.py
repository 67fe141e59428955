"""Regret nets on the MCCFR handle without a GPU: the ABI of nfsp_mccfr_net_* with every host-side
refusal of nfsp_mccfr_net_cfgs_check, and the numpy restatement of the rule
(tests/mccfr_net_ref.py) -- both target rules by hand, that with the fit replaced by a copy of
the targets the nets' sigma is regret matching on R, and that sampled regression CFR learns Kuhn.
The GPU side holds k_mccfr_net_apply to the restatement: tests/test_gpu_mccfr_net.py."""
import ctypes as C

import numpy as np
import pytest

import fitnet_ref as fr
import mccfr_net_ref as nr
import mccfr_os_ref as osr
import mccfr_ref as mr
import mccfr_vr_ref as vrr
import policy_ref as pr

GAMES = {"leduc": 0, "kuhn": 1}
EPS = 0.6
KINDS = {0: mr.MccfrRef, 1: osr.OsRef, 2: vrr.VrRef}
_TREES = {}
NEW = ["nfsp_mccfr_net_cfgs_check", "nfsp_mccfr_net_create", "nfsp_mccfr_net_tables", "nfsp_mccfr_net_weights",
       "nfsp_mccfr_net_loss", "nfsp_mccfr_set_timing", "nfsp_mccfr_get_timings"]


@pytest.fixture(scope="module")
def trees(pkg):
    import __graft_entry__
    __graft_entry__.build()
    assert hasattr(pkg.native.load(), "nfsp_mccfr_net_create")
    for name, g in GAMES.items():
        if name not in _TREES:
            _TREES[name] = pkg.evaluation.GameTree(g)
    return _TREES


def solver_nets(pkg, init_seed):
    """The nets evaluation.MccfrNetSolver starts a run from."""
    rng = np.random.RandomState(init_seed)
    return pkg.evaluation.glorot_net(rng), pkg.evaluation.glorot_net(rng)


def make(tree, sampling, seed, walkers, nets, eps=EPS, **kw):
    args = (tree, seed, walkers) + ((eps,) if sampling else ())
    return nr.NetRef(KINDS[sampling])(*args, nets=nets, **kw)


# ---- a. the ABI and its refusals ------------------------------------------------------------------
def test_new_symbols_exported_and_bound(pkg):
    import __graft_entry__
    __graft_entry__.build()
    nat = pkg.native
    L = nat.load()
    for name in NEW:
        assert name in nat.SIGNATURES and hasattr(L, name), name
    X = nat.MccfrNetCfg
    assert C.sizeof(X) == 56
    assert [getattr(X, f).offset for f, _ in X._fields_] == [0, 8, 12, 16, 24, 28, 32, 36, 40, 44, 48, 52]
    assert [f for f, _ in X._fields_] == ["seed", "walkers", "sampling", "epsilon", "regret", "average", "target",
                                          "fit_steps", "loss", "lr", "momentum", "reserved"]
    assert (nat.MCCFR_NET_TARGET_AVG, nat.MCCFR_NET_TARGET_ROWMAX, nat.MCCFR_NET_MAX_STEPS) == (0, 1, 4096)
    assert (nr.AVG, nr.ROWMAX) == (0, 1) and (fr.MSE, fr.HUBER) == (nat.FIT_MSE, nat.FIT_HUBER)
    hdr = " ".join(open(__graft_entry__.REPO + "/include/nfsp.h").read().split())
    for name in NEW:
        assert f"int {name}(" in hdr, name
    for name, v in (("TARGET_AVG", 0), ("TARGET_ROWMAX", 1), ("MAX_STEPS", 4096)):
        assert f"#define NFSP_MCCFR_NET_{name} {v}" in hdr, name
    # the struct's fields, in the header's order, are the mirror's
    body = hdr[hdr.index("#define NFSP_MCCFR_NET_MAX_STEPS"):hdr.index("} nfsp_mccfr_net_cfg;")]
    import re
    body = re.sub(r"/\*.*?\*/", "", body)
    assert re.findall(r"(\w+);", body) == [f for f, _ in X._fields_]
    ev = pkg.evaluation
    assert issubclass(ev.MccfrNetSolver, ev.MccfrXSolver)
    for name in ("run", "counts", "state", "close", "iterations", "sampling"):
        assert getattr(ev.MccfrNetSolver, name) is getattr(ev.MccfrSolver, name), name
    for name in ("rule", "weighted", "average", "average_table", "baseline", "set_baseline"):
        assert getattr(ev.MccfrNetSolver, name) is getattr(ev.MccfrXSolver, name), name
    for name in ("sigma_table", "head", "net", "set_net", "fit_loss", "current", "sigma_tv"):
        assert hasattr(ev.MccfrNetSolver, name) and not hasattr(ev.MccfrXSolver, name), name
    assert ev.MccfrNetSolver.TARGETS == {"avg": 0, "rowmax": 1}


def test_validation_names_the_field_and_the_run(pkg, trees):
    nat = pkg.native
    L = nat.load()
    X = nat.MccfrNetCfg
    check = L.nfsp_mccfr_net_cfgs_check

    def einval(rc, *words):
        assert rc == nat.EINVAL
        for word in words:
            assert word.encode() in L.nfsp_last_error(), (word, L.nfsp_last_error())

    def one(sampling=2, **kw):
        f = dict(seed=1, walkers=64, sampling=sampling, epsilon=EPS if sampling else 0.0, regret=1, average=1, target=1,
                 fit_steps=32, loss=nat.FIT_MSE, lr=0.5, momentum=0.9, reserved=0)
        f.update(kw)
        return X(*[f[name] for name, _ in X._fields_])

    def cfg(n=1, **kw):
        return (X * n)(*[one(**kw)] * n)

    inf, nan = float("inf"), float("nan")
    for g in GAMES.values():
        for sampling in (0, 1, 2):
            assert check(g, cfg(sampling=sampling), 1, 0) == nat.OK
            assert check(g, cfg(sampling=sampling, walkers=2), 1, 1) == nat.OK
            assert check(g, cfg(nat.MCCFR_MAX_RUNS, sampling=sampling, walkers=nat.MCCFR_MAX_WALKERS), nat.MCCFR_MAX_RUNS, 1) == nat.OK
            for regret in (0, 1):
                for average in (0, 1):
                    for target in (0, 1):
                        for loss in (nat.FIT_MSE, nat.FIT_HUBER):
                            assert check(g, cfg(sampling=sampling, regret=regret, average=average, target=target,
                                                loss=loss), 1, 1) == nat.OK
            for steps in (0, 1, nat.MCCFR_NET_MAX_STEPS):
                assert check(g, cfg(sampling=sampling, fit_steps=steps), 1, 1) == nat.OK
            for lr, mu in ((0.0, 0.0), (1e30, float(np.nextafter(np.float32(1), np.float32(0))))):
                assert check(g, cfg(sampling=sampling, lr=lr, momentum=mu), 1, 1) == nat.OK
            for w in (3, 65, nat.MCCFR_MAX_WALKERS - 1):
                einval(check(g, cfg(sampling=sampling, walkers=w), 1, 0), "even", "nfsp_mccfr_net_cfg.walkers", "run 0")
            for w in (1, 0, -2, nat.MCCFR_MAX_WALKERS + 2):
                einval(check(g, cfg(sampling=sampling, walkers=w), 1, 0), "nfsp_mccfr_net_cfg.walkers")
            for v in (-1, 2, 1 << 20):
                einval(check(g, cfg(sampling=sampling, regret=v), 1, 0), "nfsp_mccfr_net_cfg.regret")
                einval(check(g, cfg(sampling=sampling, average=v), 1, 0), "nfsp_mccfr_net_cfg.average")
                einval(check(g, cfg(sampling=sampling, target=v), 1, 0), "nfsp_mccfr_net_cfg.target")
            for v in (-1, nat.FIT_CE, 3, 1 << 20):
                einval(check(g, cfg(sampling=sampling, loss=v), 1, 0), "nfsp_mccfr_net_cfg.loss")
            for v in (-1, nat.MCCFR_NET_MAX_STEPS + 1, 1 << 30):
                einval(check(g, cfg(sampling=sampling, fit_steps=v), 1, 0), "nfsp_mccfr_net_cfg.fit_steps")
            for v in (-1e-3, -inf, inf, nan):
                einval(check(g, cfg(sampling=sampling, lr=v), 1, 0), "nfsp_mccfr_net_cfg.lr")
            for v in (-1e-3, 1.0, 2.0, inf, nan):
                einval(check(g, cfg(sampling=sampling, momentum=v), 1, 0), "nfsp_mccfr_net_cfg.momentum")
            for v in (1, -1):
                einval(check(g, cfg(sampling=sampling, reserved=v), 1, 0), "nfsp_mccfr_net_cfg.reserved")
            # the run is named
            two = (X * 2)(one(sampling=sampling), one(sampling=sampling, fit_steps=-1))
            einval(check(g, two, 2, 0), "nfsp_mccfr_net_cfg.fit_steps", "run 1")
            two = (X * 2)(one(sampling=sampling), one(sampling=(sampling + 1) % 3, epsilon=0.0 if sampling == 2 else EPS))
            einval(check(g, two, 2, 0), "nfsp_mccfr_net_cfg.sampling", "run 1", "run 0")
        for sampling in (1, 2):
            for eps in (nat.MCCFR_OS_EPS_MIN, 1.0):
                assert check(g, cfg(sampling=sampling, epsilon=eps), 1, 1) == nat.OK
            for eps in (0.0, -0.5, np.nextafter(nat.MCCFR_OS_EPS_MIN, 0.0), np.nextafter(1.0, 2.0), 2.0, inf, nan):
                einval(check(g, cfg(sampling=sampling, epsilon=eps), 1, 0), "nfsp_mccfr_net_cfg.epsilon")
        for eps in (EPS, 1.0, -0.5, 5e-324, inf, nan):              # external sampling has no epsilon
            einval(check(g, cfg(sampling=0, epsilon=eps), 1, 0), "nfsp_mccfr_net_cfg.epsilon", "sampling 0")
        for sampling in (-1, 3, 1 << 20):
            einval(check(g, cfg(sampling=sampling, epsilon=EPS), 1, 0), "nfsp_mccfr_net_cfg.sampling")
        for n in (0, -1, nat.MCCFR_MAX_RUNS + 1):
            einval(check(g, cfg(2), n, 0), "n must")
        einval(check(g, cfg(), 1, -1), "iters")
    einval(check(2, cfg(), 1, 0), "game")
    einval(check(0, None, 1, 0), "null")
    # the overflow bound is the sampling kind's own: the nets do not enter
    t = trees["leduc"]
    bounds = (int(2.0 ** 62 / (mr.Q * 2.0 * float(np.abs(t.pay).max()))), osr.bound(t, 0.0625), vrr.bound(t, 0.0625))
    for sampling, bound in enumerate(bounds):
        eps = 0.0625 if sampling else 0.0
        assert check(0, cfg(sampling=sampling, walkers=2, epsilon=eps), 1, bound // 2) == nat.OK
        einval(check(0, cfg(sampling=sampling, walkers=2, epsilon=eps), 1, bound // 2 + 1), "overflow", str(bound))
    # the handle's calls refuse a null handle without a device
    p = nat.P()
    out = (nat.F64 * 4)()
    einval(L.nfsp_mccfr_net_tables(None, 0, C.byref(p), None, None), "null")
    einval(L.nfsp_mccfr_net_weights(None, 0, 0, C.byref(p), None), "null")
    einval(L.nfsp_mccfr_net_loss(None, 0, out), "null")
    einval(L.nfsp_mccfr_net_create(None, cfg(), 1, None, C.byref(p)), "null")


# ---- b. the targets by hand ---------------------------------------------------------------------------
def test_both_target_rules_by_hand_on_two_rows(trees):
    """One row with an illegal raise whose R entry is the row's largest -- it must not enter m and its
    target is 0 -- and one row of zeros (m = 0)."""
    t = trees["leduc"]
    d_no = int(np.nonzero(~t.legal)[0][0])             # a decision where the raise is illegal
    d_yes = int(np.nonzero(t.legal)[0][0])
    R = np.zeros((t.ndec, 3, 3), np.int64)
    R[d_no, 1] = [-3 << 24, 1 << 24, 99 << 24]
    R[d_yes, 2] = [5 << 24, -10 << 24, 2 << 24]
    W, tw = 64, 3.0
    y = nr.targets(t, R, W, tw, nr.AVG)
    assert y.dtype == np.float64 and y.shape == R.shape
    assert list(y[d_no, 1]) == [-3.0 / (64 * 3), 1.0 / (64 * 3), 0.0]
    assert list(y[d_yes, 2]) == [5.0 / 192, -10.0 / 192, 2.0 / 192]
    assert not y[d_no, 0].any() and not y[d_yes, 0].any()
    y = nr.targets(t, R, W, tw, nr.ROWMAX)
    assert list(y[d_no, 1]) == [-1.0, 1.0 / 3.0, 0.0]              # m = 3 chips: the illegal 99 is not seen
    assert list(y[d_yes, 2]) == [0.5, -1.0, 0.2]
    assert not y[d_no, 0].any() and not y[d_no, 2].any()           # m = 0: zeros, not NaN
    assert np.isfinite(y).all()
    # AVG's denominator is ((double)W * Q) * tw, in that order
    R[d_yes, 0] = [7, 11, 13]
    y = nr.targets(t, R, 6, 7.0, nr.AVG)
    assert list(y[d_yes, 0]) == [7.0 / ((6.0 * mr.Q) * 7.0), 11.0 / ((6.0 * mr.Q) * 7.0), 13.0 / ((6.0 * mr.Q) * 7.0)]
    # sigma from heads: negative heads and an illegal raise count as 0, an all-nonpositive row is uniform over the legal
    z = np.zeros(R.shape, np.float32)
    z[d_no, 1] = [-1.0, 0.25, 7.0]
    z[d_yes, 2] = [1.0, -2.0, 3.0]
    z[d_yes, 1] = [-1.0, -2.0, 0.0]
    sg = nr.sigma_of(t, z)
    assert list(sg[d_no, 1]) == [0.0, 1.0, 0.0] and list(sg[d_yes, 2]) == [0.25, 0.0, 0.75]
    assert list(sg[d_yes, 1]) == [1.0 / 3.0] * 3 and list(sg[d_no, 0]) == [0.5, 0.5, 0.0]


# ---- c. with a perfect fit it is the table's run ---------------------------------------------------------
@pytest.mark.parametrize("target", [nr.AVG, nr.ROWMAX])
@pytest.mark.parametrize("sampling", [0, 1, 2])
@pytest.mark.parametrize("game,walkers", [("kuhn", 64), ("leduc", 32)])
def test_with_the_fit_replaced_by_a_copy_sigma_is_regret_matching(pkg, trees, game, walkers, sampling, target):
    """head_hook returns the targets themselves (f64): both scalings are positive per row, so the sigma of
    either target kind is match(R) within rounding, after every half-iteration of 3 iterations."""
    t = trees[game]
    seen = []

    def copy(i, y):
        d, r = fr.seat_sets(t, i)
        return y[d, r]
    r = make(t, sampling, 5, walkers, solver_nets(pkg, 3), target=target, fit_steps=4, regret=1, head_hook=copy)
    assert np.array_equal(r.sigma(), t.uniform())              # R = 0: targets 0, the rows uniform
    for it in range(3):
        for i in (0, 1):
            r.half(i)
            d, rk = fr.seat_sets(t, i)
            err = np.abs(r.sigma() - r.sigma_tab())[d, rk].max()
            seen.append(err)
            assert err <= 1e-12, (it, i, err)
        r.t += 1
    assert np.abs(r.sigma() - mr.match(t, r.R)).max() <= 1e-12 and r.R.any()
    print(game, sampling, target, "largest |sigma - match(R)|", max(seen))


def test_the_sigma_hook_supplies_what_a_half_iteration_reads(pkg, trees):
    """With the hook returning the tabular run's sigma, the integer tables are the tabular run's, bit for
    bit, whatever the nets do; without it they are not."""
    import mccfr_x_ref as xr
    t = trees["kuhn"]
    tab = xr.XRef(mr.MccfrRef)(t, 9, 64)
    net = make(t, 0, 9, 64, solver_nets(pkg, 1), fit_steps=2)
    free = make(t, 0, 9, 64, solver_nets(pkg, 1), fit_steps=2)
    net.sigma_hook = lambda i: mr.match(t, net.R)
    for _ in range(2):
        tab.run(1)
        net.run(1)
        free.run(1)
        assert np.array_equal(tab.R, net.R) and np.array_equal(tab.S, net.S) and tab.terminals == net.terminals
    assert not np.array_equal(tab.R, free.R)


# ---- d. it learns ------------------------------------------------------------------------------------------
def test_sampled_regression_cfr_learns_kuhn(pkg, trees):
    """External sampling, seed 1, W 64, K 32, lr 0.5, momentum 0.9, MSE, AVG, 64 iterations, from the nets
    MccfrNetSolver makes of init seed 1: the average's exploitability is at most a quarter of the uniform
    policy's, tests/test_mccfr_ref.py's own cap (the table reaches 0.0427 there).  Measured: 0.0721, the
    mean total variation between the nets' sigma and regret matching on R 0.0135."""
    t = trees["kuhn"]
    cap = 0.2917
    u = t.uniform()
    assert abs(pr.walk(t, u, u)["exploitability"] - 4 * cap) <= 5e-4
    r = make(t, 0, 1, 64, solver_nets(pkg, 1), target=nr.AVG, fit_steps=32, loss=fr.MSE, lr=0.5, momentum=0.9).run(64)
    avg = r.average()
    x = pr.walk(t, avg, avg)["exploitability"]
    tv = 0.5 * np.abs(r.sigma() - r.sigma_tab()).sum(axis=2).mean()
    print("kuhn net-mccfr exploitability", x, "sigma_tv", tv, "fit_loss", r.fit_loss.tolist())
    assert x <= cap

"""Regret matching+ and linear averaging on the MCCFR handle without a GPU: the ABI of
nfsp_mccfr_x_* with its host-side refusals, the overflow bound (the sampling kind's own), and the
numpy restatement of the rule (tests/mccfr_x_ref.py) -- that under REGRET_PLAIN it is the base
restatement's run, that the floor is exercised, that Sw is the exact integer sum at these sizes,
and that at a large W the plus rule with the linear average gets below the plain rule with the
uniform one.  The GPU side holds k_mccfr_x_apply to the restatement bit for bit:
tests/test_gpu_mccfr_x.py."""
import ctypes as C

import numpy as np
import pytest

import mccfr_os_ref as osr
import mccfr_ref as mr
import mccfr_vr_ref as vrr
import mccfr_x_ref as xr
import policy_ref as pr

GAMES = {"leduc": 0, "kuhn": 1}
EPS = 0.6
KINDS = {0: mr.MccfrRef, 1: osr.OsRef, 2: vrr.VrRef}
_TREES = {}


@pytest.fixture(scope="module")
def trees(pkg):
    import __graft_entry__
    __graft_entry__.build()
    # the restatement restates this library's rule: without its entry points there is nothing to hold to it
    assert hasattr(pkg.native.load(), "nfsp_mccfr_x_create")
    for name, g in GAMES.items():
        if name not in _TREES:
            _TREES[name] = pkg.evaluation.GameTree(g)
    return _TREES


def make(tree, sampling, seed, walkers, eps=EPS, regret=xr.PLAIN, average=xr.UNIFORM):
    args = (tree, seed, walkers) + ((eps,) if sampling else ())
    return xr.XRef(KINDS[sampling])(*args, regret=regret, average=average)


def base(tree, sampling, seed, walkers, eps=EPS):
    return KINDS[sampling](*((tree, seed, walkers) + ((eps,) if sampling else ())))


# ---- a. the ABI and its refusals ------------------------------------------------------------------
NEW = ["nfsp_mccfr_x_cfgs_check", "nfsp_mccfr_x_create", "nfsp_mccfr_rule", "nfsp_mccfr_average_of",
       "nfsp_mccfr_weighted"]


def test_new_symbols_exported_and_bound(pkg):
    import __graft_entry__
    __graft_entry__.build()
    nat = pkg.native
    L = nat.load()
    for name in NEW:
        assert name in nat.SIGNATURES and hasattr(L, name), name
    X = nat.MccfrXCfg
    assert C.sizeof(X) == 32
    assert [getattr(X, f).offset for f, _ in X._fields_] == [0, 8, 12, 16, 24, 28]
    assert [f for f, _ in X._fields_] == ["seed", "walkers", "sampling", "epsilon", "regret", "average"]
    assert (nat.MCCFR_REGRET_PLAIN, nat.MCCFR_REGRET_PLUS, nat.MCCFR_AVG_UNIFORM, nat.MCCFR_AVG_LINEAR) == (0, 1, 0, 1)
    hdr = " ".join(open(__graft_entry__.REPO + "/include/nfsp.h").read().split())
    for name in NEW:
        assert f"int {name}(" in hdr, name
    for name, v in (("REGRET_PLAIN", 0), ("REGRET_PLUS", 1), ("AVG_UNIFORM", 0), ("AVG_LINEAR", 1)):
        assert f"#define NFSP_MCCFR_{name} {v}" in hdr, name
    ev = pkg.evaluation
    assert issubclass(ev.MccfrXSolver, ev.MccfrSolver)
    for name in ("run", "counts", "state", "close", "iterations", "sampling"):
        assert getattr(ev.MccfrXSolver, name) is getattr(ev.MccfrSolver, name), name
    for name in ("baseline", "set_baseline", "baseline_table"):
        assert getattr(ev.MccfrXSolver, name) is getattr(ev.MccfrVrSolver, name), name
    for name in ("rule", "weighted"):
        assert hasattr(ev.MccfrXSolver, name) and not hasattr(ev.MccfrVrSolver, name), name
    assert ev.MccfrXSolver.REGRETS == {"plain": 0, "plus": 1} and ev.MccfrXSolver.AVERAGES == {"uniform": 0, "linear": 1}


def test_validation_names_the_field(pkg, trees):
    nat = pkg.native
    L = nat.load()
    X = nat.MccfrXCfg

    def einval(rc, *words):
        assert rc == nat.EINVAL
        for word in words:
            assert word.encode() in L.nfsp_last_error(), (word, L.nfsp_last_error())

    def cfg(walkers=64, sampling=2, n=1, seed=1, eps=None, regret=1, average=1):
        eps = (EPS if sampling else 0.0) if eps is None else eps
        return (X * n)(*[X(seed, walkers, sampling, eps, regret, average)] * n)

    check = L.nfsp_mccfr_x_cfgs_check
    for g in GAMES.values():
        for sampling in (0, 1, 2):
            assert check(g, cfg(sampling=sampling), 1, 0) == nat.OK
            assert check(g, cfg(2, sampling=sampling), 1, 1) == nat.OK
            assert check(g, cfg(nat.MCCFR_MAX_WALKERS, sampling, n=nat.MCCFR_MAX_RUNS), nat.MCCFR_MAX_RUNS, 1) == nat.OK
            for regret in (0, 1):
                for average in (0, 1):
                    assert check(g, cfg(sampling=sampling, regret=regret, average=average), 1, 1) == nat.OK
            for w in (3, 65, nat.MCCFR_MAX_WALKERS - 1):
                einval(check(g, cfg(w, sampling), 1, 0), "even", "nfsp_mccfr_x_cfg.walkers")
            for w in (1, 0, -2, nat.MCCFR_MAX_WALKERS + 2):
                einval(check(g, cfg(w, sampling), 1, 0), "nfsp_mccfr_x_cfg.walkers")
            for v in (-1, 2, 1 << 20):
                einval(check(g, cfg(sampling=sampling, regret=v), 1, 0), "nfsp_mccfr_x_cfg.regret")
                einval(check(g, cfg(sampling=sampling, average=v), 1, 0), "nfsp_mccfr_x_cfg.average")
        for sampling in (1, 2):
            for eps in (nat.MCCFR_OS_EPS_MIN, 1.0):
                assert check(g, cfg(sampling=sampling, eps=eps), 1, 1) == nat.OK
            for eps in (0.0, -0.5, np.nextafter(nat.MCCFR_OS_EPS_MIN, 0.0), np.nextafter(1.0, 2.0), 2.0, float("inf"),
                        float("nan")):
                einval(check(g, cfg(sampling=sampling, eps=eps), 1, 0), "nfsp_mccfr_x_cfg.epsilon")
        for eps in (EPS, 1.0, -0.5, 5e-324, float("inf"), float("nan")):      # external sampling has no epsilon
            einval(check(g, cfg(sampling=0, eps=eps), 1, 0), "nfsp_mccfr_x_cfg.epsilon", "sampling 0")
        for sampling in (-1, 3, 1 << 20):
            einval(check(g, cfg(sampling=sampling, eps=EPS), 1, 0), "nfsp_mccfr_x_cfg.sampling")
        for n in (0, -1, nat.MCCFR_MAX_RUNS + 1):
            einval(check(g, cfg(n=2), n, 0), "n must")
        einval(check(g, None, 1, 0), "null")
        einval(check(g, cfg(), 1, -1), "iters")
        # the second and third of three: every cfg is checked, and a handle has one sampling kind
        einval(check(g, (X * 2)(X(1, 64, 2, EPS, 1, 1), X(2, 63, 2, EPS, 1, 1)), 2, 0), "even")
        einval(check(g, (X * 2)(X(1, 64, 1, EPS, 1, 1), X(2, 64, 1, 0.01, 1, 1)), 2, 0), "epsilon")
        einval(check(g, (X * 2)(X(1, 64, 1, EPS, 0, 0), X(2, 64, 1, EPS, 0, 2)), 2, 0), "nfsp_mccfr_x_cfg.average")
        for first, other in ((2, 1), (1, 2), (0, 1), (1, 0)):
            arr = (X * 3)(X(1, 64, first, EPS if first else 0.0, 1, 1), X(2, 64, first, EPS if first else 0.0, 0, 0),
                          X(3, 64, other, EPS if other else 0.0, 1, 1))
            einval(check(g, arr, 3, 0), "nfsp_mccfr_x_cfg.sampling", "run 2")
            assert check(g, arr, 2, 0) == nat.OK                # regret and average may differ per run
    einval(check(2, cfg(), 1, 0), "game")
    # no rule needs a context, a handle or a device to answer
    h = nat.P()
    einval(L.nfsp_mccfr_x_create(None, None, 1, None), "null")
    einval(L.nfsp_mccfr_x_create(None, cfg(), 1, C.byref(h)), "null")              # the context
    einval(L.nfsp_mccfr_x_create(None, cfg(), 0, C.byref(h)), "n must")
    assert not h.value
    z = np.zeros((trees["kuhn"].ndec, 3, 3))
    out = (nat.I32 * 2)(7, 7)
    p = nat.P()
    einval(L.nfsp_mccfr_rule(None, 0, out), "null")
    einval(L.nfsp_mccfr_rule(None, -1, out), "run")
    einval(L.nfsp_mccfr_average_of(None, 0, 1, C.byref(p)), "null")
    einval(L.nfsp_mccfr_average_of(None, -1, 1, C.byref(p)), "run")
    einval(L.nfsp_mccfr_weighted(None, 0, z.ctypes.data_as(nat.P)), "null")
    einval(L.nfsp_mccfr_weighted(None, -1, z.ctypes.data_as(nat.P)), "run")
    assert not z.any() and tuple(out) == (7, 7) and not p.value


# ---- b. the bound is the sampling kind's ------------------------------------------------------------
def es_bound(tree):
    return int(2.0 ** 62 / (mr.Q * 2.0 * max(float(np.abs(tree.pay).max()), 1.0)))


@pytest.mark.parametrize("sampling", [0, 1, 2])
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_overflow_bound_is_the_sampling_kinds(pkg, trees, game, sampling):
    """|max(R + dR, 0)| <= |R| + |dR|: the floor moves no entry further from 0, so the bound on the sum of
    |dR| still bounds R, whatever the rule; Sw is f64 and needs none."""
    nat = pkg.native
    L = nat.load()
    t = trees[game]
    for eps in ((0.0,) if sampling == 0 else (0.0625, EPS, 1.0)):
        bound = (es_bound(t), osr.bound(t, eps) if sampling else 0, vrr.bound(t, eps) if sampling else 0)[sampling]
        for w in (2, 1 << 10, nat.MCCFR_MAX_WALKERS):
            for regret, average in ((0, 0), (1, 1)):
                arr = (nat.MccfrXCfg * 1)(nat.MccfrXCfg(1, w, sampling, eps, regret, average))
                assert L.nfsp_mccfr_x_cfgs_check(GAMES[game], arr, 1, bound // w) == nat.OK
                assert L.nfsp_mccfr_x_cfgs_check(GAMES[game], arr, 1, bound // w + 1) == nat.EINVAL
                msg = L.nfsp_last_error()
                assert b"overflow" in msg and str(bound).encode() in msg, msg
            # and it is the old kind's own answer
            old = {0: (L.nfsp_mccfr_cfgs_check, lambda: (nat.MccfrCfg * 1)(nat.MccfrCfg(1, w, 0))),
                   1: (L.nfsp_mccfr_os_cfgs_check, lambda: (nat.MccfrOsCfg * 1)(nat.MccfrOsCfg(1, w, 0, eps))),
                   2: (L.nfsp_mccfr_vr_cfgs_check, lambda: (nat.MccfrVrCfg * 1)(nat.MccfrVrCfg(1, w, 0, eps)))}[sampling]
            assert old[0](GAMES[game], old[1](), 1, bound // w) == nat.OK
            assert old[0](GAMES[game], old[1](), 1, bound // w + 1) == nat.EINVAL


def test_budgets_written_down(trees):
    """The budgets include/nfsp.h quotes for Leduc at eps = 0.6: outcome sampling's and the baselines'."""
    assert osr.bound(trees["leduc"], 0.6) == 197912092
    assert vrr.bound(trees["leduc"], 0.6) == 29142433


# ---- c. the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", [0, 1, 2])
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_plain_is_the_base_restatement(trees, game, sampling):
    """REGRET_PLAIN with either average, W = 66, 3 iterations: R, S, the counts and Bs / Bn are the base
    restatement's; the average named UNIFORM is its average."""
    t = trees[game]
    want = base(t, sampling, 5, 66).run(3)
    for average in (xr.UNIFORM, xr.LINEAR):
        got = make(t, sampling, 5, 66, regret=xr.PLAIN, average=average).run(3)
        assert np.array_equal(got.R, want.R) and np.array_equal(got.S, want.S)
        assert (got.t, got.traversals, got.terminals) == (want.t, want.traversals, want.terminals) == (3, 396, want.terminals)
        if sampling == 2:
            assert np.array_equal(got.Bs, want.Bs) and np.array_equal(got.Bn, want.Bn) and got.Bn.any()
        assert np.array_equal(got.average(xr.UNIFORM), want.average())
        assert np.array_equal(got.average(), got.average(average))
    assert (want.R < 0).any()                              # the plain rule keeps negative regrets


@pytest.mark.parametrize("sampling", [0, 1, 2])
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_plus_floors_the_regrets(trees, game, sampling):
    """REGRET_PLUS, W = 66: R >= 0 everywhere after every half-iteration.  In iteration 1 both runs start from
    R = 0 and sigma reads only max(R, 0), so they walk the same paths and add the same dR: R differs after
    iteration 1 exactly on the entries the plain run leaves negative -- those are the named entries, and the
    plus run holds 0 there.  From iteration 2 on a floored entry that gains regret turns positive at once
    where the plain run's is still in debt, sigma differs, and the runs part."""
    t = trees[game]
    plain = make(t, sampling, 5, 66, regret=xr.PLAIN)
    plus = make(t, sampling, 5, 66, regret=xr.PLUS)
    for i in (0, 1):
        plain.half(i)
        plus.half(i)
        assert np.array_equal(plus.sigma(), plain.sigma()) and np.array_equal(plus.S, plain.S)
        assert (plus.R >= 0).all() and np.array_equal(plus.R, np.maximum(plain.R, 0))
    plain.t += 1
    plus.t += 1
    floored = plain.R < 0                                   # the entries the floor acted on
    seats = set(t.seat[np.argwhere(floored)[:, 0]].tolist())
    print(game, sampling, "entries floored in iteration 1:", int(floored.sum()), "of", floored.size)
    assert floored.sum() >= 6 and seats == {0, 1}
    assert np.array_equal(plus.R != plain.R, floored) and np.all(plus.R[floored] == 0)
    if sampling == 2:
        assert np.array_equal(plus.Bs, plain.Bs) and np.array_equal(plus.Bn, plain.Bn)
    plain.run(1)
    plus.run(1)
    assert (plus.R >= 0).all() and (plain.R < 0).any()
    assert not np.array_equal(plus.R, np.maximum(plain.R, 0))     # no longer a floor of the plain run
    assert not np.array_equal(plus.sigma(), plain.sigma())
    plus.run(1)
    assert plus.t == 3 and (plus.R >= 0).all()


@pytest.mark.parametrize("regret", [xr.PLAIN, xr.PLUS])
@pytest.mark.parametrize("sampling", [0, 1, 2])
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_weighted_sum_is_the_exact_integer_sum(trees, game, sampling, regret):
    """Sw after 3 iterations against sum (t + 1) dS_t in Python integers, dS_t taken per half-iteration from
    S.  Every term and every partial sum is below 2^53 here (asserted), so the f64 sum is exact."""
    t = trees[game]
    r = make(t, sampling, 7, 66, regret=regret, average=xr.LINEAR)
    exact = np.zeros(r.S.shape, object)
    most = 0
    for it in range(3):
        for i in (0, 1):
            before = r.S.copy()
            r.half(i)
            dS = (r.S - before).astype(object)
            assert (dS >= 0).all()
            exact = exact + (it + 1) * dS
            most = max(most, int(exact.max()))
        r.t += 1
    assert 0 < most < 2 ** 53                               # dS >= 0: the largest partial sum is the last
    assert r.Sw.dtype == np.float64
    assert np.array_equal(r.Sw, exact.astype(np.float64))
    assert all(int(x) == y for x, y in zip(r.Sw.ravel(), exact.ravel()))
    assert not np.array_equal(r.Sw, r.S.astype(np.float64)) and r.Sw.any()
    lin, uni = r.average(xr.LINEAR), r.average(xr.UNIFORM)
    assert np.array_equal(r.average(), lin) and not np.array_equal(lin, uni)
    for avg in (lin, uni):
        assert np.abs(avg.sum(-1) - 1.0).max() <= 1e-12 and np.all(avg[~t.legal][:, :, 2] == 0)


# ---- d. at a large W the plus rule with the linear average is ahead -------------------------------------
def test_plus_linear_is_below_plain_uniform_at_a_large_w(trees):
    """External sampling on Kuhn, W = 4,096, 32 iterations, seeds 1-4: as W grows the mini-batch rule tends to
    CFR+ itself, and plus / linear ends below plain / uniform from the same seeds, for every seed.
    Measured exploitability, plain / uniform against plus / linear: 0.0295 / 0.0090, 0.0370 / 0.0228,
    0.0353 / 0.0120, 0.0395 / 0.0172 (the other two pairs lie between: plus / uniform 0.0330, 0.0342, 0.0321,
    0.0339; plain / linear 0.0153, 0.0333, 0.0218, 0.0342).  The sizes were chosen with this restatement: at the
    W = 16,384 and 64 iterations first tried the gap is wider (0.0186 / 0.0065, 0.0179 / 0.0069, 0.0191 /
    0.0068, 0.0186 / 0.0080) but a seed takes 16 s of numpy; at W = 2,048, 32 iterations it still holds for
    every seed (the closest 0.0370 / 0.0197)."""
    t = trees["kuhn"]
    for seed in (1, 2, 3, 4):
        plain = make(t, 0, seed, 4096, regret=xr.PLAIN, average=xr.UNIFORM).run(32)
        plus = make(t, 0, seed, 4096, regret=xr.PLUS, average=xr.LINEAR).run(32)
        a, b = plain.average(), plus.average()
        x = [pr.walk(t, p, p)["exploitability"] for p in (a, b)]
        print("kuhn ES W = 4096, 32 iterations, seed", seed, "plain / uniform", x[0], "plus / linear", x[1])
        assert 0 <= x[1] < x[0]

"""nfsp_mccfr_x_* (csrc/mccfr.hip k_mccfr_x_apply behind the three unchanged walks) on the GPU
against the numpy restatement of the rule (tests/mccfr_x_ref.py), as tests/test_gpu_mccfr_vr.py
holds the baselines to theirs.  R, S, Bs and Bn are int64 sums of per-walker integers and Sw is an
f64 sum accumulated by one owner in stream order, so all of them and both counts are compared bit
for bit, whatever the grid -- Sw as its 64 bits.  With REGRET_PLAIN the handle is also held to the
handle of the old create call, device against device: the shared paths did not move."""
import ctypes as C

import numpy as np
import pytest

import mccfr_os_ref as osr
import mccfr_ref as mr
import mccfr_vr_ref as vrr
import mccfr_x_ref as xr
import policy_ref as pr

pytestmark = pytest.mark.gpu
NAMES = {0: "leduc", 1: "kuhn"}
KINDS = {0: mr.MccfrRef, 1: osr.OsRef, 2: vrr.VrRef}
EPS = 0.6
PAIRS = [(xr.PLAIN, xr.UNIFORM), (xr.PLAIN, xr.LINEAR), (xr.PLUS, xr.UNIFORM), (xr.PLUS, xr.LINEAR)]
_REFS = {}


@pytest.fixture(scope="module")
def ev(pkg):
    import torch  # noqa: F401  (before libnfsp: the process must end up with one HIP runtime, torch's)
    pkg.native.lib()
    return pkg.evaluation


@pytest.fixture(scope="module")
def ctxs(pkg, ev):
    return {g: pkg.native.Context(1, game=g) for g in (0, 1)}


@pytest.fixture(scope="module")
def trees(ev):
    return {g: ev.GameTree(g) for g in (0, 1)}


def eps_of(sampling, eps=EPS):
    return eps if sampling else 0.0


def new_ref(tree, sampling, seed, walkers, eps, regret):
    args = (tree, seed, walkers) + ((eps,) if sampling else ())
    return xr.XRef(KINDS[sampling])(*args, regret=regret)


def snapshot(r):
    z = np.zeros_like(r.R)
    return {"R": r.R.copy(), "S": r.S.copy(), "Sw": r.Sw.copy(), "Bs": getattr(r, "Bs", z).copy(),
            "Bn": getattr(r, "Bn", z).copy(), "counts": (r.traversals, r.terminals), "t": r.t,
            "avg": {w: r.average(w) for w in (xr.UNIFORM, xr.LINEAR)}}


def restore(r, snap):
    r.R, r.S, r.Sw, r.t, r.terminals = snap["R"].copy(), snap["S"].copy(), snap["Sw"].copy(), snap["t"], snap["counts"][1]
    if hasattr(r, "Bs"):
        r.Bs, r.Bn = snap["Bs"].copy(), snap["Bn"].copy()
    return r


def ref_after(trees, game, sampling, seed, walkers, eps, regret, iters):
    """The restatement's tables after 1 .. iters iterations: computed once per run and left unchanged.
    The average a cfg names changes no table, so a reference serves both."""
    key = (game, sampling, seed, walkers, eps, regret)
    have = _REFS.setdefault(key, [])
    r = None
    while len(have) < iters:
        if r is None:
            r = new_ref(trees[game], sampling, seed, walkers, eps, regret)
            if have:
                restore(r, have[-1])
        r.run(1)
        have.append(snapshot(r))
    return have[iters - 1]


def bits(x):
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float64
    return x.view(np.uint64)


def same(solver, run, want, what, sampling):
    R, S = solver.state(run)
    Sw = solver.weighted(run)
    assert R.dtype == S.dtype == np.int64 and Sw.dtype == np.float64
    got = [R, S, bits(Sw)]
    ref = [want["R"], want["S"], bits(want["Sw"])]
    if sampling == 2:
        got += list(solver.baseline(run))
        ref += [want["Bs"], want["Bn"]]
    bad = tuple(int((g != r).sum()) for g, r in zip(got, ref))
    assert not any(bad), (what, "entries of R, S, Sw (as uint64)[, Bs, Bn] that differ", bad)
    assert solver.counts(run) == want["counts"], what


# ---- the bits --------------------------------------------------------------------------------------------
def walkers_cases(nat):
    B = nat.MCCFR_WG_WALKERS
    return [2, 62, 64, 66, B - 2, B, B + 2, 2 * B + 2]


@pytest.mark.parametrize("case", range(8))
@pytest.mark.parametrize("sampling", [0, 1, 2])
@pytest.mark.parametrize("game", [1, 0])
def test_tables_and_counts_equal_the_restatement(pkg, ev, ctxs, trees, game, sampling, case):
    """W = 2, 62, 64, 66, 1,022, 1,024, 1,026 and 2,050: around a wave, around a workgroup's walkers and
    past two workgroups; the four (regret, average) pairs as four runs of one handle with one seed (two
    restatements serve them: the average named changes no table); after 1, 2 and 3 iterations, each
    continued from the one before."""
    assert walkers_cases(pkg.native) == [2, 62, 64, 66, 1022, 1024, 1026, 2050]
    W, seed, eps = walkers_cases(pkg.native)[case], 11 + case, eps_of(sampling)
    t = trees[game]
    s = ev.MccfrXSolver(ctxs[game], [(seed, W, eps, reg, avg) for reg, avg in PAIRS], sampling)
    assert s.sampling == sampling and [s.rule(k) for k in range(4)] == PAIRS
    z = np.zeros((t.ndec, 3, 3), np.int64)
    zero = {"R": z, "S": z, "Sw": z.astype(np.float64), "Bs": z, "Bn": z, "counts": (0, 0)}
    for k in range(4):
        same(s, k, zero, "at creation", sampling)
        for which in (None, xr.UNIFORM, xr.LINEAR):
            assert np.array_equal(s.average_table(k, which), t.uniform())
    for it in (1, 2, 3):
        s.run(1)
        assert s.iterations == it
        for k, (reg, avg) in enumerate(PAIRS):
            want = ref_after(trees, game, sampling, seed, W, eps, reg, it)
            assert want["counts"][0] == 2 * W * it
            same(s, k, want, (NAMES[game], sampling, W, PAIRS[k], it), sampling)
    for k, (reg, avg) in enumerate(PAIRS):
        want = ref_after(trees, game, sampling, seed, W, eps, reg, 3)
        if reg == xr.PLUS:
            assert (s.state(k)[0] >= 0).all()
        for which in (xr.UNIFORM, xr.LINEAR):
            assert np.abs(s.average_table(k, which) - want["avg"][which]).max() <= 1e-15
        assert np.array_equal(s.average_table(k), s.average_table(k, avg))
        if sampling == 2:
            assert np.array_equal(s.baseline_table(k), vrr.baseline_table(t, want["Bs"], want["Bn"]))
    plain, plus = (ref_after(trees, game, sampling, seed, W, eps, reg, 3) for reg in (xr.PLAIN, xr.PLUS))
    assert (plain["R"] < 0).any() and not np.array_equal(plain["R"], plus["R"])     # the floor was met
    s.close()


@pytest.mark.parametrize("eps", [0.0625, 1.0])
@pytest.mark.parametrize("sampling", [1, 2])
@pytest.mark.parametrize("game", [1, 0])
def test_tables_at_the_ends_of_epsilon(pkg, ev, ctxs, trees, game, sampling, eps):
    """W = 66, plus / linear, at the least exploration rate (the largest increments) and at 1."""
    s = ev.MccfrXSolver(ctxs[game], [(14, 66, eps, "plus", "linear")], sampling).run(3)
    same(s, 0, ref_after(trees, game, sampling, 14, 66, eps, xr.PLUS, 3), (NAMES[game], sampling, eps), sampling)
    s.close()


# ---- the shared paths did not move -------------------------------------------------------------------------
def old_solver(ev, ctx, sampling, cfgs):
    if sampling == 0:
        return ev.MccfrSolver(ctx, [(seed, W) for seed, W, _ in cfgs])
    return (ev.MccfrOsSolver, ev.MccfrVrSolver)[sampling - 1](ctx, cfgs)


@pytest.mark.parametrize("sampling", [0, 1, 2])
@pytest.mark.parametrize("game", [1, 0])
def test_plain_equals_the_handle_of_the_old_create_call(pkg, ev, ctxs, trees, game, sampling):
    """REGRET_PLAIN with either average against nfsp_mccfr_create / _os_create / _vr_create with the same
    seed, W and eps, device against device, after 1, 2 and 3 iterations: R, S, the counts, Bs / Bn, and the
    uniform average bit for bit (k_mccfr_x_apply forms it by k_mccfr_apply's operations)."""
    B = pkg.native.MCCFR_WG_WALKERS
    eps = eps_of(sampling)
    base = [(31, 66, eps), (32, B + 2, eps)]
    old = old_solver(ev, ctxs[game], sampling, base)
    new = ev.MccfrXSolver(ctxs[game], [(seed, W, e, "plain", avg) for seed, W, e in base for avg in ("uniform", "linear")],
                          sampling)
    for it in (1, 2, 3):
        old.run(1)
        new.run(1)
        for k in range(4):
            for a, b in zip(old.state(k // 2), new.state(k)):
                assert np.array_equal(a, b), (it, k)
            assert old.counts(k // 2) == new.counts(k)
            if sampling == 2:
                for a, b in zip(old.baseline(k // 2), new.baseline(k)):
                    assert np.array_equal(a, b), (it, k)
                assert np.array_equal(bits(old.baseline_table(k // 2)), bits(new.baseline_table(k)))
            assert np.array_equal(bits(old.average_table(k // 2)), bits(new.average_table(k, "uniform")))
    assert (old.state(1)[0] < 0).any()
    old.close()
    new.close()


# ---- the handle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", [0, 1, 2])
@pytest.mark.parametrize("game", [1, 0])
def test_runs_of_a_handle_are_the_runs_alone_and_repeat(pkg, ev, ctxs, trees, game, sampling):
    """Four runs with the four rule pairs, their seeds, W and eps all different (the grid is sized by the
    second): each equals the run alone, a repeat is identical, and run(1) then run(2) equals run(3)."""
    B = pkg.native.MCCFR_WG_WALKERS
    e = (lambda x: x) if sampling else (lambda x: 0.0)
    cfgs = [(3, 66, e(0.25)) + PAIRS[0], (4, B + 2, e(EPS)) + PAIRS[3], (5, 6, e(1.0)) + PAIRS[2], (6, 130, e(EPS)) + PAIRS[1]]
    four = ev.MccfrXSolver(ctxs[game], cfgs, sampling).run(3)
    again = ev.MccfrXSolver(ctxs[game], cfgs, sampling).run(3)
    split = ev.MccfrXSolver(ctxs[game], cfgs, sampling).run(1).run(2)
    assert four.iterations == again.iterations == split.iterations == 3
    for k, (seed, W, eps, reg, avg) in enumerate(cfgs):
        want = ref_after(trees, game, sampling, seed, W, eps, reg, 3)
        same(four, k, want, ("of four", k), sampling)
        same(again, k, want, ("repeated", k), sampling)
        same(split, k, want, ("run(1) then run(2)", k), sampling)
        alone = ev.MccfrXSolver(ctxs[game], [cfgs[k]], sampling).run(3)
        same(alone, 0, want, ("alone", k), sampling)
        assert alone.rule(0) == four.rule(k) == (reg, avg)
        for which in (None, xr.UNIFORM, xr.LINEAR):
            tabs = [bits(x.average_table(j, which)) for x, j in ((alone, 0), (four, k), (again, k), (split, k))]
            assert all(np.array_equal(tabs[0], x) for x in tabs[1:]), (k, which)
        alone.close()
    split.run(0)
    same(split, 3, ref_after(trees, game, sampling, 6, 130, e(EPS), PAIRS[1][0], 3), "run(0)", sampling)
    for s in (four, again, split):
        s.close()


def test_a_handle_has_one_sampling_kind_and_strings_name_the_rule(pkg, ev, ctxs, trees):
    nat = pkg.native
    arr = (nat.MccfrXCfg * 2)(nat.MccfrXCfg(1, 64, 1, EPS, 1, 1), nat.MccfrXCfg(2, 64, 2, EPS, 1, 1))
    h = nat.P()
    assert ctxs[1].L.nfsp_mccfr_x_create(ctxs[1].h, arr, 2, C.byref(h)) == nat.EINVAL and not h.value
    msg = ctxs[1].L.nfsp_last_error()
    assert b"nfsp_mccfr_x_cfg.sampling" in msg and b"run 1" in msg, msg
    with pytest.raises(nat.NativeError, match="nfsp_mccfr_x_cfg.epsilon"):
        ev.MccfrXSolver(ctxs[1], [(1, 64, EPS, "plus", "linear")], "es")
    with pytest.raises(nat.NativeError, match="even"):
        ev.MccfrXSolver(ctxs[1], [(1, 3, EPS, "plus", "linear")], "vr")
    s = ev.MccfrXSolver(ctxs[1], [(1, 64, EPS, "plus", "linear"), (1, 64, EPS, "plain", "uniform")], "os")
    assert s.sampling == 1 and s.rule(0) == (nat.MCCFR_REGRET_PLUS, nat.MCCFR_AVG_LINEAR) and s.rule(1) == (0, 0)
    with pytest.raises(nat.NativeError, match="run"):
        s.rule(2)
    with pytest.raises(nat.NativeError, match="average must"):
        s.average(0, 2)
    s.close()


# ---- the averages ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", [0, 1, 2])
@pytest.mark.parametrize("game,walkers,iters", [(1, 64, 32), (0, 256, 8)])
def test_both_averages_score_as_the_restatement(pkg, ev, ctxs, trees, game, walkers, iters, sampling):
    """Plus / linear and plus / uniform, one seed: the two runs hold the same tables, nfsp_mccfr_average is the
    table the cfg names, and either average scores by nfsp_evaluate_batch within 1e-12 of the restatement's
    table scored by policy_ref.walk -- the bar of the other kinds."""
    t = trees[game]
    eps = eps_of(sampling)
    s = ev.MccfrXSolver(ctxs[game], [(1, walkers, eps, "plus", "linear"), (1, walkers, eps, "plus", "uniform")],
                        sampling).run(iters)
    want = snapshot(new_ref(t, sampling, 1, walkers, eps, xr.PLUS).run(iters))
    for k in (0, 1):
        same(s, k, want, ("the run", k), sampling)
    for k, named in ((0, xr.LINEAR), (1, xr.UNIFORM)):
        assert s.average(k).ptr == s.average(k, named).ptr != s.average(k, 1 - named).ptr
        assert np.array_equal(s.average_table(k), s.average_table(k, named))
        assert np.array_equal(s.average_table(k, 1 - named), s.average_table(1 - k))
    assert not np.array_equal(s.average_table(0), s.average_table(1))
    pols = [s.average(0, which) for which in (xr.UNIFORM, xr.LINEAR)]
    got = ev.evaluate_batch(ctxs[game], [(p, p) for p in pols])
    for which in (xr.UNIFORM, xr.LINEAR):
        ref = pr.walk(t, want["avg"][which], want["avg"][which])
        print(NAMES[game], sampling, ("uniform", "linear")[which], "exploitability", got[which]["exploitability"],
              "restated", ref["exploitability"])
        for key in ("br0", "br1", "exploitability", "value0"):
            assert abs(got[which][key] - ref[key]) <= 1e-12, (which, key)
        assert np.abs(s.average_table(0, which) - want["avg"][which]).max() <= 1e-15
    s.close()


# ---- what is refused ---------------------------------------------------------------------------------------
def test_the_other_kinds_have_no_weighted_sum_and_the_plain_uniform_rule(pkg, ev, ctxs, trees):
    nat = pkg.native
    z = np.zeros((trees[1].ndec, 3, 3))
    olds = [ev.MccfrSolver(ctxs[1], [(1, 2)]), ev.MccfrOsSolver(ctxs[1], [(1, 2, EPS)]), ev.MccfrVrSolver(ctxs[1], [(1, 2, EPS)])]
    for kind, s in enumerate(olds):
        L = s.ctx.L
        out = (nat.I32 * 2)(7, 7)
        assert L.nfsp_mccfr_rule(s.h, 0, out) == nat.OK and tuple(out) == (0, 0)
        assert L.nfsp_mccfr_rule(s.h, 1, out) == nat.EINVAL and b"run" in L.nfsp_last_error()
        p = nat.P()
        for which in (0, 1):
            assert L.nfsp_mccfr_average_of(s.h, 0, which, C.byref(p)) == nat.EINVAL and not p.value
            assert b"nfsp_mccfr_x_create" in L.nfsp_last_error() and b"Sw" in L.nfsp_last_error()
        assert L.nfsp_mccfr_weighted(s.h, 0, z.ctypes.data_as(nat.P)) == nat.EINVAL
        assert b"nfsp_mccfr_x_create" in L.nfsp_last_error() and not z.any()
        s.run(1)                                       # and they go on as before
        assert s.iterations == 1 and s.sampling == kind
        s.close()


@pytest.mark.parametrize("sampling", [0, 1, 2])
def test_run_past_the_kinds_bound_is_refused(pkg, ev, ctxs, trees, sampling):
    t = trees[0]
    eps = eps_of(sampling, 0.0625)
    bound = (int(2.0 ** 62 / (mr.Q * 2.0 * float(np.abs(t.pay).max()))), osr.bound(t, 0.0625), vrr.bound(t, 0.0625))[sampling]
    s = ev.MccfrXSolver(ctxs[0], [(1, 2, eps, "plus", "linear")], sampling).run(1)
    with pytest.raises(pkg.native.NativeError, match="overflow.*%d" % bound):
        s.run(bound // 2)                              # 1 + bound // 2 iterations in all: one too many
    assert s.iterations == 1
    same(s, 0, ref_after(trees, 0, sampling, 1, 2, eps, xr.PLUS, 1), "after the refusal", sampling)
    s.close()


@pytest.mark.parametrize("game", [1, 0])
def test_a_set_baseline_comes_back_and_the_next_iteration_uses_it(pkg, ev, ctxs, trees, game):
    """As on the handle of nfsp_mccfr_vr_create: an arbitrary baseline set on the second run of two after one
    iteration comes back, leaves R, S, Sw and the other run alone, and the next iteration equals the
    restatement's from the same tables.  Sampling 0 and 1 have no baseline, under this create call as well."""
    t = trees[game]
    rng = np.random.RandomState(8)
    P = vrr.maxpay(t)
    Bn = rng.randint(0, 4, (t.ndec, 3, 3)).astype(np.int64)
    Bs = mr.llrint(rng.uniform(-P, P, Bn.shape) * mr.Q) * Bn
    hot = (Bn > 0) & (rng.uniform(size=Bn.shape) < 0.1)
    Bs[hot] *= 3                                       # |Bs / (Bn Q)| up to 3 P: clamped
    s = ev.MccfrXSolver(ctxs[game], [(21, 66, EPS, "plus", "linear"), (22, 130, EPS, "plus", "uniform")], 2).run(1)
    r = new_ref(t, 2, 22, 130, EPS, xr.PLUS).run(1)
    same(s, 1, snapshot(r), "before", 2)
    assert s.set_baseline(1, Bs, Bn) is s
    got = s.baseline(1)
    assert np.array_equal(got[0], Bs) and np.array_equal(got[1], Bn)
    r.Bs, r.Bn = Bs.copy(), Bn.copy()
    B = s.baseline_table(1)
    assert np.array_equal(B, r.baseline()) and np.abs(B).max() == P and np.all(B[Bn == 0] == 0)
    same(s, 1, snapshot(r), "after set_baseline: R, S, Sw and the counts are left", 2)
    same(s, 0, ref_after(trees, game, 2, 21, 66, EPS, xr.PLUS, 1), "the other run", 2)
    s.run(1)
    same(s, 1, snapshot(r.run(1)), "the iteration after set_baseline", 2)
    same(s, 0, ref_after(trees, game, 2, 21, 66, EPS, xr.PLUS, 2), "the other run, an iteration on", 2)
    neg = Bn.copy()
    neg[0, 0, 0] = -1
    with pytest.raises(pkg.native.NativeError, match="negative"):
        s.set_baseline(1, Bs, neg)
    s.close()
    for sampling in (0, 1):
        o = ev.MccfrXSolver(ctxs[game], [(1, 2, eps_of(sampling), "plus", "linear")], sampling)
        with pytest.raises(pkg.native.NativeError, match="baseline-corrected"):
            o.baseline(0)
        with pytest.raises(pkg.native.NativeError, match="baseline-corrected"):
            o.set_baseline(0, Bs, Bn)
        o.close()

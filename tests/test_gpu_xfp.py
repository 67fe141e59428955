"""nfsp_best_response_table (csrc/evaluate.hip k_best_response) and nfsp_xfp_* (csrc/xfp.hip
k_xfp) on the GPU, against their numpy restatements (tests/xfp_ref.py: the same operations in
the same order, so the discrete path -- every argmax, S, B, W -- is equal and the f64 values
agree to 1e-12, tests/test_gpu_evaluation.py's bar for CFR+), through the existing evaluator
(nfsp_evaluate_batch) and against the brute-force oracle (1e-9 where both read one f64 table)."""
import ctypes as C

import numpy as np
import pytest

import nn_oracle as nn
import policy_ref as pr
import xfp_ref as xr

pytestmark = pytest.mark.gpu
NAMES = {0: "leduc", 1: "kuhn"}
CFGS4 = [(0.0, 0), (0.0, 1), (0.1, 0), (0.25, 1)]
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


def glorot(seed, act=nn.ACT_SOFTMAX):
    return nn.MLP(act, 64, rng=np.random.RandomState(seed)).flat()


def seats(ev, t, case):
    if case == "tables":
        return ev.Policy.table(pr.random_table(t, 0)), ev.Policy.table(pr.random_table(t, 1))
    if case == "uniform":
        return ev.Policy.table(t.uniform()), ev.Policy.table(t.uniform())
    if case == "ar_softmax":
        return ev.Policy.ar(glorot(2)), ev.Policy.ar(glorot(3))
    if case == "ar_argmax":
        return ev.Policy.ar(glorot(2), 1), ev.Policy.ar(glorot(3), 1)
    if case == "br_greedy":
        return ev.Policy.br(glorot(4, nn.ACT_RELU)), ev.Policy.br(glorot(5, nn.ACT_RELU), True)
    if case == "table_vs_br":
        return ev.Policy.table(pr.random_table(t, 6)), ev.Policy.br(glorot(7, nn.ACT_RELU))
    assert case == "ar_vs_table"
    return ev.Policy.ar(glorot(8)), ev.Policy.table(np.random.RandomState(9).dirichlet(np.ones(3), size=(t.ndec, 3)))


CASES = ["tables", "uniform", "ar_softmax", "ar_argmax", "br_greedy", "table_vs_br", "ar_vs_table"]


# ---- the best-response table ---------------------------------------------------------------------
@pytest.mark.parametrize("game", [1, 0])
@pytest.mark.parametrize("case", CASES)
def test_best_response_table_matches_restatement_and_evaluator(ev, ctxs, trees, game, case):
    """The root check: the dealer acts first, so root[d]'s rows are seat d's, and the sum over
    its ranks of max_a q there is seat d's best-response value over dealer-d hands -- which the
    evaluator gives as the per-dealer value of the table.  (Half the sum over both dealers is
    therefore half of seat 0's dealer-0 value plus half of seat 1's dealer-1 value; br0 itself
    also holds the hands the other seat deals, whose first node has no row of q.)"""
    t, ctx = trees[game], ctxs[game]
    s0, s1 = seats(ev, t, case)
    beta, q, reach = (x.cpu().numpy() for x in ev.best_response(ctx, s0, s1, values=True, tree=t))
    tabs = [ev.policy_table(ctx, s, t).cpu().numpy() for s in (s0, s1)]
    rb, rq, rr = xr.best_response(t, tabs[0], tabs[1])
    assert np.array_equal(beta, rb)
    dq, dr = np.abs(q - rq).max(), np.abs(reach - rr).max()
    print(NAMES[game], case, "max |q diff|", dq, "max |reach diff|", dr)
    assert dq <= 1e-12 and dr <= 1e-12
    assert np.array_equal(beta.sum(-1), np.ones((t.ndec, 3))) and set(np.unique(beta)) == {0.0, 1.0}
    assert np.all(beta[~t.legal][:, :, 2] == 0) and np.all(q[~t.legal][:, :, 2] == 0)
    only = ev.best_response(ctx, s0, s1, tree=t).cpu().numpy()          # dev_q = dev_reach = NULL
    assert np.array_equal(only, beta)
    # through the existing evaluator
    want = ev.evaluate(ctx, s0, s1)
    pb = ev.Policy.table(beta)
    at0, at1 = ev.evaluate(ctx, pb, s1), ev.evaluate(ctx, s0, pb)
    print(NAMES[game], case, "br0", at0["value0"] - want["br0"], "br1", -at1["value0"] - want["br1"])
    assert abs(at0["value0"] - want["br0"]) <= 1e-12
    assert abs(-at1["value0"] - want["br1"]) <= 1e-12
    rows = [int(t.nodes["row"][t.root[d]]) for d in (0, 1)]
    assert [int(t.seat[r]) for r in rows] == [0, 1]
    per = [sum(max(q[rows[d], r, :3 if t.legal[rows[d]] else 2]) for r in range(3)) for d in (0, 1)]
    assert abs(per[0] - at0["value0_dealer0"]) <= 1e-12
    assert abs(per[1] + at1["value0_dealer1"]) <= 1e-12


def test_best_response_bad_arguments_are_refused(pkg, ev, ctxs, trees):
    import torch
    ctx, nat, t = ctxs[0], pkg.native, trees[0]
    tab = ev.Policy.table(t.uniform())
    ok = tab.spec()
    out = torch.full((t.ndec, 3, 3), -7.0, dtype=torch.float64, device="cuda")
    o = nat.P(out.data_ptr())
    f = ctx.L.nfsp_best_response_table
    for bad, word in ((nat.PolicySpec(5, 0, ok.dev), b"kind"), (nat.PolicySpec(0, 1, ok.dev), b"reserved"),
                      (nat.PolicySpec(4, 0, None), b"null")):
        for a, b in ((bad, ok), (ok, bad)):
            assert f(ctx.h, C.byref(a), C.byref(b), o, None, None) == nat.EINVAL
            assert word in ctx.L.nfsp_last_error()
    assert f(ctx.h, C.byref(ok), C.byref(ok), None, None, None) == nat.EINVAL
    assert f(None, C.byref(ok), C.byref(ok), o, None, None) == nat.EINVAL
    # an output on a policy's table, or inside it
    for args in ((nat.P(tab.ptr), None, None), (o, nat.P(tab.ptr), None), (o, None, nat.P(tab.ptr + 8 * 9))):
        assert f(ctx.h, C.byref(ok), C.byref(ok), *args) == nat.EINVAL
        assert b"alias" in ctx.L.nfsp_last_error()
    # two outputs on each other: q on beta, reach inside q
    q = torch.full((t.ndec, 3, 3), -7.0, dtype=torch.float64, device="cuda")
    for args in ((o, o, None), (o, nat.P(q.data_ptr()), nat.P(q.data_ptr() + 8 * 9 * (t.ndec - 1)))):
        assert f(ctx.h, C.byref(ok), C.byref(ok), *args) == nat.EINVAL
        assert b"alias each other" in ctx.L.nfsp_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((q == -7.0).all())     # nothing was launched
    assert np.array_equal(tab.data.cpu().numpy().reshape(t.ndec, 3, 3), t.uniform())


# ---- XFP -----------------------------------------------------------------------------------------
def refs(trees, game):
    """The four restated runs of CFGS4 at 1, 2, 8 and 32 iterations: computed once, kept."""
    if game not in _REFS:
        out = {}
        runs = [xr.XfpRef(trees[game], eta, w) for eta, w in CFGS4]
        for upto in (1, 2, 8, 32):
            for r in runs:
                r.run(upto - r.t)
            out[upto] = [(r.S.copy(), r.B.copy(), r.W, r.average(), np.array(r.gaps)) for r in runs]
        _REFS[game] = out
    return _REFS[game]


def snapshot(s, k):
    return s.state(k) + (s.average_table(k),)


@pytest.mark.parametrize("game", [1, 0])
def test_xfp_state_matches_restatement(ev, ctxs, trees, game):
    t = trees[game]
    want = refs(trees, game)
    s = ev.XfpSolver(ctxs[game], CFGS4)
    assert s.iterations == 0
    for k in range(4):
        S, B, W, avg = snapshot(s, k)
        assert not S.any() and not B.any() and W == 0.0 and np.array_equal(avg, t.uniform())
    gaps = np.zeros((4, 0))
    worst = 0.0
    for upto in (1, 2, 8, 32):
        gaps = np.concatenate([gaps, s.run(upto - s.iterations, gaps=True)], axis=1)
        assert s.iterations == upto and gaps.shape == (4, upto)
        for k in range(4):
            S, B, W, avg = snapshot(s, k)
            rS, rB, rW, ravg, rgaps = want[upto][k]
            assert np.array_equal(S, rS) and np.array_equal(B, rB) and W == rW, (upto, k)
            d = max(np.abs(avg - ravg).max(), np.abs(gaps[k] - rgaps).max())
            worst = max(worst, d)
            assert d <= 1e-12, (upto, k, d)
    print(NAMES[game], "max |average, gaps diff|", worst)
    s.close()


@pytest.mark.parametrize("game", [1, 0])
def test_xfp_runs_are_independent(ev, ctxs, game):
    cfgs = CFGS4 + [(0.5, 0)]
    many = ev.XfpSolver(ctxs[game], cfgs)
    g = many.run(12, gaps=True)
    for k, cfg in enumerate(cfgs):
        one = ev.XfpSolver(ctxs[game], [cfg])
        g1 = one.run(12, gaps=True)
        assert np.array_equal(g1[0], g[k]), k
        for a, b in zip(snapshot(one, 0), snapshot(many, k)):
            assert np.array_equal(a, b), k
        one.close()
    assert len({tuple(row) for row in g}) == len(cfgs)       # and the cfgs do differ
    many.close()


def test_xfp_split_runs_are_one_run(pkg, ev, ctxs):
    cap = pkg.native.XFP_LAUNCH_ITERS
    cfgs = [(0.0, 0), (0.1, 1)]

    def final(game, *runs):
        s = ev.XfpSolver(ctxs[game], cfgs)
        gaps = np.concatenate([s.run(n, gaps=True) for n in runs], axis=1)
        out = (s.iterations, gaps) + snapshot(s, 0) + snapshot(s, 1)
        s.close()
        return out

    for game, a, b in ((0, (8, 8), (16,)), (1, (8, 8), (16,)), (1, (cap + 3,), (cap, 3)),
                       (0, (cap + 3,), (cap, 3))):
        x, y = final(game, *a), final(game, *b)
        assert x[0] == y[0] == sum(a) and x[1].shape == (2, sum(a))
        for u, v in zip(x[1:], y[1:]):
            assert np.array_equal(u, v), (game, a, b)


@pytest.mark.parametrize("game", [1, 0])
def test_xfp_gap_is_the_evaluators_exploitability(ev, ctxs, game):
    ctx = ctxs[game]
    s = ev.XfpSolver(ctx, [(0.0, 0), (0.0, 1)])

    def expl():
        return [ev.evaluate(ctx, s.average(k), s.average(k))["exploitability"] for k in (0, 1)]

    e0 = expl()
    g = s.run(8, gaps=True)
    e8 = expl()
    g8 = s.run(1, gaps=True)
    for k in (0, 1):
        print(NAMES[game], k, "t=0", g[k, 0] - e0[k], "t=8", g8[k, 0] - e8[k])
        assert abs(g[k, 0] - e0[k]) <= 1e-12 and abs(g8[k, 0] - e8[k]) <= 1e-12
    s.close()


def test_xfp_leduc_256_linear_is_an_anchor(ev, ctxs, trees):
    """Measured with the restatement: 0.04431 (eta = 0), 0.03326 (eta = 0.1)."""
    t, ctx = trees[0], ctxs[0]
    s = ev.XfpSolver(ctx, [(0.0, "linear"), (0.1, "linear")]).run(256)
    got = ev.evaluate(ctx, s.average(0), s.average(0))
    tab = s.average_table(0)
    want = pr.oracle_table_scores(t, tab, tab)
    print("leduc XFP 256 linear:", got)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-9, (k, got[k], want[k])
    assert 0 <= got["exploitability"] < 0.07
    assert abs(got["value0"]) < 0.05
    ant = ev.evaluate(ctx, s.average(1), s.average(1))
    print("leduc XFP 256 linear, eta 0.1:", ant)
    assert 0 <= ant["exploitability"] < 0.07
    s.close()


def test_xfp_bad_handles_and_arguments_are_refused(pkg, ev, ctxs):
    ctx, nat = ctxs[1], pkg.native
    L = ctx.L
    h = nat.P()

    def einval(rc, word):
        assert rc == nat.EINVAL
        assert word in L.nfsp_last_error(), L.nfsp_last_error()

    one = (nat.XfpCfg * 1)(nat.XfpCfg(0.0, 0, 0))
    einval(L.nfsp_xfp_create(ctx.h, one, 0, C.byref(h)), b"n must")
    einval(L.nfsp_xfp_create(ctx.h, one, nat.XFP_MAX_RUNS + 1, C.byref(h)), b"n must")
    for cfg, word in ((nat.XfpCfg(1.0, 0, 0), b"eta"), (nat.XfpCfg(-0.5, 0, 0), b"eta"), (nat.XfpCfg(0.0, 2, 0), b"weight"),
                      (nat.XfpCfg(0.0, 0, 3), b"reserved")):
        einval(L.nfsp_xfp_create(ctx.h, (nat.XfpCfg * 1)(cfg), 1, C.byref(h)), word)
    einval(L.nfsp_xfp_create(ctx.h, None, 1, C.byref(h)), b"null")
    einval(L.nfsp_xfp_create(ctx.h, one, 1, None), b"null")
    assert not h.value
    with pytest.raises(nat.NativeError):
        ev.XfpSolver(ctx, [(1.5, 0)])
    s = ev.XfpSolver(ctx, [(0.0, 0), (0.1, 1)])
    s.run(3)
    before = snapshot(s, 0) + snapshot(s, 1)
    p, w = nat.P(), nat.F64(0)
    buf = np.zeros(s.tree.ndec * 9)
    bp = buf.ctypes.data_as(nat.P)
    einval(L.nfsp_xfp_run(s.h, -1, None), b"iters")
    for gaps in (False, True):                               # the library's answer, not numpy's
        with pytest.raises(nat.NativeError, match="iters must be >= 0"):
            s.run(-1, gaps=gaps)
    for run in (-1, 2):
        einval(L.nfsp_xfp_average(s.h, run, C.byref(p)), b"run")
        einval(L.nfsp_xfp_state(s.h, run, bp, bp, C.byref(w)), b"run")
    einval(L.nfsp_xfp_average(s.h, 0, None), b"null")
    einval(L.nfsp_xfp_state(s.h, 0, None, bp, C.byref(w)), b"null")
    einval(L.nfsp_xfp_iterations(s.h, None), b"null")
    assert s.iterations == 3
    for a, b in zip(before, snapshot(s, 0) + snapshot(s, 1)):
        assert np.array_equal(a, b)
    s.close()


# ---- the engine ------------------------------------------------------------------------------------
def test_engine_best_response_table_ties_to_br_gap(pkg, ev, trees):
    NET_AR, NET_BR = pkg.engine.NET_AR, pkg.engine.NET_BR
    eng = pkg.engine.SelfPlayEngine(n_lanes=128, rl_capacity=2000, sl_capacity=2000, seed=13)
    eng.step()
    ctx, t = eng.ctx, trees[0]
    beta = eng.best_response_table()
    assert beta.shape == (t.ndec, 3, 3)
    pb = ev.Policy.table(beta)
    want = eng.exploitability()
    v = [ev.evaluate(ctx, pb, eng.policy(1, NET_AR))["value0"], -ev.evaluate(ctx, eng.policy(0, NET_AR), pb)["value0"]]
    assert abs(v[0] - want["br0"]) <= 1e-12 and abs(v[1] - want["br1"]) <= 1e-12
    learned = [ev.evaluate(ctx, eng.policy(0, NET_BR), eng.policy(1, NET_AR))["value0"],
               -ev.evaluate(ctx, eng.policy(0, NET_AR), eng.policy(1, NET_BR))["value0"]]
    gap = eng.br_gap()
    for i in (0, 1):
        assert abs(gap[i]["gap"] - (v[i] - learned[i])) <= 1e-9, i
    # row by row against the greedy BR nets: the seats' rows of the two tables
    greedy = [ev.policy_table(ctx, eng.policy(i, NET_BR), t).cpu().numpy() for i in (0, 1)]
    b = beta.cpu().numpy()
    for i in (0, 1):
        same = (b[t.seat == i] == greedy[i][t.seat == i]).all(-1)
        assert (gap[i]["gap"] <= 1e-9) or not same.all()     # a positive gap shows as a differing row
    # against the eta mixtures, as br_gap(eta=) builds them
    eta = 0.25
    b2, q2, r2 = eng.best_response_table(eta=eta, values=True)
    assert q2.shape == (t.ndec, 3, 3) and r2.shape == (t.ndec, 3)
    mixes = []
    for o in (0, 1):
        tabs = [ev.policy_table(ctx, eng.policy(o, n), t).cpu().numpy() for n in (NET_BR, NET_AR)]
        mixes.append(ev.Policy.table(ev.mix(t, [(eta, tabs[0]), (1 - eta, tabs[1])])))
    g2 = eng.br_gap(eta=eta)
    p2 = ev.Policy.table(b2)
    assert abs(ev.evaluate(ctx, p2, mixes[1])["value0"] - g2[0]["br_exact"]) <= 1e-12
    assert abs(-ev.evaluate(ctx, mixes[0], p2)["value0"] - g2[1]["br_exact"]) <= 1e-12
    eng.close()

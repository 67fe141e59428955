"""nfsp_evaluate_batch / nfsp_policy_table / nfsp_cfr_* on the GPU (csrc/evaluate.hip,
csrc/cfr.hip) against nfsp_exploitability (the same kernel behind a wrapper that maps modes to
kinds and drops two columns: bit for bit where they overlap), the brute-force
oracle (oracle/exploit_oracle.py, 1e-5 chips as tests/test_exploit.py: net outputs agree to
~1e-7 and payoffs are <= 6.5 chips; 1e-9 where both sides read the same f64 table) and the numpy
restatements of the kernels (tests/policy_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import exploit_oracle as eo
import nn_oracle as nn
import policy_ref as pr

pytestmark = pytest.mark.gpu
TOL = 1e-5
NAMES = {0: "leduc", 1: "kuhn"}
KEYS4 = ("br0", "br1", "exploitability", "value0")


def glorot_pair(seed, act=nn.ACT_SOFTMAX):
    rng = np.random.RandomState(seed)
    return nn.MLP(act, 64, rng=rng).flat(), nn.MLP(act, 64, rng=rng).flat()


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


class GreedyQ:
    """The oracle side of NFSP_POL_BR_GREEDY[_LINEAR]: nn_oracle's forward, one-hot argmax (first
    maximum wins); TabularPolicy-style remap of an illegal raise."""

    def __init__(self, w, linear):
        self.net = nn.MLP(nn.ACT_LINEAR if linear else nn.ACT_RELU, 64,
                          weights=nn.unpack_weights(np.asarray(w, np.float32)))
        self.tab = eo.TabularPolicy(self.onehot)

    def onehot(self, obs):
        x = np.array([[(obs >> i) & 1 for i in range(30)]], np.float32).reshape(1, 1, -1)
        q = np.zeros(3)
        q[int(np.argmax(self.net.predict(x).reshape(3)))] = 1.0
        return q

    def probs(self, obs, legal):
        return self.tab.probs(obs, legal)


def close(got, want, tol, keys=None):
    for k in keys or want:
        assert abs(got[k] - want[k]) <= tol, (k, got[k], want[k])


# ---- kinds 0 / 1 are nfsp_exploitability ------------------------------------------------------
@pytest.mark.parametrize("game", [0, 1])
@pytest.mark.parametrize("seed", [0, 7])
def test_ar_kinds_equal_exploitability_bits(pkg, ev, ctxs, game, seed):
    w0, w1 = glorot_pair(seed)
    ctx = ctxs[game]
    for mode in (0, 1):
        a, b = ev.Policy.ar(w0, mode), ev.Policy.ar(w1, mode)
        got = ev.evaluate(ctx, a, b)
        want = pkg.engine.exploitability(ctx, a.ptr, b.ptr, mode)
        assert [got[k] for k in KEYS4] == [want[k] for k in KEYS4], mode
        assert got["value0"] == 0.5 * (got["value0_dealer0"] + got["value0_dealer1"])


# ---- the greedy best-response kinds against the oracle -------------------------------------------
@pytest.mark.parametrize("linear", [False, True])
@pytest.mark.parametrize("seed", [0, 7, "zero"])
def test_br_greedy_matches_oracle(ev, ctxs, trees, linear, seed):
    if seed == "zero":
        w0 = w1 = np.zeros(nn.n_params(), np.float32)
    else:
        w0, w1 = glorot_pair(seed, nn.ACT_RELU)
    got = ev.evaluate(ctxs[0], ev.Policy.br(w0, linear), ev.Policy.br(w1, linear))
    want = pr.oracle_scores(trees[0], GreedyQ(w0, linear), GreedyQ(w1, linear), keys=("br0", "br1", "value0"))
    close(got, want, TOL)
    if seed == "zero":                        # every head ties at 0: the first maximum is fold
        tab = ev.policy_table(ctxs[0], ev.Policy.br(w0, linear), trees[0]).cpu().numpy()
        assert np.all(tab[:, :, 0] == 1.0) and np.all(tab[:, :, 1:] == 0.0)
        # the first to act folds its blind: the dealer's 0.5, averaged over the two dealers
        assert abs(got["value0"]) <= 1e-12
        assert abs(got["value0_dealer0"] + 0.5) <= 1e-12 and abs(got["value0_dealer1"] - 0.5) <= 1e-12


# ---- tables, alone and against nets ------------------------------------------------------------
@pytest.mark.parametrize("game", [0, 1])
def test_mixed_pairings_and_per_dealer_values_match_oracle(ev, ctxs, trees, game):
    t, ctx = trees[game], ctxs[game]
    w0, w1 = glorot_pair(3)
    tab = pr.random_table(t, 8)
    # un-remapped input: the raise column's mass must go to call on the device
    raw = np.random.RandomState(9).dirichlet(np.ones(3), size=(t.ndec, 3))
    cases = [(ev.Policy.table(tab), ev.Policy.ar(w1), pr.oracle_policy(t, tab, 0), eo.Policy(w1, 0)),
             (ev.Policy.ar(w0), ev.Policy.table(raw), eo.Policy(w0, 0), pr.oracle_policy(t, raw, 1))]
    got = ev.evaluate_batch(ctx, [(a, b) for a, b, _, _ in cases])
    for g, (_, _, o0, o1) in zip(got, cases):
        close(g, pr.oracle_scores(t, o0, o1), TOL)
        assert g["value0"] == 0.5 * (g["value0_dealer0"] + g["value0_dealer1"])
        assert g["exploitability"] == g["br0"] + g["br1"]
    # both seats tables: the device and the restatement read the same doubles
    g = ev.evaluate(ctx, ev.Policy.table(tab), ev.Policy.table(raw))
    close(g, pr.walk(t, tab, raw), 1e-12)


@pytest.mark.parametrize("game", [0, 1])
def test_policy_table_scores_like_its_net(ev, ctxs, trees, game):
    t, ctx = trees[game], ctxs[game]
    w0, w1 = glorot_pair(7)
    q0, q1 = glorot_pair(11, nn.ACT_RELU)
    for a, b in [(ev.Policy.ar(w0), ev.Policy.ar(w1)), (ev.Policy.ar(w0, 1), ev.Policy.br(q1)),
                 (ev.Policy.br(q0, True), ev.Policy.ar(w1))]:
        ta, tb = ev.policy_table(ctx, a, t), ev.policy_table(ctx, b, t)
        assert ta.shape == (t.ndec, 3, 3)
        h = ta.cpu().numpy()
        assert np.all(h[~t.legal][:, :, 2] == 0) and np.allclose(h.sum(-1), 1.0, atol=1e-6)
        nets = ev.evaluate(ctx, a, b)
        assert ev.evaluate(ctx, ev.Policy.table(ta), ev.Policy.table(tb)) == nets
        assert ev.evaluate(ctx, a, ev.Policy.table(tb)) == nets
        # a table of a table is the same table
        assert np.array_equal(ev.policy_table(ctx, ev.Policy.table(ta), t).cpu().numpy(), h)


def test_batch_across_the_launch_limit(ev, ctxs, trees):
    """70 pairs (two launches of up to 64 workgroups) of mixed kinds: every checked pair equals
    its own call."""
    t, ctx = trees[0], ctxs[0]
    rng = np.random.RandomState(5)
    pols = []
    for k in range(70):
        w = nn.MLP(nn.ACT_SOFTMAX, 64, rng=rng).flat() * (1 + k % 3)
        kind = k % 5
        if kind == 4:
            pols.append(ev.Policy.table(pr.random_table(t, 100 + k)))
        elif kind >= 2:
            pols.append(ev.Policy.br(w, kind == 3))
        else:
            pols.append(ev.Policy.ar(w, kind))
    pairs = [(pols[k], pols[(3 * k + 1) % 70]) for k in range(70)]
    got = ev.evaluate_batch(ctx, pairs)
    assert len(got) == 70 and ev.evaluate_batch(ctx, []) == []
    for k in (0, 63, 64, 69):
        assert got[k] == ev.evaluate(ctx, *pairs[k]), k
    assert len({g["value0"] for g in got}) > 60


def test_bad_policies_are_refused(pkg, ev, ctxs):
    ctx, nat = ctxs[0], pkg.native
    ok = ev.Policy.ar(np.zeros(nn.n_params(), np.float32)).spec()
    out = (C.c_double * 6)()
    for bad, word in ((nat.PolicySpec(5, 0, ok.dev), b"kind"), (nat.PolicySpec(-1, 0, ok.dev), b"kind"),
                      (nat.PolicySpec(0, 1, ok.dev), b"reserved"), (nat.PolicySpec(0, 0, None), b"null")):
        for s0, s1 in ((bad, ok), (ok, bad)):
            assert ctx.L.nfsp_evaluate_batch(ctx.h, C.byref(s0), C.byref(s1), 1, out) == nat.EINVAL
            assert word in ctx.L.nfsp_last_error()
        assert ctx.L.nfsp_policy_table(ctx.h, C.byref(bad), out) == nat.EINVAL
    assert ctx.L.nfsp_evaluate_batch(ctx.h, C.byref(ok), C.byref(ok), -1, out) == nat.EINVAL


# ---- the engine's learned best response ----------------------------------------------------------
def test_engine_br_gap_matches_oracle(pkg, ev, trees):
    eng = pkg.engine.SelfPlayEngine(n_lanes=4096, rl_capacity=40_000, sl_capacity=40_000, seed=11)
    for _ in range(4):
        eng.step()
    got = eng.br_gap()
    ar = [eo.Policy(eng.get_weights(a, 0), 0) for a in (0, 1)]
    br = [GreedyQ(eng.get_weights(a, 1), False) for a in (0, 1)]
    v0 = [eo.on_policy_value0(br[0], ar[1]), eo.on_policy_value0(ar[0], br[1])]
    for i in (0, 1):
        exact = eo.best_response(i, ar[1 - i])
        learned = v0[0] if i == 0 else -v0[1]
        assert abs(got[i]["br_exact"] - exact) <= TOL and abs(got[i]["br_learned"] - learned) <= TOL
        assert abs(got[i]["gap"] - (exact - learned)) <= TOL
        assert got[i]["gap"] >= -1e-9
    want = eng.exploitability(0)                  # the exact halves are nfsp_exploitability's
    assert (got[0]["br_exact"], got[1]["br_exact"]) == (want["br0"], want["br1"])


def test_engine_br_gap_against_the_eta_mixture_kuhn(pkg, ev, trees):
    """kuhn_diag's anticip, linear Q head: the opponent is the per-hand mixture
    eta x greedy BR + (1 - eta) x AR; against the oracle playing that mixture by linearity."""
    nat = pkg.native
    eng = pkg.engine.SelfPlayEngine(n_lanes=1024, rl_capacity=20_000, sl_capacity=20_000, seed=5,
                                    game=nat.GAME_KUHN, quirks=nat.TEXTBOOK)
    for _ in range(3):
        eng.step()
    eta = 0.25
    got = eng.br_gap(eta=eta)
    ar = [eo.Policy(eng.get_weights(a, 0), 0) for a in (0, 1)]
    br = [GreedyQ(eng.get_weights(a, 1), True) for a in (0, 1)]
    # value of seat i's greedy BR against the mixture: linear in the per-hand mixture
    l0 = eta * eo.on_policy_value0(br[0], br[1], "kuhn") + (1 - eta) * eo.on_policy_value0(br[0], ar[1], "kuhn")
    l1 = -(eta * eo.on_policy_value0(br[0], br[1], "kuhn") + (1 - eta) * eo.on_policy_value0(ar[0], br[1], "kuhn"))
    assert abs(got[0]["br_learned"] - l0) <= TOL and abs(got[1]["br_learned"] - l1) <= TOL
    t = trees[1]
    for i in (0, 1):
        o = 1 - i
        tabs = [ev.policy_table(eng.ctx, eng.policy(o, n), t).cpu().numpy() for n in (1, 0)]
        mixed = pr.oracle_policy(t, ev.mix(t, [(eta, tabs[0]), (1 - eta, tabs[1])]), o)
        assert abs(got[i]["br_exact"] - eo.best_response(i, mixed, "kuhn")) <= TOL
        assert got[i]["gap"] >= -1e-9


def test_group_crossplay_and_br_gap_all(pkg):
    g = pkg.engine.EngineGroup(3, n_lanes=2048, rl_capacity=20_000, sl_capacity=20_000, seed=21)
    g.step()
    g.step()
    x = g.crossplay()
    assert x.shape == (3, 3)
    assert [x[r, r] for r in range(3)] == [r["value0"] for r in g.exploitability_all()]
    one = pkg.engine.exploitability(g.ctx, g.replicas[2]._wptr(0, 0), g.replicas[0]._wptr(1, 0), 0)
    assert x[2, 0] == one["value0"] and x[2, 0] != x[0, 2]
    assert g.br_gap_all() == [e.br_gap() for e in g.replicas]
    g.close()


# ---- CFR+ ------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", [1, 0])
def test_cfr_state_matches_restatement(ev, ctxs, trees, game):
    t = trees[game]
    s = ev.CfrSolver(ctxs[game])
    assert s.iterations == 0 and np.array_equal(s.average_table(), t.uniform())
    ref = pr.CfrRef(t)
    done = 0
    for upto in (1, 2, 8):
        s.run(upto - done)
        ref.run(upto - done)
        done = upto
        assert s.iterations == upto
        R, S = s.state()
        for name, a, b in (("R", R, ref.R), ("S", S, ref.S), ("avg", s.average_table(), ref.average())):
            d = np.abs(a - b).max()
            print(NAMES[game], upto, name, "max |diff|", d)
            assert d <= 1e-12, (upto, name)
    s.close()


def test_cfr_split_runs_are_one_run(pkg, ev, ctxs):
    cap = pkg.native.CFR_LAUNCH_ITERS

    def final(game, *runs):
        s = ev.CfrSolver(ctxs[game])
        for n in runs:
            s.run(n)
        out = (s.iterations,) + s.state() + (s.average_table(),)
        s.close()
        return out

    for game, a, b in ((0, (8, 8), (16,)), (1, (8, 8), (16,)), (1, (cap + 3,), (cap, 3)),
                       (0, (cap + 3,), (cap, 3))):
        x, y = final(game, *a), final(game, *b)
        assert x[0] == y[0] == sum(a)
        for u, v in zip(x[1:], y[1:]):
            assert np.array_equal(u, v), (game, a, b)


def test_cfr_leduc_256_is_an_anchor(ev, ctxs, trees):
    t, ctx = trees[0], ctxs[0]
    s = ev.CfrSolver(ctx).run(256)
    eq = s.average()
    got = ev.evaluate(ctx, eq, eq)
    tab = s.average_table()
    want = pr.oracle_table_scores(t, tab, tab)
    print("leduc CFR+ 256:", got)
    close(got, want, 1e-9)
    assert 0 <= got["exploitability"] < 0.0016
    assert abs(got["value0"]) < 1e-3
    w0, _ = glorot_pair(0)
    assert ev.evaluate(ctx, ev.Policy.ar(w0), eq)["value0"] <= got["br0"] + 1e-12
    s.close()

"""Baseline-corrected outcome sampling (VR-MCCFR) without a GPU: the ABI of nfsp_mccfr_vr_* and
of the baseline's two entry points with their host-side refusals, the overflow recursion worked by
hand on Kuhn and held to the library's message on both games, and the numpy restatement of the
rule (tests/mccfr_vr_ref.py) -- that its paths are outcome sampling's pick for pick, that its
regret increments are unbiased under an ARBITRARY baseline, that a learned baseline lowers their
variance, and that its average converges faster than outcome sampling's at the GPU test's sizes.
The GPU side holds the kernel to the restatement, int64 for int64: tests/test_gpu_mccfr_vr.py."""
import ctypes as C

import numpy as np
import pytest

import mccfr_os_ref as osr
import mccfr_ref as mr
import mccfr_vr_ref as vrr
import policy_ref as pr

GAMES = {"leduc": 0, "kuhn": 1}
SEAT0_ENTRIES = {"leduc": 507, "kuhn": 30}          # legal (row, rank, action) where seat 0 acts
EPS = 0.6
_TREES = {}
_LEARNED = {}


@pytest.fixture(scope="module")
def trees(pkg):
    import __graft_entry__
    __graft_entry__.build()
    # the restatement restates this library's rule: without its entry points there is nothing to hold to it
    assert hasattr(pkg.native.load(), "nfsp_mccfr_vr_create")
    for name, g in GAMES.items():
        if name not in _TREES:
            _TREES[name] = pkg.evaluation.GameTree(g)
    return _TREES


# ---- a. the ABI and its refusals ------------------------------------------------------------------
NEW = ["nfsp_mccfr_vr_cfgs_check", "nfsp_mccfr_vr_create", "nfsp_mccfr_baseline", "nfsp_mccfr_set_baseline"]


def test_new_symbols_exported_and_bound(pkg):
    import __graft_entry__
    __graft_entry__.build()
    nat = pkg.native
    L = nat.load()
    for name in NEW:
        assert name in nat.SIGNATURES and hasattr(L, name), name
    assert C.sizeof(nat.MccfrVrCfg) == 24 and nat.MccfrVrCfg.epsilon.offset == 16
    hdr = " ".join(open(__graft_entry__.REPO + "/include/nfsp.h").read().split())
    for name in NEW:
        assert f"int {name}(" in hdr, name
    ev = pkg.evaluation
    assert issubclass(ev.MccfrVrSolver, ev.MccfrOsSolver)
    for name in ("run", "counts", "average", "average_table", "state", "close", "iterations", "sampling"):
        assert getattr(ev.MccfrVrSolver, name) is getattr(ev.MccfrSolver, name), name
    for name in ("baseline", "set_baseline", "baseline_table"):
        assert hasattr(ev.MccfrVrSolver, name) and not hasattr(ev.MccfrOsSolver, name), name


def test_validation_names_the_field(pkg, trees):
    nat = pkg.native
    L = nat.load()

    def einval(rc, word):
        assert rc == nat.EINVAL
        assert word.encode() in L.nfsp_last_error(), (word, L.nfsp_last_error())

    def cfg(walkers=64, reserved=0, n=1, seed=1, eps=EPS):
        return (nat.MccfrVrCfg * n)(*[nat.MccfrVrCfg(seed, walkers, reserved, eps)] * n)

    check = L.nfsp_mccfr_vr_cfgs_check
    for g in GAMES.values():
        assert check(g, cfg(), 1, 0) == nat.OK
        assert check(g, cfg(2), 1, 1) == nat.OK
        assert check(g, cfg(nat.MCCFR_MAX_WALKERS, n=nat.MCCFR_MAX_RUNS), nat.MCCFR_MAX_RUNS, 1) == nat.OK
        for eps in (nat.MCCFR_OS_EPS_MIN, 1.0):
            assert check(g, cfg(eps=eps), 1, 1) == nat.OK
        for w in (3, 65, nat.MCCFR_MAX_WALKERS - 1):
            einval(check(g, cfg(w), 1, 0), "even")
        for w in (1, 0, -2, nat.MCCFR_MAX_WALKERS + 2):
            einval(check(g, cfg(w), 1, 0), "nfsp_mccfr_vr_cfg.walkers")
        einval(check(g, cfg(reserved=1), 1, 0), "nfsp_mccfr_vr_cfg.reserved")
        for eps in (0.0, -0.5, np.nextafter(nat.MCCFR_OS_EPS_MIN, 0.0), np.nextafter(1.0, 2.0), 2.0, float("inf"),
                    float("nan")):
            einval(check(g, cfg(eps=eps), 1, 0), "nfsp_mccfr_vr_cfg.epsilon")
        for n in (0, -1, nat.MCCFR_MAX_RUNS + 1):
            einval(check(g, cfg(n=2), n, 0), "n must")
        einval(check(g, None, 1, 0), "null")
        einval(check(g, cfg(), 1, -1), "iters")
        # the second of two: every cfg is checked
        einval(check(g, (nat.MccfrVrCfg * 2)(nat.MccfrVrCfg(1, 64, 0, EPS), nat.MccfrVrCfg(2, 63, 0, EPS)), 2, 0), "even")
        einval(check(g, (nat.MccfrVrCfg * 2)(nat.MccfrVrCfg(1, 64, 0, EPS), nat.MccfrVrCfg(2, 64, 0, 0.01)), 2, 0),
               "epsilon")
    einval(check(2, cfg(), 1, 0), "game")
    # no rule needs a context, a handle or a device to answer
    h = nat.P()
    einval(L.nfsp_mccfr_vr_create(None, None, 1, None), "null")
    einval(L.nfsp_mccfr_vr_create(None, cfg(), 1, C.byref(h)), "null")            # the context
    einval(L.nfsp_mccfr_vr_create(None, cfg(), 0, C.byref(h)), "n must")
    assert not h.value
    z = np.zeros((trees["kuhn"].ndec, 3, 3), np.int64)
    zp = z.ctypes.data_as(nat.P)
    for fn in (L.nfsp_mccfr_baseline, L.nfsp_mccfr_set_baseline):
        einval(fn(None, 0, zp, zp), "null")
        einval(fn(None, -1, zp, zp), "run")
        einval(fn(None, 0, None, None), "null")
    assert not z.any()


# ---- b. the overflow recursion ------------------------------------------------------------------------
def kuhn_by_hand(eps):
    """Kuhn as the engine plays it, below a deal, P = 2.  The first to act, x, folds (the end), calls
    or raises; after the call the second, y, folds, calls (both the end) or raises, and x then folds
    or calls; after the raise y folds or calls.  Under one dealer seat i is x, under the other y.
    The recursion of include/nfsp.h, node by node: (Rmax, Bmax) in chips."""
    P, f3, f2 = 2.0, 3.0 / eps, 2.0 / eps
    # seat i is x: its second decision has L = 2 and ends the hand either way
    x2 = P + (P + P) * f2
    y_called = 2.0 * P + max(P, x2)                          # the opponent's: 2 P + the most below
    y_raised = 2.0 * P + P
    x1 = P + (max(P, y_called, y_raised) + P) * f3
    r_first = max((2.0 * x1) * 1.0, (2.0 * x2) * f3)         # x2 lies below x1's L = 3
    b_first = max(max(P, y_called, y_raised), max(P, x2), P)  # the children of x1, of y_called, of the rest
    # seat i is y: one decision on a path, nothing of its own above it
    o2 = 2.0 * P + P                                         # x's second decision, the opponent's here
    y1 = P + (max(P, o2) + P) * f3                           # after the call
    y2 = P + (P + P) * f2                                    # after the raise
    r_second = max((2.0 * y1) * 1.0, (2.0 * y2) * 1.0)
    b_second = max(max(P, y1, y2), max(P, o2), P)            # the children of the root, of y1, of the rest
    return max(r_first, r_second), max(b_first, b_second)


@pytest.mark.parametrize("eps", [0.0625, 0.6, 1.0])
def test_overflow_recursion_by_hand_on_kuhn(trees, eps):
    t = trees["kuhn"]
    assert vrr.maxpay(t) == 2.0
    rmax, bmax = kuhn_by_hand(eps)
    got = vrr.bound_parts(t, eps)
    print("kuhn", eps, "by hand", (rmax, bmax), "restated", got)
    assert abs(got[0] - rmax) <= 1e-12 * rmax and abs(got[1] - bmax) <= 1e-12 * bmax
    assert got[2] == osr.omega(t, eps) and abs(got[2] - 6.0 / eps ** 2) <= 1e-9 * got[2]   # the S entries: outcome sampling's
    if eps == 1.0:
        # in integers: x2 = 2 + 4 * 2 = 10, y_called = 4 + 10 = 14, x1 = 2 + 16 * 3 = 50, so 2 * 50 = 100 against
        # 2 * 10 * 3 = 60; as y: y1 = 2 + (6 + 2) * 3 = 26, the root's child
        assert got[:2] == (100.0, 26.0)


@pytest.mark.parametrize("eps", [0.0625, 0.6, 1.0])
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_overflow_bound_follows_the_tree(pkg, trees, game, eps):
    """W x iterations <= floor(2^62 / (Q max(Rmax, Bmax, omega))), all three from the game's own tree;
    never more than outcome sampling's budget."""
    nat = pkg.native
    L = nat.load()
    t = trees[game]
    rmax, bmax, om = vrr.bound_parts(t, eps)
    bound = int(2.0 ** 62 / (nat.MCCFR_Q * max(rmax, bmax, om)))
    assert bound == vrr.bound(t, eps) and 0 < bound <= osr.bound(t, eps)
    print(game, eps, "Rmax", rmax, "Bmax", bmax, "omega", om, "bound", bound)
    for w in (2, 1 << 10, nat.MCCFR_MAX_WALKERS):
        arr = (nat.MccfrVrCfg * 1)(nat.MccfrVrCfg(1, w, 0, eps))
        assert L.nfsp_mccfr_vr_cfgs_check(GAMES[game], arr, 1, bound // w) == nat.OK
        assert L.nfsp_mccfr_vr_cfgs_check(GAMES[game], arr, 1, bound // w + 1) == nat.EINVAL
        msg = L.nfsp_last_error()
        assert b"overflow" in msg and str(bound).encode() in msg and b"Rmax" in msg, msg


def test_budgets_written_down(trees):
    """The budgets include/nfsp.h and DESIGN quote."""
    assert vrr.bound(trees["leduc"], 0.6) == 29142433 < 1 << 25       # short of the OS curve's 2^25
    assert vrr.bound(trees["leduc"], 0.0625) == 5479
    assert vrr.bound(trees["kuhn"], 0.6) == 1264775645
    assert vrr.bound(trees["kuhn"], 0.0625) == 21047312


# ---- c. the path is outcome sampling's ----------------------------------------------------------------
def record_choices(monkeypatch, make):
    """Runs make() with every choice of the rule recorded: (probabilities, draws, picks) per call."""
    calls = []
    real = mr.choose

    def choose(ps, u):
        out = real(ps, u)
        calls.append(([np.array(p, np.float64) for p in ps], np.array(u), np.array(out)))
        return out

    monkeypatch.setattr(mr, "choose", choose)
    r = make()
    monkeypatch.setattr(mr, "choose", real)
    return r, calls


@pytest.mark.parametrize("eps", [0.0625, 0.6, 1.0])
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_the_path_is_outcome_samplings(trees, monkeypatch, game, eps):
    """The same seed, eps and R (an outcome-sampling run's, so sigma is not uniform) and a baseline that is
    not 0: one half-iteration per seat gives equal dS, equal counts and equal picks at every node."""
    t = trees[game]
    start = osr.OsRef(t, 5, 64, eps).run(3)
    rng = np.random.RandomState(4)
    P = vrr.maxpay(t)
    for i in (0, 1):
        def os_half():
            r = osr.OsRef(t, 5, 64, eps)
            r.R, r.S, r.t = start.R.copy(), start.S.copy(), start.t
            r.half(i)
            return r

        def vr_half():
            r = vrr.VrRef(t, 5, 64, eps)
            r.R, r.S, r.t = start.R.copy(), start.S.copy(), start.t
            r.Bn[:] = 1
            r.Bs = mr.llrint(rng.uniform(-P, P, r.Bs.shape) * mr.Q)
            r.half(i)
            return r

        a, ca = record_choices(monkeypatch, os_half)
        b, cb = record_choices(monkeypatch, vr_half)
        assert np.array_equal(a.S, b.S) and a.terminals == b.terminals == 64
        assert len(ca) == len(cb) > 2
        for (pa, ua, ka), (pb, ub, kb) in zip(ca, cb):
            assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
            assert np.array_equal(ua, ub) and np.array_equal(ka, kb)
        assert not np.array_equal(a.R, b.R)                  # what differs is the pass back up
        assert int(b.Bn.sum()) - b.Bn.size >= 64             # a sample per decision, and no path without one


@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_split_runs_are_equal_and_the_baseline_counts_decisions(trees, game):
    t = trees[game]
    a, b = vrr.VrRef(t, 5, 32, EPS).run(8), vrr.VrRef(t, 5, 32, EPS).run(3).run(5)
    for x, y in ((a.R, b.R), (a.S, b.S), (a.Bs, b.Bs), (a.Bn, b.Bn)):
        assert np.array_equal(x, y)
    assert (a.t, a.traversals, a.terminals) == (b.t, b.traversals, b.terminals) == (8, 2 * 32 * 8, 2 * 32 * 8)
    o = osr.OsRef(t, 5, 32, EPS).run(1)
    v = vrr.VrRef(t, 5, 32, EPS).run(1)
    assert np.array_equal(o.S[t.seat == 1], v.S[t.seat == 1])      # seat 0's half came first: the same sigma
    assert np.all(a.Bn >= 0) and np.all(a.Bn[~t.legal][:, :, 2] == 0) and np.all(a.Bs[a.Bn == 0] == 0)
    assert np.all(a.R[~t.legal][:, :, 2] == 0)
    B = a.baseline()
    assert np.abs(B).max() <= vrr.maxpay(t) and np.all(B[a.Bn == 0] == 0)


# ---- d. unbiased under any baseline -------------------------------------------------------------------
def seat_entries(tree, seat):
    m = np.zeros((tree.ndec, 3, 3), bool)
    m[tree.seat == seat] = True
    m[~tree.legal, :, 2] = False
    return m


def probe(tree, cls, seed, R, t, walkers, Bs=None, Bn=None):
    """Seat 0's half-iteration of ``walkers`` traversals at the strategy of the regrets R: per entry
    the mean increment per traversal in chips, its sample variance, its second central moment and
    the exact value."""
    p = cls(tree, seed, walkers, EPS, moments=True)
    p.R = R.copy()
    p.t = t
    if Bs is not None:
        p.Bs, p.Bn = Bs.copy(), Bn.copy()
    sigma = p.sigma()
    p.half(0)
    assert p.terminals == walkers
    n = walkers // 2                                   # the walkers of the one dealer that reaches a row
    mean = (p.R - R) / mr.Q / n
    assert np.abs(mean - p.m1 / n).max() <= 1e-9
    central = p.m2 / n - mean * mean
    return mean, central * n / (n - 1), central, mr.exact_increments(tree, sigma, 0), n


def random_baseline(tree, seed):
    """A table drawn uniformly in [-P, P] with count 1: nothing to do with any value."""
    rng = np.random.RandomState(100 + seed)
    P = vrr.maxpay(tree)
    Bs = mr.llrint(rng.uniform(-P, P, (tree.ndec, 3, 3)) * mr.Q)
    return Bs, np.ones((tree.ndec, 3, 3), np.int64)


def learned(trees, game):
    if game not in _LEARNED:
        _LEARNED[game] = (osr.OsRef(trees[game], 1, 1024, EPS).run(8), vrr.VrRef(trees[game], 1, 1024, EPS).run(8))
    return _LEARNED[game]


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("game,walkers", [("kuhn", 1 << 14), ("leduc", 1 << 16)])
def test_increments_are_unbiased_at_the_uniform_strategy(trees, game, walkers, seed):
    """The baseline pinned to a random table.  Measured: no entry unvisited, worst z 2.74 (Kuhn) and
    3.28 (Leduc)."""
    t = trees[game]
    Bs, Bn = random_baseline(t, seed)
    mean, var, _, exact, n = probe(t, vrr.VrRef, seed, np.zeros((t.ndec, 3, 3), np.int64), 0, walkers, Bs, Bn)
    e = seat_entries(t, 0)
    assert int(e.sum()) == SEAT0_ENTRIES[game]
    assert np.all(mean[~e] == 0) and np.all(exact[~e] == 0)
    assert np.all(var[e] > 0)                          # no entry is skipped
    z = np.abs(mean[e] - exact[e]) / np.sqrt(var[e] / n)
    print(game, seed, "entries", int(e.sum()), "worst z", z.max())
    assert z.max() <= 6.0


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("game,walkers", [("kuhn", 1 << 17), ("leduc", 1 << 18)])
def test_increments_are_unbiased_at_a_learned_strategy(trees, game, walkers, seed):
    """The strategy after OsRef(seed 1, W = 1024).run(8), the baseline pinned to a random table; the
    entries that no walker can reach (sigma is 0 on the way) have an exact value and a mean of 0 --
    checked, not skipped.  Measured: worst z 2.71 (Kuhn) and 2.97 (Leduc), 7 and 175 entries unreached
    (outcome sampling's test counts 191 on Leduc: it also counts entries whose every increment is 0)."""
    t = trees[game]
    r = learned(trees, game)[0]
    assert not np.array_equal(r.sigma(), t.uniform())
    Bs, Bn = random_baseline(t, seed)
    mean, var, _, exact, n = probe(t, vrr.VrRef, seed, r.R, r.t, walkers, Bs, Bn)
    e = seat_entries(t, 0)
    assert np.all(mean[~e] == 0) and np.all(exact[~e] == 0)
    pos = e & (var > 0)
    z = np.abs(mean[pos] - exact[pos]) / np.sqrt(var[pos] / n)
    rest = e & ~pos                                    # never reached
    print(game, seed, "entries", int(pos.sum()), "worst z", z.max(), "unreached", int(rest.sum()))
    assert z.max() <= 6.0
    assert np.all(mean[rest] == 0) and np.all(exact[rest] == 0)


# ---- e. a learned baseline lowers the variance ----------------------------------------------------------
@pytest.mark.parametrize("game,walkers", [("kuhn", 1 << 14), ("leduc", 1 << 16)])
def test_a_learned_baseline_lowers_the_variance(trees, game, walkers):
    """sigma after 8 outcome-sampling iterations of W = 1,024, the baseline after 8 baseline-corrected
    iterations of W = 1,024 (seed 1 both; 8 sufficed): the second central moment of seat 0's increments,
    summed over its legal entries, against outcome sampling's on the same paths (seed 7).
    Measured: Kuhn 17.66 against 37.77 (0.468), Leduc 1,269.3 against 2,662.5 (0.477)."""
    t = trees[game]
    o, v = learned(trees, game)
    e = seat_entries(t, 0)
    os_ = probe(t, osr.OsRef, 7, o.R, o.t, walkers)[2][e].sum()
    vr_ = probe(t, vrr.VrRef, 7, o.R, o.t, walkers, v.Bs, v.Bn)[2][e].sum()
    print(game, "summed second central moment: OS", os_, "VR", vr_, "ratio", vr_ / os_)
    assert 0 < vr_ < os_


# ---- f. the average converges, and sooner than outcome sampling's ---------------------------------------
def test_average_converges_below_outcome_samplings(trees):
    """Leduc, W = 256, 128 iterations, eps = 0.6, seeds 1-4: the sizes of the GPU test, which compares
    the two device solvers; here the restatements alone.  Measured: 0.350 against 0.446 (the seeds
    0.300 / 0.336 / 0.372 / 0.392 against 0.396 / 0.421 / 0.490 / 0.479)."""
    t = trees["leduc"]
    xs = {}
    for name, cls in (("os", osr.OsRef), ("vr", vrr.VrRef)):
        xs[name] = []
        for seed in (1, 2, 3, 4):
            r = cls(t, seed, 256, EPS).run(128)
            assert r.traversals == r.terminals == 2 * 256 * 128
            avg = r.average()
            assert np.abs(avg.sum(-1) - 1.0).max() <= 1e-12 and np.all(avg[~t.legal][:, :, 2] == 0)
            xs[name].append(pr.walk(t, avg, avg)["exploitability"])
    print("leduc exploitability: OS", xs["os"], "VR", xs["vr"])
    assert 0 <= np.mean(xs["vr"]) < np.mean(xs["os"])

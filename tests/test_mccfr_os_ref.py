"""Outcome-sampling MCCFR without a GPU: the ABI of nfsp_mccfr_os_* and its host-side validation,
the overflow bound against an omega computed here from the exported tree, and the numpy
restatement of the rule (tests/mccfr_os_ref.py) -- that it does not depend on how a run is split,
that a traversal is one terminal, that its regret increments are unbiased estimates of the exact
counterfactual regret differences, and that its average converges.  The GPU side holds the kernel
to the restatement, int64 for int64: tests/test_gpu_mccfr_os.py."""
import ctypes as C

import numpy as np
import pytest

import mccfr_os_ref as osr
import mccfr_ref as mr
import policy_ref as pr

GAMES = {"leduc": 0, "kuhn": 1}
UNIFORM_GAP = {"leduc": 2.3111, "kuhn": 7.0 / 6.0}
SEAT0_ENTRIES = {"leduc": 507, "kuhn": 30}          # legal (row, rank, action) where seat 0 acts
EPS = 0.6
_TREES = {}
_LEARNED = {}


@pytest.fixture(scope="module")
def trees(pkg):
    import __graft_entry__
    __graft_entry__.build()
    # the restatement restates this library's rule: without its entry points there is nothing to hold to it
    assert hasattr(pkg.native.load(), "nfsp_mccfr_os_create") and osr.OsRef.EPS_MIN == pkg.native.MCCFR_OS_EPS_MIN
    for name, g in GAMES.items():
        if name not in _TREES:
            _TREES[name] = pkg.evaluation.GameTree(g)
    return _TREES


# ---- a. the ABI and its refusals ------------------------------------------------------------------
NEW = ["nfsp_mccfr_os_cfgs_check", "nfsp_mccfr_os_create", "nfsp_mccfr_sampling"]


def test_new_symbols_exported_and_bound(pkg):
    import __graft_entry__
    __graft_entry__.build()
    nat = pkg.native
    L = nat.load()
    for name in NEW:
        assert name in nat.SIGNATURES and hasattr(L, name), name
    assert C.sizeof(nat.MccfrOsCfg) == 24
    assert nat.MccfrOsCfg.epsilon.offset == 16 and C.sizeof(nat.MccfrCfg) == 16
    assert nat.MCCFR_OS_EPS_MIN == 0.0625
    hdr = " ".join(open(__graft_entry__.REPO + "/include/nfsp.h").read().split())
    assert f"#define NFSP_MCCFR_OS_EPS_MIN {nat.MCCFR_OS_EPS_MIN}" in hdr
    assert f"#define NFSP_MCCFR_Q {nat.MCCFR_Q} " in hdr and int(osr.Q) == nat.MCCFR_Q      # one fixed point
    assert issubclass(pkg.evaluation.MccfrOsSolver, pkg.evaluation.MccfrSolver)
    for name in ("run", "counts", "average", "average_table", "state", "close", "iterations"):
        assert getattr(pkg.evaluation.MccfrOsSolver, name) is getattr(pkg.evaluation.MccfrSolver, name), name


def test_validation_names_the_field(pkg, trees):
    nat = pkg.native
    L = nat.load()

    def einval(rc, word):
        assert rc == nat.EINVAL
        assert word.encode() in L.nfsp_last_error(), (word, L.nfsp_last_error())

    def cfg(walkers=64, reserved=0, n=1, seed=1, eps=EPS):
        return (nat.MccfrOsCfg * n)(*[nat.MccfrOsCfg(seed, walkers, reserved, eps)] * n)

    check = L.nfsp_mccfr_os_cfgs_check
    for g in GAMES.values():
        assert check(g, cfg(), 1, 0) == nat.OK
        assert check(g, cfg(2), 1, 1) == nat.OK
        assert check(g, cfg(nat.MCCFR_MAX_WALKERS, n=nat.MCCFR_MAX_RUNS), nat.MCCFR_MAX_RUNS, 8) == nat.OK
        for eps in (nat.MCCFR_OS_EPS_MIN, 1.0):
            assert check(g, cfg(eps=eps), 1, 1) == nat.OK
        for w in (3, 65, nat.MCCFR_MAX_WALKERS - 1):
            einval(check(g, cfg(w), 1, 0), "even")
        for w in (1, 0, -2, nat.MCCFR_MAX_WALKERS + 2):
            einval(check(g, cfg(w), 1, 0), "walkers")
        einval(check(g, cfg(reserved=1), 1, 0), "reserved")
        for eps in (0.0, -0.5, np.nextafter(nat.MCCFR_OS_EPS_MIN, 0.0), np.nextafter(1.0, 2.0), 2.0, float("inf"),
                    float("nan")):
            einval(check(g, cfg(eps=eps), 1, 0), "epsilon")
        for n in (0, -1, nat.MCCFR_MAX_RUNS + 1):
            einval(check(g, cfg(n=2), n, 0), "n must")
        einval(check(g, None, 1, 0), "null")
        einval(check(g, cfg(), 1, -1), "iters")
        # the second of two: every cfg is checked
        einval(check(g, (nat.MccfrOsCfg * 2)(nat.MccfrOsCfg(1, 64, 0, EPS), nat.MccfrOsCfg(2, 63, 0, EPS)), 2, 0), "even")
        einval(check(g, (nat.MccfrOsCfg * 2)(nat.MccfrOsCfg(1, 64, 0, EPS), nat.MccfrOsCfg(2, 64, 0, 0.01)), 2, 0),
               "epsilon")
    einval(check(2, cfg(), 1, 0), "game")
    # no rule needs a context, a handle or a device to answer
    h = nat.P()
    einval(L.nfsp_mccfr_os_create(None, None, 1, None), "null")
    einval(L.nfsp_mccfr_os_create(None, cfg(), 1, C.byref(h)), "null")            # the context
    einval(L.nfsp_mccfr_os_create(None, cfg(), 0, C.byref(h)), "n must")
    assert not h.value
    einval(L.nfsp_mccfr_sampling(None, None), "null")
    k = nat.I32(7)
    einval(L.nfsp_mccfr_sampling(None, C.byref(k)), "null")
    assert k.value == 7


def omega_here(tree, eps):
    """omega from the exported node table, on its own: depth first from both roots, for both seats,
    the product of (legal actions / eps) over the seat's decisions, the root's factor first."""
    N = tree.nodes

    def below(n, i, w):
        if int(N["kind"][n]) == pr.DECISION and int(N["p"][n]) == i:
            w = w * (float(sum(int(c) >= 0 for c in N["child"][n])) / eps)
        kids = [int(c) for c in N["child"][n] if c >= 0]
        return max([below(c, i, w) for c in kids]) if kids else w

    return max(below(int(r), i, 1.0) for r in tree.root for i in (0, 1))


@pytest.mark.parametrize("eps", [0.0625, 0.6, 1.0])
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_overflow_bound_follows_the_tree(pkg, trees, game, eps):
    """W x iterations <= floor(2^62 / ((Q max(max|pay|, 1)) omega)), omega from the game's own tree."""
    nat = pkg.native
    L = nat.load()
    t = trees[game]
    om = omega_here(t, eps)
    assert om == osr.omega(t, eps)
    a, b = {"kuhn": (2, 3), "leduc": (2 * 2, 3 * 3)}[game]      # the longest path: L = 2 and L = 3 (twice each)
    assert abs(om - a * b / eps ** {"kuhn": 2, "leduc": 4}[game]) <= 1e-9 * om
    maxpay = float(np.abs(t.pay).max())
    assert maxpay == {"leduc": 5.0, "kuhn": 2.0}[game]
    bound = int(2.0 ** 62 / ((nat.MCCFR_Q * max(maxpay, 1.0)) * om))
    assert bound == osr.bound(t, eps)
    print(game, eps, "omega", om, "bound", bound)
    for w in (2, 1 << 10, nat.MCCFR_MAX_WALKERS):
        arr = (nat.MccfrOsCfg * 1)(nat.MccfrOsCfg(1, w, 0, eps))
        assert L.nfsp_mccfr_os_cfgs_check(GAMES[game], arr, 1, bound // w) == nat.OK
        assert L.nfsp_mccfr_os_cfgs_check(GAMES[game], arr, 1, bound // w + 1) == nat.EINVAL
        msg = L.nfsp_last_error()
        assert b"overflow" in msg and str(bound).encode() in msg, msg


# ---- b. a run does not depend on how it is split; a traversal is one hand ----------------------------
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_split_runs_are_equal_and_a_traversal_is_one_terminal(trees, game):
    t = trees[game]
    a, b = osr.OsRef(t, 5, 32, EPS).run(8), osr.OsRef(t, 5, 32, EPS).run(3).run(5)
    assert np.array_equal(a.R, b.R) and np.array_equal(a.S, b.S)
    assert (a.t, a.traversals, a.terminals) == (b.t, b.traversals, b.terminals) == (8, 2 * 32 * 8, 2 * 32 * 8)
    other = osr.OsRef(t, 6, 32, EPS).run(8)              # the seed is the run's own
    assert not np.array_equal(a.R, other.R)
    greedy = osr.OsRef(t, 5, 32, 1.0).run(8)             # and so is the exploration rate
    assert not np.array_equal(a.R, greedy.R) and greedy.terminals == greedy.traversals
    for r in (a, other, greedy):                         # an illegal raise never moves; S only grows
        assert np.all(r.R[~t.legal][:, :, 2] == 0) and np.all(r.S[~t.legal][:, :, 2] == 0) and np.all(r.S >= 0)
        assert r.S.sum() > 0 and np.abs(r.R).sum() > 0


# ---- c. a traversal's increments are unbiased ----------------------------------------------------------
def seat_entries(tree, seat):
    """[ndec, 3, 3] bool: the legal (row, rank, action) where ``seat`` acts."""
    m = np.zeros((tree.ndec, 3, 3), bool)
    m[tree.seat == seat] = True
    m[~tree.legal, :, 2] = False
    return m


def probe(tree, seed, R, t, walkers):
    """Seat 0's half-iteration of ``walkers`` traversals at the strategy of the regrets R: per entry
    the mean increment per traversal in chips, its sample variance, and the exact value."""
    p = osr.OsRef(tree, seed, walkers, EPS, moments=True)
    p.R = R.copy()
    p.t = t
    sigma = p.sigma()
    p.half(0)
    assert p.terminals == walkers
    n = walkers // 2                                   # the walkers of the one dealer that reaches a row
    mean = (p.R - R) / mr.Q / n
    assert np.abs(mean - p.m1 / n).max() <= 1e-9
    var = (p.m2 - n * mean * mean) / (n - 1)
    return mean, var, mr.exact_increments(tree, sigma, 0), n


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("game,walkers", [("kuhn", 1 << 14), ("leduc", 1 << 16)])
def test_increments_are_unbiased_at_the_uniform_strategy(trees, game, walkers, seed):
    """Prototype: no entry unvisited, worst z 2.27 (Kuhn) and 3.71 (Leduc)."""
    t = trees[game]
    mean, var, exact, n = probe(t, seed, np.zeros((t.ndec, 3, 3), np.int64), 0, walkers)
    e = seat_entries(t, 0)
    assert int(e.sum()) == SEAT0_ENTRIES[game]
    assert np.all(mean[~e] == 0) and np.all(exact[~e] == 0)
    assert np.all(var[e] > 0)                          # no entry is skipped
    z = np.abs(mean[e] - exact[e]) / np.sqrt(var[e] / n)
    print(game, seed, "entries", int(e.sum()), "worst z", z.max())
    assert z.max() <= 6.0


def learned(trees, game):
    if game not in _LEARNED:
        _LEARNED[game] = osr.OsRef(trees[game], 1, 1024, EPS).run(8)
    return _LEARNED[game]


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("game,walkers", [("kuhn", 1 << 17), ("leduc", 1 << 18)])
def test_increments_are_unbiased_at_a_learned_strategy(trees, game, walkers, seed):
    """The strategy after OsRef(seed 1, W = 1024).run(8).  Prototype: worst z 2.63 (Kuhn) and 2.65
    (Leduc); 7 and 191 entries that no walker can reach (sigma is 0 on the way), all with an exact
    value of 0 -- checked, not skipped."""
    t = trees[game]
    r = learned(trees, game)
    assert not np.array_equal(r.sigma(), t.uniform())
    mean, var, exact, n = probe(t, seed, r.R, r.t, walkers)
    e = seat_entries(t, 0)
    assert np.all(mean[~e] == 0) and np.all(exact[~e] == 0)
    pos = e & (var > 0)
    z = np.abs(mean[pos] - exact[pos]) / np.sqrt(var[pos] / n)
    rest = e & ~pos                                    # never reached
    print(game, seed, "entries", int(pos.sum()), "worst z", z.max(), "unreached", int(rest.sum()))
    assert z.max() <= 6.0
    assert np.all(mean[rest] == 0) and np.all(exact[rest] == 0)


# ---- d. the average converges ---------------------------------------------------------------------------
@pytest.mark.parametrize("game,walkers,iters,cap", [("kuhn", 64, 256, 0.2917), ("leduc", 256, 128, 0.5778)])
def test_average_converges(trees, game, walkers, iters, cap):
    """Seed 1, eps = 0.6; the caps are a quarter of the uniform policy's exploitability, the
    external-sampling test's bar.  Prototype: kuhn 0.046, leduc 0.396."""
    t = trees[game]
    assert abs(4 * cap - UNIFORM_GAP[game]) <= 5e-4
    r = osr.OsRef(t, 1, walkers, EPS).run(iters)
    avg = r.average()
    assert np.abs(avg.sum(-1) - 1.0).max() <= 1e-12 and np.all(avg[~t.legal][:, :, 2] == 0)
    x = pr.walk(t, avg, avg)["exploitability"]
    print(game, walkers, iters, "exploitability", x, "hands", r.traversals)
    assert r.traversals == r.terminals == 2 * walkers * iters
    assert 0 <= x < cap

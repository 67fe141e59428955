"""External-sampling MCCFR without a GPU: the ABI of nfsp_mccfr_* and its host-side validation,
and the numpy restatement of the rule (tests/mccfr_ref.py) -- that it does not depend on how a
run is split, that a traversal's regret increments are unbiased estimates of the exact
counterfactual regret differences, and that its average converges.  The GPU side holds the
kernels to the restatement, int64 for int64: tests/test_gpu_mccfr.py."""
import ctypes as C

import numpy as np
import pytest

import mccfr_ref as mr
import policy_ref as pr

GAMES = {"leduc": 0, "kuhn": 1}
UNIFORM_GAP = {"leduc": 2.3111, "kuhn": 7.0 / 6.0}
SEAT0_ENTRIES = {"leduc": 507, "kuhn": 30}          # legal (row, rank, action) where seat 0 acts
_TREES = {}


@pytest.fixture(scope="module")
def trees(pkg):
    import __graft_entry__
    __graft_entry__.build()
    for name, g in GAMES.items():
        if name not in _TREES:
            _TREES[name] = pkg.evaluation.GameTree(g)
    return _TREES


# ---- a. the ABI and its refusals ------------------------------------------------------------------
NEW = ["nfsp_mccfr_cfgs_check", "nfsp_mccfr_create", "nfsp_mccfr_run", "nfsp_mccfr_iterations", "nfsp_mccfr_counts",
       "nfsp_mccfr_average", "nfsp_mccfr_state", "nfsp_mccfr_destroy"]


def test_new_symbols_exported_and_bound(pkg):
    import __graft_entry__
    __graft_entry__.build()
    nat = pkg.native
    L = nat.load()
    for name in NEW:
        assert name in nat.SIGNATURES and hasattr(L, name), name
    assert C.sizeof(nat.MccfrCfg) == 16
    assert nat.MCCFR_Q == 1 << 24 == int(mr.Q)
    hdr = " ".join(open(__graft_entry__.REPO + "/include/nfsp.h").read().split())
    for name, v in (("NFSP_MCCFR_Q", nat.MCCFR_Q), ("NFSP_MCCFR_MAX_RUNS", nat.MCCFR_MAX_RUNS),
                    ("NFSP_MCCFR_MAX_WALKERS", nat.MCCFR_MAX_WALKERS), ("NFSP_MCCFR_WG_WALKERS", nat.MCCFR_WG_WALKERS)):
        assert f"#define {name} {v}" in hdr, name
    assert nat.MCCFR_MAX_WALKERS == 1 << 22 and nat.MCCFR_WG_WALKERS % 2 == 0
    assert hasattr(pkg.evaluation, "MccfrSolver")


def test_validation_names_the_field(pkg, trees):
    nat = pkg.native
    L = nat.load()

    def einval(rc, word):
        assert rc == nat.EINVAL
        assert word.encode() in L.nfsp_last_error(), (word, L.nfsp_last_error())

    def cfg(walkers=64, reserved=0, n=1, seed=1):
        return (nat.MccfrCfg * n)(*[nat.MccfrCfg(seed, walkers, reserved)] * n)

    check = L.nfsp_mccfr_cfgs_check
    for g in GAMES.values():
        assert check(g, cfg(), 1, 0) == nat.OK
        assert check(g, cfg(2), 1, 1) == nat.OK
        assert check(g, cfg(nat.MCCFR_MAX_WALKERS, n=nat.MCCFR_MAX_RUNS), nat.MCCFR_MAX_RUNS, 1024) == nat.OK
        for w in (3, 65, nat.MCCFR_MAX_WALKERS - 1):
            einval(check(g, cfg(w), 1, 0), "even")
        for w in (1, 0, -2, nat.MCCFR_MAX_WALKERS + 2):
            einval(check(g, cfg(w), 1, 0), "walkers")
        einval(check(g, cfg(reserved=1), 1, 0), "reserved")
        for n in (0, -1, nat.MCCFR_MAX_RUNS + 1):
            einval(check(g, cfg(n=2), n, 0), "n must")
        einval(check(g, None, 1, 0), "null")
        einval(check(g, cfg(), 1, -1), "iters")
        # the second of two: every cfg is checked
        two = (nat.MccfrCfg * 2)(nat.MccfrCfg(1, 64, 0), nat.MccfrCfg(2, 63, 0))
        einval(check(g, two, 2, 0), "even")
    einval(check(2, cfg(), 1, 0), "game")
    # the overflow bound: W x iterations <= 2^62 / (Q x 2 max|pay|), from the game's own pay table
    for name, g in GAMES.items():
        maxpay = float(np.abs(trees[name].pay).max())
        assert maxpay == {"leduc": 5.0, "kuhn": 2.0}[name]
        bound = int(2.0 ** 62 / (nat.MCCFR_Q * 2.0 * maxpay))
        for w in (2, 1 << 10, nat.MCCFR_MAX_WALKERS):
            assert check(g, cfg(w), 1, bound // w) == nat.OK
            einval(check(g, cfg(w), 1, bound // w + 1), "overflow")
            assert str(bound).encode() in L.nfsp_last_error(), L.nfsp_last_error()
    # no rule needs a context, a handle or a device to answer
    h = nat.P()
    einval(L.nfsp_mccfr_create(None, None, 1, None), "null")
    einval(L.nfsp_mccfr_create(None, cfg(), 1, C.byref(h)), "null")            # the context
    einval(L.nfsp_mccfr_create(None, cfg(), 0, C.byref(h)), "n must")
    assert not h.value
    einval(L.nfsp_mccfr_run(None, 1), "null")
    einval(L.nfsp_mccfr_run(None, -1), "iters")
    einval(L.nfsp_mccfr_iterations(None, None), "null")
    out = (nat.I64 * 2)()
    einval(L.nfsp_mccfr_counts(None, 0, out), "null")
    einval(L.nfsp_mccfr_counts(None, -1, out), "run")
    einval(L.nfsp_mccfr_average(None, 0, None), "null")
    einval(L.nfsp_mccfr_average(None, -1, None), "run")
    einval(L.nfsp_mccfr_state(None, 0, None, None), "null")
    einval(L.nfsp_mccfr_state(None, -1, None, None), "run")
    einval(L.nfsp_mccfr_destroy(None), "null")


def test_philox_restatement_known_answers():
    """Philox4x32-10's published vectors (Random123 kat_vectors), first word."""
    assert int(mr.philox_x(0, 0, 0, 0, 0, 0)) == 0x6627E8D5
    assert int(mr.philox_x(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)) == 0x408F276D
    assert int(mr.philox_x(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)) == 0xD16CFE09


# ---- b. a run does not depend on how it is split, nor on what runs beside it -------------------------
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_split_runs_are_equal(trees, game):
    t = trees[game]
    a, b = mr.MccfrRef(t, 5, 32).run(8), mr.MccfrRef(t, 5, 32).run(3).run(5)
    assert np.array_equal(a.R, b.R) and np.array_equal(a.S, b.S)
    assert (a.t, a.traversals, a.terminals) == (b.t, b.traversals, b.terminals) == (8, 2 * 32 * 8, a.terminals)
    assert a.terminals > a.traversals                  # a traversal is a subtree, not a hand
    other = mr.MccfrRef(t, 6, 32).run(8)               # the seed is the run's own
    assert not np.array_equal(a.R, other.R)
    # an illegal raise never moves; S only grows
    assert np.all(a.R[~t.legal][:, :, 2] == 0) and np.all(a.S[~t.legal][:, :, 2] == 0) and np.all(a.S >= 0)


# ---- c. a traversal's increments are unbiased ----------------------------------------------------------
def seat_entries(tree, seat):
    """[ndec, 3, 3] bool: the legal (row, rank, action) where ``seat`` acts."""
    m = np.zeros((tree.ndec, 3, 3), bool)
    m[tree.seat == seat] = True
    m[~tree.legal, :, 2] = False
    return m


def probe(tree, seed, R, t, walkers=4096):
    """Seat 0's half-iteration of ``walkers`` traversals at the strategy of the regrets R: per entry
    the mean increment per traversal in chips, its sample variance, and the exact value."""
    p = mr.MccfrRef(tree, seed, walkers, moments=True)
    p.R = R.copy()
    p.t = t
    sigma = p.sigma()
    p.half(0)
    n = walkers // 2                                   # the walkers of the one dealer that reaches a row
    mean = (p.R - R) / mr.Q / n
    assert np.array_equal(mean, p.m1 / n)
    var = (p.m2 - n * mean * mean) / (n - 1)
    return mean, var, mr.exact_increments(tree, sigma, 0), n


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_increments_are_unbiased_at_the_uniform_strategy(trees, game, seed):
    """Prototype: every entry has positive variance and the worst z is 4.55."""
    t = trees[game]
    mean, var, exact, n = probe(t, seed, np.zeros((t.ndec, 3, 3), np.int64), 0)
    e = seat_entries(t, 0)
    assert int(e.sum()) == SEAT0_ENTRIES[game]
    assert np.all(mean[~e] == 0) and np.all(exact[~e] == 0)
    assert np.all(var[e] > 0)                          # no entry is skipped
    z = np.abs(mean[e] - exact[e]) / np.sqrt(var[e] / n)
    print(game, seed, "entries", int(e.sum()), "worst z", z.max())
    assert z.max() <= 6.0


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_increments_are_unbiased_at_a_learned_strategy(trees, game, seed):
    """The strategy after 4 iterations at W = 64.  Prototype: worst z 4.15; the entries no
    traversal reached have |exact| <= 0.0078 chips."""
    t = trees[game]
    r = mr.MccfrRef(t, seed, 64).run(4)
    assert not np.array_equal(r.sigma(), t.uniform())
    mean, var, exact, n = probe(t, seed, r.R, r.t)
    e = seat_entries(t, 0)
    pos = e & (var > 0)
    z = np.abs(mean[pos] - exact[pos]) / np.sqrt(var[pos] / n)
    rest = e & ~pos                                    # never reached (or reached with a constant increment)
    worst = np.abs(mean[rest] - exact[rest]).max() if rest.any() else 0.0
    print(game, seed, "entries", int(pos.sum()), "worst z", z.max(), "without variance", int(rest.sum()), worst)
    assert z.max() <= 6.0
    assert worst <= 0.05


# ---- d. the average converges ---------------------------------------------------------------------------
@pytest.mark.parametrize("game,walkers,iters,cap", [("kuhn", 64, 64, 0.2917), ("leduc", 128, 32, 0.5778)])
def test_average_converges(trees, game, walkers, iters, cap):
    """Seed 1; the caps are a quarter of the uniform policy's exploitability.  Measured: kuhn
    0.0427, leduc 0.351."""
    t = trees[game]
    assert abs(4 * cap - UNIFORM_GAP[game]) <= 5e-4
    u = t.uniform()
    assert abs(pr.walk(t, u, u)["exploitability"] - UNIFORM_GAP[game]) <= 1e-4
    r = mr.MccfrRef(t, 1, walkers).run(iters)
    avg = r.average()
    assert np.abs(avg.sum(-1) - 1.0).max() <= 1e-12 and np.all(avg[~t.legal][:, :, 2] == 0)
    x = pr.walk(t, avg, avg)["exploitability"]
    print(game, walkers, iters, "exploitability", x, "traversals", r.traversals, "terminals", r.terminals)
    assert r.traversals == 2 * walkers * iters
    assert 0 <= x < cap

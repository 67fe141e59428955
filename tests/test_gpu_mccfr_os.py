"""nfsp_mccfr_os_* (csrc/mccfr.hip k_mccfr_os_walk, k_mccfr_apply) on the GPU against the numpy
restatement of the rule (tests/mccfr_os_ref.py), as tests/test_gpu_mccfr.py holds external
sampling to its own.  R and S are int64 sums of per-walker integers, so they and both counts are
compared int64 for int64, whatever the grid; the average is compared through the existing
evaluator, and the unbiasedness of the increments (tests/test_mccfr_os_ref.py) is checked at the
size only the device reaches."""
import numpy as np
import pytest

import mccfr_os_ref as osr
import mccfr_ref as mr
import policy_ref as pr

pytestmark = pytest.mark.gpu
NAMES = {0: "leduc", 1: "kuhn"}
EPS = 0.6
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


def ref_after(trees, game, seed, walkers, eps, iters):
    """The restatement's (R, S, traversals, terminals, average) after 1 .. iters iterations: computed
    once per run and left unchanged."""
    key = (game, seed, walkers, eps)
    have = _REFS.setdefault(key, [])
    r = None
    while len(have) < iters:
        if r is None:
            r = osr.OsRef(trees[game], seed, walkers, eps)
            for R, S, _, terminals, _ in have[-1:]:
                r.R, r.S, r.t, r.terminals = R.copy(), S.copy(), len(have), terminals
        r.run(1)
        have.append((r.R.copy(), r.S.copy(), r.traversals, r.terminals, r.average()))
    return have[iters - 1]


def same(solver, run, want, what):
    R, S = solver.state(run)
    assert R.dtype == S.dtype == np.int64
    bad = int((R != want[0]).sum()), int((S != want[1]).sum())
    assert bad == (0, 0), (what, "entries of R, S that differ", bad)
    assert solver.counts(run) == (want[2], want[3]), what


# ---- e. the bits ---------------------------------------------------------------------------------------
def walkers_cases(nat):
    B = nat.MCCFR_WG_WALKERS
    return [2, 62, 64, 66, B - 2, B, B + 2, 2 * B + 2]


def three_iterations(ev, ctxs, trees, game, seed, W, eps):
    s = ev.MccfrOsSolver(ctxs[game], [(seed, W, eps)])
    assert s.sampling == 1
    z = np.zeros((trees[game].ndec, 3, 3), np.int64)
    same(s, 0, (z, z, 0, 0), "at creation")
    assert np.array_equal(s.average_table(0), trees[game].uniform())
    for it in (1, 2, 3):
        s.run(1)
        assert s.iterations == it
        want = ref_after(trees, game, seed, W, eps, it)
        assert want[2] == want[3] == 2 * W * it            # one terminal per traversal
        same(s, 0, want, (NAMES[game], W, eps, it))
    s.close()


@pytest.mark.parametrize("case", range(8))
@pytest.mark.parametrize("game", [1, 0])
def test_tables_and_counts_equal_the_restatement(pkg, ev, ctxs, trees, game, case):
    """W around a wave, around a workgroup's walkers and past two workgroups; after 1, 2 and 3
    iterations, each continued from the one before."""
    three_iterations(ev, ctxs, trees, game, 11 + case, walkers_cases(pkg.native)[case], EPS)


@pytest.mark.parametrize("eps", [0.0625, 1.0])
@pytest.mark.parametrize("case", [3, 6])
@pytest.mark.parametrize("game", [1, 0])
def test_tables_at_the_ends_of_epsilon(pkg, ev, ctxs, trees, game, case, eps):
    """W = 66 and B + 2 at the least exploration rate (the largest importance weights) and at 1
    (seat i samples uniformly, sigma only weighs)."""
    three_iterations(ev, ctxs, trees, game, 11 + case, walkers_cases(pkg.native)[case], eps)


@pytest.mark.parametrize("game", [1, 0])
def test_runs_of_a_handle_are_the_runs_alone_and_repeat(pkg, ev, ctxs, trees, game):
    B = pkg.native.MCCFR_WG_WALKERS
    cfgs = [(3, 66, 0.25), (4, B + 2, EPS), (5, 6, 1.0)]  # the grid is sized by the second
    three = ev.MccfrOsSolver(ctxs[game], cfgs).run(2)
    again = ev.MccfrOsSolver(ctxs[game], cfgs).run(2)
    for k, (seed, W, eps) in enumerate(cfgs):
        want = ref_after(trees, game, seed, W, eps, 2)
        same(three, k, want, ("of three", k))
        same(again, k, want, ("repeated", k))
        alone = ev.MccfrOsSolver(ctxs[game], [cfgs[k]]).run(2)
        same(alone, 0, want, ("alone", k))
        assert np.array_equal(alone.average_table(0), three.average_table(k))
        alone.close()
    three.close()
    again.close()


@pytest.mark.parametrize("game", [1, 0])
def test_split_runs_are_equal(pkg, ev, ctxs, trees, game):
    a = ev.MccfrOsSolver(ctxs[game], [(7, 130, EPS)]).run(1).run(2)
    b = ev.MccfrOsSolver(ctxs[game], [(7, 130, EPS)]).run(3)
    assert a.iterations == b.iterations == 3
    want = ref_after(trees, game, 7, 130, EPS, 3)
    same(a, 0, want, "run(1) then run(2)")
    same(b, 0, want, "run(3)")
    assert a.counts(0) == (2 * 130 * 3, 2 * 130 * 3)
    assert np.array_equal(a.average_table(0), b.average_table(0))
    a.run(0)
    same(a, 0, want, "run(0)")
    a.close()
    b.close()


def test_sampling_names_the_kind(pkg, ev, ctxs):
    es, os_ = ev.MccfrSolver(ctxs[1], [(1, 2)]), ev.MccfrOsSolver(ctxs[1], [(1, 2, EPS)])
    assert (es.sampling, os_.sampling) == (0, 1)
    es.close()
    os_.close()


def test_run_past_the_overflow_bound_is_refused(pkg, ev, ctxs, trees):
    s = ev.MccfrOsSolver(ctxs[0], [(1, 2, 0.0625)]).run(1)
    bound = osr.bound(trees[0], 0.0625)
    with pytest.raises(pkg.native.NativeError, match="overflow.*%d" % bound):
        s.run(bound // 2)                              # 1 + bound // 2 iterations in all: one too many
    assert s.iterations == 1
    same(s, 0, ref_after(trees, 0, 1, 2, 0.0625, 1), "after the refusal")
    with pytest.raises(pkg.native.NativeError, match="epsilon"):
        ev.MccfrOsSolver(ctxs[1], [(1, 2, 0.01)])
    with pytest.raises(pkg.native.NativeError, match="even"):
        ev.MccfrOsSolver(ctxs[1], [(1, 3, EPS)])
    s.close()


# ---- f. contention -------------------------------------------------------------------------------------
def test_every_walker_on_the_same_entries(pkg, ev, ctxs, trees):
    """Kuhn has 24 information sets: 65,536 walkers a half-iteration all add to the same few LDS
    and device words."""
    W = 1 << 16
    s = ev.MccfrOsSolver(ctxs[1], [(9, W, EPS)]).run(1)
    same(s, 0, ref_after(trees, 1, 9, W, EPS, 1), "kuhn W = 65536")
    assert s.counts(0) == (2 * W, 2 * W)
    s.close()


# ---- g. the average ------------------------------------------------------------------------------------
@pytest.mark.parametrize("game,walkers,iters,cap", [(1, 64, 256, 0.2917), (0, 256, 128, 0.5778)])
def test_average_scores_as_the_restatement_and_converges(pkg, ev, ctxs, trees, game, walkers, iters, cap):
    """The runs of tests/test_mccfr_os_ref.py's convergence test, seed 1, eps = 0.6: below a quarter
    of the uniform policy's exploitability."""
    t = trees[game]
    s = ev.MccfrOsSolver(ctxs[game], [(1, walkers, EPS)]).run(iters)
    r = osr.OsRef(t, 1, walkers, EPS).run(iters)
    want = (r.R, r.S, r.traversals, r.terminals, r.average())
    same(s, 0, want, "the run")
    got = ev.evaluate(ctxs[game], s.average(0), s.average(0))
    ref = pr.walk(t, want[4], want[4])
    print(NAMES[game], "exploitability", got["exploitability"], "restated", ref["exploitability"])
    for k in ("br0", "br1", "exploitability", "value0"):
        assert abs(got[k] - ref[k]) <= 1e-12, k
    assert 0 <= got["exploitability"] < cap
    avg = s.average_table(0)
    assert np.abs(avg - want[4]).max() <= 1e-15
    s.close()


# ---- h. unbiased at full size ----------------------------------------------------------------------------
def test_increments_are_unbiased_at_a_million_walkers(pkg, ev, ctxs, trees):
    """Leduc, W = 2^20, eps = 0.6, the uniform strategy: after one iteration seat 0's rows of R hold
    its half-iteration's increments, and their mean per traversal is within 6 standard errors (the
    per-traversal variance from the restatement's W = 65,536 probe) + the fixed point's 2^-24 of the
    exact counterfactual regret difference.  The LDS atomics and the flush at full size."""
    t = trees[0]
    W, W1 = 1 << 20, 1 << 16
    p = osr.OsRef(t, 1, W1, EPS, moments=True)
    p.half(0)
    n1 = W1 // 2
    m1 = p.m1 / n1
    var1 = (p.m2 - n1 * m1 * m1) / (n1 - 1)
    exact = mr.exact_increments(t, t.uniform(), 0)
    e = np.zeros((t.ndec, 3, 3), bool)
    e[t.seat == 0] = True
    e[~t.legal, :, 2] = False
    assert int(e.sum()) == 507 and np.all(var1[e] > 0)
    s = ev.MccfrOsSolver(ctxs[0], [(1, W, EPS)]).run(1)
    R, _ = s.state(0)
    traversals, terminals = s.counts(0)
    assert traversals == terminals == 2 * W
    mean = R / mr.Q / (W // 2)
    err = np.abs(mean - exact)[e]
    bound = 6.0 * np.sqrt(var1[e] / (W // 2)) + 2.0 ** -24
    print("worst |mean - exact| / bound", (err / bound).max())
    assert np.all(err <= bound)
    s.close()

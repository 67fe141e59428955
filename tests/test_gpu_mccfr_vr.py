"""nfsp_mccfr_vr_* (csrc/mccfr.hip k_mccfr_vr_walk, k_mccfr_apply, k_mccfr_vr_apply) on the GPU
against the numpy restatement of the rule (tests/mccfr_vr_ref.py), as tests/test_gpu_mccfr_os.py
holds outcome sampling to its own.  R, S, Bs and Bn are int64 sums of per-walker integers, so they
and both counts are compared int64 for int64, whatever the grid; B enters every later iteration, so
iterations 2 and 3 hold k_mccfr_vr_apply's table to the restatement's as well."""
import numpy as np
import pytest

import mccfr_ref as mr
import mccfr_vr_ref as vrr
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


def snapshot(r):
    return (r.R.copy(), r.S.copy(), r.Bs.copy(), r.Bn.copy(), r.traversals, r.terminals, r.average())


def ref_after(trees, game, seed, walkers, eps, iters):
    """The restatement's (R, S, Bs, Bn, traversals, terminals, average) after 1 .. iters iterations:
    computed once per run and left unchanged."""
    key = (game, seed, walkers, eps)
    have = _REFS.setdefault(key, [])
    r = None
    while len(have) < iters:
        if r is None:
            r = vrr.VrRef(trees[game], seed, walkers, eps)
            for R, S, Bs, Bn, _, terminals, _ in have[-1:]:
                r.R, r.S, r.Bs, r.Bn, r.t, r.terminals = R.copy(), S.copy(), Bs.copy(), Bn.copy(), len(have), terminals
        r.run(1)
        have.append(snapshot(r))
    return have[iters - 1]


def same(solver, run, want, what):
    R, S = solver.state(run)
    Bs, Bn = solver.baseline(run)
    assert R.dtype == S.dtype == Bs.dtype == Bn.dtype == np.int64
    bad = tuple(int((got != ref).sum()) for got, ref in zip((R, S, Bs, Bn), want[:4]))
    assert bad == (0, 0, 0, 0), (what, "entries of R, S, Bs, Bn that differ", bad)
    assert solver.counts(run) == (want[4], want[5]), what


# ---- the bits --------------------------------------------------------------------------------------------
def walkers_cases(nat):
    B = nat.MCCFR_WG_WALKERS
    return [2, 62, 64, 66, B - 2, B, B + 2, 2 * B + 2]


def three_iterations(ev, ctxs, trees, game, seed, W, eps):
    s = ev.MccfrVrSolver(ctxs[game], [(seed, W, eps)])
    assert s.sampling == 2
    z = np.zeros((trees[game].ndec, 3, 3), np.int64)
    same(s, 0, (z, z, z, z, 0, 0), "at creation")
    assert np.array_equal(s.average_table(0), trees[game].uniform()) and not s.baseline_table(0).any()
    for it in (1, 2, 3):
        s.run(1)
        assert s.iterations == it
        want = ref_after(trees, game, seed, W, eps, it)
        assert want[4] == want[5] == 2 * W * it            # one terminal per traversal
        same(s, 0, want, (NAMES[game], W, eps, it))
    assert np.array_equal(s.baseline_table(0), vrr.baseline_table(trees[game], want[2], want[3]))
    s.close()


@pytest.mark.parametrize("case", range(8))
@pytest.mark.parametrize("game", [1, 0])
def test_tables_and_counts_equal_the_restatement(pkg, ev, ctxs, trees, game, case):
    """W = 2, 62, 64, 66, 1,022, 1,024, 1,026 and 2,050 at eps = 0.6: around a wave, around a
    workgroup's walkers and past two workgroups; after 1, 2 and 3 iterations, each continued from the
    one before."""
    assert walkers_cases(pkg.native) == [2, 62, 64, 66, 1022, 1024, 1026, 2050]
    three_iterations(ev, ctxs, trees, game, 11 + case, walkers_cases(pkg.native)[case], EPS)


@pytest.mark.parametrize("eps", [0.0625, 1.0])
@pytest.mark.parametrize("case", [3, 6])
@pytest.mark.parametrize("game", [1, 0])
def test_tables_at_the_ends_of_epsilon(pkg, ev, ctxs, trees, game, case, eps):
    """W = 66 and 1,026 at the least exploration rate (the largest corrections) and at 1."""
    three_iterations(ev, ctxs, trees, game, 11 + case, walkers_cases(pkg.native)[case], eps)


# ---- the handle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", [1, 0])
def test_runs_of_a_handle_are_the_runs_alone_and_repeat(pkg, ev, ctxs, trees, game):
    B = pkg.native.MCCFR_WG_WALKERS
    cfgs = [(3, 66, 0.25), (4, B + 2, EPS), (5, 6, 1.0)]  # the grid is sized by the second
    three = ev.MccfrVrSolver(ctxs[game], cfgs).run(2)
    again = ev.MccfrVrSolver(ctxs[game], cfgs).run(2)
    for k, (seed, W, eps) in enumerate(cfgs):
        want = ref_after(trees, game, seed, W, eps, 2)
        same(three, k, want, ("of three", k))
        same(again, k, want, ("repeated", k))
        alone = ev.MccfrVrSolver(ctxs[game], [cfgs[k]]).run(2)
        same(alone, 0, want, ("alone", k))
        assert np.array_equal(alone.average_table(0), three.average_table(k))
        alone.close()
    three.close()
    again.close()


@pytest.mark.parametrize("game", [1, 0])
def test_split_runs_are_equal(pkg, ev, ctxs, trees, game):
    a = ev.MccfrVrSolver(ctxs[game], [(7, 130, EPS)]).run(1).run(2)
    b = ev.MccfrVrSolver(ctxs[game], [(7, 130, EPS)]).run(3)
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


@pytest.mark.parametrize("game", [1, 0])
def test_a_set_baseline_comes_back_and_the_next_iteration_uses_it(pkg, ev, ctxs, trees, game):
    """An arbitrary baseline (random sums in [-P, P] Q x count, counts 0 .. 3, and past the clamp at a
    few entries) set on the second run of two after one iteration: the round trip returns it, the other
    run keeps its own, and the next iteration equals the restatement's from the same tables."""
    t = trees[game]
    rng = np.random.RandomState(8)
    P = vrr.maxpay(t)
    Bn = rng.randint(0, 4, (t.ndec, 3, 3)).astype(np.int64)
    Bs = mr.llrint(rng.uniform(-P, P, Bn.shape) * mr.Q) * Bn
    hot = (Bn > 0) & (rng.uniform(size=Bn.shape) < 0.1)
    Bs[hot] *= 3                                       # |Bs / (Bn Q)| up to 3 P: clamped
    cfgs = [(21, 66, EPS), (22, 130, EPS)]
    s = ev.MccfrVrSolver(ctxs[game], cfgs).run(1)
    r = vrr.VrRef(t, 22, 130, EPS).run(1)
    same(s, 1, snapshot(r), "before")
    assert s.set_baseline(1, Bs, Bn) is s
    got = s.baseline(1)
    assert np.array_equal(got[0], Bs) and np.array_equal(got[1], Bn)
    r.Bs, r.Bn = Bs.copy(), Bn.copy()
    B = s.baseline_table(1)
    assert np.array_equal(B, r.baseline()) and np.abs(B).max() == P and np.all(B[Bn == 0] == 0)
    same(s, 1, snapshot(r), "after set_baseline: R, S and the counts are left")
    same(s, 0, ref_after(trees, game, 21, 66, EPS, 1), "the other run")
    s.run(1)
    same(s, 1, snapshot(r.run(1)), "the iteration after set_baseline")
    same(s, 0, ref_after(trees, game, 21, 66, EPS, 2), "the other run, an iteration on")
    # what it refuses, the tables left as they are
    nat = pkg.native
    before = s.baseline(1)
    neg, orphan, far = Bn.copy(), Bs.copy(), Bs.copy()
    neg[0, 0, 0] = -1
    k = tuple(np.argwhere(Bn == 0)[0])
    orphan[k] = 1
    far[tuple(np.argwhere(Bn > 0)[0])] = (1 << 61) + 1
    for bs, bn, word in ((Bs, neg, "negative"), (orphan, Bn, "count is 0"), (far, Bn, "2\\^61")):
        with pytest.raises(nat.NativeError, match=word):
            s.set_baseline(1, bs, bn)
    with pytest.raises(nat.NativeError, match="run"):
        s.set_baseline(2, Bs, Bn)
    with pytest.raises(ValueError):
        s.set_baseline(1, Bs[:-1], Bn[:-1])
    after = s.baseline(1)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    s.close()


def test_every_walker_on_the_same_entries(pkg, ev, ctxs, trees):
    """Kuhn has 24 information sets: 65,536 walkers a half-iteration all add to the same few LDS
    and device words, dBn's among them."""
    W = 1 << 16
    s = ev.MccfrVrSolver(ctxs[1], [(9, W, EPS)]).run(1)
    same(s, 0, ref_after(trees, 1, 9, W, EPS, 1), "kuhn W = 65536")
    assert s.counts(0) == (2 * W, 2 * W)
    s.close()


def test_run_past_the_overflow_bound_is_refused(pkg, ev, ctxs, trees):
    s = ev.MccfrVrSolver(ctxs[0], [(1, 2, 0.0625)]).run(1)
    bound = vrr.bound(trees[0], 0.0625)
    with pytest.raises(pkg.native.NativeError, match="overflow.*%d" % bound):
        s.run(bound // 2)                              # 1 + bound // 2 iterations in all: one too many
    assert s.iterations == 1
    same(s, 0, ref_after(trees, 0, 1, 2, 0.0625, 1), "after the refusal")
    with pytest.raises(pkg.native.NativeError, match="epsilon"):
        ev.MccfrVrSolver(ctxs[1], [(1, 2, 0.01)])
    with pytest.raises(pkg.native.NativeError, match="even"):
        ev.MccfrVrSolver(ctxs[1], [(1, 3, EPS)])
    s.close()


# ---- the average -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game,walkers,iters", [(1, 64, 64), (0, 256, 16)])
def test_average_scores_as_the_restatement(pkg, ev, ctxs, trees, game, walkers, iters):
    t = trees[game]
    s = ev.MccfrVrSolver(ctxs[game], [(1, walkers, EPS)]).run(iters)
    want = snapshot(vrr.VrRef(t, 1, walkers, EPS).run(iters))
    same(s, 0, want, "the run")
    got = ev.evaluate(ctxs[game], s.average(0), s.average(0))
    ref = pr.walk(t, want[6], want[6])
    print(NAMES[game], "exploitability", got["exploitability"], "restated", ref["exploitability"])
    for k in ("br0", "br1", "exploitability", "value0"):
        assert abs(got[k] - ref[k]) <= 1e-12, k
    assert np.abs(s.average_table(0) - want[6]).max() <= 1e-15
    s.close()


# ---- convergence -------------------------------------------------------------------------------------------
def test_converges_below_outcome_sampling(pkg, ev, ctxs, trees):
    """Leduc, W = 256, 128 iterations, eps = 0.6, seeds 1-4 in one handle each: the seeds' mean
    exploitability is below MccfrOsSolver's at the same configuration.  The restatements alone
    (tests/test_mccfr_vr_ref.py): 0.350 against 0.446, so the run is not lengthened."""
    cfgs = [(seed, 256, EPS) for seed in (1, 2, 3, 4)]
    xs = {}
    for name, cls in (("os", ev.MccfrOsSolver), ("vr", ev.MccfrVrSolver)):
        s = cls(ctxs[0], cfgs).run(128)
        avgs = [s.average(k) for k in range(4)]
        xs[name] = [r["exploitability"] for r in ev.evaluate_batch(ctxs[0], [(a, a) for a in avgs])]
        assert [s.counts(k) for k in range(4)] == [(2 * 256 * 128,) * 2] * 4
        s.close()
    print("leduc exploitability: OS", xs["os"], "VR", xs["vr"])
    assert 0 <= np.mean(xs["vr"]) < np.mean(xs["os"])


# ---- the solvers that were there ---------------------------------------------------------------------------
def test_the_other_kinds_keep_their_number_and_have_no_baseline(pkg, ev, ctxs, trees):
    nat = pkg.native
    z = np.zeros((trees[1].ndec, 3, 3), np.int64)
    zp = z.ctypes.data_as(nat.P)
    es, os_ = ev.MccfrSolver(ctxs[1], [(1, 2)]), ev.MccfrOsSolver(ctxs[1], [(1, 2, EPS)])
    assert (es.sampling, os_.sampling) == (0, 1)
    for s in (es, os_):
        for fn in (s.ctx.L.nfsp_mccfr_set_baseline, s.ctx.L.nfsp_mccfr_baseline):
            assert fn(s.h, 0, zp, zp) == nat.EINVAL
            assert b"baseline-corrected" in s.ctx.L.nfsp_last_error()
        s.run(1)                                       # and they go on as before
        assert s.iterations == 1
        s.close()

"""nfsp_mccfr_net_* (csrc/mccfr.hip k_mccfr_net_apply behind the unchanged walks and k_mccfr_x_apply) on
the GPU against the numpy restatement of the rule (tests/mccfr_net_ref.py).

A free-running comparison would be wrong here: an f32 difference of 1e-7 in a net can flip a sampled
choice, and then integer tables differ.  So the restatement is teacher-forced: each of its half-iterations
reads the sigma the device's walkers read, and then R, S, Sw (as its 64 bits), Bs, Bn and the counts agree
bit for bit.  The nets are held to fitnet_ref.fit from the device's own weights before the run and the
targets of the device's own R, and the heads to the forward of the device's own weights, both within
tests/test_gpu_fitnet.py's 1e-5; sigma is regret matching of the device's own heads, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import fitnet_ref as fr
import mccfr_net_ref as nr
import mccfr_os_ref as osr
import mccfr_ref as mr
import mccfr_vr_ref as vrr
import mccfr_x_ref as xr

pytestmark = pytest.mark.gpu
NAMES = {0: "leduc", 1: "kuhn"}
KINDS = {0: mr.MccfrRef, 1: osr.OsRef, 2: vrr.VrRef}
EPS = 0.6
BAR = 1e-5                                             # tests/test_gpu_fitnet.py's, per weight and per head
# (regret, average, target, loss, lr, momentum) of the runs of a handle: all differ by run
RULES = [("plain", "uniform", "avg", "mse", 0.5, 0.9), ("plus", "linear", "rowmax", "huber", 0.1, 0.5),
         ("plus", "uniform", "rowmax", "mse", 0.25, 0.0)]
CODES = {"plain": 0, "plus": 1, "uniform": 0, "linear": 1, "avg": nr.AVG, "rowmax": nr.ROWMAX, "mse": fr.MSE,
         "huber": fr.HUBER}


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


def cfgs_of(n, sampling, W, K, seed):
    eps = EPS if sampling else 0.0
    return [(seed + k, W, eps) + RULES[k][:3] + (K,) + RULES[k][3:] for k in range(n)]


def glorot_pair(ev, init_seed):
    rng = np.random.RandomState(init_seed)
    return ev.glorot_net(rng), ev.glorot_net(rng)


def ref_of(ev, tree, sampling, cfg, init_seed):
    seed, W, eps, reg, avg, tgt, K, loss, lr, mu = cfg
    args = (tree, seed, W) + ((eps,) if sampling else ())
    return nr.NetRef(KINDS[sampling])(*args, nets=glorot_pair(ev, init_seed), target=CODES[tgt], fit_steps=K,
                                      loss=CODES[loss], lr=lr, momentum=mu, regret=CODES[reg], average=CODES[avg])


def bits(x):
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.float64, np.float32)
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def same_tables(solver, run, ref, what, sampling):
    R, S = solver.state(run)
    got = [R, S, bits(solver.weighted(run))]
    want = [ref.R, ref.S, bits(ref.Sw)]
    if sampling == 2:
        got += list(solver.baseline(run))
        want += [ref.Bs, ref.Bn]
    bad = tuple(int((g != w).sum()) for g, w in zip(got, want))
    assert not any(bad), (what, "entries of R, S, Sw (as uint64)[, Bs, Bn] that differ", bad)
    assert solver.counts(run) == (ref.traversals, ref.terminals), what


def seat_rows(tree, seat):
    return tree.seat == seat


def fit_from(tree, cfg, seat, R, tw, w, v):
    """fitnet_ref.fit of a seat's net from (w, v) on the targets of R: (w, v, losses, the heads [N, 3])."""
    seed, W, eps, reg, avg, tgt, K, loss, lr, mu = cfg
    prob = fr.problem(tree, seat, nr.targets(tree, R, W, tw, CODES[tgt]))
    w1, v1, losses = fr.fit(w, prob, fr.ACT_LINEAR, CODES[loss], lr, mu, K, v0=v)
    return w1, v1, losses, prob


def heads_of(tree, seat, w, prob):
    return fr.forward(np.asarray(w, np.float32), prob[0])[2]


def check_sigma(tree, solver, run, what):
    """sigma is regret matching in f64 of the device's own z, sigma_tab of its own R: bit for bit."""
    z = solver.head(run)
    assert z.dtype == np.float32
    assert np.array_equal(bits(solver.sigma_table(run, "net")), bits(nr.sigma_of(tree, z))), what
    assert np.array_equal(bits(solver.sigma_table(run, "table")), bits(mr.match(tree, solver.state(run)[0]))), what


def check_loss(got, want, what):
    """The row terms are f32 and summed in double on both sides; the heads agree to about 1e-6 relative, a
    squared error to twice that: 1e-4 relative, with a floor where the loss is rounding itself."""
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-12, (what, got, want)


# ---- the replay ------------------------------------------------------------------------------------------------
def walkers_cases(nat):
    return [2, 66, nat.MCCFR_WG_WALKERS + 2]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("K", [0, 1, 3])
@pytest.mark.parametrize("wcase", range(3))
@pytest.mark.parametrize("sampling", [0, 1, 2])
@pytest.mark.parametrize("game", [1, 0])
def test_replay_iteration_by_iteration(pkg, ev, ctxs, trees, game, sampling, wcase, K, n):
    """Three iterations, one run(1) each, every run of the handle with its own restatement."""
    assert walkers_cases(pkg.native) == [2, 66, 1026]
    W = walkers_cases(pkg.native)[wcase]
    t = trees[game]
    cfgs = cfgs_of(n, sampling, W, K, 100 + 10 * wcase + K)
    inits = [7 + k for k in range(n)]
    s = ev.MccfrNetSolver(ctxs[game], cfgs, sampling, inits)
    refs = [ref_of(ev, t, sampling, cfgs[k], inits[k]) for k in range(n)]
    assert s.sampling == sampling and [s.rule(k) for k in range(n)] == [(CODES[c[3]], CODES[c[4]]) for c in cfgs]
    worst = {"w": 0.0, "v": 0.0, "z": 0.0}
    rows = [seat_rows(t, 0), seat_rows(t, 1)]
    for it in (1, 2, 3):
        before = [(s.sigma_table(k), s.net(k, 0), s.net(k, 1), s.head(k)) for k in range(n)]
        s.run(1)
        assert s.iterations == it
        for k in range(n):
            sg0, net0, net1, z0 = before[k]
            sg1 = s.sigma_table(k)
            mixed = sg0.copy()
            mixed[rows[0]] = sg1[rows[0]]                  # half 1 reads seat 0's new rows and seat 1's old ones
            refs[k].sigma_hook = lambda i, a=sg0, b=mixed: a if i == 0 else b
            refs[k].run(1)
            what = (NAMES[game], sampling, W, K, n, k, it)
            same_tables(s, k, refs[k], what, sampling)
            check_sigma(t, s, k, what)
            R = s.state(k)[0]
            z1 = s.head(k)
            losses = s.fit_loss(k)
            for seat, (w_b, v_b) in ((0, net0), (1, net1)):
                w_a, v_a = s.net(k, seat)
                rw, rv, rl, prob = fit_from(t, cfgs[k], seat, R, float(it), w_b, v_b)
                d, r = fr.seat_sets(t, seat)
                dw, dv = np.abs(w_a - rw).max(), np.abs(v_a - rv).max()
                dz = np.abs(z1[d, r] - heads_of(t, seat, w_a, prob)).max()
                worst = {"w": max(worst["w"], dw), "v": max(worst["v"], dv), "z": max(worst["z"], dz)}
                assert dw <= BAR and dv <= BAR, (what, seat, dw, dv)
                assert dz <= BAR, (what, seat, dz)
                check_loss(losses[seat], rl, (what, seat))
                if K == 0:
                    assert np.array_equal(bits(w_a), bits(w_b)) and np.array_equal(bits(v_a), bits(v_b))
                    assert np.array_equal(bits(z1[d, r]), bits(z0[d, r]))
    print(NAMES[game], "sampling", sampling, "W", W, "K", K, "n", n, "largest |dw| %.3g |dv| %.3g |dz| %.3g"
          % (worst["w"], worst["v"], worst["z"]))
    s.close()


# ---- creation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 3])
@pytest.mark.parametrize("game", [1, 0])
def test_creation_is_the_fit_toward_zero_regrets(pkg, ev, ctxs, trees, game, K):
    """R and S are 0, no iteration is counted, both nets are the K-step fit toward 0 from the initial nets
    with v = 0, and the first sigma is the nets', not uniform."""
    t = trees[game]
    cfgs = cfgs_of(3, 2, 66, K, 40)
    s = ev.MccfrNetSolver(ctxs[game], cfgs, 2, [3, 4, 5])
    zero = np.zeros((t.ndec, 3, 3), np.int64)
    assert s.iterations == 0
    for k in range(3):
        R, S = s.state(k)
        assert not R.any() and not S.any() and not s.weighted(k).any() and s.counts(k) == (0, 0)
        assert np.array_equal(s.average_table(k), t.uniform())
        assert np.array_equal(s.sigma_table(k, "table"), t.uniform())
        check_sigma(t, s, k, ("creation", k))
        assert not np.array_equal(s.sigma_table(k), t.uniform())
        losses = s.fit_loss(k)
        for seat, w0 in enumerate(glorot_pair(ev, 3 + k)):
            rw, rv, rl, prob = fit_from(t, cfgs[k], seat, zero, 1.0, w0, np.zeros(fr.NP, np.float32))
            w, v = s.net(k, seat)
            assert np.abs(w - rw).max() <= BAR and np.abs(v - rv).max() <= BAR
            if K == 0:
                assert np.array_equal(bits(w), bits(w0)) and not v.any()
            d, r = fr.seat_sets(t, seat)
            assert np.abs(s.head(k)[d, r] - heads_of(t, seat, w, prob)).max() <= BAR
            check_loss(losses[seat], rl, ("creation", k, seat))
            assert losses[seat][0] > 0.0 and (K == 0) == (losses[seat][0] == losses[seat][1])
    s.close()


@pytest.mark.parametrize("sampling", [0, 1, 2])
@pytest.mark.parametrize("game", [1, 0])
def test_without_steps_the_nets_keep_their_bits(pkg, ev, ctxs, trees, game, sampling):
    """K = 0 over 2 iterations: w, v, z and so sigma are those of creation, while R moves."""
    s = ev.MccfrNetSolver(ctxs[game], cfgs_of(2, sampling, 66, 0, 50), sampling, [1, 2])
    first = [(s.net(k, 0), s.net(k, 1), s.head(k), s.sigma_table(k)) for k in (0, 1)]
    s.run(2)
    for k in (0, 1):
        for seat in (0, 1):
            for a, b in zip(s.net(k, seat), first[k][seat]):
                assert np.array_equal(bits(a), bits(b))
            assert np.array_equal(bits(s.net(k, seat)[0]), bits(glorot_pair(ev, 1 + k)[seat]))
            assert not s.net(k, seat)[1].any()
        assert np.array_equal(bits(s.head(k)), bits(first[k][2]))
        assert np.array_equal(bits(s.sigma_table(k)), bits(first[k][3]))
        assert s.state(k)[0].any()
    s.close()


# ---- determinism -------------------------------------------------------------------------------------------------
def everything(s, k, sampling):
    out = list(s.state(k)) + [bits(s.weighted(k))]
    for seat in (0, 1):
        out += [bits(x) for x in s.net(k, seat)]
    out += [bits(s.head(k)), bits(s.sigma_table(k)), bits(s.sigma_table(k, "table")), bits(s.fit_loss(k)),
            bits(s.average_table(k)), np.array(s.counts(k))]
    if sampling == 2:
        out += list(s.baseline(k))
    return out


@pytest.mark.parametrize("sampling", [0, 1, 2])
@pytest.mark.parametrize("game", [1, 0])
def test_a_run_is_a_function_of_the_run_alone(pkg, ev, ctxs, trees, game, sampling):
    """A cfg at places 0, 37 and 63 of a 64-run handle, among runs with other seeds, walkers, rules and nets,
    equals the same cfg as a handle's only run after 2 iterations, bit for bit: R, S, Sw, both nets and their
    momentum, z, both sigma tables, the losses, the average and the counts.  And run(2) is run(1) twice."""
    B = pkg.native.MCCFR_WG_WALKERS
    eps = EPS if sampling else 0.0
    mine = (77, 66, eps, "plus", "linear", "rowmax", 3, "huber", 0.25, 0.9)
    cfgs, inits = [], []
    for k in range(64):
        if k in (0, 37, 63):
            cfgs.append(mine)
            inits.append(9)
        else:
            cfgs.append((200 + k, (2, 130, B + 2)[k % 3], eps) + RULES[k % 3][:3] + (k % 4,) + RULES[k % 3][3:])
            inits.append(20 + k)
    many = ev.MccfrNetSolver(ctxs[game], cfgs, sampling, inits).run(2)
    alone = ev.MccfrNetSolver(ctxs[game], [mine], sampling, [9]).run(2)
    split = ev.MccfrNetSolver(ctxs[game], [mine], sampling, [9]).run(1).run(1)
    want = everything(alone, 0, sampling)
    assert want[0].any() and alone.iterations == many.iterations == split.iterations == 2
    for other, k in ((many, 0), (many, 37), (many, 63), (split, 0)):
        got = everything(other, k, sampling)
        bad = [j for j, (a, b) in enumerate(zip(got, want)) if not np.array_equal(a, b)]
        assert not bad, (NAMES[game], sampling, k, "tables that differ", bad)
    assert not np.array_equal(everything(many, 1, sampling)[0], want[0])
    for s in (many, alone, split):
        s.close()


# ---- the other handles -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", [0, 1, 2])
@pytest.mark.parametrize("game", [1, 0])
def test_the_tabular_handle_is_unmoved_and_refused(pkg, ev, ctxs, trees, game, sampling):
    """After a net handle has run in the context, a handle of nfsp_mccfr_x_create with the same seeds still
    equals its own restatement (tests/mccfr_x_ref.py) bit for bit, its sigma being regret matching on R; and
    the three calls of the nets refuse it, as they refuse the three older kinds."""
    nat = pkg.native
    t = trees[game]
    eps = EPS if sampling else 0.0
    net = ev.MccfrNetSolver(ctxs[game], cfgs_of(2, sampling, 66, 3, 60), sampling, [1, 2]).run(2)
    tab = ev.MccfrXSolver(ctxs[game], [(60 + k, 66, eps) + RULES[k][:2] for k in (0, 1)], sampling).run(2)
    net.run(1)
    tab.run(1)
    for k in (0, 1):
        args = (t, 60 + k, 66) + ((eps,) if sampling else ())
        ref = xr.XRef(KINDS[sampling])(*args, regret=CODES[RULES[k][0]], average=CODES[RULES[k][1]]).run(3)
        same_tables(tab, k, ref, ("the tabular handle", k), sampling)
        assert np.abs(tab.average_table(k) - ref.average()).max() <= 1e-15
    L = ctxs[game].L
    olds = [tab, ev.MccfrSolver(ctxs[game], [(1, 2)]), ev.MccfrOsSolver(ctxs[game], [(1, 2, EPS)]),
            ev.MccfrVrSolver(ctxs[game], [(1, 2, EPS)])]
    for o in olds:
        p, q = nat.P(), nat.P()
        out = (nat.F64 * 4)(7.0, 7.0, 7.0, 7.0)
        for rc in (L.nfsp_mccfr_net_tables(o.h, 0, C.byref(p), C.byref(q), None),
                   L.nfsp_mccfr_net_weights(o.h, 0, 0, C.byref(p), C.byref(q)), L.nfsp_mccfr_net_loss(o.h, 0, out)):
            assert rc == nat.EINVAL and b"nfsp_mccfr_net_create" in L.nfsp_last_error()
        assert not p.value and not q.value and list(out) == [7.0] * 4
        o.run(1)                                        # and they go on as before
    assert tab.iterations == 4
    # the net handle's own refusals
    p = nat.P()
    assert L.nfsp_mccfr_net_tables(net.h, 2, C.byref(p), None, None) == nat.EINVAL and b"run" in L.nfsp_last_error()
    assert L.nfsp_mccfr_net_weights(net.h, 0, 2, C.byref(p), None) == nat.EINVAL and b"seat" in L.nfsp_last_error()
    assert L.nfsp_mccfr_net_tables(net.h, 1, None, None, None) == nat.OK
    for o in olds + [net]:
        o.close()


def test_initial_nets_must_be_finite(pkg, ev, ctxs):
    import torch
    nat = pkg.native
    L = ctxs[1].L
    w = torch.as_tensor(np.stack(glorot_pair(ev, 1) + glorot_pair(ev, 2)), device="cuda")
    w[3, 17] = float("nan")
    torch.cuda.synchronize()
    arr = (nat.MccfrNetCfg * 2)(*[nat.MccfrNetCfg(1, 64, 0, 0.0, 0, 0, 0, 3, nat.FIT_MSE, 0.5, 0.9, 0)] * 2)
    ptrs = (nat.P * 4)(*[w[k].data_ptr() for k in range(4)])
    h = nat.P()
    assert L.nfsp_mccfr_net_create(ctxs[1].h, arr, 2, ptrs, C.byref(h)) == nat.EINVAL and not h.value
    msg = L.nfsp_last_error()
    assert b"run 1 seat 1" in msg and b"finite" in msg and b"parameter 17" in msg, msg
    with pytest.raises(nat.NativeError, match="nfsp_mccfr_net_cfg.fit_steps"):
        ev.MccfrNetSolver(ctxs[1], [(1, 64, 0.0, "plain", "uniform", "avg", -1, "mse", 0.5, 0.9)], 0, [1])
    with pytest.raises(ValueError, match="one init seed"):
        ev.MccfrNetSolver(ctxs[1], cfgs_of(2, 0, 64, 1, 1), 0, [1])


# ---- set_net -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", [1, 0])
def test_a_written_net_comes_back_and_the_next_fit_starts_from_it(pkg, ev, ctxs, trees, game):
    t = trees[game]
    cfgs = cfgs_of(2, 1, 66, 3, 70)
    s = ev.MccfrNetSolver(ctxs[game], cfgs, 1, [1, 2]).run(1)
    rng = np.random.RandomState(5)
    w = fr.glorot(123)
    v = (rng.normal(0.0, 1e-3, fr.NP)).astype(np.float32)
    others = [s.net(0, 0), s.net(0, 1), s.net(1, 1)]
    assert s.set_net(1, 0, w, v) is s
    got = s.net(1, 0)
    assert np.array_equal(bits(got[0]), bits(w)) and np.array_equal(bits(got[1]), bits(v))
    for (a, b), (k, seat) in zip(others, ((0, 0), (0, 1), (1, 1))):
        assert np.array_equal(bits(s.net(k, seat)[0]), bits(a)) and np.array_equal(bits(s.net(k, seat)[1]), bits(b))
    s.run(1)
    R = s.state(1)[0]
    rw, rv, rl, prob = fit_from(t, cfgs[1], 0, R, 2.0, w, v)
    w_a, v_a = s.net(1, 0)
    assert np.abs(rw - w).max() > 1e-4                     # the fit moved the written net
    assert np.abs(w_a - rw).max() <= BAR and np.abs(v_a - rv).max() <= BAR
    d, r = fr.seat_sets(t, 0)
    assert np.abs(s.head(1)[d, r] - heads_of(t, 0, w_a, prob)).max() <= BAR
    check_sigma(t, s, 1, "after set_net")
    v1 = s.net(1, 1)[1]
    s.set_net(1, 1, w)                                     # without v: the momentum state is left
    assert np.array_equal(bits(s.net(1, 1)[0]), bits(w)) and np.array_equal(bits(s.net(1, 1)[1]), bits(v1))
    with pytest.raises(ValueError, match="finite"):
        s.set_net(0, 0, np.full(fr.NP, np.nan, np.float32))
    s.close()


# ---- it learns ---------------------------------------------------------------------------------------------------
def test_sampled_regression_cfr_learns_kuhn_on_the_device(pkg, ev, ctxs, trees):
    """tests/test_mccfr_net_ref.py's case on the device, free-running: external sampling, seed 1, W 64, K 32,
    lr 0.5, momentum 0.9, MSE, AVG, 64 iterations from init seed 1; the same cap, a quarter of the uniform
    policy's exploitability."""
    s = ev.MccfrNetSolver(ctxs[1], [(1, 64, 0.0, "plain", "uniform", "avg", 32, "mse", 0.5, 0.9)], 0, [1]).run(64)
    avg, cur = s.average(0), s.current(0)
    res = ev.evaluate_batch(ctxs[1], [(avg, avg), (cur, cur)])
    print("kuhn net-mccfr on the device: exploitability", res[0]["exploitability"], "of the current sigma",
          res[1]["exploitability"], "sigma_tv", s.sigma_tv(0).tolist(), "fit_loss", s.fit_loss(0).tolist())
    assert s.counts(0)[0] == 2 * 64 * 64
    assert res[0]["exploitability"] <= 0.2917
    tv = s.sigma_tv(0)
    assert tv.shape == (2,) and (tv >= 0).all() and (tv <= 1).all()
    s.close()


# ---- timing ------------------------------------------------------------------------------------------------------
def test_timing_splits_walks_and_applies_and_moves_no_bit(pkg, ev, ctxs, trees):
    cfgs = cfgs_of(2, 2, 66, 3, 80)
    a = ev.MccfrNetSolver(ctxs[1], cfgs, 2, [1, 2])
    b = ev.MccfrNetSolver(ctxs[1], cfgs, 2, [1, 2])
    assert ev.mccfr_timings(a) == (0.0, 0.0, 0)
    ev.mccfr_timings(a, True)
    a.run(2)
    b.run(2)
    walk, apply_, iters = ev.mccfr_timings(a)
    assert iters == 2 and walk > 0.0 and apply_ > 0.0
    with pytest.raises(pkg.native.NativeError, match="NFSP_MCCFR_TIMED_ITERS"):
        a.run(pkg.native.MCCFR_TIMED_ITERS + 1)
    assert ev.mccfr_timings(a, False) == (0.0, 0.0, 0)
    for k in (0, 1):
        for x, y in zip(everything(a, k, 2), everything(b, k, 2)):
            assert np.array_equal(x, y)
    a.close()
    b.close()

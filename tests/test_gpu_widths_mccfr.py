"""Regret nets of hidden width 16 and 128 on the MCCFR handle (nfsp_mccfr_net_create_h; csrc/mccfr.hip
k_mccfr_net_apply_w<H>) on the GPU: the teacher-forced replay of tests/test_gpu_mccfr_net.py against the
restatement at the width (tests/widths_ref.py), with that file's bars -- R, S, Sw, Bs, Bn and the counts bit
for bit, the nets within 1e-5 of the width-general fit from the device's own weights, z within 1e-5 of the
forward of the device's own weights, sigma regret matching of the device's own z bit for bit.  Then width
64 through the new entry point against nfsp_mccfr_net_create, device against device; nfsp_mccfr_net_hidden
on the five kinds of handle; and a width-128 handle beside a width-64 one in one context."""
import ctypes as C

import numpy as np
import pytest

import mccfr_os_ref as osr
import mccfr_ref as mr
import mccfr_vr_ref as vrr
import widths_ref as wr

pytestmark = pytest.mark.gpu
NAMES = {0: "leduc", 1: "kuhn"}
KINDS = {0: mr.MccfrRef, 1: osr.OsRef, 2: vrr.VrRef}
EPS = 0.6
BAR = 1e-5                                             # tests/test_gpu_fitnet.py's, per weight and per head
# (regret, average, target, loss, lr, momentum) of the runs of a handle: all differ by run
RULES = [("plain", "uniform", "avg", "mse", 0.5, 0.9), ("plus", "linear", "rowmax", "huber", 0.1, 0.5),
         ("plus", "uniform", "rowmax", "mse", 0.25, 0.0)]
CODES = {"plain": 0, "plus": 1, "uniform": 0, "linear": 1, "avg": 0, "rowmax": 1, "mse": 1, "huber": 2}


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


def glorot_pair(ev, init_seed, hidden):
    rng = np.random.RandomState(init_seed)
    return ev.glorot_net(rng, hidden), ev.glorot_net(rng, hidden)


def ref_of(ev, tree, sampling, cfg, init_seed, hidden):
    seed, W, eps, reg, avg, tgt, K, loss, lr, mu = cfg
    args = (tree, seed, W) + ((eps,) if sampling else ())
    return wr.net_ref(hidden).NetRef(KINDS[sampling])(
        *args, nets=glorot_pair(ev, init_seed, hidden), target=CODES[tgt], fit_steps=K, loss=CODES[loss], lr=lr,
        momentum=mu, regret=CODES[reg], average=CODES[avg])


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


def check_sigma(hidden, tree, solver, run, what):
    z = solver.head(run)
    assert z.dtype == np.float32
    assert np.array_equal(bits(solver.sigma_table(run, "net")), bits(wr.net_ref(hidden).sigma_of(tree, z))), what
    assert np.array_equal(bits(solver.sigma_table(run, "table")), bits(mr.match(tree, solver.state(run)[0]))), what


def check_loss(got, want, what):
    """tests/test_gpu_mccfr_net.py's: f32 row terms summed in double on both sides, 1e-4 relative."""
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-12, (what, got, want)


def replay(ev, tree, s, refs, cfgs, sampling, hidden, iterations, what, first=1):
    """One run(1) per iteration, every run of the handle with its own teacher-forced restatement; returns the
    largest |dw|, |dv|, |dz|."""
    fr, nr = wr.fit_ref(hidden), wr.net_ref(hidden)
    n = len(cfgs)
    worst = {"w": 0.0, "v": 0.0, "z": 0.0}
    rows0 = tree.seat == 0
    for it in range(first, first + iterations):
        before = [(s.sigma_table(k), s.net(k, 0), s.net(k, 1), s.head(k)) for k in range(n)]
        s.run(1)
        assert s.iterations == it
        for k in range(n):
            sg0, net0, net1, z0 = before[k]
            mixed = sg0.copy()
            mixed[rows0] = s.sigma_table(k)[rows0]         # half 1 reads seat 0's new rows and seat 1's old ones
            refs[k].sigma_hook = lambda i, a=sg0, b=mixed: a if i == 0 else b
            refs[k].run(1)
            at = what + (k, it)
            same_tables(s, k, refs[k], at, sampling)
            check_sigma(hidden, tree, s, k, at)
            R = s.state(k)[0]
            z1 = s.head(k)
            losses = s.fit_loss(k)
            seed, W, eps, reg, avg, tgt, K, loss, lr, mu = cfgs[k]
            for seat, (w_b, v_b) in ((0, net0), (1, net1)):
                w_a, v_a = s.net(k, seat)
                assert w_a.shape == v_a.shape == (34 * hidden + 3,)
                prob = fr.problem(tree, seat, nr.targets(tree, R, W, float(it), CODES[tgt]))
                rw, rv, rl = fr.fit(w_b, prob, fr.ACT_LINEAR, CODES[loss], lr, mu, K, v0=v_b)
                d, r = fr.seat_sets(tree, seat)
                dw, dv = np.abs(w_a - rw).max(), np.abs(v_a - rv).max()
                dz = np.abs(z1[d, r] - fr.forward(np.asarray(w_a, np.float32), prob[0])[2]).max()
                worst = {"w": max(worst["w"], dw), "v": max(worst["v"], dv), "z": max(worst["z"], dz)}
                assert dw <= BAR and dv <= BAR, (at, seat, dw, dv)
                assert dz <= BAR, (at, seat, dz)
                check_loss(losses[seat], rl, (at, seat))
                if K == 0:
                    assert np.array_equal(bits(w_a), bits(w_b)) and np.array_equal(bits(v_a), bits(v_b))
                    assert np.array_equal(bits(z1[d, r]), bits(z0[d, r]))
    return worst


# ---- the replay ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("K", [0, 1, 3])
@pytest.mark.parametrize("W", [2, 66])
@pytest.mark.parametrize("sampling", [0, 1, 2])
@pytest.mark.parametrize("game", [1, 0])
@pytest.mark.parametrize("hidden", [16, 128])
def test_replay_iteration_by_iteration(pkg, ev, ctxs, trees, hidden, game, sampling, W, K, n):
    """Three iterations, one run(1) each, every run of the handle with its own restatement."""
    t = trees[game]
    cfgs = cfgs_of(n, sampling, W, K, 100 + W + K)
    inits = [7 + k for k in range(n)]
    s = ev.MccfrNetSolver(ctxs[game], cfgs, sampling, inits, hidden=hidden)
    assert s.hidden == hidden and s.sampling == sampling
    assert [s.rule(k) for k in range(n)] == [(CODES[c[3]], CODES[c[4]]) for c in cfgs]
    refs = [ref_of(ev, t, sampling, cfgs[k], inits[k], hidden) for k in range(n)]
    worst = replay(ev, t, s, refs, cfgs, sampling, hidden, 3, (NAMES[game], hidden, sampling, W, K, n))
    print(NAMES[game], "hidden", hidden, "sampling", sampling, "W", W, "K", K, "n", n,
          "largest |dw| %.3g |dv| %.3g |dz| %.3g" % (worst["w"], worst["v"], worst["z"]))
    s.close()


# ---- 64 through the new entry point ------------------------------------------------------------------------------
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
def test_width_64_through_create_h_is_create(pkg, ev, ctxs, game, sampling):
    """Device against device after 3 iterations: every table, net and momentum state, bit for bit."""
    cfgs = cfgs_of(3, sampling, 66, 3, 30)
    inits = [4, 5, 6]
    old = ev.MccfrNetSolver(ctxs[game], cfgs, sampling, inits)                       # nfsp_mccfr_net_create
    nets = [w for s in inits for w in glorot_pair(ev, s, 64)]
    new = ev.MccfrNetSolver(ctxs[game], cfgs, sampling, inits, init_nets=nets)       # nfsp_mccfr_net_create_h(64)
    assert old.hidden == new.hidden == 64
    old.run(3)
    new.run(3)
    for k in range(3):
        a, b = everything(old, k, sampling), everything(new, k, sampling)
        assert a[0].any()
        bad = [j for j, (x, y) in enumerate(zip(a, b)) if not np.array_equal(x, y)]
        assert not bad, (NAMES[game], sampling, k, "tables that differ", bad)
    old.close()
    new.close()


def test_hidden_of_the_five_kinds_of_handle(pkg, ev, ctxs):
    nat = pkg.native
    ctx = ctxs[1]
    L = ctx.L
    cfg = [(1, 2, 0.0, "plain", "uniform", "avg", 1, "mse", 0.5, 0.9)]
    for hidden in wr.WIDTHS:
        s = ev.MccfrNetSolver(ctx, cfg, 0, [1], hidden=hidden)
        out = nat.I32(-1)
        assert L.nfsp_mccfr_net_hidden(s.h, C.byref(out)) == nat.OK and out.value == hidden == s.hidden
        assert s.net(0, 1)[0].shape == (34 * hidden + 3,)
        assert L.nfsp_mccfr_net_hidden(s.h, None) == nat.EINVAL
        s.close()
    olds = [ev.MccfrSolver(ctx, [(1, 2)]), ev.MccfrOsSolver(ctx, [(1, 2, EPS)]), ev.MccfrVrSolver(ctx, [(1, 2, EPS)]),
            ev.MccfrXSolver(ctx, [(1, 2, 0.0, "plain", "uniform")], 0)]
    for o in olds:
        out = nat.I32(-1)
        assert L.nfsp_mccfr_net_hidden(o.h, C.byref(out)) == nat.EINVAL and out.value == -1
        assert b"nfsp_mccfr_net_create" in L.nfsp_last_error()
        o.close()
    # widths that are not built, mixed widths, and a net of another width written into a handle
    for hidden in (0, 48, 256):
        with pytest.raises(ValueError, match="widths built"):
            ev.MccfrNetSolver(ctx, cfg, 0, [1], hidden=hidden)
    w16, w128 = glorot_pair(ev, 1, 16)[0], glorot_pair(ev, 1, 128)[0]
    with pytest.raises(ValueError, match="one width per call"):
        ev.MccfrNetSolver(ctx, cfg, 0, [1], init_nets=[w16, w128])
    import torch
    dev = torch.as_tensor(np.stack([w16, w16]), device="cuda")
    arr = (nat.MccfrNetCfg * 1)(nat.MccfrNetCfg(1, 2, 0, 0.0, 0, 0, 0, 1, nat.FIT_MSE, 0.5, 0.9, 0))
    ptrs = (nat.P * 2)(dev[0].data_ptr(), dev[1].data_ptr())
    h = nat.P()
    assert L.nfsp_mccfr_net_create_h(ctx.h, 48, arr, 1, ptrs, C.byref(h)) == nat.EINVAL and not h.value
    assert b"16, 32, 64 and 128" in L.nfsp_last_error()
    s = ev.MccfrNetSolver(ctx, cfg, 0, [1], init_nets=[w16, w16])
    assert s.hidden == 16
    with pytest.raises(ValueError, match="547"):
        s.set_net(0, 0, w128)
    s.close()


# ---- two widths in one context -----------------------------------------------------------------------------------
@pytest.mark.parametrize("game", [1, 0])
def test_a_128_handle_and_a_64_handle_do_not_disturb_each_other(pkg, ev, ctxs, trees, game):
    """The 64 handle runs before and after the 128 handle does, and stays on its own restatement; so does the
    128 handle."""
    t = trees[game]
    c64, c128 = cfgs_of(2, 2, 66, 3, 90), cfgs_of(2, 2, 66, 3, 95)
    s64 = ev.MccfrNetSolver(ctxs[game], c64, 2, [1, 2])
    r64 = [ref_of(ev, t, 2, c64[k], 1 + k, 64) for k in (0, 1)]
    replay(ev, t, s64, r64, c64, 2, 64, 1, (NAMES[game], 64, "before"))
    s128 = ev.MccfrNetSolver(ctxs[game], c128, 2, [3, 4], hidden=128)
    r128 = [ref_of(ev, t, 2, c128[k], 3 + k, 128) for k in (0, 1)]
    replay(ev, t, s128, r128, c128, 2, 128, 2, (NAMES[game], 128, "between"))
    replay(ev, t, s64, r64, c64, 2, 64, 2, (NAMES[game], 64, "after"), first=2)
    replay(ev, t, s128, r128, c128, 2, 128, 1, (NAMES[game], 128, "last"), first=3)
    assert s64.hidden == 64 and s128.hidden == 128 and s64.iterations == s128.iterations == 3
    s64.close()
    s128.close()

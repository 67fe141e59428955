"""nfsp_fit_tables_h and nfsp_head_tables_h (csrc/fit_tables.hip k_fit_tables_w<H>, csrc/head_tables.hip
k_head_tables_h) on the GPU at hidden widths 16, 32 and 128, against tests/widths_ref.py.

Parity: the 30 cases x 2 games of tests/test_gpu_fitnet.py with that file's rule for inits (the first
Glorot seed whose float32 and float64 8-step restatements agree within 1e-6) and that file's bars: 1e-5
per weight and per momentum entry, 1e-6 relative in both losses.  The bars do not depend on the width:
the restatement differs from the kernel in the order of its sums only, and a sum of H + 1 or of N terms
of size 1 in another order moves by a few 2^-24 of its value.

The evaluate bar of net_policy against Policy.ar at 64: the two policies differ by the rounding of a
float32 probability at most, 2^-24 each; at most 8 decisions lie on a path and a pot holds 13 chips at
most, so about 6e-6 chips: 1e-5.

"Width matters": Leduc, targets RandomState(77 + seat).normal(0, 1, (ndec, 3, 3)), linear head, MSE,
uniform weights, lr 0.1, momentum 0.9, 200 steps, Glorot seed 1.  The restatement ends at 0.714 / 0.355 /
0.159 (seat 0) and 0.659 / 0.415 / 0.185 (seat 1) for widths 16 / 32 / 64; 128 is left out, its float32
and float64 runs differ by 5% at these settings.
"""
import ctypes as C

import numpy as np
import pytest

import widths_ref as wr

pytestmark = pytest.mark.gpu

STEPS = 8
NEW = (16, 32, 128)


@pytest.fixture(scope="module")
def ctxs(pkg):
    import torch  # noqa: F401  (before libnfsp: the process must end up with one HIP runtime, torch's)
    pkg.native.lib()
    return {g: pkg.native.Context(1, game=g) for g in (0, 1)}


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def run(pkg, ctx, specs, steps):
    """specs: dicts of FitJob's arguments with host arrays -> ([w], [v or None], losses [n, 2])."""
    ev = pkg.evaluation
    jobs = [ev.FitJob(**s) for s in specs]
    losses = ev.fit_tables(ctx, jobs, steps)
    return ([j.w.cpu().numpy() for j in jobs], [None if j.v is None else j.v.cpu().numpy() for j in jobs], losses)


# ---- 1. parity -----------------------------------------------------------------------------------
def make_case(fr, tree, seat, head, loss, mu, extras, salt):
    """tests/test_gpu_fitnet.py's make_case with the restatement of the width."""
    rng = np.random.RandomState(1000 * tree.game + 100 * seat + 10 * head + loss + salt)
    if loss == fr.CE:
        target = tree.remap(rng.dirichlet(np.ones(3), size=(tree.ndec, 3)))
    else:
        target = rng.normal(0.0, 1.5, size=(tree.ndec, 3, 3))
    weight = mask = None
    if extras:
        weight = rng.rand(tree.ndec, 3)
        weight[rng.rand(tree.ndec, 3) < 0.2] = 0.0
        if loss != fr.CE:
            mask = (rng.rand(tree.ndec, 3, 3) < 0.7).astype(np.uint8)
    lr = 0.5 if loss == fr.CE else 0.1
    p32 = fr.problem(tree, seat, target, weight, mask, np.float32)
    p64 = fr.problem(tree, seat, target, weight, mask, np.float64)
    for seed in range(50):
        w0 = fr.glorot(seed + salt)
        ref = fr.fit(w0, p32, head, loss, lr, mu, STEPS)
        r64 = fr.fit(w0, p64, head, loss, lr, mu, STEPS)
        if np.abs(ref[0] - r64[0]).max() < 1e-6:
            break
    else:
        raise AssertionError("no init whose float32 and float64 runs agree")
    spec = dict(w=w0, target=target, seat=seat, head=head, loss=loss, lr=lr, momentum=mu, weight=weight, mask=mask,
                v=np.zeros(fr.NP, np.float32))
    return spec, ref


_PAIRS = wr.fit_ref(64).PAIRS
CASES = [(seat, head, loss, mu, extras) for seat in (0, 1) for head, loss in _PAIRS
         for mu, extras in ((0.0, False), (0.9, False), (0.9, True))]
_PARITY = {}


@pytest.fixture(scope="module")
def parity(pkg, ctxs):
    """(game, hidden) -> every parity case in one call (30 jobs): (specs and restatement results, GPU results);
    made once where first asked for and left unchanged."""
    def get(game, hidden):
        if (game, hidden) not in _PARITY:
            tree = pkg.evaluation.GameTree.of(game)
            made = [make_case(wr.fit_ref(hidden), tree, *c, salt=k) for k, c in enumerate(CASES)]
            _PARITY[game, hidden] = (made, run(pkg, ctxs[game], [m[0] for m in made], STEPS))
        return _PARITY[game, hidden]
    return get


def differences(parity, game, hidden, case):
    made, (w, v, losses) = parity(game, hidden)
    spec, (rw, rv, rl) = made[case]
    dw, dv = np.abs(w[case] - rw).max(), np.abs(v[case] - rv).max()
    rel = max(abs(losses[case][i] - rl[i]) / abs(rl[i]) for i in (0, 1))
    return dw, dv, rel, np.abs(rw - spec["w"]).max()


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda k: "seat{}-head{}-loss{}-mu{}-{}".format(*CASES[k]))
@pytest.mark.parametrize("game", [1, 0], ids=["kuhn", "leduc"])
@pytest.mark.parametrize("hidden", NEW)
def test_eight_steps_match_the_float32_restatement(parity, hidden, game, case):
    dw, dv, rel, moved = differences(parity, game, hidden, case)
    print(f"hidden {hidden} game {game} case {CASES[case]}: |dw| {dw:.3g} |dv| {dv:.3g} loss rel {rel:.3g}")
    assert parity(game, hidden)[1][0][case].shape == (34 * hidden + 3,)
    assert moved > 1e-3                                   # the 8 steps moved the net
    assert dw < 1e-5 and dv < 1e-5
    assert rel < 1e-6


@pytest.mark.parametrize("hidden", NEW)
def test_largest_difference_of_a_width(parity, hidden):
    d = np.array([differences(parity, g, hidden, c)[:3] for g in (1, 0) for c in range(len(CASES))])
    print(f"hidden {hidden}: largest |dw| {d[:, 0].max():.3g} |dv| {d[:, 1].max():.3g} loss rel {d[:, 2].max():.3g} "
          "(64 measured 1.2e-7 and 3.3e-8)")
    assert d[:, 0].max() < 1e-5 and d[:, 1].max() < 1e-5 and d[:, 2].max() < 1e-6


# ---- 2. bits ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def leduc(pkg, ctxs):
    return ctxs[0], pkg.evaluation.GameTree.of(0)


def base_spec(fr, tree, head=None, loss=None, seed=5):
    head = fr.ACT_RELU if head is None else head
    loss = fr.HUBER if loss is None else loss
    rng = np.random.RandomState(seed)
    target = rng.normal(0.0, 1.5, size=(tree.ndec, 3, 3)) if loss != fr.CE else \
        tree.remap(rng.dirichlet(np.ones(3), size=(tree.ndec, 3)))
    weight = rng.rand(tree.ndec, 3)
    weight[rng.rand(tree.ndec, 3) < 0.2] = 0.0
    mask = None if loss == fr.CE else (rng.rand(tree.ndec, 3, 3) < 0.7).astype(np.uint8)
    v = rng.normal(0, 0.01, fr.NP).astype(np.float32)
    return dict(w=fr.glorot(seed), target=target, seat=1, head=head, loss=loss, lr=0.1, momentum=0.9,
                weight=weight, mask=mask, v=v)


def filler(fr, tree, k):
    head, loss = fr.PAIRS[k % len(fr.PAIRS)]
    s = base_spec(fr, tree, head, loss, seed=100 + k)
    s["seat"] = k & 1
    return s


def test_width_64_through_the_new_entry_point_has_the_old_ones_bits(pkg, leduc):
    ctx, tree = leduc
    nat, ev = pkg.native, pkg.evaluation
    fr = wr.fit_ref(64)
    specs = [base_spec(fr, tree)] + [filler(fr, tree, k) for k in range(1, 6)]
    res = []
    for entry in ("old", "new"):
        jobs = [ev.FitJob(**s) for s in specs]
        arr = (nat.FitJob * len(jobs))(*[j.spec() for j in jobs])
        out = np.zeros((len(jobs), 2))
        if entry == "old":
            rc = ctx.L.nfsp_fit_tables(ctx.h, 0, arr, len(jobs), STEPS, out.ctypes.data_as(nat.P))
        else:
            rc = ctx.L.nfsp_fit_tables_h(ctx.h, 0, 64, arr, len(jobs), STEPS, out.ctypes.data_as(nat.P))
        nat.check(rc, entry)
        res.append(([j.w.cpu().numpy() for j in jobs], [j.v.cpu().numpy() for j in jobs], out))
    for k in range(len(specs)):
        assert not np.array_equal(bits(res[0][0][k]), bits(specs[k]["w"]))
        assert np.array_equal(bits(res[0][0][k]), bits(res[1][0][k])), k
        assert np.array_equal(bits(res[0][1][k]), bits(res[1][1][k])), k
    assert np.array_equal(res[0][2], res[1][2])


@pytest.mark.parametrize("hidden", [128, 16])
def test_a_jobs_result_is_a_function_of_the_job_alone(pkg, leduc, hidden):
    ctx, tree = leduc
    fr = wr.fit_ref(hidden)
    J = base_spec(fr, tree)
    alone = run(pkg, ctx, [J], STEPS)
    b64 = run(pkg, ctx, [J if k in (0, 37, 63) else filler(fr, tree, k) for k in range(64)], STEPS)
    assert alone[0][0].shape == (fr.NP,)
    assert not np.array_equal(bits(alone[0][0]), bits(J["w"]))
    for k in (0, 37, 63):
        assert np.array_equal(bits(b64[0][k]), bits(alone[0][0])), k
        assert np.array_equal(bits(b64[1][k]), bits(alone[1][0])), k
        assert np.array_equal(b64[2][k], alone[2][0]), k
    assert not np.array_equal(bits(b64[0][1]), bits(alone[0][0]))


@pytest.mark.parametrize("hidden", [128, 16])
def test_steps_split_over_calls_and_lr_zero(pkg, leduc, hidden):
    ctx, tree = leduc
    fr = wr.fit_ref(hidden)
    J = base_spec(fr, tree)
    w16, v16, l16 = run(pkg, ctx, [J], 16)
    w8, v8, l8 = run(pkg, ctx, [J, dict(J, lr=0.0)], 8)
    w88, v88, l88 = run(pkg, ctx, [dict(J, w=w8[0], v=v8[0])], 8)
    assert np.array_equal(bits(w88[0]), bits(w16[0])) and np.array_equal(bits(v88[0]), bits(v16[0]))
    assert l8[0][0] == l16[0][0] and l88[0][0] == l8[0][1] and l88[0][1] == l16[0][1]
    assert not np.array_equal(bits(w8[0]), bits(w16[0]))
    # lr 0 leaves every bit of the net; v still moves
    assert np.array_equal(bits(w8[1]), bits(J["w"]))
    assert not np.array_equal(bits(v8[1]), bits(J["v"]))
    assert l8[1][0] == l8[1][1] == l8[0][0]


def test_nets_that_overlap_by_one_float_less_than_a_net_are_refused(pkg, leduc):
    import torch
    ctx, tree = leduc
    nat, ev = pkg.native, pkg.evaluation
    fr = wr.fit_ref(128)
    J = base_spec(fr, tree)
    NP = fr.NP
    for gap, ok in ((NP - 1, False), (NP, True)):
        host = np.concatenate([J["w"], J["w"]])[:gap + NP].copy()
        host[gap:] = J["w"]
        buf = torch.as_tensor(host, device="cuda")
        tgt = torch.as_tensor(J["target"], device="cuda")
        jobs = [ev.FitJob(buf.data_ptr() + 4 * off, tgt, 1, fr.ACT_LINEAR, "mse", 0.1, 0.9, hidden=128) for off in (0, gap)]
        assert jobs[0].hidden == 128
        arr = (nat.FitJob * 2)(*[j.spec() for j in jobs])
        rc = ctx.L.nfsp_fit_tables_h(ctx.h, 0, 128, arr, 2, STEPS, None)
        torch.cuda.synchronize()
        after = buf.cpu().numpy()
        if ok:
            assert rc == nat.OK
            assert not np.array_equal(bits(after[:NP]), bits(J["w"]))
            assert np.array_equal(bits(after[:NP]), bits(after[NP:]))          # the same job twice
        else:
            assert rc == nat.EINVAL and b"overlap" in ctx.L.nfsp_last_error()
            assert np.array_equal(bits(after), bits(host))                      # untouched
    # a width that is not built is refused before anything is read
    assert ctx.L.nfsp_fit_tables_h(ctx.h, 0, 48, arr, 2, STEPS, None) == nat.EINVAL
    assert b"16, 32, 64 and 128" in ctx.L.nfsp_last_error()
    with pytest.raises(ValueError, match="one width per call"):
        ev.fit_tables(ctx, [ev.FitJob(**base_spec(wr.fit_ref(16), tree)), ev.FitJob(**J)], 1)


# ---- 3. heads -------------------------------------------------------------------------------------
def biased_net(fr, seed):
    w = fr.glorot(seed)
    w[fr.OB1:fr.OW2] = np.random.RandomState(seed).normal(0, 0.2, fr.H)
    w[fr.OB2:] = (0.3, -0.2, 0.1)
    return w


@pytest.mark.parametrize("game", [1, 0], ids=["kuhn", "leduc"])
@pytest.mark.parametrize("hidden", [16, 128])
def test_heads_are_the_float32_restatement_in_the_kernels_order(pkg, ctxs, hidden, game):
    nat, ev = pkg.native, pkg.evaluation
    fr = wr.fit_ref(hidden)
    tree = ev.GameTree.of(game)
    nets = [biased_net(fr, 3 + k) for k in range(3)]
    acts = [nat.ACT_RELU, nat.ACT_LINEAR, nat.ACT_SOFTMAX]
    got = ev.head_tables(ctxs[game], nets, acts, tree).cpu().numpy()
    assert got.shape == (3, tree.ndec, 3, 3)
    for k, act in enumerate(acts):
        want = wr.heads_f32(nets[k], tree.obs.reshape(-1), act).reshape(tree.ndec, 3, 3)
        if act == nat.ACT_SOFTMAX:
            d = np.abs(got[k] - want).max()
            print(f"hidden {hidden} game {game}: softmax head |d| {d:.3g}")
            assert d <= 1e-6 and np.abs(got[k].sum(axis=2) - 1).max() < 1e-6
        else:
            assert want.any() and np.array_equal(bits(got[k]), bits(want)), (hidden, game, act)
    with pytest.raises(ValueError, match="one width per call"):
        ev.head_tables(ctxs[game], [nets[0], biased_net(wr.fit_ref(64), 1)], acts[:2], tree)


@pytest.mark.parametrize("game", [1, 0], ids=["kuhn", "leduc"])
def test_at_64_the_heads_and_the_scores_are_the_engines(pkg, ctxs, game):
    nat, ev = pkg.native, pkg.evaluation
    ctx, tree = ctxs[game], ev.GameTree.of(game)
    fr = wr.fit_ref(64)
    nets = [biased_net(fr, 11 + k) for k in range(2)]
    for act in (nat.ACT_RELU, nat.ACT_LINEAR):
        old = ev.head_tables(ctx, nets, [act] * 2, tree).cpu().numpy()
        new = ev.head_tables(ctx, nets, [act] * 2, tree, hidden=64).cpu().numpy()
        assert old.any() and np.array_equal(bits(old), bits(new)), act
    soft = [ev.head_tables(ctx, nets, [nat.ACT_SOFTMAX] * 2, tree, hidden=h).cpu().numpy() for h in (None, 64)]
    assert np.abs(soft[0] - soft[1]).max() <= 1e-6
    glorot = [ev.glorot_net(np.random.RandomState(5)), ev.glorot_net(np.random.RandomState(6))]
    for w0, w1 in (nets, glorot):
        for mode, kind in ((0, nat.POL_AR_SOFTMAX), (1, nat.POL_AR_ARGMAX)):
            a = ev.evaluate(ctx, ev.Policy.ar(w0, mode), ev.Policy.ar(w1, mode))
            b = ev.evaluate(ctx, ev.net_policy(ctx, w0, kind, tree), ev.net_policy(ctx, w1, kind, tree))
            d = max(abs(a[key] - b[key]) for key in a)
            print(f"game {game} mode {mode}: evaluate(net_policy) - evaluate(Policy.ar) {d:.3g} chips")
            assert d <= 1e-5
        for linear, kind in ((False, nat.POL_BR_GREEDY), (True, nat.POL_BR_GREEDY_LINEAR)):
            a = ev.policy_table(ctx, ev.Policy.br(w0, linear), tree).cpu().numpy()
            b = ev.policy_table(ctx, ev.net_policy(ctx, w0, kind, tree), tree).cpu().numpy()
            assert np.array_equal(a, b), (game, linear)


# ---- 4. width matters ---------------------------------------------------------------------------------
def test_a_wider_net_fits_random_targets_better(pkg, leduc):
    ctx, tree = leduc
    ev = pkg.evaluation
    ref, specs = {}, []
    for seat in (0, 1):
        target = np.random.RandomState(77 + seat).normal(0, 1, (tree.ndec, 3, 3))
        for hidden in (16, 32, 64):
            fr = wr.fit_ref(hidden)
            prob = fr.problem(tree, seat, target)
            ref[seat, hidden] = fr.fit(fr.glorot(1), prob, fr.ACT_LINEAR, fr.MSE, 0.1, 0.9, 200)[2][1]
            specs.append((seat, hidden, dict(w=fr.glorot(1), target=target, seat=seat, head=fr.ACT_LINEAR, loss="mse",
                                             lr=0.1, momentum=0.9)))
    gpu = {}
    for hidden in (16, 32, 64):                           # one width per call
        mine = [s for s in specs if s[1] == hidden]
        losses = ev.fit_tables(ctx, [ev.FitJob(**s[2]) for s in mine], 200)
        for (seat, _, _), l in zip(mine, losses):
            gpu[seat, hidden] = l[1]
    for seat in (0, 1):
        for name, loss in (("restatement", ref), ("gpu", gpu)):
            l16, l32, l64 = (loss[seat, h] for h in (16, 32, 64))
            print(f"seat {seat} {name}: final loss {l16:.4f} / {l32:.4f} / {l64:.4f} at widths 16 / 32 / 64, "
                  f"16 over 64 {l16 / l64:.2f}")
            assert l16 > l32 > l64 and l16 > 2 * l64, (seat, name)
    assert ref[0, 16] == pytest.approx(0.714, abs=1e-3) and ref[1, 64] == pytest.approx(0.185, abs=1e-3)

"""nfsp_fit_tables (csrc/fit_tables.hip k_fit_tables) on the GPU, against tests/fitnet_ref.py:
parity of 8 steps with the float32 restatement, the determinism contract bit for bit, the
refusals, that it fits a CFR+ average, and the engine's warm start built on it.

Parity inits are Glorot nets of the first seed for which the restatement's own float32 and float64
runs agree within 1e-6 after the 8 steps, so that no ReLU kink decides a case.

"It fits" settings, chosen on the CPU with the restatement alone (CfrRef tables, visit_ref
weights): lr 0.5, momentum 0.9, 500 steps.  They bring the restatement's final loss minus the
targets' weighted entropy to 1e-4 (Kuhn) and 2e-3 (Leduc) of its initial value, both seats; the
test asserts < 0.1 on the restatement before it looks at the GPU.
"""
import numpy as np
import pytest

import fitnet_ref as fr

pytestmark = pytest.mark.gpu

STEPS = 8
FIT = dict(lr=0.5, momentum=0.9, steps=500)
# |exploitability of the GPU-fitted nets - of the restatement-fitted nets|, both scored by one
# evaluate_batch: 10 x the difference of the first GPU run, not below 1e-3 chips.  That run measured
# 3.11e-6 (Kuhn: 0.000397 against 0.000400) and 1.33e-4 (Leduc: 1.037805 against 1.037672); DESIGN.md §9
FIT_MARGIN = {1: 1e-3, 0: 1.33e-3}


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


def make_case(tree, seat, head, loss, mu, extras, salt):
    """A parity case: random targets, and with ``extras`` random weights with exact zeros and
    (MSE / Huber) an explicit random mask."""
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


CASES = [(seat, head, loss, mu, extras) for seat in (0, 1) for head, loss in fr.PAIRS
         for mu, extras in ((0.0, False), (0.9, False), (0.9, True))]


@pytest.fixture(scope="module")
def parity(pkg, ctxs):
    """Every parity case of a game in one call (30 jobs): (specs, restatement results, GPU results)."""
    out = {}
    for g, ctx in ctxs.items():
        tree = pkg.evaluation.GameTree.of(g)
        made = [make_case(tree, *c, salt=k) for k, c in enumerate(CASES)]
        out[g] = (made, run(pkg, ctx, [m[0] for m in made], STEPS))
    return out


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda k: "seat{}-head{}-loss{}-mu{}-{}".format(*CASES[k]))
@pytest.mark.parametrize("game", [1, 0], ids=["kuhn", "leduc"])
def test_eight_steps_match_the_float32_restatement(parity, game, case):
    made, (w, v, losses) = parity[game]
    spec, (rw, rv, rl) = made[case]
    dw, dv = np.abs(w[case] - rw).max(), np.abs(v[case] - rv).max()
    rel = [abs(losses[case][i] - rl[i]) / abs(rl[i]) for i in (0, 1)]
    print(f"game {game} case {CASES[case]}: |dw| {dw:.3g} |dv| {dv:.3g} loss rel {rel[0]:.3g} {rel[1]:.3g}")
    assert np.abs(rw - spec["w"]).max() > 1e-3          # the 8 steps moved the net
    assert dw < 1e-5 and dv < 1e-5
    assert rel[0] < 1e-6 and rel[1] < 1e-6


# ---- bits ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def leduc(pkg, ctxs):
    return ctxs[0], pkg.evaluation.GameTree.of(0)


def base_spec(tree, head=fr.ACT_RELU, loss=fr.HUBER, seed=5):
    rng = np.random.RandomState(seed)
    target = rng.normal(0.0, 1.5, size=(tree.ndec, 3, 3)) if loss != fr.CE else \
        tree.remap(rng.dirichlet(np.ones(3), size=(tree.ndec, 3)))
    weight = rng.rand(tree.ndec, 3)
    weight[rng.rand(tree.ndec, 3) < 0.2] = 0.0
    mask = None if loss == fr.CE else (rng.rand(tree.ndec, 3, 3) < 0.7).astype(np.uint8)
    v = rng.normal(0, 0.01, fr.NP).astype(np.float32)
    return dict(w=fr.glorot(seed), target=target, seat=1, head=head, loss=loss, lr=0.1, momentum=0.9,
                weight=weight, mask=mask, v=v)


def filler(tree, k):
    head, loss = fr.PAIRS[k % len(fr.PAIRS)]
    s = base_spec(tree, head, loss, seed=100 + k)
    s["seat"] = k & 1
    return s


@pytest.mark.parametrize("head,loss", [(fr.ACT_RELU, fr.HUBER), (fr.ACT_SOFTMAX, fr.CE)])
def test_a_jobs_result_is_a_function_of_the_job_alone(pkg, leduc, head, loss):
    ctx, tree = leduc
    J = base_spec(tree, head, loss)
    alone = run(pkg, ctx, [J], STEPS)
    batch = [J if k in (0, 37, 63) else filler(tree, k) for k in range(64)]
    b64 = run(pkg, ctx, batch, STEPS)
    b65 = run(pkg, ctx, [filler(tree, k) for k in range(64)] + [J], STEPS)       # entry 64: the host's second launch
    assert not np.array_equal(bits(alone[0][0]), bits(J["w"]))
    for res, k in ((b64, 0), (b64, 37), (b64, 63), (b65, 64)):
        assert np.array_equal(bits(res[0][k]), bits(alone[0][0])), k
        assert np.array_equal(bits(res[1][k]), bits(alone[1][0])), k
        assert np.array_equal(res[2][k], alone[2][0]), k
    assert not np.array_equal(bits(b64[0][1]), bits(alone[0][0]))


def test_steps_split_over_calls_with_v_carried(pkg, leduc):
    ctx, tree = leduc
    J = base_spec(tree)
    w16, v16, l16 = run(pkg, ctx, [J], 16)
    w8, v8, l8 = run(pkg, ctx, [J], 8)
    w88, v88, l88 = run(pkg, ctx, [dict(J, w=w8[0], v=v8[0])], 8)
    assert np.array_equal(bits(w88[0]), bits(w16[0])) and np.array_equal(bits(v88[0]), bits(v16[0]))
    assert l8[0][0] == l16[0][0] and l88[0][0] == l8[0][1] and l88[0][1] == l16[0][1]
    # without the state the second half restarts from v = 0: different bits (the test can fail)
    J0 = dict(J, v=None)
    a16 = run(pkg, ctx, [J0], 16)
    a8 = run(pkg, ctx, [J0], 8)
    a88 = run(pkg, ctx, [dict(J0, w=a8[0][0])], 8)
    assert a8[1][0] is None
    assert not np.array_equal(bits(a88[0][0]), bits(a16[0][0]))


def test_lr_zero_and_rows_without_weight_or_target_change_no_bit(pkg, leduc):
    ctx, tree = leduc
    J = base_spec(tree)
    d, r = fr.seat_sets(tree, J["seat"])
    zero = [(a, b) for a, b in zip(d, r) if J["weight"][a, b] == 0.0]
    masked = [(a, b, k) for a, b in zip(d, r) for k in range(3) if J["weight"][a, b] > 0 and not J["mask"][a, b, k]]
    assert zero and masked
    t_zero, t_mask, t_live = J["target"].copy(), J["target"].copy(), J["target"].copy()
    for a, b in zero:
        t_zero[a, b] += 3.0
    for a, b, k in masked:
        t_mask[a, b, k] -= 5.0
    t_live[[x for x in range(tree.ndec) if tree.seat[x] != J["seat"]]] += 1.0      # the other seat's rows
    w, v, _ = run(pkg, ctx, [J, dict(J, lr=0.0), dict(J, target=t_zero), dict(J, target=t_mask),
                             dict(J, target=t_live)], STEPS)
    assert np.array_equal(bits(w[1]), bits(J["w"]))
    assert not np.array_equal(bits(v[1]), bits(J["v"]))                       # v still moves
    for k in (2, 3, 4):
        assert np.array_equal(bits(w[k]), bits(w[0])) and np.array_equal(bits(v[k]), bits(v[0])), k


# ---- refusals ----------------------------------------------------------------------------------
def test_refusals_leave_the_net_untouched(pkg, leduc):
    import torch
    ctx, tree = leduc
    nat, ev = pkg.native, pkg.evaluation
    good = base_spec(tree)
    d, r = fr.seat_sets(tree, good["seat"])
    t_nan = good["target"].copy()
    t_nan[d[7], r[7], 1] = np.nan
    w_neg = good["weight"].copy()
    w_neg[d[3], r[3]] = -1e-3
    w_none = good["weight"].copy()
    w_none[d, r] = 0.0
    ce = base_spec(tree, fr.ACT_SOFTMAX, fr.CE)
    t_ce = ce["target"].copy()
    t_ce[d[0], r[0]] = (1.5, -0.5, 0.0)
    for bad, word in ((dict(good, target=t_nan), "finite"), (dict(good, weight=w_neg), "weight"),
                      (dict(good, weight=w_none), "sum"), (dict(ce, seat=good["seat"], target=t_ce), "negative")):
        jobs = [ev.FitJob(**good), ev.FitJob(**bad)]
        with pytest.raises(nat.NativeError, match=word) as err:
            ev.fit_tables(ctx, jobs, STEPS)
        assert "job 1" in str(err.value)
        torch.cuda.synchronize()
        for j in jobs:                                                  # the good job did not run either
            assert np.array_equal(bits(j.w.cpu().numpy()), bits(good["w"]))
    # a NaN in the OTHER seat's rows is not the job's business
    t_other = good["target"].copy()
    t_other[[x for x in range(tree.ndec) if tree.seat[x] != good["seat"]][0]] = np.nan
    run(pkg, ctx, [dict(good, target=t_other)], 1)
    # game not the ctx's
    j = ev.FitJob(**good)
    arr = (nat.FitJob * 1)(j.spec())
    assert ctx.L.nfsp_fit_tables(ctx.h, 1, arr, 1, STEPS, None) == nat.EINVAL
    assert b"game" in ctx.L.nfsp_last_error()
    assert np.array_equal(bits(j.w.cpu().numpy()), bits(good["w"]))
    # two jobs on one net
    arr = (nat.FitJob * 2)(j.spec(), j.spec())
    assert ctx.L.nfsp_fit_tables(ctx.h, 0, arr, 2, STEPS, None) == nat.EINVAL
    assert np.array_equal(bits(j.w.cpu().numpy()), bits(good["w"]))


# ---- it fits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("game,iters", [(1, 2000), (0, 1000)], ids=["kuhn", "leduc"])
def test_ar_nets_fit_the_cfr_average(pkg, ctxs, game, iters):
    ev, dg = pkg.evaluation, pkg.diagnostics
    ctx, tree = ctxs[game], pkg.evaluation.GameTree.of(game)
    solver = ev.CfrSolver(ctx).run(iters)
    pol, tab = solver.average(), solver.average_table()
    vis = ev.visit_weights(ctx, pol, pol)
    ref_vis = fr.visit_ref(tree, tab)
    assert np.allclose(vis / vis.sum(), ref_vis / ref_vis.sum(), rtol=1e-9, atol=1e-15)
    for s in (0, 1):                                                    # a distribution per seat
        assert vis[tree.seat == s][:, :].sum() > 0
    inits = (fr.glorot(11), fr.glorot(12))
    ref = []
    for s in (0, 1):
        prob = fr.problem(tree, s, tab, vis, None, np.float32)
        w, _, (l0, l1) = fr.fit(inits[s], prob, fr.ACT_SOFTMAX, fr.CE, FIT["lr"], FIT["momentum"], FIT["steps"])
        ent = fr.entropy(prob)
        print(f"game {game} seat {s}: restatement loss - entropy {l0 - ent:.6f} -> {l1 - ent:.6f}")
        assert l1 - ent < 0.1 * (l0 - ent)                             # the settings do fit
        ref.append(w)
    res = dg.distill_policy(ctx, pol, "visit", FIT["steps"], FIT["lr"], FIT["momentum"], init=inits)
    assert (res["losses"][:, 1] < res["losses"][:, 0]).all()
    for s in (0, 1):
        prob = fr.problem(tree, s, tab, vis, None, np.float32)
        assert res["entropy"][s] == pytest.approx(fr.entropy(prob), abs=1e-6)
        assert res["losses"][s, 1] - res["entropy"][s] < 0.1 * (res["losses"][s, 0] - res["entropy"][s])
    sc = ev.evaluate_batch(ctx, [(ev.Policy.ar(res["nets"][0]), ev.Policy.ar(res["nets"][1])),
                                 (ev.Policy.ar(ref[0]), ev.Policy.ar(ref[1])), (pol, pol)])
    gpu, cpu, table = (x["exploitability"] for x in sc)
    print(f"game {game}: exploitability table {table:.6f} gpu-fitted {gpu:.6f} restatement-fitted {cpu:.6f} "
          f"diff {abs(gpu - cpu):.3g}")
    assert gpu == res["scores"]["softmax"] and table == res["scores"]["table"]
    assert abs(gpu - cpu) < FIT_MARGIN[game]


# ---- warm start -----------------------------------------------------------------------------------
WARM = dict(steps=60, lr=(0.5, 0.02), momentum=0.9)


def six_nets(e):
    return [e.get_weights(a, n) for a in (0, 1) for n in (0, 1, 2)]


@pytest.mark.parametrize("quirks", ["reference", "textbook_mse"])
def test_warm_start_is_the_fit_and_training_goes_on(pkg, quirks, tmp_path):
    nat, ev, dg, E = pkg.native, pkg.evaluation, pkg.diagnostics, pkg.engine
    q = nat.QUIRKS_REFERENCE if quirks == "reference" else nat.TEXTBOOK_MSE
    cfg = dict(game=1, n_lanes=128, seed=9, init_seed=3, inserts_per_update=16, quirks=q)
    eng = E.SelfPlayEngine(**cfg)
    tree = ev.GameTree.of(1)
    eng.step()
    pol = ev.CfrSolver(eng.ctx).run(500).average()
    start = six_nets(eng)
    stats = eng.stats()
    mem = [eng.memory_table(k)[0].raw.copy() for k in (nat.MEM_SL, nat.MEM_RL)]
    out = eng.warm_start(pol, **WARM)
    got = six_nets(eng)
    # the same fits standalone, from the nets the engine had
    ar = dg.distill_policy(eng.ctx, pol, "visit", WARM["steps"], WARM["lr"][0], WARM["momentum"], init=(start[0], start[3]))
    qx, reach, _ = dg.q_targets(eng.ctx, pol)
    head, loss = (nat.ACT_LINEAR, "mse") if quirks == "textbook_mse" else (nat.ACT_RELU, "huber")
    jobs = [ev.FitJob(start[3 * s + 1], qx, s, head, loss, WARM["lr"][1], WARM["momentum"], reach) for s in (0, 1)]
    lbr = ev.fit_tables(eng.ctx, jobs, WARM["steps"])
    for s in (0, 1):
        assert np.array_equal(bits(got[3 * s]), bits(ar["nets"][s].cpu().numpy()))
        assert np.array_equal(bits(got[3 * s + 1]), bits(jobs[s].w.cpu().numpy()))
        assert np.array_equal(bits(got[3 * s + 2]), bits(got[3 * s + 1]))          # target = BR
        assert not np.array_equal(bits(got[3 * s]), bits(start[3 * s]))
        assert not np.array_equal(bits(got[3 * s + 1]), bits(start[3 * s + 1]))
    assert np.array_equal(out["losses_ar"], ar["losses"]) and np.array_equal(out["losses_br"], lbr)
    assert (out["losses_ar"][:, 1] < out["losses_ar"][:, 0]).all() and (lbr[:, 1] < lbr[:, 0]).all()
    assert eng.exploitability()["exploitability"] == ar["scores"]["softmax"] == out["exploitability_after"]
    assert out["exploitability_after"] < out["exploitability_before"]
    np.testing.assert_equal(eng.stats(), stats)
    for k, m in zip((nat.MEM_SL, nat.MEM_RL), mem):
        assert np.array_equal(eng.memory_table(k)[0].raw, m)
    # q=None leaves the BR and target nets alone
    twin = E.SelfPlayEngine(**cfg)
    twin.step()
    twin.warm_start(pol, q=None, **WARM)
    tw = six_nets(twin)
    for s in (0, 1):
        assert np.array_equal(bits(tw[3 * s]), bits(got[3 * s]))
        assert np.array_equal(bits(tw[3 * s + 1]), bits(start[3 * s + 1]))
        assert np.array_equal(bits(tw[3 * s + 2]), bits(start[3 * s + 2]))
    # training goes on, and the state saves and reloads to the same digest
    eng.step()
    assert eng.stats()["hands"] == 2 * 128
    path = str(tmp_path / "warm.ckpt")
    eng.save(path)
    again = E.SelfPlayEngine.from_checkpoint(path)
    assert again.state_digest() == eng.state_digest()
    # off a step boundary it is refused
    eng.rollout()
    before = six_nets(eng)
    with pytest.raises(nat.NativeError):
        eng.warm_start(pol, **WARM)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before, six_nets(eng)))
    eng.update()


def test_warm_start_all_is_three_standalone_warm_starts(pkg):
    nat, ev, E = pkg.native, pkg.evaluation, pkg.engine
    cfg = dict(game=1, n_lanes=128, inserts_per_update=16, quirks=nat.TEXTBOOK_MSE)
    grp = E.EngineGroup(3, seed=40, init_seed=7, **cfg)
    pol = ev.CfrSolver(grp.ctx).run(500).average()
    out = grp.warm_start_all(pol, **WARM)
    assert len(out) == 3
    for r in range(3):
        solo = E.SelfPlayEngine(seed=40 + r, init_seed=7 + r, **cfg)
        res = solo.warm_start(ev.CfrSolver(solo.ctx).run(500).average(), **WARM)
        for a, b in zip(six_nets(grp.replicas[r]), six_nets(solo)):
            assert np.array_equal(bits(a), bits(b)), r
        assert res["exploitability_after"] == out[r]["exploitability_after"]
        assert np.array_equal(res["losses_br"], out[r]["losses_br"])
    grp.step()

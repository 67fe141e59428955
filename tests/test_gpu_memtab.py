"""The memory tables on the device (csrc/memtab.hip: nfsp_memory_table, nfsp_engine_memory_table,
nfsp_group_memory_tables) against the numpy restatement of tests/memtab_ref.py.  Every comparison
is equality of int64 arrays unless it says otherwise."""
import numpy as np
import pytest
import torch

import memtab_ref as mr
from memtab_ref import ctx_of, dev

pytestmark = pytest.mark.gpu

GAMES = ("leduc", "kuhn")


def synth(tree, seat, n, rng, keys=None):
    """n synthetic records of both kinds over one key draw: (obs, a, meta, SL words, RL words)."""
    sets = np.array([o for o, _, _ in mr.sets_of(tree, seat)], np.int64)
    obs = sets[rng.randint(len(sets), size=n)] if keys is None else np.asarray(keys, np.int64)
    a = mr.action_rows(n, rng)
    meta = mr.rl_meta(n, rng, a)
    return obs, a, meta, mr.pack_sl(obs, a), mr.pack_rl(obs, rng.randint(1 << 30, size=n), meta, a)


def run(pkg, ctx, tree, kind, seat, segs, out=None):
    out, info = pkg.evaluation.memory_table(ctx, kind, seat, segs, out=out, tree=tree)
    return out.cpu().numpy(), info


def check(pkg, ctx, tree, seat, obs, a, meta, sl, rl):
    for kind, words in ((mr.SL, sl), (mr.RL, rl)):
        got, info = run(pkg, ctx, tree, kind, seat, [dev(words)] if len(words) else [])
        want, winfo = mr.table(tree, seat, kind, obs, a=a, meta=meta)
        assert info == winfo
        assert np.array_equal(got, want)
    return want


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", GAMES)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_raw_form(pkg, game, n):
    ctx, tree = ctx_of(pkg, game)
    for seat in (0, 1):
        rng = np.random.RandomState(100 * n + seat)
        want = check(pkg, ctx, tree, seat, *synth(tree, seat, n, rng))
        assert want[..., 0].sum() == n


# 2 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nkeys", [1, 2])
def test_contention(pkg, nkeys):
    ctx, tree = ctx_of(pkg, "leduc")
    n = 100_000
    sets = [o for o, _, _ in mr.sets_of(tree, 1)]
    keys = np.array([sets[7], sets[100]][:nkeys], np.int64)[np.arange(n) % nkeys]
    want = check(pkg, ctx, tree, 1, *synth(tree, 1, n, np.random.RandomState(3), keys=keys))
    assert (want[..., 0].sum(axis=2) > 0).sum() == nkeys


# 3 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", GAMES)
def test_unmatched(pkg, game):
    ctx, tree = ctx_of(pkg, game)
    n = 3000
    rng = np.random.RandomState(8)
    obs, a, meta, _, _ = synth(tree, 0, n, rng)
    mine = {o for o, _, _ in mr.sets_of(tree, 0)}
    other = np.array([o for o, _, _ in mr.sets_of(tree, 1) if o not in mine], np.int64)
    words = np.array([w for w in rng.randint(1 << 30, size=2 * n) if int(w) not in mine], np.int64)
    bad = np.arange(n) % 3 == 1
    sub = np.concatenate([other[rng.randint(len(other), size=334)], np.zeros(333, np.int64), words[:333]])
    obs = obs.copy()
    obs[bad] = rng.permutation(sub)
    s2 = rng.randint(1 << 30, size=n)
    want = check(pkg, ctx, tree, 0, obs, a, meta, mr.pack_sl(obs, a), mr.pack_rl(obs, s2, meta, a))
    for kind in (mr.SL, mr.RL):
        raw, info = mr.table(tree, 0, kind, obs, a=a, meta=meta)
        only, oinfo = mr.table(tree, 0, kind, obs[~bad], a=a[~bad], meta=meta[~bad])
        assert info["unmatched"] == bad.sum() == 1000 and oinfo["unmatched"] == 0
        assert np.array_equal(raw, only)


# 4 ---------------------------------------------------------------------------------------------
def test_clamp(pkg):
    ctx, tree = ctx_of(pkg, "leduc")
    (o, d, r) = mr.sets_of(tree, 0)[5]
    a = np.array([[255.99998, 0, 0], [256.0, 0, 1], [0, -300.0, 0], [np.inf, 1, 0], [0, 1, -np.inf], [1, np.nan, 0],
                  [np.nan, np.inf, -256.0], [0.5, 0.25, 0.125]], np.float32)
    obs = np.full(len(a), o, np.int64)
    got, info = run(pkg, ctx, tree, mr.SL, 0, [dev(mr.pack_sl(obs, a))])
    want, winfo = mr.table(tree, 0, mr.SL, obs, a=a)
    assert info == winfo and info["clamped"] == 8
    assert np.array_equal(got, want)
    S = mr.SAT
    assert got[d, r, :, 1].tolist() == [(1 << 32) - 256 + S + S + (1 << 24) + (1 << 23), -S + 2 * (1 << 24) + S + (1 << 22),
                                        (1 << 24) - S - S + (1 << 21)]
    assert got[d, r, :, 0].tolist() == [6, 2, 0]        # first maximum; a NaN is the maximum


# 5 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [mr.SL, mr.RL])
def test_seat_rows(pkg, kind):
    ctx, tree = ctx_of(pkg, "leduc")
    sentinel = -0x0123456789ABCDEF
    sets = mr.sets_of(tree, 1)[:10]                     # the other sets of seat 1 stay empty
    rng = np.random.RandomState(4)
    obs = np.array([s[0] for s in sets], np.int64)[rng.randint(len(sets), size=500)]
    a = mr.action_rows(500, rng)
    meta = mr.rl_meta(500, rng, a)
    words = mr.pack_sl(obs, a) if kind == mr.SL else mr.pack_rl(obs, obs, meta, a)
    out = torch.full((tree.ndec, 3, 3, 3), sentinel, dtype=torch.int64, device="cuda")
    got, _ = run(pkg, ctx, tree, kind, 1, [dev(words)], out=out)
    want, _ = mr.table(tree, 1, kind, obs, a=a, meta=meta)
    assert (got[tree.seat == 0] == sentinel).all()
    assert np.array_equal(got[tree.seat == 1], want[tree.seat == 1])
    assert (got[tree.seat == 1] == 0).sum() > 1000 and (got[tree.seat == 1] != 0).any()
    # the second call completes the joint table
    got, _ = run(pkg, ctx, tree, kind, 0, [], out=out)
    assert np.array_equal(got, want)


# 6 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [mr.SL, mr.RL])
def test_segments(pkg, kind):
    ctx, tree = ctx_of(pkg, "leduc")
    nat = pkg.native
    n = 4097
    obs, a, meta, sl, rl = synth(tree, 0, n, np.random.RandomState(6))
    recs = dev(sl if kind == mr.SL else rl)
    want, winfo = mr.table(tree, 0, kind, obs, a=a, meta=meta)
    for lens in ([n], [2049, 2048], [1001, 0, 333, 2000, 763]):
        assert sum(lens) == n
        at = np.concatenate([[0], np.cumsum(lens)])
        got, info = run(pkg, ctx, tree, kind, 0, [recs[at[k]:at[k + 1]] for k in range(len(lens))])
        assert info == winfo and np.array_equal(got, want)
    assert nat.MEMTAB_MAX_SEGMENTS == 8
    run(pkg, ctx, tree, kind, 0, [recs[k:k + 1] for k in range(8)])
    with pytest.raises(nat.NativeError):
        run(pkg, ctx, tree, kind, 0, [recs[k:k + 1] for k in range(9)])
    with pytest.raises(nat.NativeError):                # refused before anything is read
        run(pkg, ctx, tree, kind, 0, [(recs.data_ptr(), 1 << 31)])
    with pytest.raises(nat.NativeError):
        run(pkg, ctx, tree, kind, 0, [(recs.data_ptr(), 1 << 30), (recs.data_ptr(), 1 << 30)])


# 7 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", GAMES)
def test_exact_policy(pkg, game):
    ev = pkg.evaluation
    ctx, tree = ctx_of(pkg, game)
    rng = np.random.RandomState(12)
    T = np.zeros((tree.ndec, 3, 3))
    out = None
    for seat in (0, 1):
        obs, hot = [], []
        for o, d, r in mr.sets_of(tree, seat):
            c0 = rng.randint(17)
            c1 = rng.randint(17 - c0) if tree.legal[d] else 16 - c0
            cnt = (c0, c1, 16 - c0 - c1)
            T[d, r] = np.array(cnt) / 16.0
            obs += [o] * 16
            hot += [k for k in range(3) for _ in range(cnt[k])]
        a = np.eye(3, dtype=np.float32)[np.array(hot)]
        out, info = ev.memory_table(ctx, mr.SL, seat, dev(mr.pack_sl(np.array(obs), a)), out=out, tree=tree)
        assert info["matched"] == len(obs) and info["clamped"] == 0
    t = ev.MemoryTable(tree, mr.SL, out)
    assert (t.n == 16).all()
    assert np.array_equal(t.policy("argmax"), T) and np.array_equal(t.policy("mass"), T)
    want = ev.evaluate(ctx, ev.Policy.table(T), ev.Policy.table(T))
    for how in ("argmax", "mass"):
        p = ev.Policy.table(t.policy(how))
        assert ev.evaluate(ctx, p, p) == want


# 8 ---------------------------------------------------------------------------------------------
def export_tables(eng, tree, st):
    """The restatement over ``memories(agent)``'s fp32 export: joint raw tables and infos."""
    raws = {mr.SL: np.zeros((tree.ndec, 3, 3, 3), np.int64), mr.RL: np.zeros((tree.ndec, 3, 3, 3), np.int64)}
    infos = {mr.SL: [], mr.RL: []}
    for p in (0, 1):
        m = eng.memories(p)
        n = int(st["sl_size"][p])
        raw, info = mr.table(tree, p, mr.SL, mr.bits_of(m["sl_s"][:n].cpu().numpy()), a=m["sl_a"][:n].cpu().numpy())
        raws[mr.SL] += raw
        infos[mr.SL].append(info)
        s, _, _, meta = mr.export_rl(m, st["rl_total"][p], int(st["rl_size"][p]))
        raw, info = mr.table(tree, p, mr.RL, s, meta=meta)
        raws[mr.RL] += raw
        infos[mr.RL].append(info)
    return raws, infos


@pytest.mark.parametrize("game,quirks", [("leduc", "reference"), ("leduc", "textbook"), ("kuhn", "reference"),
                                         ("kuhn", "textbook")])
def test_engine(pkg, game, quirks):
    ev, nat = pkg.evaluation, pkg.native
    ctx, tree = ctx_of(pkg, game)
    q = nat.QUIRKS_REFERENCE if quirks == "reference" else nat.TEXTBOOK_MSE_DECAY
    shape = dict(n_lanes=256, slices=4) if game == "leduc" else dict(n_lanes=64, slices=1)
    steps = 6 if game == "leduc" else 2
    eng = pkg.engine.SelfPlayEngine(ctx, init_seed=3, seed=77, quirks=q, rl_capacity=1024, sl_capacity=2048,
                                    eta=0.3, **shape)
    for _ in range(steps):
        eng.step()
    st = eng.stats()
    raws, infos = export_tables(eng, tree, st)
    tabs = {}
    for kind in (mr.SL, mr.RL):
        t, info = eng.memory_table(kind)
        t2, info2 = eng.memory_table(kind)
        assert np.array_equal(t.raw, t2.raw) and info == info2                       # repeatable
        assert info == infos[kind]
        assert np.array_equal(t.raw, raws[kind])
        tabs[kind] = t
        for p in (0, 1):
            want = st["sl_size"][p] if kind == mr.SL else min(st["rl_total"][p], 1024)
            assert t.counts[tree.seat == p].sum() == want == info[p]["records"] and info[p]["unmatched"] == 0
    if game == "leduc":
        # M_RL wrapped: an agent with more inserts than the circular log has rows (1,024 + 4 x 64
        # lanes per slice) has its 1,024 live records in two pieces of it
        log_cap = eng.memories(0)["log_cap"]
        print(f"rl_total {st['rl_total']} log_cap {log_cap}")
        assert log_cap == 1280 and max(st["rl_total"]) > log_cap
    assert min(st["sl_size"]) > 0
    sl = tabs[mr.SL]
    if quirks == "textbook":                            # NFSP_EXT_SL_ONEHOT
        assert np.array_equal(sl.raw[..., 1], sl.raw[..., 0] << 24)
    else:
        assert (sl.raw[..., 1] != sl.raw[..., 0] << 24).any()
    # the report against the same tables through the restatement
    rep = eng.memory_report()
    assert rep == eng.memory_report()
    ref = ev.MemoryTable(tree, mr.SL, raws[mr.SL])
    assert abs(rep["exploitability_ar"] - eng.exploitability()["exploitability"]) <= 1e-12
    for how in ("argmax", "mass"):
        p = ev.Policy.table(ref.policy(how))
        want = ev.evaluate(ctx, p, p)["exploitability"]
        assert abs(rep[f"exploitability_sl_{how}"] - want) <= 1e-12
        assert abs(rep[f"fit_gap_{how}"] - (rep["exploitability_ar"] - want)) <= 1e-12
    legal = np.ones((tree.ndec, 3, 3), bool)
    legal[~tree.legal, :, 2] = False
    assert rep["sl_empty_sets"] == (raws[mr.SL][..., 0].sum(axis=2) == 0).sum()
    assert rep["rl_empty_actions"] == ((raws[mr.RL][..., 0] == 0) & legal).sum()
    assert 0.0 <= rep["ar_mass_l1"] <= 2.0
    assert rep["sl_info"] == infos[mr.SL] and rep["rl_info"] == infos[mr.RL]
    # off a step boundary: a rollout whose update has not run
    eng.rollout()
    with pytest.raises(nat.NativeError, match="step boundary"):
        eng.memory_table(mr.SL)
    eng.update()
    eng.close()


# 9 ---------------------------------------------------------------------------------------------
def test_group(pkg):
    ctx, tree = ctx_of(pkg, "leduc")
    cfgs = [dict(n_lanes=256, slices=4, rl_capacity=1024, sl_capacity=2048, seed=50 + r, eta=eta)
            for r, eta in enumerate((0.1, 0.3, 0.6))]
    grp = pkg.engine.EngineGroup(ctx=ctx, cfgs=cfgs, init_seed=9)
    for _ in range(3):
        grp.step()
    for kind in (mr.SL, mr.RL):
        tabs = grp.memory_tables(kind)
        assert len(tabs) == 3
        for r, (t, info) in enumerate(tabs):
            one, oinfo = grp.replicas[r].memory_table(kind)
            assert info == oinfo and info[0]["records"] > 0
            assert np.array_equal(t.raw, one.raw)
        assert not np.array_equal(tabs[0][0].raw, tabs[2][0].raw)
    reps = grp.memory_report_all()
    assert len(reps) == 3 and reps[1] == grp.replicas[1].memory_report()
    grp.close()

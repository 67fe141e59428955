"""The BR half of the memory report on the device: the head read-out (csrc/head_tables.hip
nfsp_head_tables), the TD table (csrc/memtab.hip's third kind: nfsp_td_table, nfsp_engine_td_table,
nfsp_group_td_tables) and ``q_report``.  The TD references are tests/tdtab_ref.py's restatement over
the library's dense forward; every TD comparison is equality of int64 arrays and of ``info``."""
import numpy as np
import pytest
import torch

import memtab_ref as mr
import tdtab_ref as tr
from memtab_ref import ctx_of, dev

pytestmark = pytest.mark.gpu

GAMES = ("leduc", "kuhn")
TB, LIN = tr.TERMINAL_BOOTSTRAP, tr.EXT_LINEAR_Q
QUIRKS = (0, TB, LIN, LIN | TB)
GAMMAS = (0.0, 0.95, 1.0)


def net(pkg, seed, scale=1.0):
    """A Glorot net with biases that are not zero, so that every term of the forward counts."""
    rng = np.random.RandomState(seed)
    w = pkg.engine.glorot_net(rng)
    w[30 * 64:30 * 64 + 64] = rng.uniform(-0.3, 0.3, 64).astype(np.float32)
    w[-3:] = rng.uniform(-0.5, 0.5, 3).astype(np.float32)
    return (w * np.float32(scale)).astype(np.float32)


def words_with(rng, n, lo, hi):
    """n 30-bit words with popcount in [lo, hi]."""
    c = rng.randint(lo, hi + 1, size=n)
    rank = np.argsort(np.argsort(rng.rand(n, 30), axis=1), axis=1)       # a random order of the bits per word
    return ((rank < c[:, None]).astype(np.int64) << np.arange(30, dtype=np.int64)).sum(axis=1)


def synth(tree, seat, n, rng, keys=None, s2=None):
    """n synthetic M_RL records: (s, s2, meta, a).  s2 from the seat's own decision observations,
    random words with more than 9 bits set and zeros, a third each."""
    sets = np.array([o for o, _, _ in mr.sets_of(tree, seat)], np.int64)
    s = sets[rng.randint(len(sets), size=n)] if keys is None else np.asarray(keys, np.int64)
    a = mr.action_rows(n, rng)
    meta = mr.rl_meta(n, rng, a)
    if s2 is None:
        pool = rng.randint(3, size=n)
        s2 = np.where(pool == 0, sets[rng.randint(len(sets), size=n)], np.where(pool == 1, words_with(rng, n, 10, 30), 0))
    return s, np.asarray(s2, np.int64), meta, a


class Case:
    """Records on the device with the target heads' outputs at their s2, shared by every gamma."""

    def __init__(self, pkg, ctx, tree, seat, recs, w):
        self.pkg, self.ctx, self.tree, self.seat, self.w = pkg, ctx, tree, seat, w
        self.s, self.s2, self.meta, self.a = recs
        self.words = mr.pack_rl(self.s, self.s2, self.meta, self.a)
        self.dev = dev(self.words)
        self.wdev = torch.as_tensor(w).cuda()
        self._qt = {}

    def qt(self, quirks):
        act = tr.head_act(quirks)
        if act not in self._qt:
            self._qt[act] = tr.forward(self.ctx, self.w, act, self.s2)
        return self._qt[act]

    def want(self, gamma, quirks, keep=None):
        k = slice(None) if keep is None else keep
        return tr.table(self.tree, self.seat, self.s[k], self.meta[k], self.qt(quirks)[k], gamma, quirks)

    def got(self, gamma, quirks, segs=None, out=None):
        segs = ([self.dev] if len(self.words) else []) if segs is None else segs
        out, info = self.pkg.evaluation.td_table(self.ctx, self.seat, segs, self.wdev, gamma, quirks, out=out,
                                                 tree=self.tree)
        return out.cpu().numpy(), info

    def check(self, gamma, quirks):
        got, info = self.got(gamma, quirks)
        want, winfo = self.want(gamma, quirks)
        assert info == winfo, (gamma, quirks, info, winfo)
        assert np.array_equal(got, want), (gamma, quirks)
        return want, winfo


# head table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", GAMES)
def test_head_tables(pkg, game):
    ev, nat = pkg.evaluation, pkg.native
    ctx, tree = ctx_of(pkg, game)
    acts = [(nat.ACT_RELU, nat.ACT_LINEAR, nat.ACT_SOFTMAX)[k % 3] for k in range(65)]
    nets = [net(pkg, 300 + k, 60.0 if k in (1, 3, 5, 64) else 1.0) for k in range(65)]
    ref = [tr.forward(ctx, w, a, tree.obs.reshape(-1)).reshape(tree.ndec, 3, 3) for w, a in zip(nets, acts)]
    assert ev.head_tables(ctx, [], [], tree).shape == (0, tree.ndec, 3, 3)
    for n in (1, 3, 64, 65):
        got = ev.head_tables(ctx, nets[:n], acts[:n], tree).cpu().numpy()
        assert got.shape == (n, tree.ndec, 3, 3)
        for k in range(n):
            if acts[k] == nat.ACT_SOFTMAX:
                assert np.abs(got[k] - ref[k]).max() <= 1e-6
                assert np.abs(got[k].sum(axis=2) - 1.0).max() <= 1e-6
            else:
                assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), (n, k)
    # the executed first maximum of a Q head's table is the evaluator's own greedy policy
    heads = ev.head_tables(ctx, nets[:6], acts[:6], tree).cpu().numpy()
    seen = set()
    for k in range(6):
        if acts[k] == nat.ACT_SOFTMAX:
            continue
        a = np.argmax(heads[k], axis=2)
        a = np.where((a == 2) & ~tree.legal[:, None], 1, a)
        pol = ev.policy_table(ctx, ev.Policy.br(nets[k], linear=acts[k] == nat.ACT_LINEAR), tree).cpu().numpy()
        assert np.array_equal(np.eye(3)[a], pol), k
        seen |= set(a.reshape(-1).tolist())
    assert len(seen) >= 2
    assert (ref[0] == 0).any() and (ref[1] < 0).any()          # ReLU clips, the linear head does not
    with pytest.raises(nat.NativeError):
        ev.head_tables(ctx, nets[:1], [3], tree)


# TD raw form -----------------------------------------------------------------------------------
@pytest.mark.parametrize("game", GAMES)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4097])
def test_td_raw_form(pkg, game, n):
    ctx, tree = ctx_of(pkg, game)
    for seat in (0, 1):
        rng = np.random.RandomState(1000 * n + seat)
        c = Case(pkg, ctx, tree, seat, synth(tree, seat, n, rng), net(pkg, 7 + seat))
        for quirks in QUIRKS:
            for gamma in GAMMAS:
                want, info = c.check(gamma, quirks)
                assert want[..., 0].sum() == n == info["matched"] and info["clamped"] == 0
        if n >= 255:
            assert (c.want(0.95, 0)[0] != c.want(0.95, LIN)[0]).any()           # the heads differ
            assert (c.want(0.95, 0)[0] != c.want(0.95, TB)[0]).any()            # and the quirk counts


@pytest.mark.parametrize("cap", [5, 7])
def test_td_low_popcount(pkg, cap):
    """Every s2 has at most ``cap`` bits set: whole waves take fwd_lds' 5- and 7-row bodies."""
    ctx, tree = ctx_of(pkg, "leduc")
    n = 1500
    rng = np.random.RandomState(cap)
    s2 = words_with(rng, n, cap - 1, cap)
    s2[::7] = words_with(rng, len(s2[::7]), 0, cap)
    c = Case(pkg, ctx, tree, 0, synth(tree, 0, n, rng, s2=s2), net(pkg, 21))
    for quirks in (0, LIN | TB):
        c.check(0.95, quirks)


# TD segments -----------------------------------------------------------------------------------
def test_td_segments(pkg):
    nat = pkg.native
    ctx, tree = ctx_of(pkg, "leduc")
    n = 4097
    c = Case(pkg, ctx, tree, 1, synth(tree, 1, n, np.random.RandomState(6)), net(pkg, 31))
    want, winfo = c.check(0.95, LIN)
    recs = c.dev.reshape(n, 8)
    for lens in ([n], [2049, 0, 2048], [1001, 0, 333, 0, 2000, 500, 263, 0]):
        assert sum(lens) == n
        at = np.concatenate([[0], np.cumsum(lens)])
        got, info = c.got(0.95, LIN, segs=[recs[at[k]:at[k + 1]] for k in range(len(lens))])
        assert info == winfo and np.array_equal(got, want)
    with pytest.raises(nat.NativeError):
        c.got(0.95, LIN, segs=[recs[k:k + 1] for k in range(9)])
    with pytest.raises(nat.NativeError, match="aligned"):
        c.got(0.95, LIN, segs=[(recs.data_ptr() + 4, 16)])
    with pytest.raises(nat.NativeError):                # the MEM_* forms do not take the third kind
        pkg.evaluation.memory_table(ctx, nat.MEM_TD, 1, recs, tree=tree)


# identities ------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", GAMES)
def test_td_identities(pkg, game):
    nat = pkg.native
    ctx, tree = ctx_of(pkg, game)
    n = 3000
    c = Case(pkg, ctx, tree, 0, synth(tree, 0, n, np.random.RandomState(17)), net(pkg, 41))
    rl, rinfo = pkg.evaluation.memory_table(ctx, nat.MEM_RL, 0, c.dev, tree=tree)
    rl = rl.cpu().numpy()
    for quirks in QUIRKS:
        got, info = c.got(0.95, quirks)
        assert np.array_equal(got[..., 0], rl[..., 0]) and info == rinfo
        got0, _ = c.got(0.0, quirks)
        assert np.array_equal(got0[..., 1], rl[..., 1] << 23)              # r in half chips -> 2^-24 chips
    c.meta = c.meta | 0x100                                               # every record terminal
    c.dev = dev(mr.pack_rl(c.s, c.s2, c.meta, c.a))
    for quirks in (0, LIN):
        got, _ = c.got(0.95, quirks)
        assert (got[..., 2] == 0).all() and np.array_equal(got[..., 1], rl[..., 1] << 23)
    got, _ = c.got(0.95, LIN | TB)
    assert (got[..., 2] != 0).any()


# unmatched and bad records ---------------------------------------------------------------------
@pytest.mark.parametrize("game", GAMES)
def test_td_unmatched(pkg, game):
    ctx, tree = ctx_of(pkg, game)
    n = 3000
    rng = np.random.RandomState(8)
    s, s2, meta, a = synth(tree, 0, n, rng)
    mine = {o for o, _, _ in mr.sets_of(tree, 0)}
    other = np.array([o for o, _, _ in mr.sets_of(tree, 1) if o not in mine], np.int64)
    bad_s = np.arange(n) % 3 == 1                      # the other seat's s: a third of every wave
    s = s.copy()
    s[bad_s] = other[rng.randint(len(other), size=int(bad_s.sum()))]
    bad_k = np.arange(n) % 5 == 2                      # a stored argmax that is none
    meta = np.where(bad_k, (meta & ~np.uint32(0xFF)) | (3 + np.arange(n) % 250).astype(np.uint32), meta).astype(np.uint32)
    bad = bad_s | bad_k
    c = Case(pkg, ctx, tree, 0, (s, s2, meta, a), net(pkg, 51))
    for quirks in (0, LIN):
        want, info = c.check(0.95, quirks)
        assert info["unmatched"] == bad.sum() and info["matched"] == n - bad.sum()
        only, oinfo = c.want(0.95, quirks, keep=~bad)
        assert np.array_equal(want, only) and oinfo["unmatched"] == 0
        good = Case(pkg, ctx, tree, 0, (s[~bad], s2[~bad], meta[~bad], a[~bad]), c.w)
        got, ginfo = good.got(0.95, quirks)
        assert np.array_equal(got, want) and ginfo["matched"] == info["matched"]


# clamp -----------------------------------------------------------------------------------------
def test_td_clamp(pkg):
    ctx, tree = ctx_of(pkg, "leduc")
    n = 2000
    w = net(pkg, 61)
    w[30 * 64 + 64:] *= np.float32(400.0)               # W2 and b2: |Q| of some hundreds
    c = Case(pkg, ctx, tree, 0, synth(tree, 0, n, np.random.RandomState(9)), w)
    for quirks in QUIRKS:
        want, info = c.check(0.95, quirks)
        assert 0 < info["clamped"] < 2 * n
    assert (np.abs(c.qt(LIN)) >= 256).any() and (np.abs(c.qt(LIN)) < 256).any() and np.isfinite(c.qt(LIN)).all()


def test_td_nan_weight(pkg):
    ctx, tree = ctx_of(pkg, "leduc")
    n = 2000
    w = net(pkg, 62)
    w[30 * 64 + 64 + 3 * 5 + 1] = np.nan                # W2[5][1]: the call output of every forward
    c = Case(pkg, ctx, tree, 0, synth(tree, 0, n, np.random.RandomState(10)), w)
    assert np.isnan(c.qt(LIN)[:, 1]).all() and not np.isnan(c.qt(LIN)[:, [0, 2]]).any()
    assert not np.isnan(c.qt(0)).any()                  # the ReLU head's `o > 0 ? o : 0` drops it
    for quirks in QUIRKS:
        want, info = c.check(0.95, quirks)
        assert info["clamped"] == 0                     # fmaxf drops a NaN beside two numbers
    w[30 * 64 + 64 + 3 * 5:30 * 64 + 64 + 3 * 6] = np.nan    # all three outputs: v is NaN, fix gives 0
    c = Case(pkg, ctx, tree, 0, (c.s, c.s2, c.meta, c.a), w)
    want, info = c.check(0.95, LIN)
    boot = ((c.meta >> 8) & 1) == 0
    assert info["clamped"] == 2 * boot.sum() and (want[..., 2] == 0).all()
    c.check(0.95, LIN | TB)
    c.check(0.95, 0)


# contention ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nkeys", [1, 2])
def test_td_contention(pkg, nkeys):
    ctx, tree = ctx_of(pkg, "leduc")
    n = 100_000
    sets = [o for o, _, _ in mr.sets_of(tree, 1)]
    keys = np.array([sets[7], sets[100]][:nkeys], np.int64)[np.arange(n) % nkeys]
    c = Case(pkg, ctx, tree, 1, synth(tree, 1, n, np.random.RandomState(3), keys=keys), net(pkg, 71))
    want, _ = c.check(0.95, LIN)
    assert (want[..., 0].sum(axis=2) > 0).sum() == nkeys


# engine form -----------------------------------------------------------------------------------
def export_td(eng, tree, st, ctx):
    """The restatement over ``memories(agent)``'s fp32 export and the target weights (net 2)."""
    raw, infos = np.zeros((tree.ndec, 3, 3, 3), np.int64), []
    for p in (0, 1):
        m = eng.memories(p)
        s, s2, _, meta = mr.export_rl(m, st["rl_total"][p], int(st["rl_size"][p]))
        q = int(eng.cfg.quirks)
        qt = tr.forward(ctx, eng.get_weights(p, 2), tr.head_act(q), s2)
        one, info = tr.table(tree, p, s, meta, qt, float(eng.cfg.gamma), q)
        raw += one
        infos.append(info)
    return raw, infos


@pytest.mark.parametrize("game,quirks", [("leduc", "reference"), ("leduc", "textbook"), ("kuhn", "textbook")])
def test_td_engine(pkg, game, quirks):
    nat = pkg.native
    ctx, tree = ctx_of(pkg, game)
    q = (nat.QUIRKS_REFERENCE & ~nat.QUIRK_ALIAS_RL) if quirks == "reference" else nat.TEXTBOOK_MSE_DECAY
    eng = pkg.engine.SelfPlayEngine(ctx, init_seed=3, seed=77, quirks=q, n_lanes=1024, slices=4, rl_capacity=2048,
                                    sl_capacity=4096, eta=0.3)
    for _ in range(3):
        eng.step()
    st = eng.stats()
    log_cap = eng.memories(0)["log_cap"]
    print(f"rl_total {st['rl_total']} log_cap {log_cap} br_updates {st['br_updates']}")
    assert max(st["rl_total"]) > log_cap and min(st["br_updates"]) > 0      # wrapped: two pieces
    before = eng.state_digest()
    t, info = eng.td_table()
    t2, info2 = eng.td_table()
    assert np.array_equal(t.raw, t2.raw) and info == info2
    assert eng.state_digest() == before
    want, winfo = export_td(eng, tree, st, ctx)
    assert info == winfo
    assert np.array_equal(t.raw, want)
    rl, rinfo = eng.memory_table(nat.MEM_RL)
    assert np.array_equal(t.counts, rl.counts) and info == rinfo
    assert info[0]["records"] == 2048 and info[0]["unmatched"] == 0 and (t.raw[..., 2] != 0).any()
    assert np.nanmax(np.abs(t.mean_v)) < 64
    with pytest.raises(AttributeError):
        rl.mean_v
    eng.rollout()
    with pytest.raises(nat.NativeError, match="step boundary"):
        eng.td_table()
    eng.update()
    eng.close()


# group form ------------------------------------------------------------------------------------
def test_td_group(pkg):
    ctx, tree = ctx_of(pkg, "leduc")
    cfgs = [dict(n_lanes=256, slices=4, rl_capacity=1024, sl_capacity=2048, seed=50 + r, gamma=g)
            for r, g in enumerate((0.5, 0.95, 1.0))]
    grp = pkg.engine.EngineGroup(ctx=ctx, cfgs=cfgs, init_seed=9)
    for _ in range(3):
        grp.step()
    tabs = grp.td_tables()
    assert len(tabs) == 3
    for r, (t, info) in enumerate(tabs):
        one = pkg.engine.SelfPlayEngine(ctx, init_seed=9 + r, **cfgs[r])
        for _ in range(3):
            one.step()
        assert one.state_digest() == grp.replicas[r].state_digest()
        ot, oinfo = one.td_table()
        assert info == oinfo and info[0]["records"] > 0
        assert np.array_equal(t.raw, ot.raw)
        rt, rinfo = grp.replicas[r].td_table()            # the engine form on a replica's handle
        assert np.array_equal(t.raw, rt.raw) and info == rinfo
        one.close()
    assert not np.array_equal(tabs[0][0].raw, tabs[2][0].raw)
    grp.close()


# report ----------------------------------------------------------------------------------------
def same(a, b):
    """Equality of reports, a NaN equal to a NaN."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and a != a:
        return b != b
    return a == b


@pytest.mark.parametrize("game,quirks", [("leduc", "reference"), ("kuhn", "textbook")])
def test_q_report(pkg, game, quirks):
    ev, nat = pkg.evaluation, pkg.native
    NET_BR = pkg.engine.NET_BR
    ctx, tree = ctx_of(pkg, game)
    q = nat.QUIRKS_REFERENCE if quirks == "reference" else nat.TEXTBOOK_MSE_DECAY
    shape = dict(n_lanes=1024, slices=4) if game == "leduc" else dict(n_lanes=64, slices=1)
    cfgs = [dict(rl_capacity=2048, sl_capacity=4096, seed=60 + r, quirks=q, eta=0.3, **shape) for r in range(2)]
    grp = pkg.engine.EngineGroup(ctx=ctx, cfgs=cfgs, init_seed=5)
    for _ in range(2):
        grp.step()
    eng = grp.replicas[1]
    for eta in (None, 0.3):
        rep = eng.q_report(eta=eta)
        assert same(rep, eng.q_report(eta=eta))
        beta, _, reach = (t.cpu().numpy() for t in eng.best_response_table(eta=eta, values=True))
        legal = np.ones((tree.ndec, 3, 3), bool)
        legal[~tree.legal, :, 2] = False
        td, info = eng.td_table()
        for a in (0, 1):
            r = rep[a]
            mine = (tree.seat == a)[:, None]
            reached = mine & (reach > 0)
            w = np.where(reached, reach / reach[reached].sum(), 0.0)
            pol = ev.policy_table(ctx, eng.policy(a, NET_BR), tree).cpu().numpy()
            differs = np.argmax(pol, axis=2) != np.argmax(beta, axis=2)
            assert r["greedy_mismatch_share"] == float((w * differs)[reached].sum())
            assert r["td_pairs"] + r["td_empty_actions"] == (legal & mine[:, :, None]).sum()
            assert r["td_pairs"] == ((td.counts > 0) & legal & mine[:, :, None]).sum() > 0
            assert r["linear"] == (quirks == "textbook") and r["info"] == info[a]
            assert 0.0 <= r["greedy_mismatch_share"] <= 1.0 and 0.0 <= r["relu_blind_share"] <= 1.0
            assert r["q_rmse_exact"] >= 0 and r["td_rmse_exact"] >= 0 and r["fit_rmse_td"] >= 0
            print(game, quirks, eta, a, {k: v for k, v in r.items() if k != "info"})
    alls = grp.q_report_all()
    assert len(alls) == 2
    for r in range(2):
        assert same(alls[r], grp.replicas[r].q_report())
    assert not same(alls[0], alls[1])
    grp.close()

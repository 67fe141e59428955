"""Tabular NFSP on the device: the TD pass whose bootstrap reads a table (csrc/memtab.hip's fourth
kind: nfsp_tdq_table), the tables as rows (csrc/tabq.hip: nfsp_table_rows), the fitted-Q sweeps
(nfsp_engine_tabular_q, nfsp_group_tabular_q) and the tables acting (install_tabular_br / _ar).
Every comparison with tests/tabq_ref.py's restatement is equality: of int64 arrays, of ``info`` and
of float32 bit patterns."""
import numpy as np
import pytest
import torch

import act_table_ref as at
import memtab_ref as mr
import tabq_ref as tq
from memtab_ref import ctx_of, dev

pytestmark = pytest.mark.gpu

GAMES = ("leduc", "kuhn")
TB = 1                                          # NFSP_QUIRK_TERMINAL_BOOTSTRAP
GAMMAS = (0.0, 0.5, 1.0)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def words_with(rng, n, lo, hi):
    """n 30-bit words with popcount in [lo, hi]: more bits than any observation has."""
    c = rng.randint(lo, hi + 1, size=n)
    rank = np.argsort(np.argsort(rng.rand(n, 30), axis=1), axis=1)
    return ((rank < c[:, None]).astype(np.int64) << np.arange(30, dtype=np.int64)).sum(axis=1)


def synth(tree, seat, n, rng, keys=None, s2=None):
    """n synthetic M_RL records (s, s2, meta, a): s2 from the seat's own information sets, random
    words that are none, and zeros, a third each."""
    sets = np.array([o for o, _, _ in mr.sets_of(tree, seat)], np.int64)
    s = sets[rng.randint(len(sets), size=n)] if keys is None else np.asarray(keys, np.int64)
    a = mr.action_rows(n, rng)
    meta = mr.rl_meta(n, rng, a)
    if s2 is None:
        pool = rng.randint(3, size=n)
        s2 = np.where(pool == 0, sets[rng.randint(len(sets), size=n)], np.where(pool == 1, words_with(rng, n, 12, 30), 0))
    return s, np.asarray(s2, np.int64), meta, a


def rand_q(tree, rng):
    """A Q table with negatives -- every fifth row's middle rank has nothing else, so its bootstrap
    is negative -- in which the illegal raise's entry is the row's maximum in half of the rows
    where the raise is illegal."""
    q = rng.uniform(-6.0, 6.0, size=(tree.ndec, 3, 3)).astype(np.float32)
    q[::5, 1, :] = -np.abs(q[::5, 1, :]) - np.float32(0.125)
    il = np.nonzero(~tree.legal)[0]
    q[il[::2], ::2, 2] = np.float32(9.5)
    assert len(il) and (np.argmax(q[il], axis=2) == 2).any() and (q.max(axis=2) < 0).any()
    return q


class Case:
    def __init__(self, pkg, ctx, tree, seat, recs, q):
        self.pkg, self.ctx, self.tree, self.seat = pkg, ctx, tree, seat
        self.s, self.s2, self.meta, self.a = recs
        self.words = mr.pack_rl(self.s, self.s2, self.meta, self.a)
        self.dev = dev(self.words)
        self.q = q
        self.qdev = torch.as_tensor(q).cuda()

    def want(self, gamma, quirks, keep=None):
        k = slice(None) if keep is None else keep
        return tq.tdq(self.tree, self.seat, self.s[k], self.s2[k], self.meta[k], self.q, gamma, quirks)

    def got(self, gamma, quirks, segs=None, out=None):
        segs = ([self.dev] if len(self.words) else []) if segs is None else segs
        out, info = self.pkg.evaluation.tdq_table(self.ctx, self.seat, segs, self.qdev, gamma, quirks, out=out, tree=self.tree)
        return out.cpu().numpy(), info

    def check(self, gamma, quirks):
        got, info = self.got(gamma, quirks)
        want, winfo = self.want(gamma, quirks)
        assert info == winfo, (gamma, quirks, info, winfo)
        assert np.array_equal(got, want), (gamma, quirks)
        return want, winfo


# raw form --------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", GAMES)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097])
def test_tdq_raw_form(pkg, game, n):
    """The wave turn (64 x MT_U = 256 records) and the workgroup turn (4096) from both sides."""
    ctx, tree = ctx_of(pkg, game)
    for seat in (0, 1):
        rng = np.random.RandomState(1000 * n + seat)
        c = Case(pkg, ctx, tree, seat, synth(tree, seat, n, rng), rand_q(tree, rng))
        for quirks in (0, TB):
            for gamma in GAMMAS:
                want, info = c.check(gamma, quirks)
                assert want[..., 0].sum() == n == info["matched"] and info["clamped"] == 0
        if n >= 255:
            assert (c.want(0.5, 0)[0] != c.want(0.5, TB)[0]).any() and (c.want(0.5, 0)[0] != c.want(1.0, 0)[0]).any()


def test_tdq_illegal_raise_entry_counts(pkg):
    """Every s2 is a set whose largest entry is the illegal raise's: that entry is the bootstrap."""
    ctx, tree = ctx_of(pkg, "leduc")
    rng = np.random.RandomState(4)
    q = rand_q(tree, rng)
    rows = [d for d in np.nonzero(~tree.legal)[0] if tree.seat[d] == 0 and q[d, 0, 2] == q[d, 2, 2] == np.float32(9.5)]
    assert rows
    n = 600
    s2 = tree.obs[rng.choice(rows, size=n), 2 * rng.randint(2, size=n)].astype(np.int64)
    s, _, meta, a = synth(tree, 0, n, rng)
    meta = meta & ~np.uint32(0x100)                                        # no record terminal
    c = Case(pkg, ctx, tree, 0, (s, s2, meta, a), q)
    want, _ = c.check(1.0, 0)
    assert want[..., 2].sum() == n * int(9.5 * 2**24)


# segments --------------------------------------------------------------------------------------
def test_tdq_segments(pkg):
    nat = pkg.native
    ctx, tree = ctx_of(pkg, "leduc")
    n = 4097
    rng = np.random.RandomState(6)
    c = Case(pkg, ctx, tree, 1, synth(tree, 1, n, rng), rand_q(tree, rng))
    want, winfo = c.check(0.5, 0)
    recs = c.dev.reshape(n, 8)
    for lens in ([n], [2049, 0, 2048], [1001, 0, 333, 0, 2000, 500, 263, 0], [1, 500, 7, 1000, 64, 2000, 500, 25]):
        assert sum(lens) == n and len(lens) <= 8
        cut = np.concatenate([[0], np.cumsum(lens)])
        got, info = c.got(0.5, 0, segs=[recs[cut[k]:cut[k + 1]] for k in range(len(lens))])
        assert info == winfo and np.array_equal(got, want)
    with pytest.raises(nat.NativeError, match="segments"):
        c.got(0.5, 0, segs=[recs[k:k + 1] for k in range(9)])
    with pytest.raises(nat.NativeError, match="aligned"):
        c.got(0.5, 0, segs=[(recs.data_ptr() + 4, 16)])
    for kind in (nat.MEM_TD, nat.MEM_TDQ):              # the MEM_* forms take neither TD kind
        with pytest.raises(nat.NativeError, match="bad kind"):
            pkg.evaluation.memory_table(ctx, kind, 1, recs, tree=tree)
    # a seat's call leaves the other seat's rows alone
    out = torch.full((tree.ndec, 3, 3, 3), 7, dtype=torch.int64, device="cuda")
    got, _ = c.got(0.5, 0, out=out)
    other = tree.seat != 1
    assert (got[other] == 7).all() and np.array_equal(got[~other], want[~other])


# unmatched and terminal records ----------------------------------------------------------------
@pytest.mark.parametrize("game", GAMES)
def test_tdq_unmatched(pkg, game):
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
    c = Case(pkg, ctx, tree, 0, (s, s2, meta, a), rand_q(tree, rng))
    for quirks in (0, TB):
        want, info = c.check(0.5, quirks)
        assert info["unmatched"] == bad.sum() and info["matched"] == n - bad.sum()
        only, oinfo = c.want(0.5, quirks, keep=~bad)
        assert np.array_equal(want, only) and oinfo["unmatched"] == 0


@pytest.mark.parametrize("game", GAMES)
def test_tdq_s2_that_is_no_set_and_terminal_records(pkg, game):
    nat = pkg.native
    ctx, tree = ctx_of(pkg, game)
    n = 3000
    rng = np.random.RandomState(12)
    # no s2 is an information set of the seat (the other seat's, random words, zeros): every record
    # is counted, bootstraps 0 and adds 0 to field 2, so field 1 is the rewards' whatever gamma
    mine = {o for o, _, _ in mr.sets_of(tree, 0)}
    other = np.array([o for o, _, _ in mr.sets_of(tree, 1) if o not in mine], np.int64)
    pool = rng.randint(3, size=n)
    s2 = np.where(pool == 0, other[rng.randint(len(other), size=n)], np.where(pool == 1, words_with(rng, n, 12, 30), 0))
    c = Case(pkg, ctx, tree, 0, synth(tree, 0, n, rng, s2=s2), rand_q(tree, rng))
    rl, rinfo = pkg.evaluation.memory_table(ctx, nat.MEM_RL, 0, c.dev, tree=tree)
    rl = rl.cpu().numpy()
    for quirks in (0, TB):
        want, info = c.check(1.0, quirks)
        assert want[..., 0].sum() == n and (want[..., 2] == 0).all() and info == rinfo
        assert np.array_equal(want[..., 1], rl[..., 1] << 23)
    # every record terminal, every s2 a set: nothing bootstraps with the quirk off, all do with it on
    sets = np.array([o for o, _, _ in mr.sets_of(tree, 0)], np.int64)
    s, _, meta, a = synth(tree, 0, n, rng)
    c = Case(pkg, ctx, tree, 0, (s, sets[rng.randint(len(sets), size=n)], meta | np.uint32(0x100), a), c.q)
    want, _ = c.check(1.0, 0)
    assert (want[..., 2] == 0).all() and np.array_equal(want[..., 1], pkg.evaluation.memory_table(
        ctx, nat.MEM_RL, 0, c.dev, tree=tree)[0].cpu().numpy()[..., 1] << 23)
    want, _ = c.check(1.0, TB)
    assert (want[..., 2] != 0).any()


# identities ------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", GAMES)
def test_tdq_identities(pkg, game):
    nat = pkg.native
    ctx, tree = ctx_of(pkg, game)
    n = 3000
    rng = np.random.RandomState(17)
    c = Case(pkg, ctx, tree, 0, synth(tree, 0, n, rng), rand_q(tree, rng))
    rl, rinfo = pkg.evaluation.memory_table(ctx, nat.MEM_RL, 0, c.dev, tree=tree)
    rl = rl.cpu().numpy()
    for quirks in (0, TB):
        got, info = c.got(0.5, quirks)
        assert np.array_equal(got[..., 0], rl[..., 0]) and info == rinfo
        got0, _ = c.got(0.0, quirks)
        assert np.array_equal(got0[..., 1], rl[..., 1] << 23)              # r in half chips -> 2^-24 chips


# clamp -----------------------------------------------------------------------------------------
def test_tdq_clamp(pkg):
    ctx, tree = ctx_of(pkg, "leduc")
    n = 3000
    rng = np.random.RandomState(9)
    q = rand_q(tree, rng)
    rows = np.nonzero(tree.seat == 0)[0]
    q[rows[0], 0, 1] = np.float32(1e30)                 # saturates v and the bootstrap
    q[rows[1], 1, 0] = np.float32(-1e30)                # loses the maximum: no effect
    q[rows[2], 2, 1] = np.nan                           # fmaxf drops a NaN beside two numbers
    q[rows[3], 0, :] = np.nan                           # all three: the bootstrap is NaN, fix gives 0
    q[rows[4], 1, 2] = np.float32(300.0)                # finite, beyond fix's range
    hit = tree.obs[rows[:5], [0, 1, 2, 0, 1]].astype(np.int64)
    s, s2, meta, a = synth(tree, 0, n, rng)
    s2[::3] = hit[np.arange(len(s2[::3])) % 5]
    c = Case(pkg, ctx, tree, 0, (s, s2, meta, a), q)
    for quirks in (0, TB):
        for gamma in GAMMAS:
            want, info = c.check(gamma, quirks)
            assert 0 < info["clamped"] < 2 * n
    want, _ = c.want(1.0, TB)
    assert (np.abs(want[..., 1:]) >= 2**32 - 1).any()


# contention ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nkeys", [1, 2])
def test_tdq_contention(pkg, nkeys):
    ctx, tree = ctx_of(pkg, "leduc")
    n = 100_000
    rng = np.random.RandomState(3)
    sets = [o for o, _, _ in mr.sets_of(tree, 1)]
    keys = np.array([sets[7], sets[100]][:nkeys], np.int64)[np.arange(n) % nkeys]
    c = Case(pkg, ctx, tree, 1, synth(tree, 1, n, rng, keys=keys), rand_q(tree, rng))
    want, _ = c.check(0.5, 0)
    assert (want[..., 0].sum(axis=2) > 0).sum() == nkeys


# rows ------------------------------------------------------------------------------------------
def synth_tables(tree, rng, n):
    """n int64 tables of both shapes of content: counts with many zeros, sums of either sign, some
    beyond 2^53 (no memory gives them: built here), and M_SL-like rows, some with a negative mass,
    some with mass but no count, some with a count and no mass."""
    raw = np.zeros((n, tree.ndec, 3, 3, 3), np.int64)
    raw[..., 0] = rng.randint(0, 4, size=raw.shape[:-1]) * (rng.rand(*raw.shape[:-1]) < 0.6)
    raw[..., 1] = rng.randint(-(1 << 40), 1 << 40, size=raw.shape[:-1])
    pos = rng.rand(n, tree.ndec, 3) < 0.7               # most sets: non-negative masses
    raw[..., 1] = np.where(pos[..., None], np.abs(raw[..., 1]), raw[..., 1])
    huge = rng.rand(*raw.shape[:-1]) < 0.1
    raw[..., 1] = np.where(huge, (raw[..., 1] << 21) + 12345, raw[..., 1])
    raw[rng.rand(n, tree.ndec, 3) < 0.1, :, 1] = 0      # a count and no mass
    raw[..., 2] = rng.randint(-5, 5, size=raw.shape[:-1])
    assert (np.abs(raw[..., 1]) > 1 << 53).any()
    return raw


@pytest.mark.parametrize("game", GAMES)
def test_table_rows(pkg, game):
    ev, nat = pkg.evaluation, pkg.native
    ctx, tree = ctx_of(pkg, game)
    rng = np.random.RandomState(23)
    n = 3
    raw = synth_tables(tree, rng, n)
    fill = rng.uniform(-2.0, 2.0, size=(n, tree.ndec, 3, 3)).astype(np.float32)
    prev = fill.copy()
    prev[:, ::2] = rng.uniform(-2.0, 2.0, size=prev[:, ::2].shape).astype(np.float32)
    for stat in (nat.ROWS_SL_MASS, nat.ROWS_SL_ARGMAX, nat.ROWS_TD_MEAN):
        for f in (fill, None):
            want = tq.rows(stat, raw, f)
            assert (want != (0 if f is None else f)).any() and (want == (0 if f is None else f)).any()
            got, ch = ev.table_rows(ctx, stat, raw, f, tree=tree)
            assert ch is None and got.dtype == torch.float32 and tuple(got.shape) == (n, tree.ndec, 3, 3)
            assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (stat, f is None)
            got2, ch = ev.table_rows(ctx, stat, raw, f, prev=prev, tree=tree)
            assert torch.equal(got2, got) and ch == [tq.changed(prev[t], want[t]) for t in range(n)] and min(ch) > 0
            _, ch = ev.table_rows(ctx, stat, raw, f, prev=got, tree=tree)           # the output itself
            assert ch == [0] * n
        one, ch = ev.table_rows(ctx, stat, raw[1], fill[1], prev=prev[1], tree=tree)
        assert tuple(one.shape) == (tree.ndec, 3, 3) and ch == tq.changed(prev[1], tq.rows(stat, raw[1], fill[1]))
        assert np.array_equal(bits(one.cpu().numpy()), bits(tq.rows(stat, raw[1], fill[1])))
    want = tq.rows(nat.ROWS_SL_MASS, raw, fill)
    neg = (raw[..., 1] < 0).any(axis=-1) & (raw[..., 0].sum(axis=-1) > 0) & (raw[..., 1].sum(axis=-1) > 0)
    assert neg.any() and np.array_equal(want[neg], fill[neg])                       # a negative mass: fill's row
    with pytest.raises(nat.NativeError, match="bad stat"):
        ev.table_rows(ctx, 3, raw, tree=tree)
    with pytest.raises(ValueError):
        ev.table_rows(ctx, nat.ROWS_TD_MEAN, raw, fill[:2], tree=tree)


# engine ----------------------------------------------------------------------------------------
def export_recs(eng, st):
    """[(s, s2, meta) of agent p's live M_RL records] from ``memories``' fp32 export."""
    out = []
    for p in (0, 1):
        s, s2, _, meta = mr.export_rl(eng.memories(p), st["rl_total"][p], int(st["rl_size"][p]))
        out.append((s, s2, meta))
    return out


def export_sl(eng, tree, st):
    """The joint M_SL table of the restatement from ``memories``' export."""
    raw = np.zeros((tree.ndec, 3, 3, 3), np.int64)
    for p in (0, 1):
        m, n = eng.memories(p), int(st["sl_size"][p])
        raw += mr.table(tree, p, mr.SL, mr.bits_of(m["sl_s"][:n].cpu().numpy()), a=m["sl_a"][:n].cpu().numpy())[0]
    return raw


def engine_of(pkg, ctx, game, quirks, **kw):
    shape = dict(n_lanes=1024, slices=4) if game == "leduc" else dict(n_lanes=64, slices=1)
    cfg = dict(init_seed=3, seed=77, quirks=quirks, rl_capacity=2048, sl_capacity=4096, eta=0.3, **shape)
    cfg.update(kw)
    return pkg.engine.SelfPlayEngine(ctx, **cfg)


@pytest.mark.parametrize("game,quirks,filled", [("leduc", "reference", True), ("leduc", "textbook", False),
                                                ("kuhn", "reference", False), ("kuhn", "textbook", True)])
def test_tabular_q_engine(pkg, game, quirks, filled):
    nat = pkg.native
    ctx, tree = ctx_of(pkg, game)
    q = nat.QUIRKS_REFERENCE if quirks == "reference" else nat.TEXTBOOK_MSE_DECAY
    eng = engine_of(pkg, ctx, game, q, gamma=0.9)
    for _ in range(3):
        eng.step()
    st = eng.stats()
    log_cap = eng.memories(0)["log_cap"]
    print(f"rl_total {st['rl_total']} log_cap {log_cap} nlev {tree.nlev}")
    assert min(st["rl_total"]) > 0 and (game == "kuhn" or max(st["rl_total"]) > log_cap)      # wrapped: two pieces
    fill = np.random.RandomState(5).uniform(-1.0, 1.0, size=(tree.ndec, 3, 3)).astype(np.float32) if filled else None
    recs = export_recs(eng, st)
    before = eng.state_digest()
    last = {}
    for K in (1, 2, tree.nlev, tree.nlev + 1):
        got_q, tab, info, ch = eng.tabular_q(sweeps=K, fill=fill)
        want_q, want_raw, winfo, wch = tq.sweeps(tree, recs, 0.9, q, K, fill)
        assert info == winfo and ch == wch, (K, info, winfo, ch, wch)
        assert np.array_equal(tab.raw, want_raw), K
        assert np.array_equal(bits(got_q.cpu().numpy()), bits(want_q)), K
        assert tab.kind == nat.MEM_TDQ and info[0]["unmatched"] == 0 and info[0]["records"] == int(st["rl_size"][0])
        last[K] = (bits(got_q.cpu().numpy()), ch)
        print(f"sweeps {K}: changed {ch}")
    assert last[1][1] > 0 and (last[1][0] != last[tree.nlev][0]).any()
    if quirks == "textbook":                                                 # no aliasing: nlev sweeps are the fixed point
        assert last[tree.nlev + 1][1] == 0 and np.array_equal(last[tree.nlev + 1][0], last[tree.nlev][0])
    got_q, tab, info, ch = eng.tabular_q(fill=fill)                          # sweeps None: nlev, and the same bits again
    assert np.array_equal(bits(got_q.cpu().numpy()), last[tree.nlev][0]) and ch == last[tree.nlev][1]
    if fill is not None:
        unseen = tab.counts == 0
        assert unseen.any() and np.array_equal(bits(got_q.cpu().numpy())[unseen], bits(fill)[unseen])
    assert eng.state_digest() == before
    for bad in (0, 65):
        with pytest.raises(nat.NativeError, match="sweeps"):
            eng.tabular_q(sweeps=bad)
    eng.rollout()
    with pytest.raises(nat.NativeError, match="step boundary"):
        eng.tabular_q()
    eng.update()
    eng.close()


@pytest.mark.parametrize("game", GAMES)
def test_tabular_q_report(pkg, game):
    nat = pkg.native
    ctx, tree = ctx_of(pkg, game)
    eng = engine_of(pkg, ctx, game, nat.TEXTBOOK_MSE_DECAY)
    for _ in range(3):
        eng.step()
    for eta in (None, 0.3):
        rep = eng.tabular_q_report(eta=eta)
        for a in (0, 1):
            r = rep[a]
            print(game, eta, a, {k: v for k, v in r.items() if k != "info"})
            assert r["fit_rmse_td"] == 0.0 and r["linear"] is True and r["td_pairs"] > 0
            for k in ("q_rmse_exact", "greedy_mismatch_share", "relu_blind_share", "td_rmse_exact", "mean_bootstrap_share"):
                assert np.isfinite(r[k]), k
            assert 0.0 <= r["greedy_mismatch_share"] <= 1.0
    eng.close()


# acting ----------------------------------------------------------------------------------------
ACT_QUIRKS = 1 | 2 | 64                        # TERMINAL_BOOTSTRAP | ROW0_TARGET | EXT_EPS_CONST: no alias, no sampling


def new_records(eng, p, kind, before):
    """(observation words, action vectors) of the records agent p's memory ``kind`` gained since
    the stats ``before``; asserts that none was overwritten."""
    st, m = eng.stats(), eng.memories(p)
    t0, t1 = int(before[f"{kind}_total"][p]), int(st[f"{kind}_total"][p])
    cap = m["log_cap"] if kind == "rl" else m["sl_s"].shape[0]
    assert t0 < t1 <= cap
    idx = torch.arange(t0, t1, device=m[f"{kind}_s"].device)
    return mr.bits_of(m[f"{kind}_s"][idx].cpu().numpy()), m[f"{kind}_a"][idx].cpu().numpy()


def rows_at(tree, lib, game_id, p, words, rows):
    sid = np.array([lib.nfsp_memtab_lookup(game_id, p, int(x)) for x in words], np.int64)
    assert sid.min() >= 0
    return sid, np.asarray(rows, np.float32).reshape(tree.ndec * 3, 3)[sid]


@pytest.mark.parametrize("game", GAMES)
def test_tabular_br_acts(pkg, lib, game):
    """eta = 1 and a constant epsilon of 0: every decision of the rollout after
    ``install_tabular_br`` is the BR role's, so every new M_RL and M_SL record holds the Q row of
    its information set, raw bits (a random action has probability 2^-24 per decision; the seeds
    are fixed).  ``fill`` has no zero, so no row is all-zero (the fold that leaves no record)."""
    E = pkg.engine
    ctx, tree = ctx_of(pkg, game)
    eng = engine_of(pkg, ctx, game, ACT_QUIRKS, eta=1.0, epsilon=0.0, rl_capacity=1 << 16, sl_capacity=1 << 16)
    for _ in range(2):
        eng.step()
    st = eng.stats()
    fill = np.random.RandomState(8).uniform(0.25, 1.0, size=(tree.ndec, 3, 3)).astype(np.float32)
    q, tab, info, ch = eng.install_tabular_br(fill=fill)
    want_q = tq.sweeps(tree, export_recs(eng, st), float(eng.cfg.gamma), ACT_QUIRKS, tree.nlev, fill)[0]
    assert np.array_equal(bits(q.cpu().numpy()), bits(want_q)) and ch == 0
    assert (tab.counts > 0).any() and (tab.counts == 0).any()
    eng.step()
    for p in (0, 1):
        rows, misses = eng.act_table(p, E.NET_BR)
        assert misses == 0 and np.array_equal(bits(rows.cpu().numpy()), bits(want_q)) and eng.act_table(p, E.NET_AR)[0] is None
        seen = set()
        for kind in ("rl", "sl"):
            words, a = new_records(eng, p, kind, st)
            sid, want = rows_at(tree, lib, mr.game_id(pkg, game), p, words, want_q)
            assert np.array_equal(bits(a), bits(want)), f"agent {p} {kind}: a record differs from its Q row"
            seen |= set(sid.tolist())
        at = np.array(sorted(seen))
        cnt = tab.counts.reshape(-1, 3)[at]
        print(f"game {game} agent {p}: records at {len(seen)} sets, {int((cnt.sum(axis=1) > 0).sum())} with fitted entries, "
              f"{int((cnt == 0).sum())} entries of fill's among their rows")
        assert (cnt > 0).any() and (cnt == 0).any()                         # fitted entries act, and fill's do
    eng.clear_act_tables()
    assert all(eng.act_table(a, r)[0] is None for a in (0, 1) for r in (0, 1))
    eng.close()


@pytest.mark.parametrize("stat,filled", [("mass", True), ("argmax", False)])
def test_tabular_ar_acts(pkg, lib, stat, filled):
    """eta = 0.5 and a constant epsilon of 0, Leduc.  After two steps M_SL has records at some
    information sets and none at others (the restatement's table shows both).  The AR role then acts
    with M_SL's table, the BR role with ``act_table_ref.lookup_table`` (every value >= 2), so a new
    M_RL record is the BR role's if a[0] >= 2 and the AR role's otherwise, and must hold that
    table's row of its information set, raw bits; M_SL gains BR-role records only."""
    E, nat = pkg.engine, pkg.native
    ctx, tree = ctx_of(pkg, "leduc")
    eng = engine_of(pkg, ctx, "leduc", ACT_QUIRKS, eta=0.5, epsilon=0.0, rl_capacity=1 << 16, sl_capacity=1 << 16)
    for _ in range(2):
        eng.step()
    st = eng.stats()
    raw = export_sl(eng, tree, st)
    if filled:
        fill = at.full_support_table(tree, 11)
    else:                                               # the AR nets' own softmax rows, each agent's where it acts
        heads = pkg.evaluation.head_tables(ctx, [eng._wptr(a, E.NET_AR) for a in (0, 1)], [nat.ACT_SOFTMAX] * 2, tree).cpu().numpy()
        fill = np.where((tree.seat == 0)[:, None, None], heads[0], heads[1])
    want = tq.rows(tq.ROWS_SL_MASS if stat == "mass" else tq.ROWS_SL_ARGMAX, raw, fill)
    empty = raw[..., 0].sum(axis=2) == 0
    assert empty.any() and (~empty).any() and not np.array_equal(want[~empty], fill[~empty])
    rows = eng.install_tabular_ar(stat, fill if filled else None)
    assert np.array_equal(bits(rows.cpu().numpy()), bits(want))
    assert np.array_equal(bits(want[empty]), bits(fill[empty]))              # fill's rows where M_SL never was
    marker = at.lookup_table(tree, 36)
    for a in (0, 1):
        eng.set_act_table(a, E.NET_BR, marker)
    eng.step()
    at_empty = 0
    for p in (0, 1):
        assert eng.act_table(p, E.NET_AR)[1] == 0 and eng.act_table(p, E.NET_BR)[1] == 0
        assert np.array_equal(bits(eng.act_table(p, E.NET_AR)[0].cpu().numpy()), bits(want))
        words, a = new_records(eng, p, "rl", st)
        br = a[:, 0] >= 2.0
        assert br.any() and (~br).any()
        sid, got_ar = rows_at(tree, lib, mr.game_id(pkg, "leduc"), p, words[~br], want)
        assert np.array_equal(bits(a[~br]), bits(got_ar)), f"agent {p}: an AR-role record differs from M_SL's row"
        assert np.array_equal(bits(a[br]), bits(rows_at(tree, lib, mr.game_id(pkg, "leduc"), p, words[br], marker)[1]))
        at_empty += int(empty.reshape(-1)[sid].sum())
        words, a = new_records(eng, p, "sl", st)
        assert np.array_equal(bits(a), bits(rows_at(tree, lib, mr.game_id(pkg, "leduc"), p, words, marker)[1]))
    print(f"{stat}: {int(empty.sum())} of {empty.size} sets without an M_SL record; {at_empty} AR-role records there")
    assert at_empty > 0
    eng.close()


def test_clear_act_tables_restores_the_trajectory(pkg):
    ctx, tree = ctx_of(pkg, "leduc")
    nat = pkg.native
    eng, twin = (engine_of(pkg, ctx, "leduc", nat.QUIRKS_REFERENCE) for _ in range(2))
    for _ in range(2):
        eng.step()
        twin.step()
    eng.install_tabular_br()
    eng.install_tabular_ar("argmax")
    assert all(eng.act_table(a, r)[0] is not None for a in (0, 1) for r in (0, 1))
    assert eng.state_digest() == twin.state_digest()                        # tables are not state
    eng.clear_act_tables()
    for _ in range(2):
        eng.step()
        twin.step()
        assert eng.state_digest() == twin.state_digest()
    eng.install_tabular_br()
    eng.install_tabular_ar("mass")
    eng.step()
    twin.step()
    assert eng.state_digest() != twin.state_digest()                        # and they do act
    eng.close()
    twin.close()


# group -----------------------------------------------------------------------------------------
def test_tabular_group(pkg):
    E, nat = pkg.engine, pkg.native
    ctx, tree = ctx_of(pkg, "leduc")
    cfgs = [dict(n_lanes=256, slices=4, rl_capacity=1024, sl_capacity=2048, seed=50 + r, gamma=g)
            for r, g in enumerate((0.5, 0.9, 1.0))]
    grp, plain = (E.EngineGroup(ctx=ctx, cfgs=cfgs, init_seed=9) for _ in range(2))
    solo = [E.SelfPlayEngine(ctx, init_seed=9 + r, **cfgs[r]) for r in range(3)]
    for _ in range(3):
        grp.step()
        plain.step()
        for e in solo:
            e.step()
    fill = np.random.RandomState(2).uniform(-1.0, 1.0, size=(3, tree.ndec, 3, 3)).astype(np.float32)
    for f in (None, fill):
        alls = grp.tabular_q_all(sweeps=3, fill=f)
        assert len(alls) == 3
        for r, (q, tab, info, ch) in enumerate(alls):
            oq, otab, oinfo, och = solo[r].tabular_q(sweeps=3, fill=None if f is None else f[r])
            assert info == oinfo and ch == och and info[0]["records"] > 0
            assert np.array_equal(tab.raw, otab.raw) and torch.equal(q.view(torch.int32), oq.view(torch.int32))
            rq, rtab, rinfo, rch = grp.replicas[r].tabular_q(sweeps=3, fill=None if f is None else f[r])   # a replica's handle
            assert np.array_equal(rtab.raw, tab.raw) and torch.equal(rq.view(torch.int32), q.view(torch.int32)) and rinfo == info
        assert not torch.equal(alls[0][0], alls[2][0])
    # replica 1 acts by tables: the others' runs are a table-free group's
    res = grp.replicas[1].install_tabular_br()
    rows = grp.replicas[1].install_tabular_ar("mass")
    assert torch.equal(grp.replicas[1].act_table(0, E.NET_BR)[0], res[0]) and torch.equal(grp.replicas[1].act_table(1, E.NET_AR)[0], rows)
    assert grp.replicas[0].act_table(0, E.NET_BR)[0] is None
    grp.step()
    plain.step()
    dg, dp = grp.state_digest(), plain.state_digest()
    assert dg[0] == dp[0] and dg[2] == dp[2] and dg[1] != dp[1]
    assert all(grp.replicas[1].act_table(a, r)[1] == 0 for a in (0, 1) for r in (0, 1))
    # the group forms install for every replica, and clear_act_tables undoes a replica's
    br = grp.install_tabular_br_all(sweeps=2)
    ar = grp.install_tabular_ar_all("argmax")
    for r in range(3):
        assert torch.equal(grp.replicas[r].act_table(1, E.NET_BR)[0], br[r][0])
        assert torch.equal(grp.replicas[r].act_table(0, E.NET_AR)[0], ar[r])
        grp.replicas[r].clear_act_tables()
        assert all(grp.replicas[r].act_table(a, k)[0] is None for a in (0, 1) for k in (0, 1))
    for e in solo:
        e.close()
    grp.close()
    plain.close()

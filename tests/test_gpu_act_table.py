"""Tables that act (nfsp_engine_set_act_table; rollout.hip k_rollout_t, k_rollout_gt) on the device.

1. lookup      every record a table produced holds the installed row of its information set, bit
               for bit, at every information set of Leduc and Kuhn; every other record is an
               epsilon-random vector.
2. head tables a net's own head table (nfsp_head_tables) in its slot is the net: three steps with
               the learner running leave the digest, the stats and the six nets of a twin engine
               without tables, with all four slots set and with one.
3. frequencies a played full-support table's records per (information set, stored action) against
               the exact tree probabilities of tests/act_table_ref.py, with teeth.
4. oracle BR   install_oracle_br's first iteration: M_SL holds exactly the installed best response,
               whose gap to the exact best response is 0.
5. group       a replica with tables among replicas without, pipelined slices, against standalone
               engines.
"""
import numpy as np
import pytest
import torch

import act_table_ref as at
import rollout_dist_ref as rd
from engine_ref import nets

pytestmark = pytest.mark.gpu

TABLE_SEED = 36
_TREES = {}


def tree_of(pkg, game):
    if game not in _TREES:
        _TREES[game] = pkg.evaluation.GameTree(game)
    return _TREES[game]


def _bits(x):
    """[n, 30] 0/1 float rows (device) -> int64 bit masks (device), a million rows at a time."""
    w = torch.ones(30, dtype=torch.int64, device=x.device) << torch.arange(30, device=x.device)
    return torch.cat([((x[i:i + (1 << 20)] != 0).to(torch.int64) * w).sum(dim=1) for i in range(0, x.shape[0], 1 << 20)]
                     or [torch.zeros(0, dtype=torch.int64, device=x.device)])


def _records(eng, p, kind):
    """(observation bits, action vectors) of agent p's stored M_RL / M_SL records, on the device;
    asserts that the memory has not wrapped."""
    st, m = eng.stats(), eng.memories(p)
    n = int(st[f"{kind}_size"][p])
    assert n == st[f"{kind}_total"][p] and n <= (m["log_cap"] if kind == "rl" else m["sl_s"].shape[0])
    return _bits(m[f"{kind}_s"][:n]), m[f"{kind}_a"][:n]


# ---- 1: the lookup, bit for bit ----------------------------------------------------------------------
# game -> lanes: 2^k + 100 (no multiple of 512: a partial last workgroup), the smallest k at which
# the least-visited information set expects >= 20 table-valued records (see the test's docstring)
LOOKUP_LANES = {0: (1 << 21) + 100, 1: (1 << 12) + 100}


@pytest.mark.parametrize("game", [0, 1])
def test_lookup_is_bit_exact_at_every_information_set(pkg, lib, game):
    """Both agents' BR role plays ``act_table_ref.lookup_table`` (seed 36) at eta = 1 with a constant
    epsilon of 0.5, reference quirks without the alias.  A record whose a[0] >= 2 came from a table
    and must hold the row at ``nfsp_memtab_lookup(game, seat, s)``, all three components, raw bits;
    every other record is an epsilon-random vector, all components < 1.  No lookup may miss.

    Coverage (``act_table_ref.eps_greedy_visits``, computed before the lane count was fixed): per lane
    the least-visited information set expects 1.286e-5 table-valued decisions on Leduc (the best of
    table seeds 0..59: deep raise lines need several random actions) and 5.787e-3 on Kuhn.  With
    2^k + 100 lanes the smallest k with >= 20 expected records there is 21 on Leduc (26.97; k = 20
    gives 13.5) and 12 on Kuhn (24.28).  Every (row, rank) of both seats must occur among the
    table-valued records of each memory."""
    nat = pkg.native
    tree = tree_of(pkg, game)
    rows = at.lookup_table(tree, TABLE_SEED)
    n = LOOKUP_LANES[game]
    exp_min = at.eps_greedy_visits(tree, rows, 0.5).min() * n
    print(f"game {game}: {n} lanes, least expected table-valued records per information set {exp_min:.2f}")
    assert exp_min >= 20.0 and n % 512 != 0
    eng = pkg.engine.SelfPlayEngine(game=game, n_lanes=n, seed=77, init_seed=3, eta=1.0, epsilon=0.5,
                                    quirks=nat.QUIRK_TERMINAL_BOOTSTRAP | nat.QUIRK_ROW0_TARGET | nat.EXT_EPS_CONST,
                                    rl_capacity=4 * n, sl_capacity=4 * n, inserts_per_update=1 << 30)
    for a in (0, 1):
        eng.set_act_table(a, pkg.engine.NET_BR, rows)
    eng.step()
    want = torch.as_tensor(rows.view(np.int32).reshape(-1, 3), device=eng.dev)      # [ndec * 3, 3]
    for p in (0, 1):
        got_rows, misses = eng.act_table(p, pkg.engine.NET_BR)
        assert misses == 0 and np.array_equal(got_rows.cpu().numpy().view(np.uint32), rows.view(np.uint32))
        for kind in ("rl", "sl"):
            bits, a = _records(eng, p, kind)
            tab = a[:, 0] >= 2.0
            assert bool((a[~tab] < 1.0).all()), "a record that is neither a table's row nor an epsilon-random vector"
            u, inv = torch.unique(bits[tab], return_inverse=True)
            sid = [lib.nfsp_memtab_lookup(game, p, int(x)) for x in u.cpu().tolist()]
            assert min(sid) >= 0
            sid_t = torch.as_tensor(sid, device=eng.dev)[inv]
            assert torch.equal(a[tab].view(torch.int32), want[sid_t]), f"agent {p} {kind}: a record differs from its row"
            seen = {s for s in sid}
            need = {int(d) * 3 + r for d in np.nonzero(tree.seat == p)[0] for r in range(3)}
            assert seen == need, f"agent {p} {kind}: information sets without a table-valued record: {sorted(need - seen)}"
            cnt = torch.bincount(sid_t, minlength=tree.ndec * 3).cpu().numpy()
            print(f"agent {p} {kind}: {int(tab.sum())} table-valued of {len(a)} records, least per information set "
                  f"{cnt[sorted(need)].min()}")
    eng.close()


# ---- 2: a net's own head table is the net --------------------------------------------------------------
def _install_heads(pkg, eng, slots):
    nat, E = pkg.native, pkg.engine
    br_act = nat.ACT_LINEAR if eng.cfg.quirks & nat.EXT_LINEAR_Q else nat.ACT_RELU
    ws = [eng._wptr(a, role) for a, role in slots]
    heads = pkg.evaluation.head_tables(eng.ctx, ws, [nat.ACT_SOFTMAX if role == E.NET_AR else br_act for _, role in slots])
    for k, (a, role) in enumerate(slots):
        eng.set_act_table(a, role, heads[k])


def _same_state(a, b):
    assert a.state_digest() == b.state_digest()
    sa, sb = a.stats(), b.stats()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(np.asarray(sa[k], np.float64).view(np.uint64), np.asarray(sb[k], np.float64).view(np.uint64)), k
    for x, y in zip(nets(a), nets(b)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("quirks", ["reference", "textbook_mse_decay"])
@pytest.mark.parametrize("slots", ["all", "one"])
def test_own_head_tables_are_the_nets(pkg, quirks, slots):
    """The TAB variant's control flow against the shipped kernel over everything a step writes."""
    nat, E = pkg.native, pkg.engine
    q = nat.QUIRKS_REFERENCE if quirks == "reference" else nat.TEXTBOOK_MSE_DECAY
    cfg = dict(n_lanes=1000, seed=5, init_seed=9, quirks=q, rl_capacity=3000, sl_capacity=3000, slices=1)
    eng, twin = E.SelfPlayEngine(**cfg), E.SelfPlayEngine(**cfg)
    which = [(a, r) for a in (0, 1) for r in (E.NET_AR, E.NET_BR)] if slots == "all" else [(1, E.NET_BR)]
    for _ in range(3):
        _install_heads(pkg, eng, which)
        eng.step()
        twin.step()
        _same_state(eng, twin)
    st = eng.stats()
    assert min(st["br_updates"]) > 0 and min(st["ar_updates"]) > 0          # the learner ran
    assert all(eng.act_table(a, r)[1] == 0 and eng.act_table(a, r)[0] is not None for a, r in which)
    assert twin.act_table(0, 0) == (None, 0)
    eng.close()
    twin.close()


# ---- 3: frequencies of a played table ------------------------------------------------------------------
FREQ_LANES = 262_144


def test_frequencies_of_a_played_table(pkg):
    """Both agents' AR role plays one full-support table, sampled (NFSP_EXT_SAMPLE_AR), at eta = 0:
    M_RL's counts per (row, rank, stored argmax) against ``act_table_ref.TableModel``.

    The bound is rollout_dist_ref's, derived and not measured: a binomial z per cell whose expectation
    lies in [100, n - 100], the other cells pooled per seat with variance 4 E, cells of probability 0
    exactly 0 (none here: the table has full support) -- no cell is left out -- and |z| <= z*(K)
    for the at most K = 9 ndec + 2 statistics asserted, K erfc(z* / sqrt 2) <= 1e-6.  Not modelled (each moves
    an expectation by less than 0.1 counts at 262,144 lanes, see act_table_ref): the 2^-24
    probability of BR mode at eta = 0 and the 24-bit grid of the sampling draw.
    Teeth: the same counts against the model of another seed's table must fail the bound."""
    nat = pkg.native
    tree = tree_of(pkg, 0)
    rows = at.full_support_table(tree, 17)
    eng = pkg.engine.SelfPlayEngine(n_lanes=FREQ_LANES, seed=1234, init_seed=11, eta=0.0,
                                    quirks=nat.QUIRK_TERMINAL_BOOTSTRAP | nat.QUIRK_ROW0_TARGET | nat.EXT_SAMPLE_AR,
                                    rl_capacity=4 * FREQ_LANES, inserts_per_update=1 << 30)
    for a in (0, 1):
        eng.set_act_table(a, pkg.engine.NET_AR, rows)
    eng.step()
    tab, info = eng.memory_table(nat.MEM_RL)
    st = eng.stats()
    for p in (0, 1):
        assert info[p]["matched"] == info[p]["records"] == st["rl_total"][p] <= 4 * FREQ_LANES
        assert eng.act_table(p, pkg.engine.NET_AR)[1] == 0
    assert sum(st["sl_total"]) <= 1                        # eta = 0: BR mode has probability 2^-24 per seat
    obs = tab.counts.astype(np.float64)
    nb = rd.dealer_lanes(0, FREQ_LANES, 0)
    K = 9 * tree.ndec + 2
    zs = rd.z_star(K)

    def check(model):
        out = dict(failures=[], z_cells=[], z_other=[], n_stats=0)
        n_row = nb[model.dealer_of_row].astype(np.float64)
        p = model.p_rec[model.dealer_of_row, np.arange(tree.ndec)]
        rd._cells(out, "RL", obs.reshape(-1), (n_row[:, None, None] * p).reshape(-1), p.reshape(-1), np.repeat(n_row, 9),
                  np.repeat(model.seat, 9), 100.0, zs,
                  lambda i: f"{tree.describe(i // 9)}, holding rank {i // 3 % 3}, action {i % 3}")
        assert 2 < out["n_stats"] <= K                     # the cells outside [100, n - 100] are in the two pools
        return out

    out = check(at.TableModel(tree, rows))
    print(f"played table: z* {zs:.2f}; {rd.summary(out)}")
    assert not out["failures"], out["failures"]
    assert len(out["z_cells"]) >= 200 and 0.7 <= rd.rms(out) <= 1.3
    wrong = check(at.TableModel(tree, at.full_support_table(tree, 18)))
    print(f"another seed's table: {len(wrong['failures'])} failures; {rd.summary(wrong)}")
    assert wrong["failures"]
    eng.close()


# ---- 4: oracle BR, first iteration ---------------------------------------------------------------------
@pytest.mark.parametrize("game,lanes", [(1, (1 << 12) + 100), (0, (1 << 14) + 100)])
def test_oracle_br_first_iteration_is_exact(pkg, game, lanes):
    """eta = 1, epsilon = 0, NFSP_EXT_SL_ONEHOT | NFSP_EXT_RESERVOIR and no reference quirk: after
    ``install_oracle_br()`` and one step M_SL's argmax table is the installed best response at every
    information set with records, and no other action has a count.  epsilon = 0 still draws a
    random action with probability 2^-24 (rollout_dist_ref's rule 6); the table's rows are one-hot,
    so an M_RL record whose components are all < 1 is such a draw: they are counted, reported, and
    at most that many SL records may lie off the table."""
    nat, E, ev = pkg.native, pkg.engine, pkg.evaluation
    tree = tree_of(pkg, game)
    eng = E.SelfPlayEngine(game=game, n_lanes=lanes, seed=21, init_seed=4, eta=1.0, epsilon=0.0,
                           quirks=nat.EXT_SL_ONEHOT | nat.EXT_RESERVOIR, rl_capacity=4 * lanes, sl_capacity=4 * lanes,
                           inserts_per_update=1 << 30)
    beta = eng.install_oracle_br().cpu().numpy()
    assert set(np.unique(beta)) == {0.0, 1.0} and (beta.sum(axis=2) == 1.0).all()
    for a in (0, 1):
        got, _ = eng.act_table(a, E.NET_BR)
        assert np.array_equal(got.cpu().numpy(), beta.astype(np.float32)) and eng.act_table(a, E.NET_AR)[0] is None
    # the installed tables against the exact best response to the opponent they were computed for
    ar = [ev.Policy.table(eng.acting_policy(o, E.NET_AR, None, tree)) for o in (0, 1)]
    res = ev.evaluate_batch(eng.ctx, [(ev.Policy.table(beta), ar[1]), (ar[0], ev.Policy.table(beta))])
    gaps = [res[0]["br0"] - res[0]["value0"], res[1]["br1"] + res[1]["value0"]]
    print(f"game {game}: gap of the installed tables {gaps}")
    assert all(abs(g) <= 2e-16 for g in gaps)
    eng.step()
    n_random = 0
    for p in (0, 1):
        _, a = _records(eng, p, "rl")
        n_random += int((a.max(dim=1).values < 1.0).sum())
    sl, info = eng.memory_table(nat.MEM_SL)
    st = eng.stats()
    for p in (0, 1):
        assert info[p]["matched"] == info[p]["records"] == st["sl_total"][p] > 0
        assert eng.act_table(p, E.NET_BR)[1] == 0
    off = int(sl.counts[beta == 0.0].sum())
    print(f"game {game}: {int(sl.n.sum())} SL records at {int((sl.n > 0).sum())} information sets; "
          f"{n_random} epsilon-random actions, {off} records off the table")
    assert off <= n_random
    if n_random == 0:
        has = sl.n > 0
        assert np.array_equal(sl.policy("argmax")[has], beta[has])
    eng.clear_act_tables()
    assert all(eng.act_table(a, r)[0] is None for a in (0, 1) for r in (0, 1))
    eng.close()


# ---- 5: a group with one replica acting by tables ------------------------------------------------------
def test_group_replica_with_tables(pkg):
    E, ev = pkg.engine, pkg.evaluation
    tree = tree_of(pkg, 0)
    cfg = dict(n_lanes=1000, slices=2, slice_lag=2, rl_capacity=3000, sl_capacity=3000)
    t_br = ev.act_rows(at.lookup_table(tree, 5))
    t_ar = ev.act_rows(at.full_support_table(tree, 6))
    grp = E.EngineGroup(3, seed=40, init_seed=7, **cfg)
    with pytest.raises(pkg.native.NativeError, match="EngineGroup"):
        grp.replicas[1].set_act_table(0, E.NET_BR, t_br)
    rc = grp.L.nfsp_engine_set_act_table(grp.replicas[1].h, 0, E.NET_BR, None)
    assert rc == pkg.native.EINVAL and b"group call" in grp.L.nfsp_last_error()
    grp.set_act_table(1, 0, E.NET_BR, t_br)
    grp.set_act_table(1, 1, E.NET_AR, t_ar)
    solo = [E.SelfPlayEngine(seed=40 + r, init_seed=7 + r, **cfg) for r in range(3)]
    solo[1].set_act_table(0, E.NET_BR, t_br)
    solo[1].set_act_table(1, E.NET_AR, t_ar)
    for _ in range(2):
        grp.step()
        for e in solo:
            e.step()
    for r in range(3):
        assert grp.replicas[r].state_digest() == solo[r].state_digest(), f"replica {r}"
        for x, y in zip(nets(grp.replicas[r]), nets(solo[r])):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert grp.replicas[1].act_table(0, E.NET_BR)[1] == 0 and grp.replicas[0].act_table(0, E.NET_BR)[0] is None
    # the tables changed replica 1's run: it differs from the same engine without them
    plain = E.SelfPlayEngine(seed=41, init_seed=8, **cfg)
    plain.step()
    plain.step()
    assert plain.state_digest() != solo[1].state_digest()
    for e in solo + [plain]:
        e.close()
    grp.close()


def test_setting_is_refused_off_a_step_boundary_and_for_bad_rows(pkg):
    E = pkg.engine
    tree = tree_of(pkg, 1)
    eng = E.SelfPlayEngine(game=1, n_lanes=64, seed=1, inserts_per_update=1 << 30)
    rows = at.lookup_table(tree, 1)
    eng.rollout()
    with pytest.raises(pkg.native.NativeError, match="step boundary"):
        eng.set_act_table(0, E.NET_BR, rows)
    eng.update()
    bad = rows.copy()
    d = int(np.nonzero(tree.seat == 1)[0][2])
    bad[d, 1, 0] = np.inf
    eng.set_act_table(0, E.NET_BR, bad)                    # not seat 0's row: never read
    with pytest.raises(pkg.native.NativeError, match=f"row {d} "):
        eng.set_act_table(1, E.NET_BR, bad)
    assert eng.act_table(1, E.NET_BR)[0] is None
    eng.close()

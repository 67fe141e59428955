"""Frequencies and independence of the rollout path (k_rollout, k_rollout_g, the scans, k_commit)
against the exact game-tree probabilities of tests/rollout_dist_ref.py -- a reference that
shares nothing with the kernel, where the oracle replays of the other rollout tests restate it
(the Philox counter layout, ``below`` / ``u01``, the deal, the dealer rule, the draw indices).

Every engine runs with ``inserts_per_update = 1 << 30``: ``update()`` only consumes the inserts,
the nets stay at ``init_seed`` and epsilon at its start.  Two rollouts per engine (hand index
g = 0 and 1); each one's RL rows are read from the log at [rl_before, rl_before + last_rl), the
observations packed on the device and mapped with ``GameTree.row_of``.

Frequencies: per-cell binomial z of the RL records and of the SL records, exact zeros, the
pools, the action counters, the records per seat and seat 0's reward (``rd.check_counts``;
the bound and its derivation are in rollout_dist_ref's docstring).  Independence: a lane's
fingerprint is its ``lane_counts()`` row packed into one code, and for disjoint pairs of hands
the number of equal codes is binomial under independence (``rd.match_z``).

MEASURED (MI355X; K = 43,523 statistics in this file, z* = 6.69; per case over its rollouts: the
binomial cells tested, their max |z| and rms z, the max |z| of the other statistics; every new
test runs in under 0.1 s after the first, which pays 1 s of device start-up):
    a  leduc 3, eta 0.3, eps .06          308 cells  max |z| 4.05  rms 1.10  others 2.04
    b  leduc 248, eta 0.1, eps (.3, .06) 1468 cells  max |z| 3.28  rms 1.02  others 2.16
    c  leduc 7, defaults (SL cells only)   98 cells  max |z| 3.42  rms 1.09  others 2.47
    d  kuhn 248, eta 0.2, eps .1          192 cells  max |z| 3.31  rms 1.13  others 2.02
    e  eta 0                               42 cells  max |z| 1.98  rms 0.74  others 1.79
    f  eta 1, eps 0                        42 cells  max |z| 1.98  rms 0.87  others 2.21
    e0 eta -1 (1,149 cells exactly 0)      42 cells  max |z| 1.98  rms 0.74  others 1.79
    f0 eta 1, eps -1 (1,161 exactly 0)     42 cells  max |z| 1.98  rms 0.87  others 2.21
    g  eta 1, eps 1                      2064 cells  max |z| 3.87  rms 1.00  others 3.23
       its closed form (1/3 per action)  2 x 1032 cells  max |z| 3.44
    h  3 slices of 87,381, 6 rollouts     768 cells  max |z| 3.63  rms 1.04  others 3.25
    i  2 replicas of 87,381, 2 steps      510 cells  max |z| 3.63  rms 1.14 / 1.01  others 2.71
    wrong models on case a, g = 0: eta + 0.01 max |z| 9.37 (3 statistics out); public card with
    replacement 41.1 (65 out); random actions remapped: 62 and more records in cells of
    probability 0 (6 out); remapped action counters 20.9 (2 out)
    independence, 11 pairings: |z| <= 1.27; with 2 % of one side copied from the other z >= 10.05
    env joint deal (test_gpu_env.py): K = 25, z* = 5.49, max |z| 1.88, X^2 16.8 on 23 dof (bound 60.2)
"""
import time

import numpy as np
import pytest
import torch

import rollout_dist_ref as rd
from engine_ref import weights_flat

pytestmark = pytest.mark.gpu

N = 262_144
N_ODD = 87_381                  # 262,143 / 3: odd, and no multiple of a 64-lane wave
SEED = 1234
CUT = 100.0
# name: game, quirks, cfg, epsilons handed to rollout_with (None: the engine's own)
CASES = {
    "a": ("leduc", 3, dict(eta=0.3, epsilon=0.06), None),
    "b": ("leduc", 248, dict(eta=0.1, epsilon=0.06), (0.3, 0.06)),
    "c": ("leduc", 7, dict(), None),
    "d": ("kuhn", 248, dict(eta=0.2, epsilon=0.1), None),
    "e": ("leduc", 3, dict(eta=0.0, epsilon=0.06), None),
    "f": ("leduc", 3, dict(eta=1.0, epsilon=0.0), None),
    "g": ("leduc", 3, dict(eta=1.0, epsilon=1.0), None),
    # eta = 0 and eps = 0 still act the other way with probability 2^-24 per draw (rule 6), so
    # no cell there has probability exactly 0.  A negative value makes ``u > x`` certain: pure
    # AR argmax play (e0) and pure greedy BR play (f0), where most cells are exactly 0
    # (tests/test_rollout_dist.py::test_negative_eta_and_epsilon_are_accepted keeps the cfg rules open to them)
    "e0": ("leduc", 3, dict(eta=-1.0, epsilon=0.06), None),
    "f0": ("leduc", 3, dict(eta=1.0, epsilon=-1.0), None),
}
INIT_SEED = 11
_TREES = {}
_RUNS = {}


def tree_of(pkg, game):
    if game not in _TREES:
        _TREES[game] = pkg.evaluation.GameTree(pkg.native.GAME_KUHN if game == "kuhn" else pkg.native.GAME_LEDUC)
    return _TREES[game]


def z_file(pkg):
    """z* of this file.  K: the frequency statistics of every rollout compared with the model
    (cases a-g, e0 and f0 twice each, 6 slices of case h, 2 replicas twice of case i), the cells of the
    closed form of case g (twice) and the 11 independence statistics."""
    led, kuhn = rd.stats_per_rollout(tree_of(pkg, "leduc").ndec), rd.stats_per_rollout(tree_of(pkg, "kuhn").ndec)
    return rd.z_star(16 * led + 2 * kuhn + 6 * led + 4 * led + 2 * 9 * tree_of(pkg, "leduc").ndec + 11)


def _cell_counts(tree, p, codes, counts, shape):
    """(bits << 2 | action, count) pairs of seat p -> counts per (row, rank[, action])."""
    out = np.zeros(shape, np.int64)
    for c, k in zip(codes.tolist(), counts.tolist()):
        row, rank = tree.row_of(p, c >> 2)
        if len(shape) == 3:
            out[row, rank, c & 3] += k
        else:
            out[row, rank] += k
    return out


def observe(eng, tree, before):
    """``rd.check_counts``'s observation of the engine's last rollout, and its lanes'
    fingerprints.  ``before``: ``stats()`` just before that rollout."""
    st = eng.stats()
    alias = bool(eng.cfg.quirks & 4)
    rl = None if alias else np.zeros((tree.ndec, 3, 3), np.int64)
    sl = np.zeros((tree.ndec, 3), np.int64)
    w30 = None
    for p in (0, 1):
        m = eng.memories(p)
        dev = m["rl_s"].device
        if w30 is None:
            w30 = torch.ones(30, dtype=torch.int64, device=dev) << torch.arange(30, device=dev)
        n = int(st["last_rl"][p])
        assert st["rl_total"][p] - before["rl_total"][p] == n
        if not alias and n:
            idx = (torch.arange(n, device=dev, dtype=torch.int64) + int(before["rl_total"][p])) % m["log_cap"]
            bits = ((m["rl_s"][idx] != 0).to(torch.int64) * w30).sum(dim=1)
            code = bits * 4 + m["rl_a"][idx].argmax(dim=1)
            u, c = torch.unique(code, return_counts=True)
            rl += _cell_counts(tree, p, u.cpu().numpy(), c.cpu().numpy(), rl.shape)
        k = int(st["last_sl"][p])
        if k:
            px = (m["pend_x"][:k].to(torch.int64) & 0xFFFFFFFF) * 4
            u, c = torch.unique(px, return_counts=True)
            sl += _cell_counts(tree, p, u.cpu().numpy(), c.cpu().numpy(), sl.shape)
    obs = dict(rl=rl, sl=sl, actions=np.array(st["actions"]) - np.array(before["actions"]),
               reward0=st["reward"][0] - before["reward"][0], n_rl=st["last_rl"], n_sl=st["last_sl"])
    assert st["reward"][0] + st["reward"][1] == 0.0
    cnt = eng.lane_counts()
    code = cnt[:, 0] | (cnt[:, 1] << 4) | (cnt[:, 2] << 8) | (cnt[:, 3] << 12)
    return obs, code


def run_engine(pkg, game, quirks, cfg, eps_with, n_lanes=N, slices=1, rollouts=2, seed=SEED):
    """[(obs, codes, lane0, g)] of ``rollouts`` rollouts of a fresh engine, and its nets."""
    g_id = pkg.native.GAME_KUHN if game == "kuhn" else pkg.native.GAME_LEDUC
    eng = pkg.engine.SelfPlayEngine(n_lanes=n_lanes, slices=slices, seed=seed, quirks=quirks, init_seed=INIT_SEED,
                                    game=g_id, inserts_per_update=1 << 30, **cfg)
    tree = tree_of(pkg, game)
    w = weights_flat(eng)
    out = []
    for k in range(rollouts):
        before = eng.stats()
        if eps_with is None:
            eng.rollout()
        else:
            eng.rollout_with(w, eps_with)
        obs, code = observe(eng, tree, before)
        lane0, g = eng.last_slice()
        assert (lane0, g) == ((k % slices) * (n_lanes // slices), k // slices)
        out.append((obs, code, lane0, g))
        eng.update()
    eps = eps_with if eps_with is not None else (eng.cfg.epsilon, eng.cfg.epsilon)
    model = rd.Model(tree, w, eng.cfg.eta, eps, quirks)
    eng.close()
    return dict(rollouts=out, w=w, model=model, eta=eng.cfg.eta, eps=eps, quirks=quirks, tree=tree)


def case_run(pkg, name):
    """One case's engine run, shared by the tests that read it (teeth, independence)."""
    if name not in _RUNS:
        if name == "h":
            _RUNS[name] = run_engine(pkg, "leduc", 3, dict(eta=0.3, epsilon=0.06), None, n_lanes=3 * N_ODD, slices=3,
                                     rollouts=6)
        elif name == "a+1":
            _RUNS[name] = run_engine(pkg, *CASES["a"], rollouts=1, seed=SEED + 1)
        else:
            _RUNS[name] = run_engine(pkg, *CASES[name])
    return _RUNS[name]


def check_run(pkg, name, run, n_lanes):
    zs = z_file(pkg)
    zc, zo, ns = [], [], 0
    for obs, _, lane0, g in run["rollouts"]:
        out = rd.check_counts(run["model"], obs, lane0, n_lanes, g, zs, cut=CUT)
        print(f"case {name} lane0 {lane0} g {g}: z* {zs:.2f}; {rd.summary(out)}")
        assert not out["failures"], out["failures"]
        zc += out["z_cells"]
        zo += out["z_other"]
        ns += out["n_stats"]
    tot = dict(z_cells=zc, z_other=zo, n_stats=ns)
    print(f"case {name} total: {rd.summary(tot)}")
    if len(zc) >= 200:
        assert 0.7 <= rd.rms(tot) <= 1.3


# ---- frequencies -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_rollout_frequencies(pkg, name):
    t0 = time.time()
    run = case_run(pkg, name)
    check_run(pkg, name, run, N)
    if name in ("e0", "f0"):                # deterministic play: most cells are exact zeros
        m, (obs, _, _, _) = run["model"], run["rollouts"][0]
        zero = m.p_rec[m.dealer_of_row, np.arange(run["tree"].ndec)] == 0.0
        print(f"case {name}: {int(zero.sum())} RL cells of probability 0")
        assert zero.sum() >= 900 and obs["rl"][zero].sum() == 0 and obs["rl"].sum() > N
        assert (sum(obs["n_sl"]) == 0) == (name == "e0")
    print(f"case {name}: {time.time() - t0:.2f} s")


def test_uniform_play_closed_form(pkg):
    """Case g without the model: eta 1 and eps (1, 1) play every action with probability 1/3,
    so within an information set the three RL cells are one multinomial with equal cells and
    each holds a third of the row's records."""
    run = case_run(pkg, "g")
    zs = z_file(pkg)
    worst = 0.0
    for obs, _, _, _ in run["rollouts"]:
        rl = obs["rl"].astype(np.float64)
        tot = rl.sum(axis=2, keepdims=True)
        big = np.broadcast_to(tot >= 3 * CUT, rl.shape)
        z = (rl - tot / 3.0)[big] / np.sqrt(np.broadcast_to(tot * (2.0 / 9.0), rl.shape)[big])
        worst = max(worst, float(np.abs(z).max()))
        assert big.sum() >= 200 and np.abs(z).max() <= zs
        assert np.array_equal(obs["sl"], rl.sum(axis=2))      # every decision is a BR-mode decision
    print(f"uniform play: max |z| {worst:.2f}")


def test_sliced_rollout_with_odd_slices(pkg):
    """Case h: 262,143 lanes in 3 slices of 87,381 (odd, a tail wave in every kernel of the
    rollout path; lane0 = 87,381 flips slice 1's dealer parity).  Each slice against its own
    dealer counts."""
    t0 = time.time()
    run = case_run(pkg, "h")
    assert [r[2] for r in run["rollouts"]] == [0, N_ODD, 2 * N_ODD] * 2
    assert [int(c) for c in rd.dealer_lanes(N_ODD, N_ODD, 0)] == [N_ODD // 2, N_ODD // 2 + 1]
    check_run(pkg, "h", run, N_ODD)
    print(f"case h: {time.time() - t0:.2f} s")


def group_run(pkg):
    if "i" not in _RUNS:
        tree = tree_of(pkg, "leduc")
        grp = pkg.engine.EngineGroup(2, n_lanes=N_ODD, seed=SEED, quirks=3, init_seed=INIT_SEED, eta=0.3,
                                     inserts_per_update=1 << 30)
        ws = [weights_flat(e) for e in grp.replicas]
        per = [[], []]
        for g in (0, 1):
            before = [e.stats() for e in grp.replicas]
            grp.step()
            for r, e in enumerate(grp.replicas):
                obs, code = observe(e, tree, before[r])
                per[r].append((obs, code, 0, g))
        _RUNS["i"] = [dict(rollouts=per[r], w=ws[r], tree=tree,
                           model=rd.Model(tree, ws[r], 0.3, (grp.cfg.epsilon, grp.cfg.epsilon), 3)) for r in (0, 1)]
        grp.close()
    return _RUNS["i"]


def test_group_rollout_with_odd_lanes(pkg):
    """Case i: the group kernels (k_rollout_g, k_scan1_g) at 87,381 lanes per replica; each
    replica (seed + r, nets of init_seed + r) on its own."""
    t0 = time.time()
    for r, run in enumerate(group_run(pkg)):
        check_run(pkg, f"i{r}", run, N_ODD)
    print(f"case i: {time.time() - t0:.2f} s")


# ---- teeth: wrong models against case a's device counts ------------------------------------------------
@pytest.mark.parametrize("wrong", ["eta", "public", "remap_random", "remap_counters"])
def test_teeth_on_device_counts(pkg, wrong):
    run = case_run(pkg, "a")
    tree = run["tree"]
    kw = dict(eta=run["eta"], eps=run["eps"])
    extra = {}
    if wrong == "eta":
        kw["eta"] = run["eta"] + 0.01
    elif wrong == "public":                 # a public card drawn with replacement
        extra["p_public"] = np.full((3, 3, 3), 1.0 / 3.0)
    else:
        extra[wrong] = True
    model = rd.Model(tree, run["w"], kw["eta"], kw["eps"], run["quirks"], **extra)
    obs, _, lane0, g = run["rollouts"][0]
    out = rd.check_counts(model, obs, lane0, N, g, z_file(pkg), cut=CUT)
    print(f"wrong model {wrong}: {len(out['failures'])} failures; {rd.summary(out)}; {out['failures'][:2]}")
    assert out["failures"]


# ---- independence ----------------------------------------------------------------------------------------
def _dealer(lane0, n, g):
    return (np.arange(lane0, lane0 + n) + g) & 1


def _pairs_in_rollout(code, dealer, shift, phase):
    """Disjoint pairs (L, L + shift) of one rollout: L from every other block of ``shift``
    lanes (the even blocks, or with ``phase`` 1 the odd ones), so no hand is in two pairs."""
    L = np.arange(len(code) - shift)
    L = L[(L // shift) % 2 == phase]
    return code[L], code[L + shift], dealer[L] * 2 + dealer[L + shift]


def independence_sets(pkg):
    """name -> (codes A, codes B, classes) for every pairing the issue lists."""
    a, a1, h, grp = case_run(pkg, "a"), case_run(pkg, "a+1"), case_run(pkg, "h"), group_run(pkg)
    (_, c0, _, _), (_, c1, _, _) = a["rollouts"]
    d0, d1 = _dealer(0, N, 0), _dealer(0, N, 1)
    sets = {}
    for shift in (1, 2):
        for phase in (0, 1):
            sets[f"L / L+{shift} (phase {phase})"] = _pairs_in_rollout(c0, d0, shift, phase)
    sets["same lane at g and g+1"] = (c0, c1, d0 * 2 + d1)
    sets["lane L at g+1 / lane L+1 at g"] = (c1[:-1], c0[1:], d1[:-1] * 2 + d0[1:])
    sets["lane L+1 at g+1 / lane L at g"] = (c1[1:], c0[:-1], d1[1:] * 2 + d0[:-1])
    hs = h["rollouts"]
    for k in (0, 1):
        sets[f"slices {k} / {k + 1}, same local lane"] = (
            hs[k][1], hs[k + 1][1], _dealer(hs[k][2], N_ODD, 0) * 2 + _dealer(hs[k + 1][2], N_ODD, 0))
    dg = _dealer(0, N_ODD, 0)
    sets["replica 0 / replica 1"] = (grp[0]["rollouts"][0][1], grp[1]["rollouts"][0][1], dg * 2 + dg)
    sets["seeds s / s+1"] = (c0, a1["rollouts"][0][1], d0 * 2 + d0)
    return sets


def test_streams_are_independent(pkg):
    zs = z_file(pkg)
    sets = independence_sets(pkg)
    assert len(sets) == 11                         # z_file counts them
    rng = np.random.RandomState(7)
    for name, (ca, cb, cls) in sets.items():
        z, obs, exp = rd.match_z(ca, cb, cls)
        # teeth: 2 % of B's hands replaced by their partners in A
        cb2 = np.array(cb)
        hit = rng.rand(len(cb2)) < 0.02
        cb2[hit] = np.asarray(ca)[hit]
        z2 = rd.match_z(ca, cb2, cls)[0]
        print(f"{name}: pairs {len(ca)} equal {obs:.0f} expected {exp:.1f} z {z:.2f}; with 2 % copied z {z2:.2f}")
        assert abs(z) <= zs, name
        assert z2 > zs, name

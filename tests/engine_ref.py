"""TEST INFRASTRUCTURE ONLY -- what the GPU parity tests share: the engine's state in the layouts
of the oracles (oracle/learner_oracle.py, oracle/rollout_oracle.py) and the comparisons of a
rollout's records with rollout_oracle's.  Helpers that belong to one study stay in its file.
"""
import numpy as np
import torch

import learner_oracle as LO
import nn_oracle as nn
import rollout_oracle as R

# BASELINE.json's configs[1] and configs[2]
C2 = dict(n_lanes=65_536, rl_capacity=40_000, sl_capacity=40_000, eta=0.1)
C3 = dict(n_lanes=1_048_576, rl_capacity=200_000, sl_capacity=2_000_000)

STAT_KEYS = ("hands", "rl_total", "sl_total", "rl_size", "sl_size", "br_updates", "ar_updates",
             "iteration", "target_syncs", "actions", "reward", "epsilon", "temp", "lr_br",
             "exploitability")


# ---- observations as bit masks ----------------------------------------------------------
def obs_bits(rows):
    """[n, 30] 0/1 rows (host) -> integer bit masks."""
    x = np.asarray(rows)
    x = x.reshape(x.shape[0], int(np.prod(x.shape[1:])))
    assert np.all((x == 0) | (x == 1))
    return (x.astype(np.int64) << np.arange(x.shape[1])).sum(axis=1)


def obs_bits_dev(x):
    """[n, 30] 0/1 float rows (device) -> int64 bit masks (host)."""
    n = x.shape[1]
    w = (torch.ones(n, dtype=torch.int64, device=x.device) << torch.arange(n, device=x.device))
    return ((x != 0).to(torch.int64) * w).sum(dim=1).cpu().numpy()


# ---- nets and memories ------------------------------------------------------------------
def nets(eng):
    return [eng.get_weights(a, n) for a in (0, 1) for n in (0, 1, 2)]


def weights_flat(eng):
    return np.concatenate(nets(eng))


def mem(eng, a):
    m = eng.memories(a)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in m.items() if isinstance(v, torch.Tensor)}


# ---- the learner's input, as learner_oracle takes it --------------------------------------
def oracle_cfg(c):
    """learner_oracle's cfg dict from an engine's cfg (nfsp_engine_cfg)."""
    return dict(c=c.inserts_per_update, batch=c.batch, epochs=c.epochs, rl_capacity=c.rl_capacity,
                sl_capacity=c.sl_capacity, target_every=c.target_every, lr_br=c.lr_br, lr_ar=c.lr_ar,
                gamma=c.gamma, seed=c.seed, epsilon=c.epsilon)


def learner_state(eng):
    """(stats, per-agent state) of the engine after a rollout, in learner_oracle's state layout
    (bits computed on the device)."""
    st = eng.stats()
    out = []
    for a in (0, 1):
        m = eng.memories(a)
        n_sl = int(st["last_sl"][a])
        out.append(dict(
            w={n: eng.get_weights(a, n) for n in (0, 1, 2)},
            rl_total=int(st["rl_total"][a]), last_rl=int(st["last_rl"][a]),
            sl_total=int(st["sl_total"][a]), last_sl=n_sl,
            iteration=int(st["iteration"][a]), br_updates=int(st["br_updates"][a]),
            epsilon=float(st["epsilon"][a]),
            rl_s_bits=obs_bits_dev(m["rl_s"]), rl_s2_bits=obs_bits_dev(m["rl_s2"]),
            rl_a=m["rl_a"].cpu().numpy(), rl_r=m["rl_r"].cpu().numpy(), rl_t=m["rl_t"].cpu().numpy(),
            sl_s_bits=obs_bits_dev(m["sl_s"]), sl_a=m["sl_a"].cpu().numpy(),
            pend_x=m["pend_x"][:n_sl].cpu().numpy().astype(np.int64) & 0xFFFFFFFF,
            pend_a=m["pend_a"][:n_sl].cpu().numpy(), pend_pos=m["pend_pos"][:n_sl].cpu().numpy()))
    return st, out


# ---- AR updates on the oracle, with probes at its two discrete decisions -------------------
def replay_ar(cfg, mbs, u0, u1, w, lr, rel=4e-7, closest=None, relu_closest=None):
    """Oracle AR updates [u0, u1) from weights w; returns (weights, set of updates with an
    ambiguous clip decision: some p within a relative `rel` of a clip bound).  `closest`
    (dict): per update, the smallest relative distance of any p to a clip bound."""
    net = nn.MLP(nn.ACT_SOFTMAX, 64, weights=nn.unpack_weights(w))
    amb = set()
    cur = [None]
    lo, hi = float(nn.CE_EPS), 1.0 - float(nn.CE_EPS)

    def probe(p):
        p = np.asarray(p, np.float64)
        r = np.minimum(np.abs(p - hi) / hi, np.abs(p - lo) / lo)
        if closest is not None:
            closest[cur[0]] = min(closest.get(cur[0], np.inf), float(r.min()))
        if (r <= rel).any():
            amb.add(cur[0])
    net.clip_probe = probe

    def rprobe(z):
        if relu_closest is not None:
            relu_closest[cur[0]] = min(relu_closest.get(cur[0], np.inf), float(np.abs(z).min()))
    net.relu_probe = rprobe
    for u, xb, ya, perms in mbs[u0:u1]:
        if xb is None:
            continue
        cur[0] = u
        net.fit(LO.bits_to_x(xb), ya, np.float32(lr), epochs=cfg["epochs"], perms=perms)
    return net.flat(), amb


# ---- a rollout's records against rollout_oracle -------------------------------------------
def check_rollout(eng, ref, rl_before=(0, 0)):
    """Every record of the last rollout against rollout_oracle.rollout_with_positions' `ref`."""
    for p in (0, 1):
        m = eng.memories(p)
        st = eng.stats()
        n = st["last_rl"][p]
        assert n == len(ref["rl"][p]), (p, n, len(ref["rl"][p]))
        lo = rl_before[p]
        rows = (np.arange(lo, lo + n) % m["log_cap"])
        s = m["rl_s"].cpu().numpy()[rows]
        s2 = m["rl_s2"].cpu().numpy()[rows]
        a = m["rl_a"].cpu().numpy()[rows]
        r = m["rl_r"].cpu().numpy()[rows]
        t = m["rl_t"].cpu().numpy()[rows]
        exp = ref["rl"][p]
        assert np.array_equal(obs_bits(s), np.array([e[0] for e in exp], np.uint64))
        assert np.array_equal(obs_bits(s2), np.array([e[3] for e in exp], np.uint64))
        assert np.abs(a - np.array([e[1] for e in exp])).max() <= 1e-6
        assert np.array_equal(r, np.array([e[2] for e in exp], np.float32))
        assert np.array_equal(t, np.array([e[4] for e in exp], np.uint8))
        k = st["last_sl"][p]
        assert k == len(ref["sl"][p])
        px = m["pend_x"][:k].cpu().numpy().astype(np.uint32)
        pa = m["pend_a"][:k].cpu().numpy()
        pp = m["pend_pos"][:k].cpu().numpy()
        assert np.array_equal(px, np.array([e[0] for e in ref["sl"][p]], np.uint32))
        exp_a = np.array([e[1] for e in ref["sl"][p]], np.float32).reshape(-1, 3)    # k may be 0 (eta = 0)
        assert np.abs(pa - exp_a).max(initial=0.0) <= 1e-6
        assert np.array_equal(pp, np.array([e[2] for e in ref["sl"][p]]))


def sample_lanes(n, k, seed):
    """Lanes at wave / workgroup edges, the last lanes and k random ones."""
    edges = [0, 1, 63, 64, 255, 256, 4095, 4096, n // 2, n - 2, n - 1]
    rng = np.random.RandomState(seed)
    return sorted(set(edges) | set(rng.randint(0, n, size=k).tolist()))


def check_lanes(eng, seed, g, lanes, game="leduc", rl_before=(0, 0)):
    """`lanes` of rollout g replayed one by one (rollout_oracle._one_lane) and found in the
    memories through the exclusive prefix of the per-lane record counts."""
    st = eng.stats()
    cnt = eng.lane_counts()
    assert cnt[:, 0].sum() == st["last_rl"][0] and cnt[:, 1].sum() == st["last_rl"][1]
    assert cnt[:, 2].sum() == st["last_sl"][0] and cnt[:, 3].sum() == st["last_sl"][1]
    pre = np.zeros_like(cnt)
    pre[1:] = np.cumsum(cnt, axis=0)[:-1]
    w = weights_flat(eng)
    alias = bool(eng.cfg.quirks & 4)
    eps = (float(st["epsilon"][0]), float(st["epsilon"][1]))
    mems = [eng.memories(p) for p in (0, 1)]
    for L in lanes:
        ref = R._one_lane(L, g, seed, w, eps, eng.cfg.eta, alias, game)
        for p in (0, 1):
            m = mems[p]
            n = len(ref["rl"][p])
            assert cnt[L, p] == n, (L, p)
            rows = torch.tensor((rl_before[p] + pre[L, p] + np.arange(n)) % m["log_cap"],
                                dtype=torch.int64, device=m["rl_s"].device)
            if n:
                exp = ref["rl"][p]
                assert np.array_equal(obs_bits_dev(m["rl_s"][rows]), [e[0] for e in exp]), (L, p)
                assert np.array_equal(obs_bits_dev(m["rl_s2"][rows]), [e[3] for e in exp]), (L, p)
                a = m["rl_a"][rows].cpu().numpy()
                assert np.abs(a - np.array([e[1] for e in exp])).max() <= 1e-6, (L, p)
                assert np.array_equal(m["rl_r"][rows].cpu().numpy(), np.array([e[2] for e in exp], np.float32))
                assert np.array_equal(m["rl_t"][rows].cpu().numpy(), np.array([e[4] for e in exp], np.uint8))
            k = len(ref["sl"][p])
            assert cnt[L, 2 + p] == k, (L, p)
            if k:
                q = slice(int(pre[L, 2 + p]), int(pre[L, 2 + p]) + k)
                px = m["pend_x"][q].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
                assert np.array_equal(px, [e[0] for e in ref["sl"][p]]), (L, p)
                pa = m["pend_a"][q].cpu().numpy()
                assert np.abs(pa - np.array([e[1] for e in ref["sl"][p]])).max() <= 1e-6
                pos = m["pend_pos"][q].cpu().numpy()
                assert np.array_equal(pos, [rl_before[p] + pre[L, p] + e[2] for e in ref["sl"][p]])
    return cnt

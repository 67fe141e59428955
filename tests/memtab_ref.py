"""The memory tables (include/nfsp.h nfsp_memory_table) restated in numpy.

Shares nothing with csrc/memtab.hip but the ``GameTree`` export: the key of a record is looked up
in ``tree._rows``, the argmax is ``np.argmax`` (first maximum, a NaN counts as the maximum) and
fix(x) = ``np.rint(x.astype(np.float64) * 2**24)`` with the header's saturation rule.
"""
import numpy as np

SL, RL = 0, 1
SAT = 2**32 - 1


def fix(a):
    """(fix(a) as int64, the components that were saturated) of a float32 array."""
    a = np.asarray(a, np.float32)
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(a) < np.float32(256.0))
        v = np.rint(np.where(bad, np.float32(0), a).astype(np.float64) * 2.0**24).astype(np.int64)
        v[bad & (a > 0)] = SAT
        v[bad & (a < 0)] = -SAT
    return v, bad


def sets_of(tree, seat):
    """[(obs, row, rank)] of the seat's information sets, in row order."""
    return sorted(((obs, d, r) for (s, obs), (d, r) in tree._rows.items() if s == seat), key=lambda e: (e[1], e[2]))


def table(tree, seat, kind, obs, a=None, meta=None):
    """(raw int64 [ndec, 3, 3, 3] with the seat's rows filled and the rest 0, info)."""
    obs = np.asarray(obs, np.int64).reshape(-1)
    n = len(obs)
    u, inv = np.unique(obs, return_inverse=True)
    sid_u = np.array([tree._rows.get((seat, int(x)), (-1, 0)) for x in u], np.int64).reshape(-1, 2)
    sid = (np.where(sid_u[:, 0] < 0, -1, sid_u[:, 0] * 3 + sid_u[:, 1]))[inv.reshape(-1)] if n else np.zeros(0, np.int64)
    raw = np.zeros((tree.ndec * 3, 3, 3), np.int64)
    clamped = 0
    if kind == SL:
        a = np.asarray(a, np.float32).reshape(n, 3)
        m = sid >= 0
        k = np.argmax(a, axis=1) if n else np.zeros(0, np.int64)
        f, bad = fix(a)
        np.add.at(raw, (sid[m], k[m], 0), 1)
        for j in range(3):
            np.add.at(raw, (sid[m], j, 1), f[m, j])
        clamped = int(bad[m].sum())
    else:
        meta = np.asarray(meta, np.int64).reshape(-1) & 0xFFFFFFFF
        k = meta & 0xFF
        m = (sid >= 0) & (k <= 2)
        r = ((meta >> 16) & 0xFF).astype(np.uint8).view(np.int8).astype(np.int64)
        t = (meta >> 8) & 1
        np.add.at(raw, (sid[m], k[m], 0), 1)
        np.add.at(raw, (sid[m], k[m], 1), r[m])
        np.add.at(raw, (sid[m], k[m], 2), t[m])
    info = dict(records=n, matched=int(m.sum()), unmatched=int(n - m.sum()), clamped=clamped)
    return raw.reshape(tree.ndec, 3, 3, 3), info


def pack_sl(obs, a):
    """SlRec rows as uint32 [n, 4]: {obs bits, a[3]}."""
    out = np.zeros((len(obs), 4), np.uint32)
    out[:, 0] = np.asarray(obs, np.uint32)
    out[:, 1:] = np.asarray(a, np.float32).reshape(-1, 3).view(np.uint32)
    return out


def pack_rl(s, s2, meta, a):
    """RlRec rows as uint32 [n, 8]: {s, s2, argmax | t << 8 | r << 16, a[3], pad[2]}."""
    out = np.zeros((len(s), 8), np.uint32)
    out[:, 0] = np.asarray(s, np.uint32)
    out[:, 1] = np.asarray(s2, np.uint32)
    out[:, 2] = np.asarray(meta, np.uint32)
    out[:, 3:6] = np.asarray(a, np.float32).reshape(-1, 3).view(np.uint32)
    return out


def action_rows(n, rng):
    """[n, 3] float32 action vectors: one-hot rows, 24-bit uniform draws, non-negative floats up
    to about 13 and all-zero rows, a quarter each."""
    a = np.zeros((n, 3), np.float32)
    kind = rng.randint(4, size=n)
    hot = kind == 0
    a[hot, rng.randint(3, size=int(hot.sum()))] = 1.0
    uni = kind == 1
    a[uni] = (rng.randint(1 << 24, size=(int(uni.sum()), 3)) / float(1 << 24)).astype(np.float32)
    pos = kind == 2
    a[pos] = (rng.rand(int(pos.sum()), 3) * 13.0).astype(np.float32)
    return a


def rl_meta(n, rng, a):
    """Stored M_RL meta words for the action rows a: argmax | t << 8 | (r in half units) << 16."""
    k = np.argmax(a, axis=1).astype(np.int64) if n else np.zeros(0, np.int64)
    t = rng.randint(2, size=n).astype(np.int64)
    r = rng.randint(-26, 27, size=n).astype(np.int64)
    return (k | (t << 8) | ((r & 0xFF) << 16)).astype(np.uint32)


def bits_of(x30):
    """Observation words of fp32 0/1 rows [n, 30]."""
    return ((np.asarray(x30) != 0).astype(np.int64) << np.arange(30, dtype=np.int64)).sum(axis=1)


# shared by the GPU tests of the tables (test_gpu_memtab.py, test_gpu_qreport.py, test_gpu_checkpoint.py)
_CTX = {}
_TREES = {}


def game_id(pkg, game):
    return pkg.native.GAME_KUHN if game == "kuhn" else pkg.native.GAME_LEDUC


def ctx_of(pkg, game):
    """(a context, the game's tree), one of each per game and session."""
    if game not in _CTX:
        _CTX[game] = pkg.native.Context(1, game=game_id(pkg, game))
        _TREES[game] = pkg.evaluation.GameTree(game_id(pkg, game))
    return _CTX[game], _TREES[game]


def dev(words):
    """Packed records (uint32 rows) on the device."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda()


def export_rl(m, rl_total, live):
    """The live M_RL records of ``memories(agent)``'s fp32 export m, oldest first: record k of the
    agent's rl_total lies at row k % log_cap.  (s words, s2 words, a [live, 3], stored meta words)."""
    import torch
    idx = torch.as_tensor((int(rl_total) - live + np.arange(live)) % m["log_cap"], device=m["rl_s"].device)
    a = m["rl_a"][idx].cpu().numpy()
    r2 = np.rint(m["rl_r"][idx].cpu().numpy().astype(np.float64) * 2).astype(np.int64)
    meta = np.argmax(a, axis=1).astype(np.int64) | (m["rl_t"][idx].cpu().numpy().astype(np.int64) << 8) | ((r2 & 0xFF) << 16)
    return bits_of(m["rl_s"][idx].cpu().numpy()), bits_of(m["rl_s2"][idx].cpu().numpy()), a, meta

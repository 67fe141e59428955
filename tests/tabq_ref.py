"""Tabular NFSP's tables (include/nfsp.h nfsp_tdq_table, nfsp_table_rows, nfsp_engine_tabular_q)
restated in numpy, on tests/memtab_ref.py's and tests/tdtab_ref.py's helpers.

Shares nothing with csrc/memtab.hip's fourth kind and csrc/tabq.hip but the ``GameTree`` export:
the information set of s and of s2 is looked up in ``tree._rows``, the bootstrap is the row of Q
there (zeros where s2 is no information set of the seat, so that fmax gives the declared 0), the
TD value and the sums are ``tdtab_ref.table``'s, and the rows are float64 divisions of the int64
sums with one rounding to float32.
"""
import numpy as np

import tdtab_ref as tr

TDQ = 3
ROWS_SL_MASS, ROWS_SL_ARGMAX, ROWS_TD_MEAN = 0, 1, 2


def q_at(tree, seat, q, s2):
    """float32 [n, 3]: Q's row at the information set in which ``seat`` observes each word of s2,
    zeros where there is none."""
    q = np.asarray(q, np.float32).reshape(tree.ndec * 3, 3)
    s2 = np.asarray(s2, np.int64).reshape(-1)
    at = np.array([tree._rows.get((seat, int(x)), (-1, 0)) for x in s2], np.int64).reshape(-1, 2)
    found = at[:, 0] >= 0
    out = np.zeros((len(s2), 3), np.float32)
    out[found] = q[at[found, 0] * 3 + at[found, 1]]
    return out


def tdq(tree, seat, s, s2, meta, q, gamma, quirks):
    """One seat's sums of one sweep: (raw int64 [ndec, 3, 3, 3], info)."""
    return tr.table(tree, seat, s, meta, q_at(tree, seat, q, s2), gamma, quirks & tr.TERMINAL_BOOTSTRAP)


def rows(stat, raw, fill=None):
    """float32 [..., ndec, 3, 3] of int64 tables [..., ndec, 3, 3, 3]."""
    raw = np.asarray(raw, np.int64)
    fill = np.zeros(raw.shape[:-1], np.float32) if fill is None else np.asarray(fill, np.float32).reshape(raw.shape[:-1])
    c, S = raw[..., 0], raw[..., 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        if stat == ROWS_TD_MEAN:
            ok = c > 0
            v = (S.astype(np.float64) / np.where(ok, c, 1).astype(np.float64)) * 2.0**-24
        else:
            n = c.sum(axis=-1)
            M = (S[..., 0] + S[..., 1]) + S[..., 2]
            ok = ((n > 0) & (M > 0) & (S >= 0).all(axis=-1))[..., None] & np.ones(3, bool)
            num, den = (S, M) if stat == ROWS_SL_MASS else (c, n)
            v = num.astype(np.float64) / np.where(ok[..., 0], den, 1).astype(np.float64)[..., None]
    return np.where(ok, v.astype(np.float32), fill)


def changed(prev, new):
    """Entries whose float32 bits differ."""
    return int((np.asarray(prev, np.float32).view(np.uint32) != np.asarray(new, np.float32).view(np.uint32)).sum())


def sweeps(tree, recs, gamma, quirks, K, fill=None):
    """K Jacobi sweeps from Q_0 = fill.  recs[seat] = (s, s2, meta); gamma, quirks: one value or one
    per seat.  (Q float32 [ndec, 3, 3], the last sweep's raw table, its infos by seat, the entries
    the last sweep changed)."""
    g = gamma if isinstance(gamma, (list, tuple)) else (gamma, gamma)
    qk = quirks if isinstance(quirks, (list, tuple)) else (quirks, quirks)
    q = np.zeros((tree.ndec, 3, 3), np.float32) if fill is None else np.array(fill, np.float32).reshape(tree.ndec, 3, 3)
    raw, infos, ch = None, None, None
    for _ in range(K):
        raw, infos = np.zeros((tree.ndec, 3, 3, 3), np.int64), []
        for seat in (0, 1):
            s, s2, meta = recs[seat]
            one, info = tdq(tree, seat, s, s2, meta, q, g[seat], qk[seat])
            raw += one
            infos.append(info)
        new = rows(ROWS_TD_MEAN, raw, fill)
        ch = changed(q, new)
        q = new
    return q, raw, infos, ch

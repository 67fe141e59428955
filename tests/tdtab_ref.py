"""The TD table (include/nfsp.h nfsp_td_table) restated in numpy, on tests/memtab_ref.py's helpers.

Shares nothing with csrc/memtab.hip's third kind but the ``GameTree`` export.  Q_target(s2) is not
restated here: it comes from the library's dense forward ``nfsp_mlp_forward`` (csrc/mlp.hip
k_mlp_forward, pinned bit-exact against oracle/nn_oracle.py), where the kernel under test gathers
rows in LDS (``fwd_lds``).  From it v = float32(float64(r) + gamma * float64(qmax)) with the product
and the sum each rounded, fix in float64 (``memtab_ref.fix``) and integer sums.
"""
import numpy as np

import memtab_ref as mr

TD = 2
TERMINAL_BOOTSTRAP, EXT_LINEAR_Q = 1, 32
ACT_RELU, ACT_SOFTMAX, ACT_LINEAR = 0, 1, 2


def obs_rows(words):
    """fp32 0/1 rows [n, 30] of observation words."""
    w = np.asarray(words, np.int64).reshape(-1, 1)
    return ((w >> np.arange(30, dtype=np.int64)) & 1).astype(np.float32)


def forward(ctx, w, act, words):
    """``nfsp_mlp_forward`` of the packed net ``w`` on observation words: float32 [n, 3]."""
    import torch
    x = torch.from_numpy(obs_rows(words)).cuda()
    wd = torch.as_tensor(np.asarray(w, np.float32)).cuda()
    y = torch.zeros((x.shape[0], 3), dtype=torch.float32, device="cuda")
    if x.shape[0]:
        ctx.call("nfsp_mlp_forward", wd.data_ptr(), 64, int(act), x.data_ptr(), y.data_ptr(), x.shape[0])
        torch.cuda.synchronize()
    return y.cpu().numpy()


def head_act(quirks):
    return ACT_LINEAR if quirks & EXT_LINEAR_Q else ACT_RELU


def table(tree, seat, s, meta, qt, gamma, quirks):
    """(raw int64 [ndec, 3, 3, 3] with the seat's rows filled and the rest 0, info) of records with
    stored observations ``s``, meta words ``meta`` and target head outputs ``qt[n, 3]`` at their s2."""
    s = np.asarray(s, np.int64).reshape(-1)
    n = len(s)
    meta = np.asarray(meta, np.int64).reshape(-1) & 0xFFFFFFFF
    qt = np.asarray(qt, np.float32).reshape(n, 3)
    at = np.array([tree._rows.get((seat, int(x)), (-1, 0)) for x in s], np.int64).reshape(-1, 2)
    sid = np.where(at[:, 0] < 0, -1, at[:, 0] * 3 + at[:, 1])
    k = meta & 0xFF
    m = (sid >= 0) & (k <= 2)
    r = ((meta >> 16) & 0xFF).astype(np.uint8).view(np.int8).astype(np.float32) * np.float32(0.5)
    terminal = (((meta >> 8) & 1) == 1) & (not quirks & TERMINAL_BOOTSTRAP)
    with np.errstate(invalid="ignore", over="ignore"):
        qmax = np.fmax(np.fmax(qt[:, 0], qt[:, 1]), qt[:, 2])           # fmaxf: a NaN loses
        prod = np.float64(gamma) * qmax.astype(np.float64)
        v = np.where(terminal, r.astype(np.float64), r.astype(np.float64) + prod).astype(np.float32)
    fv, bad_v = mr.fix(v)
    fq, bad_q = mr.fix(qmax)
    boot = m & ~terminal
    raw = np.zeros((tree.ndec * 3, 3, 3), np.int64)
    np.add.at(raw, (sid[m], k[m], 0), 1)
    np.add.at(raw, (sid[m], k[m], 1), fv[m])
    np.add.at(raw, (sid[boot], k[boot], 2), fq[boot])
    info = dict(records=n, matched=int(m.sum()), unmatched=int(n - m.sum()),
                clamped=int(bad_v[m].sum() + bad_q[boot].sum()))
    return raw.reshape(tree.ndec, 3, 3, 3), info

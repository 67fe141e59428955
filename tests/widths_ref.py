"""TEST INFRASTRUCTURE ONLY -- the restatements of the fit (tests/fitnet_ref.py) and of the regret
nets (tests/mccfr_net_ref.py) at a hidden width H other than their 64.

A packed net of width H is W1[30][H] | b1[H] | W2[H][3] | b2[3]: NP = 34 H + 3 floats at the offsets
0, 30 H, 31 H, 34 H.  Nothing else of either restatement depends on the width, so ``fit_ref(H)`` is a
private copy of the fitnet_ref module (the same source, executed again) with those six constants set,
and ``net_ref(H)`` a private copy of mccfr_net_ref whose ``fr`` is that copy.  The two files
themselves stay as they are, and ``fit_ref(64)`` computes what fitnet_ref computes.

``heads_f32`` restates nfsp_head_tables_h (csrc/head_tables.hip k_head_tables_h) in the kernel's own
order with one float32 add or multiply per term.
"""
import functools
import importlib.util

import numpy as np

import fitnet_ref
import mccfr_net_ref

WIDTHS = (16, 32, 64, 128)


def offsets(hidden):
    return 0, 30 * hidden, 31 * hidden, 34 * hidden


def _copy(mod, name):
    spec = importlib.util.spec_from_file_location(name, mod.__file__)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@functools.lru_cache(maxsize=None)
def fit_ref(hidden):
    assert hidden in WIDTHS
    m = _copy(fitnet_ref, f"fitnet_ref_h{hidden}")
    m.H, m.NP = hidden, 34 * hidden + 3
    m.OW1, m.OB1, m.OW2, m.OB2 = offsets(hidden)
    return m


@functools.lru_cache(maxsize=None)
def net_ref(hidden):
    m = _copy(mccfr_net_ref, f"mccfr_net_ref_h{hidden}")
    m.fr = fit_ref(hidden)
    return m


def heads_f32(w, obs, act):
    """The heads [n, 3] of the packed float32 net ``w`` at the observations ``obs`` (uint32 words):
    per hidden unit the set bits' W1 entries ascending from +0, plus b1, ReLU; the units ascending
    into the three sums, plus b2; then ReLU (act 0), softmax (1) or nothing (2).  Every add and
    multiply is one float32 operation, vectorised over the observations only."""
    f = np.float32
    w = np.asarray(w, f)
    hidden = (len(w) - 3) // 34
    assert len(w) == 34 * hidden + 3
    o1, ob1, ow2, ob2 = offsets(hidden)
    obs = np.asarray(obs, np.uint32).reshape(-1)
    o = np.zeros((len(obs), 3), f)
    for j in range(hidden):
        a = np.zeros(len(obs), f)
        for i in range(30):
            on = ((obs >> np.uint32(i)) & np.uint32(1)).astype(bool)
            a = np.where(on, a + w[o1 + i * hidden + j], a)      # a bit that is not set adds nothing
        h = a + w[ob1 + j]
        h = np.where(h > 0, h, f(0))
        for k in range(3):
            o[:, k] = o[:, k] + h * w[ow2 + 3 * j + k]
    for k in range(3):
        o[:, k] = o[:, k] + w[ob2 + k]
    if act == 0:
        return np.where(o > 0, o, f(0))
    if act == 2:
        return o
    m = np.maximum(np.maximum(o[:, 0], o[:, 1]), o[:, 2])
    e = np.exp(o - m[:, None]).astype(f)
    s = (e[:, 0] + e[:, 1]) + e[:, 2]
    return e / s[:, None]

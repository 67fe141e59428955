"""TEST INFRASTRUCTURE ONLY -- numpy restatement of ``nfsp_fit_tables`` (csrc/fit_tables.hip
k_fit_tables; include/nfsp.h states the operations) over ``evaluation.GameTree``'s exported
arrays, parametrised by dtype: float32 is what the GPU tests compare with, float64 what the finite
differences and the choice of inits use.

The data are the kernel's in either dtype: a row's target is rounded to float32 once and its weight
is ``float32(w / W)`` with W the seat's sum in double in row order.  The sums over inputs, hidden
units and rows are matrix products here, so their order is numpy's, not the kernel's: equal to
rounding, not bit for bit.
"""
import numpy as np

H, NP = 64, 30 * 64 + 64 + 64 * 3 + 3
OW1, OB1, OW2, OB2 = 0, 30 * H, 30 * H + H, 30 * H + H + 3 * H
ACT_RELU, ACT_SOFTMAX, ACT_LINEAR = 0, 1, 2
CE, MSE, HUBER = 0, 1, 2
PAIRS = ((ACT_SOFTMAX, CE), (ACT_RELU, MSE), (ACT_RELU, HUBER), (ACT_LINEAR, MSE), (ACT_LINEAR, HUBER))


def glorot(seed):
    """A packed net: Glorot-uniform kernels, zero biases (Keras' Dense default)."""
    rng = np.random.RandomState(seed)
    w = np.zeros(NP, np.float32)
    l1, l2 = np.sqrt(6.0 / (30 + H)), np.sqrt(6.0 / (H + 3))
    w[OW1:OB1] = rng.uniform(-l1, l1, 30 * H)
    w[OW2:OB2] = rng.uniform(-l2, l2, 3 * H)
    return w


def seat_sets(tree, seat):
    """The job's rows: (d, r) with the seat acting at d, ascending, as two index arrays."""
    d = np.nonzero(tree.seat == seat)[0]
    return np.repeat(d, 3), np.tile(np.arange(3), len(d))


def problem(tree, seat, target, weight=None, mask=None, dtype=np.float32):
    """(X [N, 30], T [N, 3], what [N], M [N, 3]) of a job, in ``dtype``."""
    d, r = seat_sets(tree, seat)
    X = ((tree.obs[d, r][:, None] >> np.arange(30, dtype=np.uint32)) & 1).astype(dtype)
    T = np.asarray(target, np.float64).reshape(tree.ndec, 3, 3)[d, r].astype(np.float32).astype(dtype)
    w = np.ones(len(d)) if weight is None else np.asarray(weight, np.float64).reshape(tree.ndec, 3)[d, r]
    W = 0.0
    for x in w:
        W += float(x)
    what = (w / W).astype(np.float32).astype(dtype)
    if mask is None:
        M = np.ones((len(d), 3), dtype)
        M[:, 2] = tree.legal[d]
    else:
        M = (np.asarray(mask).reshape(tree.ndec, 3, 3)[d, r] != 0).astype(dtype)
    return X, T, what, M


def forward(w, X):
    W1, b1 = w[OW1:OB1].reshape(30, H), w[OB1:OW2]
    W2, b2 = w[OW2:OB2].reshape(H, 3), w[OB2:]
    z1 = X @ W1 + b1
    h = np.where(z1 > 0, z1, 0).astype(w.dtype)
    return z1, h, h @ W2 + b2


def rows(z, T, what, M, head, loss):
    """(dz [N, 3], row losses [N]) from the head sums."""
    dt = z.dtype.type
    if loss == CE:
        c = z - np.maximum(np.maximum(z[:, 0], z[:, 1]), z[:, 2])[:, None]
        e = np.exp(c)
        s = (e[:, 0] + e[:, 1]) + e[:, 2]
        Tt = (T[:, 0] + T[:, 1]) + T[:, 2]
        dz = what[:, None] * ((e / s[:, None]) * Tt[:, None] - T)
        lp = c - np.log(s)[:, None]
        tl = T * lp
        return dz, what * -((tl[:, 0] + tl[:, 1]) + tl[:, 2])
    on = np.ones(z.shape, bool) if head == ACT_LINEAR else z > 0
    e = np.where(on, z, dt(0)) - T
    a = np.abs(e)
    clip = (a > 1) if loss == HUBER else np.zeros(z.shape, bool)
    g = np.where(clip, np.sign(e), e).astype(z.dtype)
    dz = np.where(on, (what[:, None] * M) * g, dt(0)).astype(z.dtype)
    lk = M * np.where(clip, a - dt(0.5), (dt(0.5) * e) * e)
    return dz, what * ((lk[:, 0] + lk[:, 1]) + lk[:, 2])


def loss_of(w, prob, head, loss):
    """The weighted loss: the row terms in w's dtype, summed in double."""
    X, T, what, M = prob
    _, _, z = forward(w, X)
    return float(np.sum(rows(z, T, what, M, head, loss)[1].astype(np.float64)))


def grad(w, prob, head, loss):
    X, T, what, M = prob
    z1, h, z = forward(w, X)
    dz, _ = rows(z, T, what, M, head, loss)
    W2 = w[OW2:OB2].reshape(H, 3)
    dh = (dz[:, 0:1] * W2[:, 0] + dz[:, 1:2] * W2[:, 1]) + dz[:, 2:3] * W2[:, 2]
    dz1 = np.where(z1 > 0, dh, 0).astype(w.dtype)
    return np.concatenate([(X.T @ dz1).ravel(), dz1.sum(axis=0), (h.T @ dz).ravel(), dz.sum(axis=0)]).astype(w.dtype)


def fit(w0, prob, head, loss, lr, momentum, steps, v0=None):
    """``steps`` of v <- mu v + g, w <- w - lr v in the dtype of ``prob``.
    Returns (w, v, (loss before step 1, loss at the end))."""
    dtype = prob[0].dtype
    w = np.array(w0, dtype)
    v = np.zeros(NP, dtype) if v0 is None else np.array(v0, dtype)
    lr, mu = dtype.type(lr), dtype.type(momentum)
    l0 = loss_of(w, prob, head, loss)
    for _ in range(int(steps)):
        v = mu * v + grad(w, prob, head, loss)
        w = w - lr * v
    return w, v, (l0, loss_of(w, prob, head, loss))


def entropy(prob):
    """The targets' own weighted entropy: the floor of the CE loss."""
    _, T, what, _ = prob
    T = T.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.sum(what.astype(np.float64) * -np.where(T > 0, T * np.log(T), 0.0).sum(axis=1)))


def visit_ref(tree, table):
    """[ndec, 3]: the probability that a hand reaches each information set when both seats play
    ``table`` -- ``evaluation.visit_weights`` without a GPU, up to one constant factor."""
    t = tree.remap(table)
    N = tree.nodes
    pub = np.array([[[(2.0 - (a == r) - (b == r)) / 4.0 for b in range(3)] for a in range(3)] for r in range(3)])
    reach = np.zeros((tree.nn, 3, 3))                     # [node][seat 0's rank][seat 1's rank]
    out = np.zeros((tree.ndec, 3))
    for n in range(tree.nn):                              # depth order: parents first
        par = int(N["parent"][n])
        if par < 0:
            reach[n] = tree.deal
        elif N["kind"][par] == 1:
            reach[n] = reach[par] * pub[int(N["via"][n])]
        else:
            a = t[int(N["row"][par]), :, int(N["via"][n])]
            reach[n] = reach[par] * (a[:, None] if N["p"][par] == 0 else a[None, :])
        if N["kind"][n] == 0:
            out[int(N["row"][n])] = reach[n].sum(axis=1 if N["p"][n] == 0 else 0)
    return out

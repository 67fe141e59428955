"""GPU parity of the network kernels against oracle/nn_oracle.py.

Tolerances (north_star: "network outputs match within a stated fp32 tolerance"):
* predict, ReLU head: BIT-EXACT (same fixed summation order, no FMA contraction);
* predict, softmax head: |delta| <= 1e-6 (device expf vs numpy exp, ~1 ulp);
* fit (8 SGD steps): weights |delta| <= 1e-5 (parallel gradient sums);
* BR targets: |delta| <= 1e-6, exploitability proxy |delta| <= 1e-6.
The same bars hold at the kernels' shape edges (test_fit_shapes: measured <= 1.2e-7 over 1 to
37 SGD steps; test_br_targets_shapes; test_predict_block_edges).
"""
import numpy as np
import pytest
import torch

import nfsp_oracle as orc
import nn_oracle as nn

pytestmark = pytest.mark.gpu


def dev(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda", dtype=dtype)


def make(pkg, act, seed):
    ctx = pkg.native.Context(1)
    m = pkg.agent.DeviceMLP(act, 64, np.random.RandomState(seed), ctx)
    o = nn.MLP(act, 64, weights=m.get_weights())
    return m, o


@pytest.mark.parametrize("B", [1, 7, 128, 5000])
def test_predict_relu_bit_exact(pkg, B):
    m, o = make(pkg, nn.ACT_RELU, B)
    rng = np.random.RandomState(B)
    x = (rng.rand(B, 1, 30) < 0.3).astype(np.float32)
    assert np.array_equal(m.predict(x), o.predict(x))


def test_predict_relu_nonbinary_inputs_bit_exact(pkg):
    m, o = make(pkg, nn.ACT_RELU, 5)
    x = np.random.RandomState(0).randn(300, 1, 30).astype(np.float32)
    assert np.array_equal(m.predict(x), o.predict(x))


@pytest.mark.parametrize("B", [1, 128, 4096])
def test_predict_softmax(pkg, B):
    m, o = make(pkg, nn.ACT_SOFTMAX, 10 + B)
    x = (np.random.RandomState(B).rand(B, 1, 30) < 0.3).astype(np.float32)
    y, yo = m.predict(x), o.predict(x)
    assert np.abs(y - yo).max() <= 1e-6
    assert np.allclose(y.sum(-1), 1.0, atol=1e-6)


@pytest.mark.parametrize("act", [nn.ACT_RELU, nn.ACT_SOFTMAX])
def test_fit_matches_keras_restatement(pkg, act):
    m, o = make(pkg, act, 21 + act)
    rng = np.random.RandomState(4)
    x = (rng.rand(128, 30) < 0.3).astype(np.float32)
    if act == nn.ACT_RELU:
        t = (rng.rand(128, 3) * 3).astype(np.float32)      # regression targets
    else:
        t = rng.rand(128, 3).astype(np.float32)            # unnormalised SL targets
    np.random.seed(5)
    perms = m.fit_device(dev(x), dev(t), 0.1)
    o.fit(x, t, np.float32(0.1), perms=perms)
    for a, b in zip(m.get_weights(), o.get_weights()):
        assert np.abs(a - b).max() <= 1e-5


def test_fit_ce_clip_edge(pkg):
    """A saturated softmax (p < 1e-7) exercises the clip mask of the CE gradient."""
    m, o = make(pkg, nn.ACT_SOFTMAX, 3)
    ws = m.get_weights()
    ws[3] = np.array([40.0, 0.0, -40.0], np.float32)
    m.set_weights(ws)
    o.set_weights(ws)
    x = np.zeros((32, 30), np.float32)
    t = np.ones((32, 3), np.float32)
    perms = m.fit_device(dev(x), dev(t), 0.1, epochs=1)
    o.fit(x, t, np.float32(0.1), perms=perms, epochs=1)
    for a, b in zip(m.get_weights(), o.get_weights()):
        assert np.abs(a - b).max() <= 1e-5


@pytest.mark.parametrize("quirks", [3, 0])
def test_br_targets(pkg, quirks):
    nat = pkg.native
    m, o = make(pkg, nn.ACT_RELU, 77)
    rng = np.random.RandomState(8)
    n = 128
    s = (rng.rand(n, 30) < 0.3).astype(np.float32)
    s2 = (rng.rand(n, 30) < 0.3).astype(np.float32)
    a = rng.rand(n, 3).astype(np.float32)
    r = (rng.randint(-10, 11, size=n) * 0.5).astype(np.float32)
    t = (rng.rand(n) < 0.3).astype(np.uint8)
    out = torch.empty((n, 3), device="cuda")
    ex = torch.zeros(1, dtype=torch.float64, device="cuda")
    ds, da, dr, ds2, dt = dev(s), dev(a), dev(r), dev(s2), dev(t)
    m.ctx.call("nfsp_br_targets", nat.ptr(m.w), 64, nat.ptr(ds), nat.ptr(da), nat.ptr(dr),
               nat.ptr(ds2), nat.ptr(dt), n, nat.F64(0.95), quirks, nat.ptr(out), nat.ptr(ex))
    ag = orc.Agent.__new__(orc.Agent)
    ag.target_br_model, ag.gamma, ag.quirks = o, 0.95, quirks == 3
    tb = t.astype(bool)          # np.bool_ entries: `t is True` never holds (quirk)
    tgt, expl = ag.br_targets(s.reshape(n, 1, 30), a.reshape(n, 1, 3), r.astype(np.float64),
                              s2.reshape(n, 1, 30), tb)
    assert np.abs(out.cpu().numpy() - tgt.reshape(n, 3)).max() <= 1e-6
    assert abs(ex.item() - expl) <= 1e-6


# ---------------------------------------------------------------------------
# Shape edges of the three kernels: what a user reaches by editing MiniBatchSize (the ragged
# last minibatch of k_mlp_fit, bs = 1 and bs = MAXB), k_br_targets' stride loop past one
# block of rows up to MAXT, exact ties in argmax3, and k_mlp_forward's block boundary.
# ---------------------------------------------------------------------------
FIT_SHAPES = [(100, 32, 2), (5, 32, 2), (37, 1, 1), (130, 64, 3), (64, 64, 1), (1, 1, 4)]


def _fit_data(act, n):
    rng = np.random.RandomState(4)
    x = (rng.rand(n, 30) < 0.3).astype(np.float32)
    if act == nn.ACT_RELU:
        t = (rng.rand(n, 3) * 3).astype(np.float32)
    else:
        t = rng.rand(n, 3).astype(np.float32)
    return x, t


@pytest.mark.parametrize("act", [nn.ACT_RELU, nn.ACT_SOFTMAX])
@pytest.mark.parametrize("n,bs,epochs", FIT_SHAPES)
def test_fit_shapes(pkg, act, n, bs, epochs):
    """Ragged last minibatch (m = n % bs rows: the 1/(3m) and 1/m factors), bs = 1, bs = MAXB
    and n < bs.  Bar: the file's 1e-5 on every weight.  A ragged case also shows that its
    partial step ran: the oracle replayed WITHOUT that step is more than 1e-3 away."""
    m, o = make(pkg, act, 21 + act)
    w0 = o.get_weights()
    x, t = _fit_data(act, n)
    np.random.seed(5)
    perms = m.fit_device(dev(x), dev(t), 0.1, epochs=epochs, batch_size=bs)
    assert perms.shape == (epochs, n)
    o.fit(x, t, np.float32(0.1), perms=perms, batch_size=bs, epochs=epochs)
    got = m.get_weights()
    worst = max(float(np.abs(a - b).max()) for a, b in zip(got, o.get_weights()))
    print(f"fit act={act} n={n} bs={bs} epochs={epochs}: max|device - oracle| = {worst:.2e}")
    assert worst <= 1e-5
    if n % bs:
        d = nn.MLP(act, 64, weights=w0)
        for ep in range(epochs):
            for b0 in range(0, n - n % bs, bs):
                sel = perms[ep][b0:b0 + bs]
                d.sgd_step(x[sel], t[sel], np.float32(0.1))
        gap = max(float(np.abs(a - b).max()) for a, b in zip(d.get_weights(), o.get_weights()))
        print(f"  oracle without the ragged step: {gap:.2e} from the full one")
        assert gap > 1e-3
        assert max(float(np.abs(a - b).max()) for a, b in zip(got, d.get_weights())) > 1e-3


def _fit_rc(pkg, m, x, t, n, perm, epochs, bs):
    nat = pkg.native
    return m.ctx.L.nfsp_mlp_fit(m.ctx.h, nat.ptr(m.w), 64, m.act, nat.ptr(x), nat.ptr(t), n, nat.ptr(perm),
                                epochs, bs, nat.F32(0.1))


@pytest.mark.parametrize("act", [nn.ACT_RELU, nn.ACT_SOFTMAX])
def test_fit_empty_and_rejected_sizes(pkg, act):
    """epochs = 0 and n = 0 are no-ops that return OK; bs outside [1, MAXB = 64] is refused."""
    nat = pkg.native
    m, _ = make(pkg, act, 21 + act)
    x, t = _fit_data(act, 8)
    dx, dt = dev(x), dev(t)
    perm = dev(np.arange(8, dtype=np.int32))
    before = m.w.cpu().numpy().copy()
    assert _fit_rc(pkg, m, dx, dt, 8, perm, 0, 32) == nat.OK
    assert _fit_rc(pkg, m, dx, dt, 0, perm, 2, 32) == nat.OK
    assert _fit_rc(pkg, m, dx, dt, 8, perm, 1, 65) == nat.EINVAL
    assert _fit_rc(pkg, m, dx, dt, 8, perm, 1, 0) == nat.EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(m.w.cpu().numpy().view(np.uint32), before.view(np.uint32))


# action rows whose argmax is decided by a tie (np.argmax and argmax3 take the first maximum),
# one-hot rows, and ordinary ones
_TIES = np.array([[0.0, 0.0, 0.0], [0.7, 0.7, 0.1], [0.1, 0.7, 0.7], [0.5, 0.2, 0.5], [0.4, 0.4, 0.4],
                  [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], np.float32)
_ALL_ACTION_1 = np.array([[0.0, 1.0, 0.0], [0.1, 0.7, 0.7], [0.2, 0.9, 0.3]], np.float32)


@pytest.mark.parametrize("quirks", [3, 0])
@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("n", [1, 129, 257, 1024])
def test_br_targets_shapes(pkg, n, gamma, quirks):
    """k_br_targets past one block of rows (its blockDim stride loop), at n = MAXT, at the ends
    of gamma, and with exact ties in the stored action rows.  Bar: the file's 1e-6."""
    nat = pkg.native
    m, o = make(pkg, nn.ACT_RELU, 77)
    rng = np.random.RandomState(8 + n)
    s = (rng.rand(n, 30) < 0.3).astype(np.float32)
    s2 = (rng.rand(n, 30) < 0.3).astype(np.float32)
    a = rng.rand(n, 3).astype(np.float32)
    last_wins = n == 1024 and quirks == 3
    if last_wins:            # every row names action 1: row n - 1 must win target[0][1]
        a = _ALL_ACTION_1[np.arange(n) % len(_ALL_ACTION_1)]
    else:                    # two rows in three are a tie or a one-hot row
        k = np.arange(n)
        a = np.where((k % 3 != 2)[:, None], _TIES[(k // 3 * 2 + k % 3) % len(_TIES)], a)
    r = (rng.randint(-9, 10, size=n) * 0.5).astype(np.float32)
    r[-1] = 6.5              # the last row's value is unlike every other one
    t = (rng.rand(n) < 0.3).astype(np.uint8)
    out = torch.full((n, 3), -777.0, device="cuda")
    ex = torch.zeros(1, dtype=torch.float64, device="cuda")
    ds, da, dr, ds2, dt = dev(s), dev(a), dev(r), dev(s2), dev(t)
    m.ctx.call("nfsp_br_targets", nat.ptr(m.w), 64, nat.ptr(ds), nat.ptr(da), nat.ptr(dr),
               nat.ptr(ds2), nat.ptr(dt), n, nat.F64(gamma), quirks, nat.ptr(out), nat.ptr(ex))
    ag = orc.Agent.__new__(orc.Agent)
    ag.target_br_model, ag.gamma, ag.quirks = o, gamma, quirks == 3
    tgt, expl = ag.br_targets(s.reshape(n, 1, 30), a.reshape(n, 1, 3), r.astype(np.float64),
                              s2.reshape(n, 1, 30), t.astype(bool))
    got = out.cpu().numpy()
    assert np.abs(got - tgt.reshape(n, 3)).max() <= 1e-6
    assert abs(ex.item() - expl) <= 1e-6
    # the same targets from first principles, so that a tie rule shared by kernel and oracle
    # code would still be seen: first maximum wins; gamma = 0 leaves the reward alone
    first = np.array([0 if (v[0] >= v[1] and v[0] >= v[2]) else (1 if v[1] >= v[2] else 2) for v in a])
    qn = o.predict(s2).max(axis=1).astype(np.float64)
    terminal = t.astype(bool) & (quirks == 0)
    vals = np.where(terminal, r.astype(np.float64), r.astype(np.float64) + gamma * qn)
    if gamma == 0.0:
        assert np.array_equal(vals, r.astype(np.float64))
    if quirks == 0:
        assert np.abs(got[np.arange(n), first] - vals).max() <= 1e-6
    else:
        for c in range(3):
            rows = np.nonzero(first == c)[0]
            if len(rows):
                assert abs(got[0, c] - vals[rows[-1]]) <= 1e-6, (c, rows[-1])
    if last_wins:
        assert (first == 1).all() and np.abs(vals[:-1] - vals[-1]).min() > 1e-3
        assert abs(got[0, 1] - vals[-1]) <= 1e-6


def test_br_targets_rejects_more_rows_than_its_lds_holds(pkg):
    nat = pkg.native
    m, _ = make(pkg, nn.ACT_RELU, 77)
    n = 1025
    z = torch.zeros((n, 30), device="cuda")
    a = torch.zeros((n, 3), device="cuda")
    r = torch.zeros(n, device="cuda")
    t = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out = torch.zeros((n, 3), device="cuda")
    ex = torch.zeros(1, dtype=torch.float64, device="cuda")
    rc = m.ctx.L.nfsp_br_targets(m.ctx.h, nat.ptr(m.w), 64, nat.ptr(z), nat.ptr(a), nat.ptr(r), nat.ptr(z),
                                 nat.ptr(t), n, nat.F64(0.95), 3, nat.ptr(out), nat.ptr(ex))
    assert rc == nat.EINVAL


@pytest.mark.parametrize("B", [255, 256, 257])
def test_predict_block_edges(pkg, B):
    """One row short of a 256-row block, exactly one block, one row into the next."""
    x = (np.random.RandomState(B).rand(B, 1, 30) < 0.3).astype(np.float32)
    m, o = make(pkg, nn.ACT_RELU, B)
    assert np.array_equal(m.predict(x), o.predict(x))
    m, o = make(pkg, nn.ACT_SOFTMAX, 10 + B)
    y, yo = m.predict(x), o.predict(x)
    assert np.abs(y - yo).max() <= 1e-6
    assert np.allclose(y.sum(-1), 1.0, atol=1e-6)

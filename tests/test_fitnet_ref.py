"""tests/fitnet_ref.py, the restatement the GPU tests of nfsp_fit_tables compare with, checked
three ways without a GPU: its gradient against central differences of its own loss in float64,
one step on two rows against numbers worked by hand, and the library's host-side validation
(nfsp_fit_jobs_check), which needs no device.

The two rows by hand (softmax head, cross-entropy).  The net is zero but for b1[0] = 1 and
W2[0] = (ln 2, 0, 0): every row has h_0 = 1, every other hidden unit z1 = 0 (off), so
z = (ln 2, 0, 0) and p = (1/2, 1/4, 1/4) at both rows.

    row A  inputs {0, 3}, t = (1, 0, 0),     w = 3  ->  what = 3/4
    row B  inputs {3},    t = (0, 1/2, 1/2), w = 1  ->  what = 1/4

    dz_A = 3/4 (p - t) = (-3/8, 3/16, 3/16),  dz_B = 1/4 (p - t) = (1/8, -1/16, -1/16)
    db2 = dW2[0] = dz_A + dz_B = (-1/4, 1/8, 1/8)
    dz1_0 = dz_0 ln 2:  -3/8 ln 2 at A,  1/8 ln 2 at B;  db1_0 = -1/4 ln 2
    dW1[0][0] = -3/8 ln 2 (A only),  dW1[3][0] = -1/4 ln 2 (both);  every other entry 0
    loss = 3/4 ln 2 + 1/4 (1/2 ln 4 + 1/2 ln 4) = 5/4 ln 2
"""
import ctypes as C

import numpy as np
import pytest

import fitnet_ref as fr

LN2 = np.log(2.0)


@pytest.fixture(scope="module")
def kuhn(pkg):
    import __graft_entry__
    __graft_entry__.build()
    return pkg.evaluation.GameTree.of(1)


@pytest.mark.parametrize("head,loss", fr.PAIRS)
@pytest.mark.parametrize("seat", [0, 1])
def test_gradient_is_the_finite_difference_of_the_loss(kuhn, seat, head, loss):
    rng = np.random.RandomState(10 * seat + 3 * head + loss)
    if loss == fr.CE:
        target, mask = kuhn.remap(rng.dirichlet(np.ones(3), size=(kuhn.ndec, 3))), None
    else:
        target = rng.normal(0.0, 1.5, size=(kuhn.ndec, 3, 3))      # some |e| past Huber's delta
        mask = rng.rand(kuhn.ndec, 3, 3) < 0.7
    weight = rng.rand(kuhn.ndec, 3)
    weight[rng.rand(kuhn.ndec, 3) < 0.25] = 0.0
    prob = fr.problem(kuhn, seat, target, weight, mask, np.float64)
    assert (prob[2] == 0).any() and prob[2].sum() == pytest.approx(1.0, abs=1e-6)
    assert mask is None or (prob[3] == 0).any()
    w = fr.glorot(seat + 7).astype(np.float64)
    w[fr.OB1:fr.OW2] = rng.normal(0, 0.1, fr.H)
    # a ReLU head with a negative sum passes no gradient: keep two outputs on, one mostly off
    w[fr.OB2:] = rng.normal(0, 0.3, 3) if head == fr.ACT_SOFTMAX else (0.8, 0.4, -0.1)
    g = fr.grad(w, prob, head, loss)
    fd = np.zeros_like(g)
    eps = 1e-6
    for k in range(fr.NP):
        wp, wm = w.copy(), w.copy()
        wp[k] += eps
        wm[k] -= eps
        fd[k] = (fr.loss_of(wp, prob, head, loss) - fr.loss_of(wm, prob, head, loss)) / (2 * eps)
    assert np.abs(g).max() > 1e-3
    assert np.abs(g - fd).max() < 1e-8


def test_two_rows_by_hand():
    X = np.zeros((2, 30))
    X[0, [0, 3]] = 1.0
    X[1, 3] = 1.0
    T = np.array([[1.0, 0.0, 0.0], [0.0, 0.5, 0.5]])
    what = np.array([0.75, 0.25])
    prob = (X, T, what, np.ones((2, 3)))
    w = np.zeros(fr.NP)
    w[fr.OB1] = 1.0
    w[fr.OW2] = LN2
    g = fr.grad(w, prob, fr.ACT_SOFTMAX, fr.CE)
    want = np.zeros(fr.NP)
    want[fr.OW1 + 0 * fr.H + 0] = -0.375 * LN2
    want[fr.OW1 + 3 * fr.H + 0] = -0.25 * LN2
    want[fr.OB1] = -0.25 * LN2
    want[fr.OW2:fr.OW2 + 3] = (-0.25, 0.125, 0.125)
    want[fr.OB2:] = (-0.25, 0.125, 0.125)
    assert np.allclose(g, want, rtol=0, atol=1e-15)
    assert fr.loss_of(w, prob, fr.ACT_SOFTMAX, fr.CE) == pytest.approx(1.25 * LN2, abs=1e-15)
    # one step with momentum 1/2 from v = (1, 1, ...): v <- v / 2 + g, w <- w - 2 v
    w1, v1, (l0, l1) = fr.fit(w, prob, fr.ACT_SOFTMAX, fr.CE, 2.0, 0.5, 1, v0=np.ones(fr.NP))
    assert np.allclose(v1, 0.5 + want, rtol=0, atol=1e-15)
    assert np.allclose(w1, w - 2.0 * (0.5 + want), rtol=0, atol=1e-15)
    assert l0 == pytest.approx(1.25 * LN2, abs=1e-15)


def test_float32_data_are_the_kernels(kuhn):
    """The weight is float32(w / W), the target float32(t), in either dtype."""
    rng = np.random.RandomState(5)
    target, weight = rng.normal(size=(kuhn.ndec, 3, 3)), rng.rand(kuhn.ndec, 3)
    a = fr.problem(kuhn, 1, target, weight, None, np.float32)
    b = fr.problem(kuhn, 1, target, weight, None, np.float64)
    assert a[0].shape == (12, 30) and a[0].dtype == np.float32 and b[0].dtype == np.float64
    for x, y in zip(a, b):
        assert np.array_equal(x.astype(np.float64), y)
    d, r = fr.seat_sets(kuhn, 1)
    assert (kuhn.seat[d] == 1).all() and np.array_equal(np.lexsort((r, d)), np.arange(12))
    assert np.array_equal(a[3][:, 2], kuhn.legal[d].astype(np.float32)) and (a[3][:, :2] == 1).all()


def _jobs(pkg, **kw):
    base = dict(dev_w=64, dev_v=None, dev_target=128, dev_weight=None, dev_mask=None, seat=0,
                head=pkg.native.ACT_SOFTMAX, loss=pkg.native.FIT_CE, lr=0.1, momentum=0.9)
    base.update(kw)
    return base


def test_jobs_check_refuses_with_a_message(pkg):
    """Host only: the pointers are never followed."""
    import __graft_entry__
    __graft_entry__.build()
    nat = pkg.native
    L = nat.load()

    def check(jobs, n=None, steps=8):
        arr = (nat.FitJob * max(len(jobs), 1))(*[nat.FitJob(**j) for j in jobs])
        rc = L.nfsp_fit_jobs_check(arr, len(jobs) if n is None else n, steps)
        return rc, L.nfsp_last_error().decode()

    ok = [_jobs(pkg), _jobs(pkg, seat=1, head=nat.ACT_RELU, loss=nat.FIT_HUBER, dev_mask=256, momentum=0.0),
          _jobs(pkg, head=nat.ACT_LINEAR, loss=nat.FIT_MSE, lr=0.0, dev_v=512, dev_weight=1024)]
    assert check(ok)[0] == nat.OK
    assert check([], 0, 0)[0] == nat.OK
    assert C.sizeof(nat.FitJob) == 64
    bad = [(dict(), -1, 8, "n must be"), (dict(), None, -1, "steps must be"),
           (dict(seat=2), None, 8, "seat"), (dict(seat=-1), None, 8, "seat"),
           (dict(head=nat.ACT_RELU), None, 8, "pair"), (dict(loss=nat.FIT_MSE), None, 8, "pair"),
           (dict(head=nat.ACT_LINEAR, loss=nat.FIT_CE), None, 8, "pair"),
           (dict(head=3), None, 8, "head"), (dict(loss=3), None, 8, "loss"),
           (dict(dev_mask=256), None, 8, "mask"),
           (dict(lr=-0.1), None, 8, "lr"), (dict(lr=float("nan")), None, 8, "lr"), (dict(lr=float("inf")), None, 8, "lr"),
           (dict(momentum=1.0), None, 8, "momentum"), (dict(momentum=-0.1), None, 8, "momentum"),
           (dict(momentum=float("nan")), None, 8, "momentum"),
           (dict(dev_w=None), None, 8, "null"), (dict(dev_target=None), None, 8, "null")]
    for kw, n, steps, word in bad:
        rc, msg = check([ok[1], _jobs(pkg, **kw)], n, steps)
        assert rc == nat.EINVAL and word in msg, (kw, n, steps, msg)
        if kw:
            assert "job 1" in msg, msg                      # the job is named
    arr = (nat.FitJob * 1)(nat.FitJob(**ok[0]))
    assert L.nfsp_fit_jobs_check(None, 1, 8) == nat.EINVAL
    assert L.nfsp_fit_tables(None, 0, arr, 1, 8, None) == nat.EINVAL

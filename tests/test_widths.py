"""Hidden widths 16, 32, 64 and 128 of the nets fitted off the engine, without a GPU: the host-only
entry points (nfsp_net_params, nfsp_fit_width_check), evaluation.net_width / heads_table on
hand-made heads, and the width-general restatement (tests/widths_ref.py) against central
differences.

The finite-difference bar is tests/test_fitnet_ref.py's: float64, eps 1e-6, so the truncation is of
order eps^2 and the rounding of order 1e-16 / eps = 1e-10 of the loss; 1e-8 per parameter.
"""
import ctypes as C

import numpy as np
import pytest

import widths_ref as wr

LDS_LEDUC = {16: 29472, 32: 46368, 64: 80160, 128: 147744}


@pytest.fixture(scope="module")
def L(pkg):
    import __graft_entry__
    __graft_entry__.build()
    return pkg.native.load()


@pytest.fixture(scope="module")
def kuhn(pkg, L):
    return pkg.evaluation.GameTree.of(1)


def test_net_params_at_the_four_widths_and_its_refusals(pkg, L):
    nat = pkg.native
    for h in wr.WIDTHS:
        np_ = nat.I64(-1)
        assert L.nfsp_net_params(h, C.byref(np_)) == nat.OK
        assert np_.value == 34 * h + 3 == nat.net_params(h) == wr.fit_ref(h).NP
    assert nat.net_params(64) == nat.NP
    for h in (0, 8, 48, 256, -1):
        np_ = nat.I64(-1)
        assert L.nfsp_net_params(h, C.byref(np_)) == nat.EINVAL and np_.value == -1
        msg = L.nfsp_last_error().decode()
        assert "16, 32, 64 and 128" in msg and str(h) in msg, msg
        with pytest.raises(ValueError, match="widths built"):
            nat.net_params(h)
    assert L.nfsp_net_params(64, None) == nat.EINVAL


def test_width_check_gives_the_carves_bytes_and_refuses_what_does_not_fit(pkg, L):
    nat = pkg.native
    for h, want in LDS_LEDUC.items():
        lds = nat.I64(-1)
        assert L.nfsp_fit_width_check(nat.GAME_LEDUC, h, C.byref(lds)) == nat.OK
        assert lds.value == want
        npp = (34 * h + 3 + 3) & ~3
        assert want == 4 * (2 * npp + 196 * (15 + h + 1))             # the carve's formula, nm = 196
        assert L.nfsp_fit_width_check(nat.GAME_LEDUC, h, None) == nat.OK
    # Kuhn: 4 rows a seat, nm = 12
    lds = nat.I64(-1)
    assert L.nfsp_fit_width_check(nat.GAME_KUHN, 64, C.byref(lds)) == nat.OK and lds.value == 21280
    assert L.nfsp_fit_width_check(nat.GAME_KUHN, 128, C.byref(lds)) == nat.OK
    assert lds.value == 4 * (2 * 4356 + 12 * (15 + 129))
    # 256 does not fit on Leduc: the message names the bytes and the bound
    lds = nat.I64(-1)
    assert L.nfsp_fit_width_check(nat.GAME_LEDUC, 256, C.byref(lds)) == nat.EINVAL and lds.value == -1
    msg = L.nfsp_last_error().decode()
    assert "282912" in msg and "153600" in msg, msg
    # it would fit on Kuhn, but is not built
    assert L.nfsp_fit_width_check(nat.GAME_KUHN, 256, C.byref(lds)) == nat.EINVAL and lds.value == -1
    assert "16, 32, 64 and 128" in L.nfsp_last_error().decode()
    for h in (0, 8, 48, -1):
        assert L.nfsp_fit_width_check(nat.GAME_LEDUC, h, C.byref(lds)) == nat.EINVAL and lds.value == -1
    assert L.nfsp_fit_width_check(7, 64, C.byref(lds)) == nat.EINVAL


def test_net_width_reads_the_length_and_refuses_others(pkg):
    ev = pkg.evaluation
    for h in wr.WIDTHS:
        w = ev.glorot_net(np.random.RandomState(h), h)
        assert w.shape == (34 * h + 3,) and ev.net_width(w) == h
        assert ev.net_width(w.reshape(1, -1)) == h
    assert ev.net_width(12345) == 64                                  # a device address carries no length
    for n in (0, 2178, 2180, 34 * 48 + 3, 34 * 256 + 3):
        with pytest.raises(ValueError, match="34 H \\+ 3"):
            ev.net_width(np.zeros(n, np.float32))
    with pytest.raises(ValueError, match="one width per call"):
        ev._one_width([np.zeros(547, np.float32), np.zeros(2179, np.float32)], "x")
    assert ev._one_width([np.zeros(547, np.float32)] * 2, "x") == 16


def test_heads_table_follows_the_policy_kinds(pkg):
    """A tie, an all-zero head and an illegal raise, by hand."""
    nat, ev = pkg.native, pkg.evaluation
    legal = np.array([True, False])
    soft = np.array([[[0.2, 0.3, 0.5], [0.25, 0.5, 0.25], [1.0, 0.0, 0.0]],
                     [[0.2, 0.3, 0.5], [0.0, 0.0, 1.0], [0.5, 0.25, 0.25]]], np.float32)
    t = ev.heads_table(soft, legal, nat.POL_AR_SOFTMAX)
    assert t.dtype == np.float64
    assert np.array_equal(t[0], soft[0].astype(np.float64))           # softmax rows pass through
    assert np.array_equal(t[1], [[np.float32(0.2), np.float64(np.float32(0.3)) + np.float64(np.float32(0.5)), 0.0],
                                 [0.0, 1.0, 0.0], [0.5, 0.5, 0.0]])    # an illegal raise's mass goes to call
    t = ev.heads_table(soft, legal, nat.POL_AR_ARGMAX)
    assert np.array_equal(t[0], [[0, 0, 1], [0, 1, 0], [1, 0, 0]])
    assert np.array_equal(t[1], [[0, 1, 0], [0, 1, 0], [1, 0, 0]])     # raise -> call where it is illegal
    q = np.array([[[0.0, 0.0, 0.0], [0.0, 1.5, 1.5], [2.0, 2.0, 2.0]],
                  [[0.0, 0.0, 0.0], [-1.0, -3.0, -0.5], [0.0, 0.5, 0.5]]], np.float32)
    for kind in (nat.POL_BR_GREEDY, nat.POL_BR_GREEDY_LINEAR):
        t = ev.heads_table(q, legal, kind)
        assert np.array_equal(t[0], [[1, 0, 0], [0, 1, 0], [1, 0, 0]])   # all zero folds; the first maximum wins
        assert np.array_equal(t[1], [[1, 0, 0], [0, 1, 0], [0, 1, 0]])   # the raise that won becomes call
        assert (t.sum(axis=2) == 1).all()
    with pytest.raises(ValueError, match="net kinds"):
        ev.heads_table(q, legal, nat.POL_TABLE)
    with pytest.raises(ValueError, match="legal flag"):
        ev.heads_table(q, legal[:1], nat.POL_BR_GREEDY)


def test_the_restatement_at_64_is_the_restatement(kuhn):
    import fitnet_ref as fr
    f64 = wr.fit_ref(64)
    assert f64 is not fr and (f64.H, f64.NP, f64.OW1, f64.OB1, f64.OW2, f64.OB2) == (fr.H, fr.NP, fr.OW1, fr.OB1,
                                                                                     fr.OW2, fr.OB2)
    rng = np.random.RandomState(3)
    prob = fr.problem(kuhn, 0, rng.normal(size=(kuhn.ndec, 3, 3)))
    a = fr.fit(fr.glorot(4), prob, fr.ACT_LINEAR, fr.MSE, 0.1, 0.9, 5)
    b = f64.fit(f64.glorot(4), prob, fr.ACT_LINEAR, fr.MSE, 0.1, 0.9, 5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert (fr.H, fr.NP) == (64, 2179)                                # and the original is untouched
    assert wr.net_ref(16).fr is wr.fit_ref(16) and wr.net_ref(16).fr.NP == 547


@pytest.mark.parametrize("pair", range(5), ids=["softmax-ce", "relu-mse", "relu-huber", "linear-mse", "linear-huber"])
@pytest.mark.parametrize("seat", [0, 1])
@pytest.mark.parametrize("hidden", [16, 128])
def test_gradient_is_the_finite_difference_of_the_loss_at_other_widths(kuhn, hidden, seat, pair):
    fr = wr.fit_ref(hidden)
    head, loss = fr.PAIRS[pair]
    rng = np.random.RandomState(1000 * hidden + 10 * seat + 3 * head + loss)
    if loss == fr.CE:
        target, mask = kuhn.remap(rng.dirichlet(np.ones(3), size=(kuhn.ndec, 3))), None
    else:
        target = rng.normal(0.0, 1.5, size=(kuhn.ndec, 3, 3))
        mask = rng.rand(kuhn.ndec, 3, 3) < 0.7
    weight = rng.rand(kuhn.ndec, 3)
    weight[rng.rand(kuhn.ndec, 3) < 0.25] = 0.0
    prob = fr.problem(kuhn, seat, target, weight, mask, np.float64)
    w = fr.glorot(seat + 7).astype(np.float64)
    assert w.shape == (34 * hidden + 3,)
    w[fr.OB1:fr.OW2] = rng.normal(0, 0.1, hidden)
    w[fr.OB2:] = rng.normal(0, 0.3, 3) if head == fr.ACT_SOFTMAX else (0.8, 0.4, -0.1)
    g = fr.grad(w, prob, head, loss)
    assert g.shape == w.shape
    fd = np.zeros_like(g)
    eps = 1e-6
    for k in range(fr.NP):
        wp, wm = w.copy(), w.copy()
        wp[k] += eps
        wm[k] -= eps
        fd[k] = (fr.loss_of(wp, prob, head, loss) - fr.loss_of(wm, prob, head, loss)) / (2 * eps)
    print(f"hidden {hidden} seat {seat} head {head} loss {loss}: |g - fd| {np.abs(g - fd).max():.3g}")
    assert np.abs(g).max() > 1e-3
    # every block of the layout carries gradient: an offset that is off would leave one empty
    for lo, hi in ((fr.OW1, fr.OB1), (fr.OB1, fr.OW2), (fr.OW2, fr.OB2), (fr.OB2, fr.NP)):
        assert np.abs(g[lo:hi]).max() > 0
    assert np.abs(g - fd).max() < 1e-8


def test_heads_f32_is_the_forward_of_the_restatement(kuhn):
    """The per-term float32 restatement of the head read-out against the matrix-product forward."""
    for hidden in (16, 128):
        fr = wr.fit_ref(hidden)
        w = fr.glorot(hidden)
        w[fr.OB1:] += np.random.RandomState(1).normal(0, 0.1, fr.NP - fr.OB1).astype(np.float32)
        obs = kuhn.obs.reshape(-1)
        X = ((obs[:, None] >> np.arange(30, dtype=np.uint32)) & 1).astype(np.float64)
        z = fr.forward(w.astype(np.float64), X)[2]
        assert np.abs(wr.heads_f32(w, obs, 2) - z).max() < 1e-5
        assert np.abs(wr.heads_f32(w, obs, 0) - np.maximum(z, 0)).max() < 1e-5
        e = np.exp(z - z.max(axis=1, keepdims=True))
        assert np.abs(wr.heads_f32(w, obs, 1) - e / e.sum(axis=1, keepdims=True)).max() < 1e-6


def test_warm_start_refuses_another_width(pkg):
    with pytest.raises(ValueError, match="engine is 64 wide"):
        pkg.diagnostics.warm_start([], None, hidden=128)

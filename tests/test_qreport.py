"""``evaluation.q_report_from`` on hand-made arrays over the Kuhn tree: every key's value is
written out by hand.  No GPU."""
import math

import numpy as np
import pytest

F = float(1 << 24)


@pytest.fixture(scope="module")
def tree(pkg):
    t = pkg.evaluation.GameTree(pkg.native.GAME_KUHN)
    # seat 0 acts in rows 0 and 4 (three legal actions) and 5 and 6 (a raise becomes a call)
    assert t.ndec == 8 and t.seat.tolist() == [0, 1, 1, 1, 0, 0, 0, 1]
    assert t.legal.tolist() == [True, True, True, False, True, False, False, False]
    return t


def blank(tree):
    z = np.zeros((tree.ndec, 3, 3))
    beta = z.copy()
    beta[..., 0] = 1.0                                   # unreached sets fold
    return beta, z.copy(), np.zeros((tree.ndec, 3)), z.copy(), np.zeros((tree.ndec, 3, 3, 3), np.int64)


def test_exact_head_and_empty_table(pkg, tree):
    ev = pkg.evaluation
    rng = np.random.RandomState(2)
    beta, q, reach, head, td = blank(tree)
    reach[:] = rng.uniform(0.1, 1.0, reach.shape)
    qx = rng.uniform(-2.0, 2.0, q.shape)
    qx[~tree.legal, :, 2] = -np.inf                      # never the best action
    best = np.argmax(qx, axis=2)
    beta = np.eye(3)[best]
    qx[~tree.legal, :, 2] = 0.0
    q = qx * reach[:, :, None]
    head = q / reach[:, :, None]                         # the division q_report_from makes
    head[~tree.legal, :, 2] = -100.0                     # an illegal raise's output is not compared
    for seat in (0, 1):
        r = ev.q_report_from(tree, seat, beta, q, reach, head, td, linear=True)
        assert r["q_rmse_exact"] == 0.0 and r["greedy_mismatch_share"] == 0.0
        assert r["td_pairs"] == 0 and r["td_empty_actions"] == 30
        assert math.isnan(r["td_rmse_exact"]) and math.isnan(r["fit_rmse_td"]) and math.isnan(r["mean_bootstrap_share"])
        assert r["linear"] is True and "info" not in r
        assert r["neg_value_actions"] == int(((qx < 0) & (tree.seat == seat)[:, None, None]).sum())
    # the illegal raise as the head's maximum is executed as a call
    head[5, :, 2] = 100.0
    beta[5] = [0.0, 1.0, 0.0]
    head[5, :, 1] = head[5, :, 0] - 1.0
    r = ev.q_report_from(tree, 0, beta, q, reach, head, td, linear=False)
    w5 = reach[5].sum() / reach[tree.seat == 0].sum()
    assert abs(r["greedy_mismatch_share"] - 0.0) < 1e-15 and r["q_rmse_exact"] > 0 and r["linear"] is False
    head[5, :, 2] = -100.0                               # now the fold is the first maximum
    r = ev.q_report_from(tree, 0, beta, q, reach, head, td, linear=False)
    assert abs(r["greedy_mismatch_share"] - w5) < 1e-15


def test_by_hand(pkg, tree):
    ev, nat = pkg.evaluation, pkg.native
    beta, q, reach, head, td = blank(tree)
    # A = (row 5, rank 1): reach 0.25, fold -1, call -0.5: the best action is a call worth <= 0, and
    # a head of zeros folds there
    reach[5, 1] = 0.25
    q[5, 1] = [-0.25, -0.125, 0.0]
    beta[5, 1] = [0.0, 1.0, 0.0]
    # B = (row 0, rank 2): reach 0.75, fold -1, call 1, raise 2, and the head holds exactly that
    reach[0, 2] = 0.75
    q[0, 2] = [-0.75, 0.75, 1.5]
    beta[0, 2] = [0.0, 0.0, 1.0]
    head[0, 2] = [-1.0, 1.0, 2.0]
    # C = (row 4, rank 0) is not reached; the head says 1 for its fold
    head[4, 0] = [1.0, 0.0, 0.0]
    # the other seat's rows must not count
    reach[1] = 0.5
    q[1] = -3.0
    head[1] = 7.0
    td[1, :, :, 0] = 9
    # TD: A-call 4 records of mean -0.25, two of them bootstrapping 0.5 each; B-raise 2 records of
    # mean 1.5; C-fold 1 record of 3; records stored at A's illegal raise, in no figure
    td[5, 1, 1] = [4, int(4 * -0.25 * F), int(2 * 0.5 * F)]
    td[0, 2, 2] = [2, int(2 * 1.5 * F), 0]
    td[4, 0, 0] = [1, int(3.0 * F), 0]
    td[5, 1, 2] = [5, int(5 * 50.0 * F), 0]
    info = {"records": 12, "matched": 12, "unmatched": 0, "clamped": 0}
    r = ev.q_report_from(tree, 0, beta, q, reach, head, ev.MemoryTable(tree, nat.MEM_TD, td), linear=False, gamma=0.5,
                         info=info)
    assert set(r) == {"q_rmse_exact", "greedy_mismatch_share", "neg_value_actions", "relu_blind_share", "td_pairs",
                      "td_empty_actions", "td_rmse_exact", "fit_rmse_td", "mean_bootstrap_share", "linear", "info"}
    # A: (0 + 1)^2 + (0 + 0.5)^2 = 1.25 over 2 legal actions; B: 0 over 3
    assert abs(r["q_rmse_exact"] - math.sqrt(0.25 * 1.25 / (0.25 * 2 + 0.75 * 3))) < 1e-15
    assert r["greedy_mismatch_share"] == 0.25 and r["relu_blind_share"] == 0.25
    assert r["neg_value_actions"] == 3                   # A's fold and call, B's fold
    assert r["td_pairs"] == 3 and r["td_empty_actions"] == 27
    # A-call -0.25 against -0.5 (4 records), B-raise 1.5 against 2 (2 records); C is not reached
    assert abs(r["td_rmse_exact"] - math.sqrt((4 * 0.25**2 + 2 * 0.5**2) / 6)) < 1e-15
    # the head: A-call 0 against -0.25 (4), B-raise 2 against 1.5 (2), C-fold 1 against 3 (1)
    assert abs(r["fit_rmse_td"] - math.sqrt((4 * 0.25**2 + 2 * 0.5**2 + 1 * 2.0**2) / 7)) < 1e-15
    # gamma x (2 x 0.5) over |-1| + |3| + |3| of the seat's legal pairs
    assert abs(r["mean_bootstrap_share"] - 0.5 * 1.0 / 7.0) < 1e-15
    assert r["linear"] is False and r["info"] == info
    # the same head, exact on A as well: nothing is left but the blind share
    head[5, 1] = [-1.0, -0.5, 0.0]
    r = ev.q_report_from(tree, 0, beta, q, reach, head, td, linear=True, gamma=0.5)
    assert r["q_rmse_exact"] == 0.0 and r["greedy_mismatch_share"] == 0.0 and r["relu_blind_share"] == 0.25
    # seat 1 sees only its own rows
    r1 = ev.q_report_from(tree, 1, beta, q, reach, head, td, linear=True)
    assert r1["td_pairs"] == 9 and r1["neg_value_actions"] == 9 and r1["relu_blind_share"] == 0.0


def test_memory_table_td_fields(pkg, tree):
    ev, nat = pkg.evaluation, pkg.native
    td = np.zeros((tree.ndec, 3, 3, 3), np.int64)
    td[0, 0, 1] = [4, int(-1.0 * F), int(2.0 * F)]
    t = ev.MemoryTable(tree, nat.MEM_TD, td)
    assert t.mean_v[0, 0, 1] == -0.25 and t.mean_bootstrap[0, 0, 1] == 0.5
    assert np.isnan(t.mean_v[0, 0, 0]) and t.n[0, 0] == 4
    with pytest.raises(AttributeError):
        t.mean_r
    with pytest.raises(AttributeError):
        ev.MemoryTable(tree, nat.MEM_RL, td).mean_v

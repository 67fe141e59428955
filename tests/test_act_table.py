"""Tables that act, without a GPU: the C ABI's argument checks, ``evaluation.act_rows`` and the
host model of the frequency test (tests/act_table_ref.py) against ``policy_ref.walk``."""
import numpy as np
import pytest
import torch

import act_table_ref as at
import policy_ref as pr


@pytest.fixture(scope="module")
def L(pkg):
    import __graft_entry__
    __graft_entry__.build()
    return pkg.native.load()


def test_null_handles_are_refused_without_a_device(pkg, L):
    for call in (lambda: L.nfsp_engine_set_act_table(None, 0, 0, None),
                 lambda: L.nfsp_engine_get_act_table(None, 0, 0, None, None),
                 lambda: L.nfsp_group_set_act_table(None, 0, 0, 0, None)):
        assert call() == pkg.native.EINVAL
        assert b"null" in L.nfsp_last_error()


def test_the_calls_are_bound_and_declared(pkg):
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nfsp.h")).read()
    for name in ("nfsp_engine_set_act_table", "nfsp_engine_get_act_table", "nfsp_group_set_act_table"):
        assert name in pkg.native.SIGNATURES and f"int {name}(" in header


@pytest.mark.parametrize("game", [0, 1])
def test_act_rows_is_exact_on_one_hot_tables(pkg, game):
    ev = pkg.evaluation
    tree = ev.GameTree(game)
    rng = np.random.RandomState(5)
    onehot = np.eye(3)[rng.randint(3, size=(tree.ndec, 3))]
    rows = ev.act_rows(onehot)
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (tree.ndec, 3, 3)
    assert np.array_equal(rows.numpy().astype(np.float64), onehot)
    # a best response's shape of table, built by hand: one-hot over the legal actions, a fold
    # where the set is unreached (nfsp_best_response_table's tie rule)
    beta = np.zeros((tree.ndec, 3, 3))
    pick = rng.randint(3, size=(tree.ndec, 3))
    pick[~tree.legal] = np.minimum(pick[~tree.legal], 1)
    pick[rng.rand(tree.ndec, 3) < 0.3] = 0
    np.put_along_axis(beta, pick[..., None], 1.0, axis=2)
    rows = ev.act_rows(torch.as_tensor(beta))
    assert rows.numpy().view(np.uint32).tolist() == beta.astype(np.float32).view(np.uint32).tolist()
    assert np.array_equal(np.argmax(rows.numpy(), axis=2), pick)


def test_act_rows_refuses_what_is_not_finite(pkg):
    ev = pkg.evaluation
    tree = ev.GameTree(1)
    t = tree.uniform()
    assert np.array_equal(ev.act_rows(t).numpy(), t.astype(np.float32))     # one rounding per value
    for bad in (np.nan, np.inf, 1e300):                                      # 1e300: not finite as float32
        u = t.copy()
        u[3, 1, 2] = bad
        with pytest.raises(ValueError, match="finite"):
            ev.act_rows(u)
    with pytest.raises(ValueError, match="9 values"):
        ev.act_rows(np.zeros(10))


@pytest.mark.parametrize("game", [0, 1])
def test_the_frequency_model_walks_the_tree_as_the_evaluator_does(pkg, game):
    """``TableModel``'s reach walk gives ``policy_ref.walk``'s on-policy value of the same table
    pair per dealer to 1e-12, its probabilities are a distribution per visit, and every
    information set of the dealer's tree is visited."""
    tree = pkg.evaluation.GameTree(game)
    rows = at.full_support_table(tree, 17)
    m = at.TableModel(tree, rows)
    ref = pr.walk(tree, m.t_raw, m.t_raw)
    for d in (0, 1):
        assert abs(m.reward_mean[d] - ref[f"value0_dealer{d}"]) <= 1e-12
    assert abs(0.5 * m.reward_mean.sum() - ref["value0"]) <= 1e-12
    assert np.abs(m.t_raw.sum(axis=2) - 1.0).max() <= 1e-15 and m.t_raw.min() > 0.0
    assert np.allclose(m.p_rec.sum(axis=3), m.visit, rtol=0, atol=1e-15)
    rows_d = np.arange(tree.ndec)
    assert (m.visit[m.dealer_of_row, rows_d] > 0).all() and (m.visit[1 - m.dealer_of_row, rows_d] == 0).all()
    # the first decision of a hand is reached with the deal's marginal
    for d in (0, 1):
        first = int(tree.nodes["row"][tree.root[d]])
        marg = tree.deal.sum(axis=1 - int(tree.seat[first]))
        assert np.allclose(m.visit[d, first], marg, rtol=0, atol=1e-15)


def test_lookup_table_and_coverage_helper(pkg):
    tree = pkg.evaluation.GameTree(1)
    t = at.lookup_table(tree, 3)
    assert len({int(a) for a in np.argmax(t, axis=2).reshape(-1)}) == 3
    v = at.eps_greedy_visits(tree, t, 0.5)
    assert v.shape == (tree.ndec, 3) and (v > 0).all()
    # a seat decides at most twice per Kuhn hand and at least the dealer once
    per_seat = [v[tree.seat == s].sum() for s in (0, 1)]
    assert all(0.25 <= x <= 1.0 for x in per_seat)

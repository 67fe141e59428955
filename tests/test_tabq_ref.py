"""tests/tabq_ref.py, the restatement the GPU tests of tabular NFSP compare with, checked by hand.

The chain: Kuhn, seat 0, holding rank 1.  s_a is seat 0's first decision of a hand it deals, s_b its
second decision of that hand (after check, bet), and the hand ends there.  Three M_RL records:

    R1  s = s_a, action 1, r = +0.5, s2 = s_b,  not terminal
    R2  s = s_b, action 1, r = +2.0, s2 = 0,    terminal      (0 is no information set)
    R3  s = s_b, action 0, r = -1.0, s2 = 0,    terminal

fill is 0 but for two unseen actions: fill[s_a][2] = 7.25 and fill[s_b][2] = -3.  Q_0 = fill.

    sweep 1  Q[s_b] = (-1, 2, -3);  Q[s_a][1] = 0.5 + gamma max(Q_0[s_b]) = 0.5 + gamma max(0, 0, -3) = 0.5
             3 entries change
    sweep 2  Q[s_a][1] = 0.5 + gamma max(-1, 2, -3) = 0.5 + 2 gamma:  2.5 at gamma = 1, 1.5 at gamma = 0.5
             1 entry changes (none at gamma = 0)
    sweep 3  nothing changes: s_a -> s_b -> terminal has depth 2

Q[s_a][2] = 7.25 and Q[s_b][2] = -3 throughout.  The last sweep's table holds at (s_a, 1) the count 1,
fix(0.5 + 2 gamma) and fix(2); at (s_b, 1) the count 1, fix(2) and 0: a terminal record adds nothing
to field 2.  With NFSP_QUIRK_TERMINAL_BOOTSTRAP R2 and R3 bootstrap -- from s2 = 0, which is no
information set, so from 0: every value is the same."""
import numpy as np
import pytest

import tabq_ref as tq

FIX = 2.0**24


@pytest.fixture(scope="module")
def chain(pkg):
    import __graft_entry__
    __graft_entry__.build()
    tree = pkg.evaluation.GameTree(1)
    mine = [d for d in range(tree.ndec) if tree.seat[d] == 0 and tree.path(d)[0] == 0]
    depth = {d: len(tree.path(d)[1]) for d in mine}
    da = min(mine, key=depth.get)
    db = next(d for d in mine if d != da and int(tree.node_of_row[da]) in tree.path(d)[1])
    s_a, s_b = int(tree.obs[da, 1]), int(tree.obs[db, 1])
    assert tree.row_of(0, s_a) == (da, 1) and tree.row_of(0, s_b) == (db, 1) and (0, 0) not in tree._rows
    s = np.array([s_a, s_b, s_b], np.int64)
    s2 = np.array([s_b, 0, 0], np.int64)
    r2 = np.array([1, 4, -2], np.int64)                        # half chips
    meta = np.array([1, 1, 0], np.int64) | (np.array([0, 1, 1], np.int64) << 8) | ((r2 & 0xFF) << 16)
    fill = np.zeros((tree.ndec, 3, 3), np.float32)
    fill[da, 1, 2], fill[db, 1, 2] = 7.25, -3.0
    none = (np.zeros(0, np.int64),) * 3
    return tree, da, db, [(s, s2, meta), none], fill


@pytest.mark.parametrize("gamma", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("quirks", [0, 1])
def test_chain_by_hand(chain, gamma, quirks):
    tree, da, db, recs, fill = chain
    want = fill.copy()
    want[db, 1] = (-1.0, 2.0, -3.0)
    want[da, 1, 1] = 0.5
    q1, raw1, info1, ch1 = tq.sweeps(tree, recs, gamma, quirks, 1, fill)
    assert np.array_equal(q1, want) and ch1 == 3
    assert info1[0] == dict(records=3, matched=3, unmatched=0, clamped=0) and info1[1]["records"] == 0
    want[da, 1, 1] = 0.5 + 2.0 * gamma
    q2, raw2, _, ch2 = tq.sweeps(tree, recs, gamma, quirks, 2, fill)
    assert np.array_equal(q2, want) and ch2 == (1 if gamma else 0)
    assert raw2[da, 1, 1].tolist() == [1, int((0.5 + 2.0 * gamma) * FIX), int(2.0 * FIX)]
    assert raw2[db, 1, 1].tolist() == [1, int(2.0 * FIX), 0] and raw2[db, 1, 0].tolist() == [1, int(-1.0 * FIX), 0]
    assert raw2.sum(axis=(0, 1, 2))[0] == 3 and (raw2[..., 0] > 0).sum() == 3
    q3, raw3, _, ch3 = tq.sweeps(tree, recs, gamma, quirks, 3, fill)
    assert ch3 == 0 and np.array_equal(q3.view(np.uint32), q2.view(np.uint32)) and np.array_equal(raw3, raw2)
    assert q3[da, 1, 2] == np.float32(7.25) and q3[db, 1, 2] == np.float32(-3.0)       # unseen actions stay at fill


def test_fill_none_is_zero_and_the_illegal_raise_counts(chain):
    tree, da, db, recs, _ = chain
    q, _, _, _ = tq.sweeps(tree, recs, 1.0, 0, 2)
    assert q[da, 1].tolist() == [0.0, 2.5, 0.0] and (q[da, 0] == 0).all()
    # the largest entry at s_b is its third, whatever the row's legality: all three entries count
    hi = np.zeros((tree.ndec, 3, 3), np.float32)
    hi[db, 1, 2] = 9.0
    one, _ = tq.tdq(tree, 0, *recs[0], hi, 0.5, 0)
    assert one[da, 1, 1].tolist() == [1, int(5.0 * FIX), int(9.0 * FIX)]


def test_rows_of_the_three_stats():
    raw = np.zeros((5, 3, 3, 3), np.int64)
    fill = np.arange(5 * 9, dtype=np.float32).reshape(5, 3, 3) + 100.0
    # TD means: count 3 and sum 2^24 -> 1/3 in float32; a negative mean; count 0 -> fill
    raw[0, 0, 0, :2] = (3, 1 << 24)
    raw[0, 0, 1, :2] = (2, -(5 << 23))
    got = tq.rows(tq.ROWS_TD_MEAN, raw, fill)
    assert got[0, 0, 0] == np.float32(1.0 / 3.0) and got[0, 0, 1] == np.float32(-1.25) and got[0, 0, 2] == fill[0, 0, 2]
    assert np.array_equal(got[1:], fill[1:]) and (tq.rows(tq.ROWS_TD_MEAN, raw)[1:] == 0).all()
    assert tq.changed(fill, got) == 2 and tq.changed(got, got) == 0
    # M_SL: counts (2, 1, 0), masses (1.5, 0.5, 0) in 2^-24 units
    sl = np.zeros((5, 3, 3, 3), np.int64)
    sl[1, 2, :, 0] = (2, 1, 0)
    sl[1, 2, :, 1] = (3 << 23, 1 << 23, 0)
    sl[2, 0, :, 0] = (1, 0, 0)                                # n > 0 and M == 0: all-zero action vectors
    sl[3, 1, :, 0] = (0, 4, 0)
    sl[3, 1, :, 1] = (-1, 5, 0)                               # a negative mass
    sl[4, 0, :, 1] = (7, 7, 7)                                # mass without a record: n == 0
    mass, arg = tq.rows(tq.ROWS_SL_MASS, sl, fill), tq.rows(tq.ROWS_SL_ARGMAX, sl, fill)
    assert mass[1, 2].tolist() == [0.75, 0.25, 0.0]
    assert arg[1, 2].tolist() == [float(np.float32(2.0 / 3.0)), float(np.float32(1.0 / 3.0)), 0.0]
    keep = np.ones((5, 3), bool)
    keep[1, 2] = False
    for got in (mass, arg):
        assert np.array_equal(got[keep], fill[keep])          # n == 0, M <= 0 and a negative mass: fill's row
        assert got.dtype == np.float32
    assert (tq.rows(tq.ROWS_SL_MASS, sl)[keep] == 0).all()
    # a sum above 2^53 rounds once to double, then the quotient once to float
    big = np.zeros((1, 3, 3, 3), np.int64)
    big[0, 0, 0, :2] = (3, (1 << 60) + 1)
    assert tq.rows(tq.ROWS_TD_MEAN, big)[0, 0, 0] == np.float32((float((1 << 60) + 1) / 3.0) * 2.0**-24)

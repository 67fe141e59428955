"""Host side of the memory tables (include/nfsp.h nfsp_memtab_*): the lookup the kernel stages,
the fixed-point rule, and ``evaluation.MemoryTable.policy``.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import memtab_ref as mr


@pytest.fixture(scope="module")
def L(pkg):
    return pkg.native.load()


@pytest.mark.parametrize("game", ["leduc", "kuhn"])
def test_lookup_is_the_trees(pkg, L, game):
    g = pkg.native.GAME_KUHN if game == "kuhn" else pkg.native.GAME_LEDUC
    tree = pkg.evaluation.GameTree(g)
    assert len(tree._rows) == 3 * tree.ndec == (24 if game == "kuhn" else 390)
    shared = 0
    for (seat, obs), (row, rank) in tree._rows.items():
        assert L.nfsp_memtab_lookup(g, seat, obs) == row * 3 + rank
        assert tree.row_of(seat, obs) == (row, rank)
        # asked of the other seat there is no such set -- but for the dealer's first decision,
        # which both seats meet with the same observation (each as dealer, in rows of their own)
        other = tree._rows.get((1 - seat, obs))
        if other is None:
            assert L.nfsp_memtab_lookup(g, 1 - seat, obs) == -1
        else:
            shared += 1
            assert other[0] != row and L.nfsp_memtab_lookup(g, 1 - seat, obs) == other[0] * 3 + other[1]
    assert shared == 6                                  # 3 ranks x 2 seats
    keys = {obs for _, obs in tree._rows}
    rng = np.random.RandomState(5)
    words = [int(w) for w in rng.randint(1 << 30, size=10_000) if int(w) not in keys]
    assert len(words) > 9_900
    for seat in (0, 1):
        assert L.nfsp_memtab_lookup(g, seat, 0) == -1
        assert all(L.nfsp_memtab_lookup(g, seat, w) == -1 for w in words)
    assert L.nfsp_memtab_lookup(g, 2, next(iter(keys))) == -1
    assert L.nfsp_memtab_lookup(7, 0, next(iter(keys))) == -1


def test_fix_is_the_numpy_rule(pkg, L):
    assert pkg.native.MEMTAB_FIX_SHIFT == 24
    vals = [0.0, 2.0**-25, -2.0**-25, 3 * 2.0**-25, 1.0, 0.99999994, 255.99998, 256.0, -256.0, np.inf, -np.inf, np.nan,
            0.5, -13.25, 1e-30]
    want = {0.0: 0, 2.0**-25: 0, -2.0**-25: 0, 3 * 2.0**-25: 2, 1.0: 1 << 24, 0.99999994: (1 << 24) - 1,
            255.99998: (1 << 32) - 256, 256.0: mr.SAT, -256.0: -mr.SAT, np.inf: mr.SAT, -np.inf: -mr.SAT}
    ref, bad = mr.fix(np.array(vals, np.float32))
    for x, r, b in zip(vals, ref.tolist(), bad.tolist()):
        got = L.nfsp_memtab_fix(C.c_float(x))
        assert got == r, (x, got, r)
        if x in want:
            assert got == want[x], (x, got)
        assert b == (not abs(np.float32(x)) < 256)
    assert L.nfsp_memtab_fix(C.c_float(np.nan)) == 0
    # the plain rule where nothing saturates
    x = np.random.RandomState(1).uniform(-255, 255, 1000).astype(np.float32)
    assert [L.nfsp_memtab_fix(C.c_float(v)) for v in x] == np.rint(x.astype(np.float64) * 2**24).astype(np.int64).tolist()


def test_memory_table_policy(pkg):
    ev, nat = pkg.evaluation, pkg.native
    tree = ev.GameTree(nat.GAME_LEDUC)
    il = int(np.nonzero(~tree.legal)[0][0])             # a row where a raise is illegal
    lg = int(np.nonzero(tree.legal)[0][0])
    raw = np.zeros((tree.ndec, 3, 3, 3), np.int64)
    raw[lg, 0, :, 0] = (1, 2, 5)
    raw[lg, 0, :, 1] = (3 << 24, 0, 1 << 24)
    raw[lg, 1, :, 0] = (0, 0, 4)                        # records, but their vectors are all zero
    raw[il, 2, :, 0] = (0, 7, 0)
    raw[il, 2, :, 1] = (1 << 22, 1 << 22, 1 << 23)
    t = ev.MemoryTable(tree, nat.MEM_SL, raw)
    assert np.array_equal(t.counts, raw[..., 0]) and t.n[lg, 0] == 8 and t.n[lg, 1] == 4 and t.n.sum() == 19
    uni = tree.uniform()
    am, ms = t.policy("argmax"), t.policy("mass")
    assert am.dtype == np.float64 and am.shape == (tree.ndec, 3, 3)
    assert np.array_equal(am[lg, 0], np.array([1, 2, 5]) / 8.0) and np.array_equal(ms[lg, 0], [0.75, 0.0, 0.25])
    assert np.array_equal(am[lg, 1], [0.0, 0.0, 1.0]) and np.array_equal(ms[lg, 1], uni[lg, 1])
    assert np.array_equal(am[il, 2], [0.0, 1.0, 0.0]) and np.array_equal(ms[il, 2], [0.25, 0.25, 0.5])
    # rows without records: uniform over the legal actions
    assert np.array_equal(am[il, 0], [0.5, 0.5, 0.0]) and np.array_equal(ms[il, 0], [0.5, 0.5, 0.0])
    assert np.array_equal(am[lg, 2], [1 / 3.0] * 3)
    rest = np.ones((tree.ndec, 3), bool)
    rest[lg, :2] = rest[il, 2] = False
    assert np.array_equal(am[rest], uni[rest]) and np.array_equal(ms[rest], uni[rest])
    with pytest.raises(ValueError):
        t.policy("mean")
    with pytest.raises(AttributeError):
        t.mean_r
    raw[lg, 0, :, 1] = (-3, 0, 4)                       # half chips
    raw[lg, 0, :, 2] = (1, 0, 2)
    r = ev.MemoryTable(tree, nat.MEM_RL, raw)
    assert np.array_equal(r.mean_r[lg, 0], [-1.5, 0.0, 0.4]) and np.isnan(r.mean_r[lg, 2]).all()
    assert np.array_equal(r.terminal[lg, 0], [1, 0, 2])


def test_restatement_on_a_hand_made_case(pkg):
    tree = pkg.evaluation.GameTree(pkg.native.GAME_KUHN)
    (o0, d0, r0), (o1, d1, r1) = mr.sets_of(tree, 0)[:2]
    obs = [o0, o0, o1, 0, o0]
    a = np.array([[0.5, 0.5, 0], [0, 0, 300.0], [0, 1, 0], [1, 0, 0], [np.nan, 2, 1]], np.float32)
    raw, info = mr.table(tree, 0, mr.SL, obs, a=a)
    assert info == dict(records=5, matched=4, unmatched=1, clamped=2)
    assert raw[d0, r0, :, 0].tolist() == [2, 0, 1]       # first maximum; NaN is the maximum; 300 wins
    assert raw[d0, r0, :, 1].tolist() == [1 << 23, (1 << 23) + (2 << 24), mr.SAT + (1 << 24)]
    assert raw[d1, r1, :, 0].tolist() == [0, 1, 0] and raw.sum(axis=(1, 2))[:, 2].sum() == 0
    meta = [0 | (1 << 8) | ((-3 & 0xFF) << 16), 0 | (5 << 16), 2, 1, 3]
    raw, info = mr.table(tree, 0, mr.RL, obs, meta=meta)
    assert info == dict(records=5, matched=3, unmatched=2, clamped=0)
    assert raw[d0, r0, 0].tolist() == [2, 2, 1] and raw[d1, r1, 2].tolist() == [1, 0, 0]

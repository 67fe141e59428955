"""The evaluator's tree as data, the table walk, per-hand mixtures and CFR+, without a GPU:
``evaluation.GameTree`` / ``mix`` (host code of the product) and the numpy restatements of the
device kernels (tests/policy_ref.py) against the brute-force oracle (oracle/exploit_oracle.py),
which plays full histories through the reference-restated Env and knows nothing of the tree.
The GPU side of the same checks is tests/test_gpu_evaluation.py."""
import ctypes as C

import numpy as np
import pytest

import exploit_oracle as eo
import policy_ref as pr

GAMES = {"leduc": 0, "kuhn": 1}
_TREES = {}


@pytest.fixture(scope="module")
def trees(pkg):
    import __graft_entry__
    __graft_entry__.build()
    for name, g in GAMES.items():
        if name not in _TREES:
            _TREES[name] = pkg.evaluation.GameTree(g)
    return _TREES


def oracle_infosets(game):
    """{(seat, obs): raise legal} over every decision the oracle's replay reaches."""
    seen = {}
    for deal in eo.rank_deals(game):
        for dealer in (0, 1):
            stack = [[]]
            while stack:
                acts = stack.pop()
                r = eo.replay(deal, dealer, acts, game)
                if r[0] == "terminal":
                    continue
                _, seat, obs, legal = r
                assert seen.setdefault((seat, obs), legal) == legal
                for a in eo._legal_actions(legal):
                    stack.append(acts + [a])
    return seen


# ---- sizes and information sets ---------------------------------------------------------------
@pytest.mark.parametrize("game,nn,ndec", [("leduc", 364, 130), ("kuhn", 22, 8)])
def test_tree_sizes_and_information_sets(trees, game, nn, ndec):
    t = trees[game]
    assert (t.nn, t.ndec) == (nn, ndec)
    assert t.nn == t.ndec + t.nterm + int((t.nodes["kind"] == pr.CHANCE).sum())
    assert t.lev[0] == 0 and t.lev[-1] == t.nn and np.all(np.diff(t.lev) > 0)
    keys = {(int(t.seat[d]), int(t.obs[d, r])) for d in range(t.ndec) for r in range(3)}
    assert len(keys) == 3 * ndec                      # (seat, obs) is unique per (row, rank)
    want = oracle_infosets(game)
    assert len(want) == 3 * ndec
    assert keys == set(want)
    for (seat, obs), legal in want.items():
        row, rank = t.row_of(seat, obs)
        assert t.seat[row] == seat and t.obs[row, rank] == obs and bool(t.legal[row]) == legal
    assert t.deal.sum() == pytest.approx(1.0)


def test_tree_is_in_depth_order_and_describes_rows(trees):
    t = trees["leduc"]
    N = t.nodes
    for n in range(t.nn):
        assert N["parent"][n] < n
        for a, c in enumerate(N["child"][n]):
            if c >= 0:
                assert N["parent"][c] == n and N["via"][c] == a
    assert sorted(t.root) == [0, 1]
    d0 = t.describe(int(N["row"][t.root[0]]))
    assert d0.startswith("dealer 0, history -, public rank none, seat 0 to act")
    deep = int(np.argmax([len(t.path(r)[1]) for r in range(t.ndec)]))
    text = t.describe(deep)
    assert "public" in text and ":raise" in text
    dealer, chain = t.path(deep)
    assert chain[0] == t.root[dealer] and N["row"][chain[-1]] == deep


# ---- the walk restated, against the brute force ------------------------------------------------
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
@pytest.mark.parametrize("case", ["seed0", "seed1", "uniform"])
def test_walk_restatement_matches_oracle(trees, game, case):
    t = trees[game]
    if case == "uniform":
        t0 = t1 = t.uniform()
    else:
        s = int(case[-1])
        t0, t1 = pr.random_table(t, 10 * s), pr.random_table(t, 10 * s + 1)
    got = pr.walk(t, t0, t1)
    want = pr.oracle_table_scores(t, t0, t1)
    for k in ("br0", "br1", "value0", "value0_dealer0", "value0_dealer1"):
        assert abs(got[k] - want[k]) <= 1e-9, (k, got[k], want[k])
    assert got["value0"] == 0.5 * (got["value0_dealer0"] + got["value0_dealer1"])


# ---- per-hand mixtures -----------------------------------------------------------------------
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_mix_is_linear_in_value(pkg, trees, game):
    t = trees[game]
    a, b, c = (pr.random_table(t, s) for s in (3, 4, 5))
    eta = 0.1
    m = pkg.evaluation.mix(t, [(eta, a), (1 - eta, b)])
    assert np.allclose(m.sum(-1), 1.0, atol=1e-12) and np.all(m[~t.legal][:, :, 2] == 0)
    for seat in (0, 1):
        v = [pr.walk(t, x, c)["value0"] if seat == 0 else pr.walk(t, c, x)["value0"] for x in (m, a, b)]
        assert abs(v[0] - (eta * v[1] + (1 - eta) * v[2])) <= 1e-12, seat
    # a per-row average is a different strategy: the per-hand mixture is not it
    assert np.abs(m - (eta * a + (1 - eta) * b)).max() > 1e-3


def test_mix_of_one_table_and_zero_reach(pkg, trees):
    t = trees["leduc"]
    a = pr.random_table(t, 6)
    a[int(t.nodes["row"][t.root[0]]), 1] = [0.0, 1.0, 0.0]     # rank 1 never folds or raises first
    reach = t.own_reach(a)
    assert (reach == 0).any() and (reach > 0).any()
    m = pkg.evaluation.mix(t, [(1.0, a)])
    assert np.allclose(m[reach > 0], a[reach > 0], atol=1e-15)
    assert np.array_equal(m[reach == 0], t.uniform()[reach == 0])


# ---- CFR+ restated, scored by the brute force ----------------------------------------------------
@pytest.mark.parametrize("game,iters,bound", [("kuhn", 128, 0.005), ("leduc", 64, 0.03)])
def test_cfr_restatement_converges(trees, game, iters, bound):
    t = trees[game]
    avg = pr.CfrRef(t).run(iters).average()
    assert np.allclose(avg.sum(-1), 1.0, atol=1e-12) and np.all(avg[~t.legal][:, :, 2] == 0)
    s = pr.oracle_table_scores(t, avg, avg, keys=("br0", "br1"))
    print(game, iters, "exploitability", s["exploitability"])
    assert 0 <= s["exploitability"] < bound


# ---- ABI ------------------------------------------------------------------------------------
def test_new_symbols_exported_bound_and_validated(pkg):
    import __graft_entry__
    __graft_entry__.build()
    nat = pkg.native
    L = nat.load()
    new = ["nfsp_tree_size", "nfsp_tree_export", "nfsp_evaluate_batch", "nfsp_policy_table", "nfsp_cfr_create",
           "nfsp_cfr_run", "nfsp_cfr_iterations", "nfsp_cfr_average", "nfsp_cfr_state", "nfsp_cfr_destroy"]
    for name in new:
        assert name in nat.SIGNATURES and hasattr(L, name), name
    assert C.sizeof(nat.TreeNode) == 24 and C.sizeof(nat.PolicySpec) == 16

    def einval(rc, word):
        assert rc == nat.EINVAL
        assert word.encode() in L.nfsp_last_error(), L.nfsp_last_error()

    n = C.c_int32(0)
    einval(L.nfsp_tree_size(0, None, None, None, None), "null")
    einval(L.nfsp_tree_size(7, C.byref(n), C.byref(n), C.byref(n), C.byref(n)), "game")
    einval(L.nfsp_tree_export(0, None, None, None, None, None, None, None), "null")
    einval(L.nfsp_evaluate_batch(None, None, None, 1, None), "null")
    einval(L.nfsp_policy_table(None, None, None), "null")
    einval(L.nfsp_cfr_create(None, None), "null")
    einval(L.nfsp_cfr_run(None, 1), "null")
    einval(L.nfsp_cfr_iterations(None, None), "null")
    einval(L.nfsp_cfr_average(None, None), "null")
    einval(L.nfsp_cfr_state(None, None, None), "null")
    einval(L.nfsp_cfr_destroy(None), "null")

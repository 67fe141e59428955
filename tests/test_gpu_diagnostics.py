"""What the engine diagnostics score, pinned against the evaluator through public API only.

``br_gap``, ``best_response_table`` and ``install_oracle_br`` each face seat o with "what seat o
plays".  This file states that rule once (``opponent`` below) from ``acting_policy``, ``policy`` and
``evaluation.mix``, and asserts bit equality with the evaluator called directly, on Kuhn and Leduc,
with the default quirks and with ``EXT_SAMPLE_AR | EXT_LINEAR_Q`` (another default ``ar_mode``,
another head kind), with no table installed, one on (0, AR), and on (0, AR) and (1, BR), at ``eta``
None and 0.1; then the same through an ``EngineGroup``.  Fresh glorot nets are non-degenerate, so
no learner runs: 64 lanes, no update.
"""
import numpy as np
import pytest

import act_table_ref as at

pytestmark = pytest.mark.gpu

GAMES = [1, 0]                       # Kuhn, Leduc
QUIRKS = ["default", "sample_linear"]
TABLES = ["none", "ar0", "ar0_br1"]
ETAS = [None, 0.1]
_TREES = {}


def tree_of(pkg, game):
    if game not in _TREES:
        _TREES[game] = pkg.evaluation.GameTree(game)
    return _TREES[game]


def cfg_of(pkg, game, quirks):
    cfg = dict(game=game, n_lanes=64, inserts_per_update=1 << 30, seed=13, init_seed=5)
    if quirks == "sample_linear":
        cfg["quirks"] = pkg.native.EXT_SAMPLE_AR | pkg.native.EXT_LINEAR_Q
    return cfg


def tables_of(pkg, tree, tables):
    """{(agent, role): float32 rows} of a table set-up."""
    E = pkg.engine
    out = {}
    if tables in ("ar0", "ar0_br1"):
        out[(0, E.NET_AR)] = at.full_support_table(tree, 3)
    if tables == "ar0_br1":
        out[(1, E.NET_BR)] = at.lookup_table(tree, 4)
    return out


def opponent(pkg, eng, o, ar_mode, eta, tree, tables=False):
    """What seat o plays, as the diagnostics score it: its AR part is ``acting_policy(o, NET_AR,
    ar_mode)``, its BR part ``acting_policy(o, NET_BR)``.  Without ``eta`` the AR part, as the net
    itself while no table is installed there (unless ``tables``); with ``eta`` the per-hand mixture
    eta x BR + (1 - eta) x AR."""
    E, ev = pkg.engine, pkg.evaluation
    if eta is None:
        if eng.act_table(o, E.NET_AR)[0] is None and not tables:
            return eng.policy(o, E.NET_AR, ar_mode)
        return ev.Policy.table(eng.acting_policy(o, E.NET_AR, ar_mode, tree))
    ar = eng.acting_policy(o, E.NET_AR, ar_mode, tree)
    br = eng.acting_policy(o, E.NET_BR, None, tree)
    return ev.Policy.table(ev.mix(tree, [(eta, br), (1.0 - eta, ar)]))


def gap_figures(pkg, eng, ar_mode, eta, tree):
    """``br_gap``'s figures from one ``evaluate_batch`` of (BR net of 0, P_1) and (P_0, BR net of 1)."""
    E, ev = pkg.engine, pkg.evaluation
    p0, p1 = (opponent(pkg, eng, o, ar_mode, eta, tree) for o in (0, 1))
    r0, r1 = ev.evaluate_batch(eng.ctx, [(eng.policy(0, E.NET_BR), p1), (p0, eng.policy(1, E.NET_BR))])
    return [{"br_exact": r0["br0"], "br_learned": r0["value0"], "gap": r0["br0"] - r0["value0"]},
            {"br_exact": r1["br1"], "br_learned": -r1["value0"], "gap": r1["br1"] + r1["value0"]}]


def slots(eng):
    return {(a, r): eng.act_table(a, r)[0] for a in (0, 1) for r in (0, 1)}


@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("tables", TABLES)
@pytest.mark.parametrize("quirks", QUIRKS)
@pytest.mark.parametrize("game", GAMES)
def test_diagnostics_score_what_the_seat_plays(pkg, game, quirks, tables, eta):
    E, ev = pkg.engine, pkg.evaluation
    tree = tree_of(pkg, game)
    eng = E.SelfPlayEngine(**cfg_of(pkg, game, quirks))
    installed = tables_of(pkg, tree, tables)
    for (a, role), rows in installed.items():
        eng.set_act_table(a, role, rows)
    assert {k for k, v in slots(eng).items() if v is not None} == set(installed)

    # best_response_table: AR mode 0
    p0, p1 = (opponent(pkg, eng, o, 0, eta, tree) for o in (0, 1))
    want = ev.best_response(eng.ctx, p0, p1).cpu().numpy()
    got = eng.best_response_table(eta).cpu().numpy()
    assert np.array_equal(got, want)
    assert set(np.unique(got)) == {0.0, 1.0} and (got.sum(axis=2) == 1.0).all()

    # br_gap: the given AR mode
    for ar_mode in (0, 1):
        got = eng.br_gap(ar_mode, eta)
        want = gap_figures(pkg, eng, ar_mode, eta, tree)
        print(f"game {game} {quirks} {tables} eta {eta} ar_mode {ar_mode}: {got}")
        assert got == want
    assert eng.br_gap(eta=eta) == eng.br_gap(0, eta)

    # install_oracle_br: both opponents as tables at the executed AR mode
    p0, p1 = (opponent(pkg, eng, o, None, eta, tree, tables=True) for o in (0, 1))
    want = ev.best_response(eng.ctx, p0, p1).cpu().numpy()
    beta = eng.install_oracle_br(eta)
    assert np.array_equal(beta.cpu().numpy(), want)
    rows = ev.act_rows(beta).cpu().numpy()
    now = slots(eng)
    for a in (0, 1):
        assert np.array_equal(now[(a, E.NET_BR)].cpu().numpy(), rows)
    ar_kept = installed.get((0, E.NET_AR))
    assert (now[(0, E.NET_AR)] is None) == (ar_kept is None) and now[(1, E.NET_AR)] is None
    if ar_kept is not None:
        assert np.array_equal(now[(0, E.NET_AR)].cpu().numpy(), ar_kept)
    eng.clear_act_tables()
    assert all(v is None for v in slots(eng).values())
    eng.close()


@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("quirks", QUIRKS)
@pytest.mark.parametrize("game", GAMES)
def test_group_replicas_install_and_score_as_engines(pkg, game, quirks, eta):
    E, ev = pkg.engine, pkg.evaluation
    tree = tree_of(pkg, game)
    cfg = cfg_of(pkg, game, quirks)
    grp = E.EngineGroup(2, **cfg)
    assert grp.br_gap_all(0, eta) == [e.br_gap(0, eta) for e in grp.replicas]
    r1 = grp.replicas[1]
    p0, p1 = (opponent(pkg, r1, o, None, None, tree, tables=True) for o in (0, 1))
    want = ev.best_response(grp.ctx, p0, p1).cpu().numpy()
    beta = r1.install_oracle_br()
    assert np.array_equal(beta.cpu().numpy(), want)
    rows = ev.act_rows(beta).cpu().numpy()
    for a in (0, 1):
        assert np.array_equal(r1.act_table(a, E.NET_BR)[0].cpu().numpy(), rows)
        assert r1.act_table(a, E.NET_AR)[0] is None
    assert all(v is None for v in slots(grp.replicas[0]).values())
    # replica 1's BR slots now act with tables: with eta they are its BR part
    gaps = grp.br_gap_all(0, eta)
    for r, e in enumerate(grp.replicas):
        assert gaps[r] == e.br_gap(0, eta) == gap_figures(pkg, e, 0, eta, tree)
    r1.clear_act_tables()
    assert all(v is None for v in slots(r1).values())
    grp.close()

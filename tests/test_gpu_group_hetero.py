"""Heterogeneous engine groups (nfsp_group_create_v, EngineGroup(cfgs=...)): the replicas of one
group differ in seed, eta, lr_br, lr_ar, gamma, epsilon, target_every and quirks -- a
hyperparameter sweep in one launch.

Bar, everywhere: replica r is BIT-IDENTICAL to a standalone SelfPlayEngine built from cfgs[r]
and the same init seed and stepped as often -- the six nets, the counters and schedules
(engine_ref.STAT_KEYS), the memories and state_digest().  No tolerance anywhere."""
import numpy as np
import pytest

from engine_ref import STAT_KEYS, mem, nets

pytestmark = pytest.mark.gpu

SHAPE = dict(n_lanes=2048, rl_capacity=3000, sl_capacity=2000)      # test_gpu_group.SMALL's
INIT0 = 5


def everything_cfgs(nat):
    """Case 1: every field that may differ, at once."""
    return [dict(SHAPE, seed=777, target_every=7),
            dict(SHAPE, seed=778, lr_ar=0.02, lr_br=0.01, target_every=5),
            dict(SHAPE, seed=31337, gamma=0.9, eta=0.3, epsilon=0.2),
            dict(SHAPE, seed=780,
                 quirks=nat.EXT_SL_ONEHOT | nat.EXT_RESERVOIR | nat.EXT_EPS_CONST | nat.EXT_SAMPLE_AR)]


def fields(c):
    """An nfsp_engine_cfg by value (ctypes structures compare by identity)."""
    return tuple(getattr(c, n) for n, _ in c._fields_)


def view(e, with_mem=False):
    """What the bar compares of one engine (a standalone one or a group's replica)."""
    st = e.stats()
    out = {"stats": {k: st[k] for k in STAT_KEYS + ("rollouts",)}, "nets": nets(e), "digest": e.state_digest()}
    if with_mem:
        out["mem"] = [mem(e, a) for a in (0, 1)]
    return out


def assert_same(got, want, where):
    for k, v in want["stats"].items():
        assert got["stats"][k] == v, (where, k, got["stats"][k], v)
    for n, (x, y) in enumerate(zip(got["nets"], want["nets"])):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (where, "net", n)
    assert got["digest"] == want["digest"], (where, "digest")
    if "mem" in want:
        for a in (0, 1):
            assert got["mem"][a].keys() == want["mem"][a].keys()
            for k, v in want["mem"][a].items():
                assert np.array_equal(got["mem"][a][k], v), (where, "memory", a, k)


def solo_reference(pkg, cfgs, init_seeds, steps, game=None):
    """ref[step][r]: standalone engines of cfgs[r] after step + 1 steps (memories at the last)."""
    kw = {} if game is None else {"game": game}
    solo = [pkg.engine.SelfPlayEngine(init_seed=s, **kw, **c) for c, s in zip(cfgs, init_seeds)]
    ref = []
    for k in range(steps):
        for e in solo:
            e.step()
        ref.append([view(e, with_mem=k == steps - 1) for e in solo])
    for e in solo:
        e.close()
    return ref


def run_against(pkg, g, ref, picks=None, each_step=None):
    picks = range(g.R) if picks is None else picks
    for k, want in enumerate(ref):
        g.step()
        g.check()
        if each_step:
            each_step(k)
        for i, r in enumerate(picks):
            assert_same(view(g.replicas[r], with_mem="mem" in want[i]), want[i], (k, r))


@pytest.fixture(scope="module")
def ref1(pkg):
    """Case 1's standalone engines, 3 steps: shared by the cases that use its group."""
    cfgs = everything_cfgs(pkg.native)
    return solo_reference(pkg, cfgs, [INIT0 + r for r in range(len(cfgs))], 3)


def group1(pkg, **kw):
    return pkg.engine.EngineGroup(cfgs=everything_cfgs(pkg.native), init_seed=INIT0, **kw)


def test_everything_at_once(pkg, ref1):
    g = group1(pkg)
    if g.sched()["br_persist"]:          # (the environment's default: this case is the rounds')
        g.set_sched(br_persist=0)
    # read back through nfsp_group_replica_cfg: exactly as given, the seeds not offset
    want = everything_cfgs(pkg.native)
    for r, c in enumerate(g.cfgs):
        assert fields(c) == fields(pkg.engine.make_cfg(g.L, **want[r])), r
        assert fields(c) == fields(g.replicas[r].cfg)
    assert [c.target_every for c in g.cfgs] == [7, 5, 150, 150]

    def rounds(k):                       # several BR segments per call, differing between replicas
        assert g.rounds() >= 2, (k, g.rounds())
    run_against(pkg, g, ref1, each_step=rounds)
    # each replica syncs its target nets at its own period: update k syncs iff k % target_every == 0
    for r, c in enumerate(g.cfgs):
        st = g.replicas[r].stats()
        assert st["target_syncs"] == [-(-n // c.target_every) for n in st["br_updates"]], (r, st["target_syncs"])
        assert min(st["br_updates"]) > 2 * 7
    # the replicas are different runs
    assert len({g.replicas[r].state_digest() for r in range(g.R)}) == g.R
    g.close()


def test_sliced_and_pipelined(pkg):
    shape = dict(n_lanes=1024, slices=4, slice_lag=2, rl_capacity=3000, sl_capacity=2000)
    cfgs = [dict(shape, seed=555, target_every=7),
            dict(shape, seed=556, target_every=11, lr_br=0.01, gamma=0.9),
            dict(shape, seed=557, target_every=5, lr_br=0.02, gamma=1.0)]
    ref = solo_reference(pkg, cfgs, [1, 2, 3], 3)
    g = pkg.engine.EngineGroup(cfgs=cfgs, init_seed=1)
    run_against(pkg, g, ref)
    assert g.replicas[0].stats()["rollouts"] == 3 * 4
    assert min(min(e.stats()["br_updates"]) for e in g.replicas) > 0
    g.close()


@pytest.mark.parametrize("head", ["TEXTBOOK_MSE", "TEXTBOOK"])
def test_linear_head(pkg, head):
    """Every replica with the linear Q head (k_chain3<2 / 3>), the targets' gamma and lr_br per
    job.  TEXTBOOK_MSE is the case the feature names; TEXTBOOK is the Huber form of the same path."""
    q = getattr(pkg.native, head)
    cfgs = [dict(SHAPE, seed=91, quirks=q, target_every=7),
            dict(SHAPE, seed=92, quirks=q, target_every=7, lr_br=0.01, gamma=0.8)]
    ref = solo_reference(pkg, cfgs, [3, 4], 2)
    g = pkg.engine.EngineGroup(cfgs=cfgs, init_seed=3)
    run_against(pkg, g, ref)
    g.close()


@pytest.mark.parametrize("R", [80, 200])
def test_shared_cus(pkg, R):
    """test_gpu_group's shared-CU shape (2 or 4 chain workgroups per CU), the cfgs cycling
    through four variants; replicas 0, 1, R / 2 and R - 1 against standalone engines."""
    nat = pkg.native
    shape = dict(n_lanes=256, rl_capacity=1500, sl_capacity=1000, target_every=7)
    variants = [dict(), dict(lr_ar=0.02, lr_br=0.01, target_every=5), dict(gamma=0.9, eta=0.3, epsilon=0.2),
                dict(quirks=nat.EXT_SL_ONEHOT | nat.EXT_RESERVOIR | nat.EXT_EPS_CONST | nat.EXT_SAMPLE_AR)]
    cfgs = [dict(shape, seed=4242 + r, **variants[r % 4]) for r in range(R)]
    picks = [0, 1, R // 2, R - 1]
    ref = solo_reference(pkg, [cfgs[r] for r in picks], [3 + r for r in picks], 2)
    g = pkg.engine.EngineGroup(cfgs=cfgs, init_seed=3)
    run_against(pkg, g, ref, picks=picks)
    st = g.stats()
    assert st["hands"] == 2 * R * 256 and st["rollouts"] == 2 * R and sum(st["br_updates"]) > 0
    g.close()


def test_persist_falls_back_to_the_rounds(pkg, ref1):
    """br_persist on a group whose replicas differ in gamma, lr_br and quirks: k_br_persist takes
    one of each per launch, so the group keeps the BR rounds -- the same bits."""
    g = group1(pkg)
    g.set_sched(br_persist=1)

    def rounds(k):
        assert g.rounds() >= 1
    run_against(pkg, g, ref1, each_step=rounds)
    assert g.rounds() >= 2               # (one k_br_persist launch would report 1)
    g.close()


def test_wrapper_equivalence(pkg):
    """nfsp_group_create(cfg, R) = nfsp_group_create_v with cfgs[r] = cfg, seed + r."""
    a = pkg.engine.EngineGroup(3, seed=777, init_seed=INIT0, target_every=7, **SHAPE)
    b = pkg.engine.EngineGroup(cfgs=[dict(SHAPE, seed=777 + r, target_every=7) for r in range(3)], init_seed=INIT0)
    assert [fields(c) for c in a.cfgs] == [fields(c) for c in b.cfgs]
    for _ in range(2):
        a.step()
        b.step()
    assert a.state_digest() == b.state_digest()
    assert len(set(a.state_digest())) == 3
    a.close()
    b.close()


def test_exchange_is_refused_on_a_live_group(pkg, ref1):
    nat = pkg.native
    with pytest.raises(nat.NativeError, match="AVG_AR"):
        group1(pkg, avg_ar=True)
    g = group1(pkg)
    before = g.state_digest()
    with pytest.raises(nat.NativeError, match="heterogeneous"):
        g.set_exchange(nat.XCHG_AR, every=1)
    with pytest.raises(nat.NativeError, match="heterogeneous"):
        g.average_ar()
    g.set_exchange(nat.XCHG_AR, every=0)             # "off" stays legal
    assert g.state_digest() == before
    g.step()                                         # unchanged, and it still steps
    for r in range(g.R):
        assert g.replicas[r].state_digest() == ref1[0][r]["digest"], r
    # a seeds-only list is a uniform group: its exchange works
    u = pkg.engine.EngineGroup(cfgs=[dict(SHAPE, seed=s) for s in (9, 10)], avg_ar=True)
    u.step()
    assert np.array_equal(u.replicas[0].get_weights(0, 0), u.replicas[1].get_weights(0, 0))
    u.close()
    g.close()


def test_checkpoint(pkg, ref1, tmp_path):
    nat = pkg.native
    path = str(tmp_path / "hetero.nfsp")
    g = group1(pkg)
    g.step()
    g.step()
    g.save(path)
    data = np.fromfile(path, dtype=np.uint8)
    for r in range(g.R):
        assert fields(pkg.checkpoint.stored_cfg(data, r)[0]) == fields(g.cfgs[r]), r
    two = g.state_digest()
    g.close()
    # a fresh group from the file (every replica's own cfg), one more step: the uninterrupted run
    h = pkg.engine.EngineGroup.from_checkpoint(path)
    assert [fields(c) for c in h.cfgs] == [fields(pkg.checkpoint.stored_cfg(data, r)[0]) for r in range(h.R)]
    assert h.state_digest() == two == [ref1[1][r]["digest"] for r in range(h.R)]
    h.step()
    assert h.state_digest() == [ref1[2][r]["digest"] for r in range(h.R)]
    # (the digest covers the memories' live records; the raw M_RL log also has dead rows, which a
    # load does not restore, so the memory dump is not compared here)
    for r in range(h.R):
        want = {k: v for k, v in ref1[2][r].items() if k != "mem"}
        assert_same(view(h.replicas[r]), want, ("resumed", r))
    h.close()
    # a group whose replica 1 has another lr_ar: refused, the replica named, nothing written
    cfgs = everything_cfgs(nat)
    cfgs[1]["lr_ar"] = 0.03
    o = pkg.engine.EngineGroup(cfgs=cfgs, init_seed=INIT0)
    o.step()
    before = o.state_digest()
    with pytest.raises(nat.NativeError, match="replica 1"):
        o.load(path)
    assert o.state_digest() == before
    o.close()

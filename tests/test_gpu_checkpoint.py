"""Checkpoint and resume (include/nfsp.h nfsp_*_state_*, checkpoint.py).

Bar: a run continued from a checkpoint in a fresh engine is BIT-IDENTICAL to the uninterrupted
run -- all six nets, the counters and schedules, the memories and the state digest -- because
every random draw is a Philox counter of (seed, lane, hand) or (agent, update, row) and a step
boundary joins every stream.  No tolerances anywhere: np.array_equal on raw views.

Every save point is made to be a meaningful one (asserted): M_RL's circular log has wrapped,
M_SL replaces, and a target-sync cycle is under way."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# test_gpu_group.py's shape with a smaller M_SL: the log wraps and the reservoir replaces early
BASE = dict(n_lanes=2048, rl_capacity=3000, sl_capacity=600, target_every=7)
MAX_STEPS = 16


def nets(eng):
    return np.stack([eng.get_weights(a, n) for a in (0, 1) for n in (0, 1, 2)])


def bits(x):
    return np.atleast_1d(np.asarray(x)).view(np.uint8)


def logical_memories(eng):
    """Per agent: the live M_RL records oldest first and the M_SL rows [0, sl_size), every
    column of the fp32 export."""
    st = eng.stats()
    out = []
    for a in (0, 1):
        m = eng.memories(a)
        torch.cuda.synchronize()
        tot, live = st["rl_total"][a], st["rl_size"][a]
        idx = torch.as_tensor((np.arange(tot - live, tot) % m["log_cap"]).astype(np.int64), device=eng.dev)
        d = {k: m[k][idx].cpu().numpy() for k in ("rl_s", "rl_a", "rl_r", "rl_s2", "rl_t")}
        d.update({k: m[k][:st["sl_size"][a]].cpu().numpy() for k in ("sl_s", "sl_a")})
        out.append(d)
    return out


def assert_same_state(x, y, what=""):
    assert np.array_equal(bits(nets(x)), bits(nets(y))), what
    sx, sy = x.stats(), y.stats()
    assert sx.keys() == sy.keys()
    for k in sx:
        assert np.array_equal(bits(sx[k]), bits(sy[k])), (what, k, sx[k], sy[k])
    for a, (mx, my) in enumerate(zip(logical_memories(x), logical_memories(y))):
        for k in mx:
            assert mx[k].shape == my[k].shape and np.array_equal(bits(mx[k]), bits(my[k])), (what, a, k)
    assert x.state_digest() == y.state_digest(), what


def meaningful(eng):
    """The save point exercises what a resume can get wrong."""
    st = eng.stats()
    log_cap = eng.cfg.rl_capacity + 4 * eng.slice_lanes
    return (min(st["rl_total"]) > log_cap and min(st["sl_total"]) > eng.cfg.sl_capacity
            and any(it % eng.cfg.target_every for it in st["iteration"]))


def step_until_meaningful(obj, probe=None, at_least=1):
    probe = probe or obj
    n = 0
    while n < at_least or not meaningful(probe):
        obj.step()
        n += 1
        assert n <= MAX_STEPS, probe.stats()
    assert meaningful(probe)
    return n


CASES = {
    "unsliced": dict(),
    "slices4": dict(slices=4),
    "slices4_lag2": dict(slices=4, slice_lag=2),
    "kuhn_textbook": dict(kuhn=True),
}


def make(pkg, case, **over):
    kw = dict(BASE, seed=4242, **CASES[case])
    game = pkg.native.GAME_LEDUC
    if kw.pop("kuhn", False):
        game = pkg.native.GAME_KUHN
        kw["quirks"] = pkg.native.TEXTBOOK_MSE_DECAY     # linear-Q chain, true reservoir, sampled AR
    kw.update(over)
    return pkg.engine.SelfPlayEngine(init_seed=3, game=game, **kw)


@pytest.mark.parametrize("case", list(CASES))
def test_resume_is_bit_exact(pkg, tmp_path, case):
    n2 = 2
    path = tmp_path / "b.nfsp"
    b = make(pkg, case)
    n1 = step_until_meaningful(b)
    b.save(path)
    b.close()
    c = pkg.engine.SelfPlayEngine.from_checkpoint(path, init_seed=99)     # its own initial nets: overwritten
    assert (c.cfg.slices, c.cfg.slice_lag) == (CASES[case].get("slices", 1), CASES[case].get("slice_lag", 1))
    a = make(pkg, case)
    for _ in range(n1):
        a.step()
    assert_same_state(a, c, "at the checkpoint")
    for _ in range(n2):
        a.step()
        c.step()
    assert_same_state(a, c, "after the continuation")
    assert a.stats()["hands"] == (n1 + n2) * BASE["n_lanes"] and min(a.stats()["br_updates"]) > 0


NP = 30 * 64 + 64 + 64 * 3 + 3


def replica_payload(ck, r):
    """Replica r's engine payload of a parsed group file: the bytes a standalone save holds."""
    off = 24 + 24 * NP                                    # the group record and w0
    for k, e in enumerate(ck["engines"]):
        n = 192 + 296 + 24 * NP + 32 * sum(len(x) for x in e["rl"]) + 16 * sum(len(x) for x in e["sl"])
        if k == r:
            return ck["payload"][off:off + n]
        off += n


def _digests_agree(pkg, eng, path):
    eng.save(path)
    ck = pkg.checkpoint.read(path)
    d = eng.state_digest()
    assert d == ck["header"]["digest"] == pkg.checkpoint.digest(ck["payload"])
    return ck, d


def test_digest_of_device_state_equals_the_files(pkg, tmp_path):
    ck_mod = pkg.checkpoint
    # a fresh engine: both memories empty, the table's memory segments have zero length
    e = make(pkg, "unsliced")
    ck, d0 = _digests_agree(pkg, e, tmp_path / "fresh.nfsp")
    assert [len(x) for x in ck["engines"][0]["rl"] + ck["engines"][0]["sl"]] == [0, 0, 0, 0]
    # a partial reservoir (and an M_RL log that has not wrapped)
    p = make(pkg, "unsliced", sl_capacity=2000)
    p.step()
    st = p.stats()
    assert 0 < max(st["sl_size"]) < 2000
    ck, _ = _digests_agree(pkg, p, tmp_path / "partial.nfsp")
    assert [len(x) for x in ck["engines"][0]["sl"]] == st["sl_size"]
    # wrapped log, replacing reservoir, target cycle under way
    step_until_meaningful(e)
    ck, d1 = _digests_agree(pkg, e, tmp_path / "wrapped.nfsp")
    assert [len(x) for x in ck["engines"][0]["rl"]] == [3000, 3000]
    assert np.array_equal(bits(ck["engines"][0]["nets"]), bits(nets(e).reshape(2, 3, -1)))
    hands, g = e.stats()["hands"], ck["engines"][0]["g"]
    assert hands == g * BASE["n_lanes"]
    e.step()
    d2 = e.state_digest()
    assert len({d0, d1, d2}) == 3
    # the one blob in engines of other slicings: log_cap 3000 + 8192 and 3000 + 1024, one digest
    for slices, log_cap in ((1, 11192), (8, 4024)):
        t = pkg.engine.SelfPlayEngine.from_checkpoint(tmp_path / "wrapped.nfsp", slices=slices)
        assert t.memories(0)["log_cap"] == log_cap
        assert t.state_digest() == d1 == ck["header"]["digest"]
        assert t.stats()["hands"] == hands and t.stats()["rollouts"] == g * slices
    assert ck_mod.digest(ck["payload"]) == d1


def test_reslicing_keeps_the_payload(pkg, tmp_path):
    e = make(pkg, "slices4")
    step_until_meaningful(e)
    e.save(tmp_path / "s4.nfsp")
    hands = e.stats()["hands"]
    t = pkg.engine.SelfPlayEngine.from_checkpoint(tmp_path / "s4.nfsp", slices=2)
    t.save(tmp_path / "s2.nfsp")
    a, b = pkg.checkpoint.read(tmp_path / "s4.nfsp"), pkg.checkpoint.read(tmp_path / "s2.nfsp")
    assert np.array_equal(a["payload"], b["payload"])
    assert (a["header"]["slices"], b["header"]["slices"]) == (4, 2)
    t.step()
    st = t.stats()
    assert st["hands"] == hands + BASE["n_lanes"] and st["rollouts"] == 2 * (hands // BASE["n_lanes"] + 1)
    with pytest.raises(TypeError):
        pkg.engine.SelfPlayEngine.from_checkpoint(tmp_path / "s4.nfsp", n_lanes=1024)


def test_group_resume_restores_the_exchange_base(pkg, tmp_path):
    def group():
        return pkg.engine.EngineGroup(3, avg_ar=True, slices=2, seed=808, init_seed=6, **BASE)
    n2 = 2
    b = group()
    n1 = step_until_meaningful(b, probe=b.replicas[0])
    b.save(tmp_path / "g.nfsp")
    b.close()
    ck = pkg.checkpoint.read(tmp_path / "g.nfsp")
    assert ck["group"]["R"] == 3 and ck["group"]["w0_valid"] == pkg.native.XCHG_AR and ck["group"]["calls"] == 2 * n1
    assert np.array_equal(bits(ck["group"]["w0"][0]), bits(ck["engines"][1]["nets"][:, 0]))   # W0 == W_AR at a boundary
    c = pkg.engine.EngineGroup.from_checkpoint(tmp_path / "g.nfsp", init_seed=50)
    a = group()
    for _ in range(n1):
        a.step()
    assert a.state_digest() == c.state_digest() == [
        pkg.checkpoint.digest(replica_payload(ck, r)) for r in range(3)]
    for _ in range(n2):
        a.step()
        c.step()
    for r in range(3):
        assert np.array_equal(bits(nets(a.replicas[r])), bits(nets(c.replicas[r]))), r
    assert a.state_digest() == c.state_digest()
    # the averaged nets are common, the rest is each replica's own
    assert np.array_equal(nets(c.replicas[0])[0], nets(c.replicas[2])[0])
    assert len(set(c.state_digest())) == 3


def test_group_resume_with_a_br_exchange(pkg, tmp_path):
    """A group exchanging AR and BR nets after every slice, saved, loaded and its exchange
    re-issued (the cadence is a session setting), continues as the uninterrupted run.  The
    re-issued nfsp_group_set_exchange must not start the BR exchange over: a broadcast of replica
    0's BR net takes its target net along, and the target nets are each replica's own (their
    syncs fall mid-call at each replica's own update count) -- asserted at the save, without
    which the case could not fail."""
    XB = pkg.native.XCHG_AR | pkg.native.XCHG_BR

    def group():
        g = pkg.engine.EngineGroup(3, slices=2, seed=909, init_seed=7, **BASE)
        g.set_exchange(XB, every=1)
        return g
    b = group()
    n1 = step_until_meaningful(b, probe=b.replicas[0])
    torch.cuda.synchronize()
    at_save = [nets(e) for e in b.replicas]              # [a * 3 + net]
    for r in (1, 2):
        for a in (0, 1):
            assert np.array_equal(bits(at_save[r][3 * a]), bits(at_save[0][3 * a]))            # one AR net
            assert np.array_equal(bits(at_save[r][3 * a + 1]), bits(at_save[0][3 * a + 1]))    # one BR net
            assert not np.array_equal(bits(at_save[r][3 * a + 2]), bits(at_save[0][3 * a + 2]))   # own targets
    b.save(tmp_path / "g.nfsp")
    b.close()
    ck = pkg.checkpoint.read(tmp_path / "g.nfsp")
    assert ck["group"]["R"] == 3 and ck["group"]["w0_valid"] == XB and ck["group"]["calls"] == 2 * n1
    c = pkg.engine.EngineGroup.from_checkpoint(tmp_path / "g.nfsp", init_seed=50)
    c.set_exchange(XB, every=1)
    a = group()
    for _ in range(n1):
        a.step()
    assert a.state_digest() == c.state_digest()
    for step in range(2):
        a.step()
        c.step()
        torch.cuda.synchronize()
        for r in range(3):
            na, nc = nets(a.replicas[r]), nets(c.replicas[r])
            for k in range(6):
                d = np.flatnonzero(na[k].view(np.uint32) != nc[k].view(np.uint32))
                assert not len(d), (f"step {step} replica {r} agent {k // 3} net {('AR', 'BR', 'target')[k % 3]} "
                                    f"index {d[0]}: {na[k][d[0]]!r} uninterrupted, {nc[k][d[0]]!r} resumed")
    assert a.state_digest() == c.state_digest()
    assert len(set(c.state_digest())) == 3
    # on, off, on after a load still starts over: replica 0's BR and target nets everywhere
    c.set_exchange(XB, every=0)
    c.step()
    c.set_exchange(XB, every=1)
    torch.cuda.synchronize()
    w_r0 = nets(c.replicas[0])
    c.average_ar()
    torch.cuda.synchronize()
    for r in (1, 2):
        assert np.array_equal(bits(nets(c.replicas[r])), bits(w_r0))
    a.close()
    c.close()
    # a load honours the blob's W0 only while the nets are the blob's: after a step without the
    # exchange (the replicas' nets apart) a set_exchange starts over
    d = pkg.engine.EngineGroup.from_checkpoint(tmp_path / "g.nfsp", init_seed=51)
    d.step()
    d.set_exchange(XB, every=1)
    torch.cuda.synchronize()
    w_r0 = nets(d.replicas[0])
    assert not np.array_equal(bits(nets(d.replicas[1])[1]), bits(w_r0[1]))
    d.average_ar()
    torch.cuda.synchronize()
    for r in (1, 2):
        assert np.array_equal(bits(nets(d.replicas[r])), bits(w_r0))
    d.close()


def test_exchange_continues_after_a_load(pkg, tmp_path):
    """A host-callback exchange that is not the identity (S = 2 D, scale 0.75, every slice):
    re-issued after the load, the continuation is the uninterrupted run's."""
    wrap = pkg.native.wrap_device

    def doubling(_user, ptr, n):
        try:
            wrap(ptr, n, torch.float32, torch.device("cuda", torch.cuda.current_device())).mul_(2.0)
            torch.cuda.synchronize()
            return 0
        except BaseException:
            return 1
    fn = pkg.native.EXCHANGE_FN(doubling)
    kw = dict(slices=2, slice_lag=2)
    a, b = make(pkg, "unsliced", **kw), make(pkg, "unsliced", **kw)
    for e in (a, b):
        e.set_exchange(1, 0.75, fn=fn)
    n1 = step_until_meaningful(b)
    b.save(tmp_path / "x.nfsp")
    assert b.exchanges() == 2 * n1
    b.close()
    c = pkg.engine.SelfPlayEngine.from_checkpoint(tmp_path / "x.nfsp")
    c.set_exchange(1, 0.75, fn=fn)
    for _ in range(n1):
        a.step()
    for _ in range(2):
        a.step()
        c.step()
    assert c.exchanges() == 4
    assert_same_state(a, c, "exchange")
    # the exchange mattered: without it the AR nets differ
    d = make(pkg, "unsliced", **kw)
    for _ in range(n1 + 2):
        d.step()
    assert not np.array_equal(nets(a)[0], nets(d)[0])


def test_refusals_leave_the_engine_as_it_was(pkg, tmp_path):
    nat = pkg.native
    e = make(pkg, "unsliced")
    e.step()
    e.step()
    good = tmp_path / "good.nfsp"
    e.save(good)
    before = e.state_digest()
    w_before = nets(e)
    # a blob of an engine that differs in one field the state depends on
    others = {"n_lanes": dict(n_lanes=1024), "sl_capacity": dict(sl_capacity=700), "seed": dict(seed=4243),
              "quirks": dict(quirks=nat.QUIRKS_REFERENCE & ~nat.QUIRK_ALIAS_RL)}
    for field, over in others.items():
        o = make(pkg, "unsliced", **over)
        o.save(tmp_path / "o.nfsp")
        o.close()
        with pytest.raises(nat.NativeError, match=field):
            e.load(tmp_path / "o.nfsp")
        assert e.state_digest() == before, field
    o = pkg.engine.SelfPlayEngine(init_seed=3, game=nat.GAME_KUHN, seed=4242, **BASE)
    o.save(tmp_path / "o.nfsp")
    o.close()
    with pytest.raises(nat.NativeError, match="game"):
        e.load(tmp_path / "o.nfsp")
    # one corrupted payload byte
    raw = bytearray(good.read_bytes())
    raw[len(raw) // 2] ^= 0x40
    (tmp_path / "bad.nfsp").write_bytes(bytes(raw))
    with pytest.raises(nat.NativeError, match="digest"):
        e.load(tmp_path / "bad.nfsp")
    # a group's file into an engine
    g = pkg.engine.EngineGroup(2, seed=4242, init_seed=3, **BASE)
    g.save(tmp_path / "grp.nfsp")
    with pytest.raises(nat.NativeError, match="group"):
        e.load(tmp_path / "grp.nfsp")
    with pytest.raises(nat.NativeError, match="single engine"):
        g.load(good)
    g.close()
    assert e.state_digest() == before and np.array_equal(bits(nets(e)), bits(w_before))
    # mid-step: a rollout whose update has not run
    e.rollout()
    for call in (lambda: e.save(tmp_path / "mid.nfsp"), e.state_digest, lambda: e.load(good)):
        with pytest.raises(nat.NativeError, match="step boundary"):
            call()
    assert not (tmp_path / "mid.nfsp").exists() and not (tmp_path / "mid.nfsp.tmp").exists()
    e.update()
    assert e.state_digest() != before
    # and the good file still loads: back to the saved state
    e.load(good)
    assert e.state_digest() == before and np.array_equal(bits(nets(e)), bits(w_before))


def test_the_readers_of_the_memories_agree(pkg):
    """The digest, the checkpoint's writer and loader and the memory tables read one view of the
    memories (csrc/mem_view.h): at every step boundary the blob's RL and SL sections, counted by
    the raw table form, are the engine form's tables, and the device digest is the blob's --
    before the log is full, after it has wrapped, and in an engine of another log_cap."""
    import memtab_ref as mr
    ck, ev = pkg.checkpoint, pkg.evaluation
    ctx, tree = mr.ctx_of(pkg, "leduc")
    kw = dict(n_lanes=256, rl_capacity=1024, sl_capacity=2048, eta=0.3, seed=77)

    def agree(eng, blob):
        p = ck.parse(blob)
        assert eng.state_digest() == p["header"]["digest"]
        for kind, key in ((mr.RL, "rl"), (mr.SL, "sl")):
            out, infos = None, []
            for seat in (0, 1):                 # the agent's slice of the section, oldest first
                recs = p["engines"][0][key][seat].copy()
                words = recs.view(np.uint32).reshape(-1, recs.dtype.itemsize // 4)
                out, info = ev.memory_table(ctx, kind, seat, [mr.dev(words)] if len(words) else [], out=out, tree=tree)
                assert info["records"] == len(recs)
                infos.append(info)
            t, tinfo = eng.memory_table(kind)
            assert tinfo == infos
            assert np.array_equal(t.raw, out.cpu().numpy())

    e = pkg.engine.SelfPlayEngine(ctx, init_seed=3, slices=4, **kw)
    log_cap = e.memories(0)["log_cap"]
    assert log_cap == 1280
    totals = []
    for _ in range(6):
        e.step()
        blob = ck._blob(e)
        agree(e, blob)
        totals += e.stats()["rl_total"]
    print(f"rl_total per boundary and agent {totals}")
    assert min(totals) < kw["rl_capacity"] and max(totals) > log_cap
    t = pkg.engine.SelfPlayEngine(ctx, init_seed=5, slices=1, **kw)
    assert t.memories(0)["log_cap"] == 2048
    ck.load_bytes(t, blob)
    agree(t, blob)
    assert t.state_digest() == e.state_digest()
    t.close()
    e.close()

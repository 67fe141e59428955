"""The stream contract (include/nfsp.h: "All work is enqueued on the ctx's stream"), on a stream
that is not the null stream.

Every scenario runs twice (tests/stream_ref.py) and the two results are compared bit for bit:
twin A on the null stream, where the rest of the suite pins it to the oracles, and twin B inside
``torch.cuda.stream(s)`` for a side stream ``s`` -- the ctx, engines, groups and solvers are
created there and every call is made there.  In twin B each input a call consumes is written by
torch on ``s`` behind a delay (plain torch matmuls), over other valid contents, with no host
synchronisation before the call; the outputs are read the way the wrappers read them.  A launch
or copy on another stream, a synchronous null-stream copy standing in for an ordered one, or an
internal stream that is not joined back into ``s`` reads the old contents, and B differs from A.
No tolerance appears anywhere.

The delay is sized once per module against how late a wrongly-streamed kernel can start
(``delay`` fixture: busy >= 50 t_launch), and ``test_teeth`` shows the method detecting the one
deliberate race of the module.

Measured on an MI355X (the fixture prints both): busy = 3.684 ms for one delay of 4 matmuls
of 4096 x 4096 f32, t_launch = 30.8 us (the median of 20 wall-clock timings of nfsp_mlp_forward
with B = 1 followed by nfsp_synchronize on an idle ctx): busy / t_launch = 120.  In that run the
raced forward of ``test_teeth`` returned exactly the forward of the old contents (249 of 257
rows differ from twin A's).
"""
import contextlib
import ctypes as C
import statistics
import time

import numpy as np
import pytest
import torch

import stream_ref as sr

pytestmark = pytest.mark.gpu

F32 = np.float32
ENG = dict(n_lanes=1024, rl_capacity=3000, sl_capacity=2000, target_every=7)
GRP = dict(n_lanes=256, rl_capacity=3000, sl_capacity=2000, target_every=7)


# ---- fixtures ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nat(pkg, lib):
    return pkg.native


@pytest.fixture(scope="module")
def delay(pkg, nat):
    """The delay of every twin B, sized on the GPU: ``busy`` (event-timed) is at least 50 times
    ``t_launch``, an upper bound on how late a kernel on a wrong, idle stream can start after its
    call.  The work is grown until that holds; the assertion is the fixture's, not a skip."""
    d = sr.Delay()
    s = torch.cuda.Stream()
    ctx = nat.Context(1)
    w = torch.as_tensor(pkg.evaluation.glorot_net(np.random.RandomState(0)), device="cuda")
    x = torch.zeros((1, 30), dtype=torch.float32, device="cuda")
    y = torch.zeros((1, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ts = []
    for k in range(23):
        t0 = time.perf_counter()
        ctx.call("nfsp_mlp_forward", nat.ptr(w), 64, nat.ACT_RELU, nat.ptr(x), nat.ptr(y), 1)
        ctx.call("nfsp_synchronize")
        ts.append(time.perf_counter() - t0)
    t_launch = statistics.median(ts[3:])          # 20 timings, after 3 warm-up calls
    busy = d.busy_seconds(s)
    while busy < 50 * t_launch and d.reps < 1024:
        d.reps *= 2
        busy = d.busy_seconds(s)
    print(f"\nstream delay: busy {busy * 1e3:.3f} ms ({d.reps} matmuls), t_launch {t_launch * 1e6:.1f} us, "
          f"ratio {busy / t_launch:.0f}")
    ctx.close()
    assert busy >= 50 * t_launch, (busy, t_launch, d.reps)
    d.busy, d.t_launch = busy, t_launch
    return d


@pytest.fixture(scope="module")
def tree_side(pkg, nat, delay):
    """Scenario 5's shared ctxs (one per game and twin) and trees: twin B's ctxs are created on
    the module's side stream, where all of scenario 5's twin B runs."""
    s = torch.cuda.Stream()
    trees = {g: pkg.evaluation.GameTree.of(g) for g in (nat.GAME_LEDUC, nat.GAME_KUHN)}
    a = {g: nat.Context(1, game=g) for g in trees}
    with torch.cuda.stream(s):
        b = {g: nat.Context(1, game=g) for g in trees}
    torch.cuda.synchronize()
    yield {"stream": s, "trees": trees, False: a, True: b}
    torch.cuda.synchronize()
    for c in list(a.values()) + list(b.values()):
        c.close()


def both(scenario, delay, *args, **kw):
    a, b = sr.twins(scenario, delay, *args, **kw)
    sr.same(a, b)
    return a


def tree_both(scenario, delay, tree_side, game, *args):
    """A scenario of the shared ctxs: ``scenario(T, ctx, tree, ...)`` on the twin's own ctx."""
    def go(T, *a):
        return scenario(T, tree_side[T.side][game], tree_side["trees"][game], *a)
    return both(go, delay, *args, stream=tree_side["stream"])


def glorot(pkg, seed, hidden=64):
    return pkg.evaluation.glorot_net(np.random.RandomState(seed), hidden)


def obs(rng, n):
    return (rng.rand(n, 30) < 0.3).astype(F32)


def random_policy(tree, seed):
    """A valid policy table [ndec, 3, 3] f64: positive rows summing to 1 over the legal actions."""
    rng = np.random.RandomState(seed)
    t = rng.rand(tree.ndec, 3, 3) + 0.05
    t[~np.asarray(tree.legal, bool), :, 2] = 0.0
    return t / t.sum(axis=2, keepdims=True)


# ---- 1. stand-alone kernels -------------------------------------------------------------------
def forward_inputs(pkg):
    rng = np.random.RandomState(11)
    return dict(w_old=glorot(pkg, 1), w_new=glorot(pkg, 2), x_old=obs(rng, 257), x_new=obs(rng, 257))


def sc_forward(T, pkg, act):
    nat = pkg.native
    d = forward_inputs(pkg)
    w, x, W, X = T.dev(d["w_old"]), T.dev(d["x_old"]), T.dev(d["w_new"]), T.dev(d["x_new"])
    y = T.dev(np.full((257, 3), -1.0, F32))
    T.ready()
    ctx = nat.Context(1)            # after the setup's last synchronisation: nothing drains the device before the call
    T.put(w, W)
    T.put(x, X)
    ctx.call("nfsp_mlp_forward", nat.ptr(w), 64, act, nat.ptr(x), nat.ptr(y), 257)
    out = y.cpu().numpy()
    T.ready()
    ctx.close()
    return out


@pytest.mark.parametrize("act", ["relu", "softmax"])
def test_mlp_forward(pkg, nat, delay, act):
    y = both(sc_forward, delay, pkg, {"relu": nat.ACT_RELU, "softmax": nat.ACT_SOFTMAX}[act])
    assert np.isfinite(y).all() and y.any()


def test_teeth(pkg, nat, delay):
    """The one deliberate race: the ctx is bound to a second side stream while the producer runs
    on the first.  The forward then reads what w and x held before (valid, finite contents of
    valid allocations), and the result differs from twin A's -- the difference every other test
    of this module asserts the absence of."""
    a = sr.run(sc_forward, sr.Twin(), pkg, nat.ACT_RELU)
    d = forward_inputs(pkg)
    s, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    T = sr.Twin(delay, s)
    with torch.cuda.stream(s2):
        ctx = nat.Context(1)
    with torch.cuda.stream(s):
        w, x, W, X = T.dev(d["w_old"]), T.dev(d["x_old"]), T.dev(d["w_new"]), T.dev(d["x_new"])
        y = T.dev(np.full((257, 3), -1.0, F32))
    T.ready()
    with torch.cuda.stream(s):
        T.put(w, W)
        T.put(x, X)
    with torch.cuda.stream(s2):
        ctx.call("nfsp_mlp_forward", nat.ptr(w), 64, nat.ACT_RELU, nat.ptr(x), nat.ptr(y), 257)
        raced = y.cpu().numpy()
    torch.cuda.synchronize()
    # what a forward of the old contents gives, for the report
    w0, x0 = T.dev(d["w_old"]), T.dev(d["x_old"])
    ctx.call("nfsp_mlp_forward", nat.ptr(w0), 64, nat.ACT_RELU, nat.ptr(x0), nat.ptr(y), 257)
    torch.cuda.synchronize()
    stale = y.cpu().numpy()
    ctx.close()
    print("\nteeth: the raced forward equals the all-stale one:", np.array_equal(raced, stale),
          "; rows differing from twin A:", int((raced != a).any(axis=1).sum()), "of 257")
    assert np.isfinite(raced).all()
    assert sr.differs(a, raced), "a forward on another stream than its producer's went unnoticed"


def sc_fit(T, pkg, act):
    nat = pkg.native
    rng = np.random.RandomState(21)
    n, bs, ep = 70, 32, 2
    w, W = T.dev(glorot(pkg, 3)), T.dev(glorot(pkg, 4))
    x, X = T.dev(obs(rng, n)), T.dev(obs(rng, n))
    t, Tt = T.dev(rng.rand(n, 3).astype(F32)), T.dev(rng.rand(n, 3).astype(F32))
    p, Pm = (T.dev(np.stack([rng.permutation(n) for _ in range(ep)]).astype(np.int32)) for _ in range(2))
    T.ready()
    ctx = nat.Context(1)
    for dst, src in ((w, W), (x, X), (t, Tt), (p, Pm)):
        T.put(dst, src)
    ctx.call("nfsp_mlp_fit", nat.ptr(w), 64, act, nat.ptr(x), nat.ptr(t), n, nat.ptr(p), ep, bs, nat.F32(0.05))
    out = w.cpu().numpy()
    T.ready()
    ctx.close()
    return out


@pytest.mark.parametrize("act", ["relu", "softmax"])
def test_mlp_fit(pkg, nat, delay, act):
    w = both(sc_fit, delay, pkg, {"relu": nat.ACT_RELU, "softmax": nat.ACT_SOFTMAX}[act])
    assert np.isfinite(w).all() and not np.array_equal(w, glorot(pkg, 4))


def sc_br_targets(T, pkg):
    nat = pkg.native
    rng = np.random.RandomState(31)
    n = 129

    def draw():
        return [glorot(pkg, rng.randint(1 << 30)), obs(rng, n), rng.rand(n, 3).astype(F32),
                rng.randint(-6, 7, n).astype(F32) * F32(0.5), obs(rng, n), (rng.rand(n) < 0.4).astype(np.uint8)]
    bufs, srcs = [T.dev(a) for a in draw()], [T.dev(a) for a in draw()]
    out = T.dev(np.full((n, 3), -1.0, F32))
    expl = T.dev(np.full(1, -1.0, np.float64))
    T.ready()
    ctx = nat.Context(1)
    for dst, src in zip(bufs, srcs):
        T.put(dst, src)
    w, s, a, r, s2, t = bufs
    ctx.call("nfsp_br_targets", nat.ptr(w), 64, nat.ptr(s), nat.ptr(a), nat.ptr(r), nat.ptr(s2), nat.ptr(t), n,
             nat.F64(0.95), 3, nat.ptr(out), nat.ptr(expl))
    res = (out.cpu().numpy(), expl.cpu().numpy())
    T.ready()
    ctx.close()
    return res


def test_br_targets(pkg, delay):
    out, expl = both(sc_br_targets, delay, pkg)
    assert np.isfinite(out).all() and expl[0] >= 0.0 and (out != -1.0).all()


def sc_env(T, pkg):
    nat = pkg.native
    rng = np.random.RandomState(41)
    n = 300

    def deals():
        r = rng.randint(3, size=(n, 3))
        same3 = (r[:, 0] == r[:, 1]) & (r[:, 1] == r[:, 2])
        r[same3, 2] = (r[same3, 2] + 1) % 3           # a deck holds two cards of a rank
        return r.astype(np.uint8)

    def acts():
        return rng.rand(n, 3).astype(F32)
    dealer_h = [rng.randint(2, size=n).astype(np.uint8) for _ in range(2)]
    ranks, RANKS = T.dev(deals()), T.dev(deals())
    dealer, DEALER = T.dev(dealer_h[0]), T.dev(dealer_h[1])
    act = T.dev(acts())
    ACTS = [T.dev(acts()) for _ in range(6)]
    pl = T.dev(dealer_h[0])
    PL = [T.dev(dealer_h[1] ^ np.uint8(k & 1)) for k in range(6)]
    o = dict(s=T.dev(np.full((n, 30), -1.0, F32)), a=T.dev(np.full((n, 3), -1.0, F32)), r=T.dev(np.full(n, -1.0, F32)),
             s2=T.dev(np.full((n, 30), -1.0, F32)), t=T.dev(np.full(n, 9, np.uint8)), fold=T.dev(np.full(n, 9, np.uint8)),
             status=T.dev(np.full(n, 9, np.int8)), rnd=T.dev(np.full(n, 9, np.uint8)),
             hands=T.dev(np.full((n, 64), 0xAB, np.uint8)), mid=T.dev(np.full((n, 64), 0xAB, np.uint8)),
             first=T.dev(np.full((n, 64), 0xAB, np.uint8)))
    T.ready()
    # the ctx after the setup's last synchronisation, and a first hand straight after its creation
    # (no delay): these calls write the hands that nfsp_create has just cleared
    ctx = nat.Context(n, seed=5)
    ctx.call("nfsp_env_set_deal", nat.ptr(ranks))
    ctx.call("nfsp_env_reset", nat.ptr(dealer))
    ctx.call("nfsp_env_step", nat.ptr(act), 0, nat.ptr(pl), None)
    ctx.call("nfsp_env_export", nat.ptr(o["first"]))
    T.put(ranks, RANKS)
    ctx.call("nfsp_env_set_deal", nat.ptr(ranks))
    T.put(dealer, DEALER)
    ctx.call("nfsp_env_reset", nat.ptr(dealer))
    for k in range(5):
        T.put(pl, PL[k])
        T.put(act, ACTS[k])
        ctx.call("nfsp_env_step", nat.ptr(act), 0, nat.ptr(pl), None)
        if k == 1:
            ctx.call("nfsp_env_export", nat.ptr(o["mid"]))
            ctx.call("nfsp_env_round_status", nat.ptr(o["status"]))
            ctx.call("nfsp_env_round", nat.ptr(o["rnd"]))
    T.put(pl, PL[5])
    ctx.call("nfsp_env_get_state", 0, nat.ptr(pl), nat.ptr(o["s"]), nat.ptr(o["a"]), nat.ptr(o["r"]), nat.ptr(o["s2"]),
             nat.ptr(o["t"]))
    T.put(act, ACTS[5])
    ctx.call("nfsp_env_do_action", nat.ptr(act), 0, nat.ptr(pl), None, nat.ptr(o["fold"]))
    ctx.call("nfsp_env_export", nat.ptr(o["hands"]))
    res = {k: v.cpu().numpy() for k, v in o.items()}
    T.ready()
    ctx.close()
    return res


def test_env(pkg, delay):
    res = both(sc_env, delay, pkg)
    assert res["t"].max() <= 1 and set(np.unique(res["status"]).tolist()) <= {-1, 0, 1}
    assert not (res["hands"] == 0xAB).all() and not np.array_equal(res["hands"], res["mid"])


def sc_buf(T, pkg):
    nat = pkg.native
    rng = np.random.RandomState(51)
    cap, n, k = 500, 64, 96
    ctx = nat.Context(1)
    tab = pkg.buffers._Table

    def fill(t, rows):
        for col, a in zip((t.s, t.a, t.r, t.s2, t.t), rows):
            col.copy_(T.dev(a))

    def rows(m):
        return [obs(rng, m), rng.rand(m, 3).astype(F32), rng.randn(m).astype(F32), obs(rng, m),
                (rng.rand(m) < 0.5).astype(np.uint8)]
    dst, stage, out, prime = tab(cap, True, "cuda"), tab(n, True, "cuda"), tab(k, True, "cuda"), tab(cap, True, "cuda")
    fill(dst, rows(cap))
    fill(stage, rows(n))
    fill(out, rows(k))
    NEW = [T.dev(a) for a in rows(n)]

    def slots_of():
        s = rng.randint(cap, size=n).astype(np.int64)
        s[n // 2:] = s[:n - n // 2][::-1]           # every slot twice: the last writer wins
        s[5] = s[6] = s[7]                          # and one three times
        return s
    slots, SLOTS = T.dev(slots_of()), T.dev(slots_of())
    idx, IDX = T.dev(rng.randint(cap, size=k).astype(np.int64)), T.dev(np.concatenate(
        [rng.randint(cap, size=k - 8), [0, 0, cap - 1, cap - 1, 7, 7, 7, 7]]).astype(np.int64))
    # The ctx's per-row scratch grows on the first insert into a table larger than any before, and
    # that path synchronises the ctx stream.  A priming insert into another table of dst's capacity
    # takes it here, in the setup: the insert under test launches with nothing waited for.
    ctx.call("nfsp_buf_insert", C.byref(prime.rec), C.byref(stage.rec), nat.ptr(slots), n)
    T.ready()
    for col, src in zip((stage.s, stage.a, stage.r, stage.s2, stage.t), NEW):
        T.put(col, src)
    T.put(slots, SLOTS)
    ctx.call("nfsp_buf_insert", C.byref(dst.rec), C.byref(stage.rec), nat.ptr(slots), n)
    T.put(idx, IDX)
    ctx.call("nfsp_buf_sample", C.byref(dst.rec), nat.ptr(idx), k, C.byref(out.rec))
    res = [[c.cpu().numpy() for c in (t.s, t.a, t.r, t.s2, t.t)] for t in (out, dst)]
    T.ready()
    ctx.close()
    return res


def test_buffers(pkg, delay):
    both(sc_buf, delay, pkg)


# ---- 2. one engine ----------------------------------------------------------------------------
SLOTS6 = [(a, n) for a in (0, 1) for n in (0, 1, 2)]


def engine_outputs(eng, first="w"):
    """Read the way the wrappers read, straight after the last call: the weights, the memories, the
    digest and the stats.  Every one of these reads waits on the host, so only the first meets a
    busy stream; ``first`` names the one that goes first, the others keep their order."""
    def mem():
        return [{k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in eng.memories(a).items()}
                for a in (0, 1)]
    reads = {"w": lambda: [eng.get_weights(a, n) for a, n in SLOTS6], "mem": mem,
             "digest": lambda: np.array(eng.state_digest(), np.uint64), "stats": eng.stats}
    return {k: reads[k]() for k in [first] + [k for k in reads if k != first]}


# which read meets the busy stream in which variant (the others: the weights, the issue's order)
FIRST_READ = {"textbook": "stats", "sliced": "digest", "act_table": "mem"}


def new_nets(pkg, T, seed):
    rng = np.random.RandomState(seed)
    host = []
    for a in (0, 1):
        ar, br = pkg.evaluation.glorot_net(rng), pkg.evaluation.glorot_net(rng)
        host += [ar, br, br.copy()]
    return host, [T.dev(w) for w in host]


def write_nets(T, eng, host, src):
    """All six nets after a delay each: the first through the wrapper (a pageable copy), the
    others device to device with nothing between the last write and the next call."""
    T.delay()
    eng.set_weights(0, 0, host[0])
    for (a, n), s in list(zip(SLOTS6, src))[1:]:
        T.put(eng.weights_tensor(a, n), s)


def sc_engine(T, pkg, variant):
    nat = pkg.native
    kw = dict(ENG, seed=4242)
    if variant == "textbook":
        kw["quirks"] = nat.TEXTBOOK_MSE
    if variant in ("sliced", "exchange"):
        kw.update(slices=4 if variant == "sliced" else 2, slice_lag=2)
    eng = pkg.engine.SelfPlayEngine(init_seed=3, **kw)
    host, src = new_nets(pkg, T, 17)
    tree = pkg.evaluation.GameTree.of(nat.GAME_LEDUC)
    rows = T.dev(pkg.evaluation.act_rows(tree.uniform()).numpy())
    ROWS = T.dev(pkg.evaluation.act_rows(random_policy(tree, 5)).numpy())
    late = T.dev(glorot(pkg, 99))
    fn = None
    if variant == "exchange":
        def doubling(user, ptr, n):
            try:        # S = 2 D on the current stream, as a two-shard sum of equal shards
                nat.wrap_device(ptr, n, torch.float32, torch.device("cuda", torch.cuda.current_device())).mul_(2.0)
                torch.cuda.current_stream().synchronize()
                return 0
            except BaseException:
                return 1
        fn = nat.EXCHANGE_FN(doubling)
    if variant == "losses":
        eng.set_loss_log(True)
    T.ready()
    write_nets(T, eng, host, src)
    if variant == "exchange":
        eng.set_exchange(1, 0.75, fn=fn)
    out = {}
    for k in range(3):
        if k == 2:      # a producer in mid-run: the last call's chains may still be in flight
            T.put(eng.weights_tensor(1, nat.NET_AR), late)
        if variant in ("sliced", "exchange"):
            eng.step()
            continue
        if variant == "rollout_with" and k == 0:
            T.delay()
            eng.rollout_with(np.concatenate(host[::-1]), (0.25, 0.5))
        elif variant == "act_table" and k == 1:
            T.put(rows, ROWS)
            eng.set_act_table(1, nat.NET_BR, rows)
            eng.rollout()
        else:
            eng.rollout()
        eng.update()
    if variant == "losses":             # straight after the last update: its copy is a synchronous one
        out["losses"] = eng.losses()
    out.update(engine_outputs(eng, FIRST_READ.get(variant, "w")))
    if variant == "exchange":
        out["exchanges"] = eng.exchanges()
    if variant == "reference":      # scenario 5's memory tables, on these memories (the stream is idle by now)
        out["tables"] = [eng.memory_table(nat.MEM_SL)[0].raw, eng.memory_table(nat.MEM_RL)[0].raw, eng.td_table()[0].raw]
        out["table_info"] = [eng.memory_table(nat.MEM_SL)[1], eng.td_table()[1]]
        out["exploitability"] = [eng.exploitability(mode) for mode in (0, 1)]
        out["br_gap"] = eng.br_gap()
        q, tdq, info, changed = eng.tabular_q()
        out["tabular_q"] = [q.cpu().numpy(), tdq.raw, info, changed]
    T.ready()
    eng.close()
    return out


@pytest.mark.parametrize("variant", ["reference", "textbook", "sliced", "losses", "rollout_with", "exchange", "act_table"])
def test_engine(pkg, delay, variant):
    out = both(sc_engine, delay, pkg, variant)
    st = out["stats"]
    assert st["hands"] == 3 * ENG["n_lanes"] and min(st["br_updates"]) > 0 and min(st["ar_updates"]) > 0
    if variant == "exchange":
        assert out["exchanges"] == 6
    if variant == "reference":
        assert all(t.any() for t in out["tables"])


# ---- 3. an engine group -----------------------------------------------------------------------
def sc_group(T, pkg, br_streams):
    nat = pkg.native
    g = pkg.engine.EngineGroup(3, slices=2, seed=808, init_seed=6, **GRP)
    if br_streams:
        g.set_sched(br_streams=br_streams)
    host, src = new_nets(pkg, T, 23)
    late = T.dev(glorot(pkg, 98))
    T.ready()
    for e in g.replicas[1:]:
        write_nets(T, e, host, src)
    g.set_exchange(nat.XCHG_AR, every=1)
    g.step()
    T.put(g.replicas[1].weights_tensor(0, nat.NET_BR), late)      # a producer in mid-run
    g.step()
    out = {"digests": np.array(g.state_digest(), np.uint64), "w": [e.get_weights(a, n) for e in g.replicas for a, n in SLOTS6],
           "stats": [e.stats() for e in g.replicas], "exploitability": g.exploitability_all(),
           "tables": [t.raw for t, _ in g.memory_tables(nat.MEM_RL)]}
    T.ready()
    g.close()
    return out


@pytest.mark.parametrize("br_streams", [0, 2])
def test_group(pkg, delay, br_streams):
    out = both(sc_group, delay, pkg, br_streams)
    assert len({tuple(d) for d in out["digests"]}) == 3
    assert all(s["hands"] == 2 * GRP["n_lanes"] and min(s["br_updates"]) > 0 for s in out["stats"])


# ---- 4. checkpoint ----------------------------------------------------------------------------
def sc_checkpoint(T, pkg, tmp, group):
    def make(init_seed):
        if group:
            return pkg.engine.EngineGroup(3, avg_ar=True, slices=2, seed=808, init_seed=init_seed, **GRP)
        return pkg.engine.SelfPlayEngine(init_seed=init_seed, seed=4242, **ENG)
    path = tmp / ("b.nfsp" if T.side else "a.nfsp")
    b = make(3)
    host, src = new_nets(pkg, T, 29)
    T.ready()
    write_nets(T, b.replicas[2] if group else b, host, src)
    b.step()
    b.step()
    b.save(path)                        # straight after the step: no host synchronisation first
    c = make(99)
    c.load(path)
    c.step()
    d = c.state_digest()
    out = {"file": path.read_bytes(), "digest": np.array(d, np.uint64),
           "w": [e.get_weights(a, n) for e in (c.replicas if group else [c]) for a, n in SLOTS6]}
    T.ready()
    b.close()
    c.close()
    return out


@pytest.mark.parametrize("group", [False, True], ids=["engine", "group"])
def test_checkpoint(pkg, delay, tmp_path, group):
    out = both(sc_checkpoint, delay, pkg, tmp_path, group)
    ck = pkg.checkpoint.parse(out["file"])
    assert len(ck["engines"]) == (3 if group else 1)
    if group:
        assert ck["group"]["w0_valid"] == pkg.native.XCHG_AR


# ---- 5. tree-side handles ---------------------------------------------------------------------
GAMES = pytest.mark.parametrize("game", [1, 0], ids=["kuhn", "leduc"])


def sc_heads(T, ctx, tree, pkg, hidden):
    nat, ev = pkg.native, pkg.evaluation
    nets = [T.dev(glorot(pkg, 40 + k, hidden)) for k in range(3)]
    NEW = [T.dev(glorot(pkg, 50 + k, hidden)) for k in range(3)]
    T.ready()
    for w, s in zip(nets, NEW):
        T.put(w, s)
    out = ev.head_tables(ctx, nets, [nat.ACT_RELU, nat.ACT_SOFTMAX, nat.ACT_LINEAR], tree).cpu().numpy()
    T.ready()
    return out


@GAMES
@pytest.mark.parametrize("hidden", [16, 64])
def test_head_tables(pkg, delay, tree_side, game, hidden):
    z = tree_both(sc_heads, delay, tree_side, game, pkg, hidden)
    assert np.isfinite(z).all() and z.any()


def sc_evaluators(T, ctx, tree, pkg):
    ev = pkg.evaluation
    w_ar, w_br = T.dev(glorot(pkg, 60)), T.dev(glorot(pkg, 61))
    tab = T.dev(tree.uniform())
    W_AR, W_AR2, W_BR = T.dev(glorot(pkg, 62)), T.dev(glorot(pkg, 65)), T.dev(glorot(pkg, 63))
    TAB, TAB2 = T.dev(random_policy(tree, 64)), T.dev(random_policy(tree, 66))
    p_ar, p_br, p_tab = ev.Policy.ar(w_ar), ev.Policy.br(w_br), ev.Policy.table(tab)
    assert p_ar.ptr == w_ar.data_ptr() and p_tab.ptr == tab.data_ptr()      # the policies read the buffers in place
    T.ready()
    out = {}
    T.put(w_ar, W_AR)
    out["policy_ar"] = ev.policy_table(ctx, p_ar, tree).cpu().numpy()
    T.put(w_br, W_BR)
    out["policy_br"] = ev.policy_table(ctx, p_br, tree).cpu().numpy()
    T.put(w_ar, W_AR2)
    T.put(tab, TAB)
    out["evaluate"] = ev.evaluate_batch(ctx, [(p_ar, p_tab), (p_tab, p_br), (p_tab, p_tab)])
    T.put(tab, TAB2)
    T.put(w_ar, W_AR)
    beta, q, reach = ev.best_response(ctx, p_ar, p_tab, values=True, tree=tree)
    out["best_response"] = [beta.cpu().numpy(), q.cpu().numpy(), reach.cpu().numpy()]
    T.ready()
    return out


@GAMES
def test_evaluators(pkg, delay, tree_side, game):
    out = tree_both(sc_evaluators, delay, tree_side, game, pkg)
    assert out["policy_ar"].any() and out["best_response"][0].any()


def sc_fit_tables(T, ctx, tree, pkg, hidden):
    nat, ev = pkg.native, pkg.evaluation
    heads = [(nat.ACT_SOFTMAX, "ce"), (nat.ACT_RELU, "huber"), (nat.ACT_LINEAR, "mse")]
    ws = [T.dev(glorot(pkg, 70 + k, hidden)) for k in range(3)]
    WS = [T.dev(glorot(pkg, 80 + k, hidden)) for k in range(3)]
    tg = [T.dev(random_policy(tree, 90 + k)) for k in range(3)]
    TG = [T.dev(random_policy(tree, 95 + k)) for k in range(3)]
    jobs = [ev.FitJob(ws[k], tg[k], k & 1, heads[k][0], heads[k][1], 0.1, 0.9) for k in range(3)]
    assert all(j.w.data_ptr() == ws[k].data_ptr() and j.target.data_ptr() == tg[k].data_ptr() for k, j in enumerate(jobs))
    T.ready()
    for dst, src in zip(ws + tg, WS + TG):
        T.put(dst, src)
    losses = ev.fit_tables(ctx, jobs, 4, tree)
    out = {"losses": losses, "w": [w.cpu().numpy() for w in ws]}
    T.ready()
    return out


@GAMES
@pytest.mark.parametrize("hidden", [64, 128])
def test_fit_tables(pkg, delay, tree_side, game, hidden):
    out = tree_both(sc_fit_tables, delay, tree_side, game, pkg, hidden)
    assert np.isfinite(out["losses"]).all() and (out["losses"] > 0).all()


def sc_table_rows(T, ctx, tree, pkg):
    nat, ev = pkg.native, pkg.evaluation
    rng = np.random.RandomState(101)

    def tabs():
        t = rng.randint(0, 1 << 20, size=(2, tree.ndec, 3, 3, 3)).astype(np.int64)
        t[rng.rand(2, tree.ndec, 3) < 0.2] = 0          # sets without records take the fill
        return t
    tab, fill = T.dev(tabs()), T.dev(rng.rand(2, tree.ndec, 3, 3).astype(F32))
    TABS = [T.dev(tabs()) for _ in range(3)]
    FILLS = [T.dev(rng.rand(2, tree.ndec, 3, 3).astype(F32)) for _ in range(3)]
    prev = T.dev(np.zeros((2, tree.ndec, 3, 3), F32))
    T.ready()
    out = {}
    for k, stat in enumerate((nat.ROWS_SL_MASS, nat.ROWS_SL_ARGMAX, nat.ROWS_TD_MEAN)):
        T.put(tab, TABS[k])
        T.put(fill, FILLS[k])
        rows, changed = ev.table_rows(ctx, stat, tab, fill, prev, tree)
        out[stat] = (rows.cpu().numpy(), changed)
    T.ready()
    return out


@GAMES
def test_table_rows(pkg, delay, tree_side, game):
    out = tree_both(sc_table_rows, delay, tree_side, game, pkg)
    assert all(np.isfinite(r).all() and min(c) > 0 for r, c in out.values())


def sc_tabular_solvers(T, ctx, tree, pkg):
    ev = pkg.evaluation
    out = {}
    cfr = ev.CfrSolver(ctx).run(10)
    out["cfr"] = [cfr.average_table(), *cfr.state()]
    xfp = ev.XfpSolver(ctx, [(0.0, "uniform"), (0.1, "linear")])
    out["xfp_gaps"] = xfp.run(5, gaps=True)
    out["xfp"] = [xfp.average_table(1), *xfp.state(1)]
    mx = ev.MccfrXSolver(ctx, [(7, 2, 0.6, "plus", "linear")], sampling=2).run(3)
    out["mccfr_x"] = [mx.average_table(0), *mx.state(0), mx.weighted(0), *mx.baseline(0), np.array(mx.counts(0))]
    T.ready()
    for s in (cfr, xfp, mx):
        s.close()
    return out


@GAMES
def test_tabular_solvers(pkg, delay, tree_side, game):
    out = tree_both(sc_tabular_solvers, delay, tree_side, game, pkg)
    assert out["cfr"][0].any() and out["mccfr_x"][1].any() and np.isfinite(out["xfp_gaps"]).all()


NET_CFG = [(9, 2, 0.0, "plain", "uniform", "avg", 1, "mse", 0.5, 0.9)]


def sc_mccfr_net(T, ctx, tree, pkg):
    ev = pkg.evaluation
    s = ev.MccfrNetSolver(ctx, NET_CFG, 0, [1])
    w0, W1 = glorot(pkg, 111), T.dev(glorot(pkg, 112))
    T.ready()
    T.delay()
    s.set_net(0, 0, w0)                     # the wrapper: writes, then synchronises the current stream
    T.put(s._net(0, 1)[0], W1)              # and a write with nothing between it and the run
    s.run(3)
    out = {"nets": [s.net(0, seat) for seat in (0, 1)], "sigma": s.sigma_table(0), "head": s.head(0),
           "state": s.state(0), "avg": s.average_table(0), "loss": s.fit_loss(0)}
    T.ready()
    s.close()
    return out


@GAMES
def test_mccfr_net(pkg, delay, tree_side, game):
    out = tree_both(sc_mccfr_net, delay, tree_side, game, pkg)
    assert out["state"][0].any() and np.isfinite(out["loss"]).all()


# ---- 6. rebinding -----------------------------------------------------------------------------
def sc_rebind_engine(T, pkg):
    """Not under ``T.on()``: the ctx and the engine are created on the null stream in both twins."""
    s2, s3 = (T.stream, torch.cuda.Stream()) if T.side else (None, None)
    eng = pkg.engine.SelfPlayEngine(init_seed=3, seed=4242, **ENG)
    host, src = new_nets(pkg, T, 37)
    late = T.dev(glorot(pkg, 97))
    T.ready()
    eng.step()
    with torch.cuda.stream(s2) if T.side else contextlib.nullcontext():
        if T.side:
            s2.wait_stream(torch.cuda.default_stream())
            eng.ctx.set_stream()
        write_nets(T, eng, host, src)
        eng.step()
        eng.step()
    with torch.cuda.stream(s3) if T.side else contextlib.nullcontext():
        if T.side:
            s3.wait_stream(s2)
            eng.ctx.set_stream()
        T.put(eng.weights_tensor(1, pkg.native.NET_BR), late)      # a rebinding that did not take would miss it
        eng.step()
        out = engine_outputs(eng)
    T.ready()
    eng.close()
    return out


def test_rebind_engine(pkg, delay):
    a = sc_rebind_engine(sr.Twin(), pkg)
    b = sc_rebind_engine(sr.Twin(delay, torch.cuda.Stream()), pkg)
    sr.same(a, b)
    assert a["stats"]["hands"] == 4 * ENG["n_lanes"]


def sc_rebind_solver(T, pkg):
    nat, ev = pkg.native, pkg.evaluation
    s2, s3 = (T.stream, torch.cuda.Stream()) if T.side else (None, None)
    ctx = nat.Context(1, game=nat.GAME_KUHN)
    s = ev.MccfrNetSolver(ctx, NET_CFG, 0, [1])
    W, late = T.dev(glorot(pkg, 121)), T.dev(glorot(pkg, 122))
    T.ready()
    s.run(1)
    with torch.cuda.stream(s2) if T.side else contextlib.nullcontext():
        if T.side:
            s2.wait_stream(torch.cuda.default_stream())
            ctx.set_stream()
        T.put(s._net(0, 0)[0], W)
        s.run(2)
    with torch.cuda.stream(s3) if T.side else contextlib.nullcontext():
        if T.side:
            s3.wait_stream(s2)
            ctx.set_stream()
        T.put(s._net(0, 1)[0], late)
        s.run(1)
        out = {"nets": [s.net(0, seat) for seat in (0, 1)], "state": s.state(0), "sigma": s.sigma_table(0)}
    T.ready()
    s.close()
    ctx.close()
    return out


def test_rebind_solver(pkg, delay):
    a = sc_rebind_solver(sr.Twin(), pkg)
    b = sc_rebind_solver(sr.Twin(delay, torch.cuda.Stream()), pkg)
    sr.same(a, b)
    assert a["state"][0].any()

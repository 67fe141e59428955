"""The exchange of nets between learners against its numpy restatement (tests/exchange_ref.py):

    W = W0 + (sum_r (W_r - W0)) * scale,   W0 = W      (replica order, from +0, no contraction)

a. k_group_xchg alone (nfsp_group_average_ar, no step): broadcast, deltas, zero deltas; AR, BR
   and both; R up to the unrolled replica loop plus a remainder; on, off and on again;
b. whole steps of a group with a BR exchange against standalone engines + GroupModel, at
   cadences that cross step boundaries;
c. the serial slice loop of nfsp_group_step at slice_lag 2 (a BR exchange, or sched serial);
d. k_xchg_delta / k_xchg_apply of one engine with a host callback standing for the other shards.
(e, the resume of a BR-exchanging group, is in test_gpu_checkpoint.py.)

Every comparison is on bits: the ABI promises bit-exactness, so there are no tolerances here.
torch writes (set_weights) and the library's launches are on different streams: a
torch.cuda.synchronize() stands between them."""
import numpy as np
import pytest
import torch

import exchange_ref as X
from engine_ref import STAT_KEYS, nets, weights_flat

pytestmark = pytest.mark.gpu

F = np.float32
AR, BR = X.XCHG_AR, X.XCHG_BR
TINY = dict(n_lanes=64, rl_capacity=200, sl_capacity=150)
SMALL = dict(n_lanes=1024, rl_capacity=3000, sl_capacity=2000, target_every=11)
NET_NAMES = ("AR", "BR", "target")


# ---- helpers --------------------------------------------------------------------------------
def read_all(engines):
    """[R][2 agents][3 nets][NP] of the engines' nets as they are once every stream is idle."""
    torch.cuda.synchronize()
    return np.stack([np.stack(nets(e)).reshape(2, 3, X.NP) for e in engines])


def write_all(engines, W, only=None):
    for r, e in enumerate(engines):
        for a in (0, 1):
            for n in (0, 1, 2):
                if only is None or only[n]:
                    e.set_weights(a, n, W[r, a, n])
    torch.cuda.synchronize()


def assert_nets(got, exp, what):
    """got, exp [R][2][3][NP]: equal bits, or the first differing replica, agent, net, index."""
    if X.same_bits(got, exp):
        return
    for r in range(got.shape[0]):
        for a in (0, 1):
            for n in (0, 1, 2):
                d = X.first_diff(got[r, a, n], exp[r, a, n])
                assert d is None, (what, f"replica {r} agent {a} net {NET_NAMES[n]} index {d[0]}",
                                   f"got {d[1]!r} expected {d[2]!r}")


def masked(nets_mask, broadcast=False):
    """Which of (AR, BR, target) an exchange of `nets_mask` writes."""
    return (bool(nets_mask & AR), bool(nets_mask & BR), bool(nets_mask & BR) and broadcast)


def first_write(W0, W):
    """Nets for the call that broadcasts: replica 0 holds the base, the others something else."""
    first = np.roll(W, 1, axis=0)
    first[0] = W0
    return first


def three_calls(g, model, R, nets_mask, scale):
    """a's three calls of nfsp_group_average_ar, each against the model and against the rule
    spelled out."""
    W0, W = X.make_nets(R)
    first = first_write(W0, W)
    # 1. the broadcast: masked nets are replica 0's (with BR the target too), the rest untouched
    write_all(g.replicas, first)
    g.average_ar()
    got = read_all(g.replicas)
    assert_nets(got, model.exchange(first), "broadcast")
    assert model.last_broadcast == nets_mask
    for n, on in enumerate(masked(nets_mask, True)):
        for r in range(R):
            assert X.same_bits(got[r, :, n], first[0 if on else r, :, n]), ("broadcast", r, NET_NAMES[n])
    # 2. every net rewritten: the rule against the broadcast W0; target and unmasked nets untouched
    write_all(g.replicas, W)
    g.average_ar()
    got2 = read_all(g.replicas)
    assert_nets(got2, model.exchange(W), "deltas")
    assert model.last_broadcast == 0
    for n, on in enumerate(masked(nets_mask, False)):
        for r in range(R):
            exp = X.group_exchange(W[:, :, n], W0[:, n], scale) if on else W[r, :, n]
            assert X.same_bits(got2[r, :, n], exp), ("deltas", r, NET_NAMES[n])
        zero = X.bits(got2[..., n, list(X.PLANT_NEG0_EQUAL)])
        assert np.all(zero == (0 if on else 0x80000000))        # -0.0 + (+0) = +0.0 where exchanged
    # 3. nothing rewritten: every delta is +0 and nothing moves
    g.average_ar()
    got3 = read_all(g.replicas)
    assert_nets(got3, model.exchange(got2), "zero deltas")
    assert_nets(got3, got2, "zero deltas leave the nets")


# ---- a. the group kernel alone ------------------------------------------------------------------
@pytest.mark.parametrize("R,nets_mask,scale", X.KERNEL_CASES,
                         ids=[f"R{R}-nets{m}-scale{float(s):.4g}" for R, m, s in X.KERNEL_CASES])
def test_group_kernel_against_the_rule(pkg, R, nets_mask, scale):
    g = pkg.engine.EngineGroup(R, seed=11, init_seed=1, **TINY)
    model = X.GroupModel(R)
    g.set_exchange(nets_mask, every=1, scale=float(scale))
    model.set_exchange(nets_mask, 1, scale)
    three_calls(g, model, R, nets_mask, scale)
    g.close()


@pytest.mark.parametrize("avg_ar", [False, True])
def test_group_kernel_with_no_exchange_configured(pkg, avg_ar):
    """nfsp_group_average_ar by itself (AR at the mean), and after NFSP_GROUP_AVG_AR."""
    R = 3
    g = pkg.engine.EngineGroup(R, seed=11, init_seed=1, avg_ar=avg_ar, **TINY)
    model = X.GroupModel(R, avg_ar_slices=1 if avg_ar else None)
    three_calls(g, model, R, AR, F(1) / F(R))
    g.close()


def test_group_kernel_on_off_on(pkg):
    """A net turned off and on again is broadcast again (BR with its target); a net that stayed
    on while the other was toggled goes on applying deltas against its W0.  GroupModel says
    which at every call."""
    R, scale = 3, F(0.75)
    g = pkg.engine.EngineGroup(R, seed=11, init_seed=1, **TINY)
    model = X.GroupModel(R)
    k = [0]

    def both(nets_mask, every):
        g.set_exchange(nets_mask, every=every, scale=float(scale))
        model.set_exchange(nets_mask, every, scale)

    def call(expect_broadcast, what):
        k[0] += 1
        W0, W = X.make_nets(R, X.SEED + k[0])
        W = first_write(W0, W)
        write_all(g.replicas, W)
        g.average_ar()
        exp = model.exchange(W)
        assert model.last_broadcast == expect_broadcast, what
        got = read_all(g.replicas)
        assert_nets(got, exp, what)
        return W, got

    both(AR | BR, 1)
    call(AR | BR, "both on: broadcast")
    call(0, "both on: deltas")
    both(AR, 1)                                   # BR off, AR stays
    W, got = call(0, "BR off: AR deltas go on")
    assert X.same_bits(got[:, :, 1:], W[:, :, 1:])
    assert not X.same_bits(got[:, :, 0], W[:, :, 0])
    both(AR | BR, 1)                              # BR on again
    W, got = call(BR, "BR on again: BR and target broadcast, AR deltas go on")
    for r in range(R):
        assert X.same_bits(got[r, :, 1:], W[0, :, 1:])
    assert not any(X.same_bits(got[0, :, 0], W[r, :, 0]) for r in range(R))
    call(0, "both on again: deltas")
    both(BR, 1)                                   # AR off, BR stays
    W, got = call(0, "AR off: BR deltas go on")
    assert X.same_bits(got[:, :, 0], W[:, :, 0]) and X.same_bits(got[:, :, 2], W[:, :, 2])
    both(AR | BR, 0)                              # all off ...
    assert model.nets == 0
    both(AR | BR, 1)                              # ... and on: everything starts over
    call(AR | BR, "all on again: broadcast")
    g.close()


def test_group_exchange_refusals(pkg):
    """Unknown bits in nets, and every > 0 without nets, are refused and change nothing."""
    R, scale = 2, F(0.5)
    g = pkg.engine.EngineGroup(R, seed=11, init_seed=1, **TINY)
    model = X.GroupModel(R)
    g.set_exchange(AR | BR, every=1, scale=float(scale))
    model.set_exchange(AR | BR, 1, scale)
    W0, W = X.make_nets(R)
    write_all(g.replicas, first_write(W0, W))
    g.average_ar()
    model.exchange(first_write(W0, W))
    for bad_nets, every in ((4, 1), (7, 1), (AR | 8, 0), (0, 1)):
        with pytest.raises(pkg.native.NativeError):
            g.set_exchange(bad_nets, every=every, scale=1.0)
        with pytest.raises(ValueError):
            model.set_exchange(bad_nets, every, 1.0)
    with pytest.raises(pkg.native.NativeError):
        g.set_exchange(AR, every=-1, scale=1.0)
    write_all(g.replicas, W)
    g.average_ar()                                # still AR | BR at 0.5 against the same W0
    assert_nets(read_all(g.replicas), model.exchange(W), "after the refusals")
    assert model.last_broadcast == 0
    g.close()


# ---- b, c. whole steps against standalone engines + GroupModel ---------------------------------
class Restated:
    """R standalone engines (seed + r, init_seed + r) stepped slice by slice, the group's exchange
    done by GroupModel in numpy and written back with set_weights -- test_group_ar_exchange's
    method, for any nets and cadence."""

    def __init__(self, pkg, R, model, seed, init_seed, **cfg):
        self.solo = [pkg.engine.SelfPlayEngine(seed=seed + r, init_seed=init_seed + r, **cfg) for r in range(R)]
        self.model, self.K = model, cfg.get("slices", 1)
        self.due = 0                  # exchanges the cadence made due
        self.delta_checks = 0

    def exchange(self):
        m = self.model
        W = read_all(self.solo)
        W0, valid = m.W0.copy(), m.w0_valid
        out = m.exchange(W)
        nets_mask = m.nets if m.nets else AR
        only = masked(nets_mask, bool(m.last_broadcast & BR))     # the target on a broadcast only
        for n in (0, 1, 2):
            if not only[n]:
                assert X.same_bits(out[:, :, n], W[:, :, n])
        write_all(self.solo, out, only)
        # nfsp.h's equality claim on these very nets: shards applying the honest sum of their
        # deltas, in rank order, hold what the group's exchange gives
        for n, bit in ((0, AR), (1, BR)):
            if nets_mask & bit & valid:
                S = X.sum_in_rank_order([X.shard_delta(W[r, :, n], W0[n]) for r in range(len(self.solo))])
                assert X.same_bits(X.shard_apply(W0[n], S, m.scale), out[0, :, n]), NET_NAMES[n]
                self.delta_checks += 1

    def step(self, lag2=False):
        """nfsp_group_step restated: common nets first where a net has no W0 yet; every slice its
        rollout, learner call and (when due) the exchange; at slice_lag 2 slice j acts with
        snapshot j & 1, the nets and epsilon slice j - 2's learner and exchange left."""
        if self.model.begin_step():
            self.exchange()
        snap = [[self.acting(e)] * 2 for e in self.solo] if lag2 else None
        for j in range(self.K):
            for r, e in enumerate(self.solo):
                if lag2:
                    e.rollout_with(*snap[r][j & 1])
                else:
                    e.rollout()
                e.update()
            if self.model.due():
                self.due += 1
                self.exchange()
            if lag2 and j + 2 < self.K:
                for r, e in enumerate(self.solo):
                    snap[r][j & 1] = self.acting(e)

    @staticmethod
    def acting(e):
        eps = tuple(float(v) for v in e.stats()["epsilon"])      # (synchronises)
        torch.cuda.synchronize()
        return weights_flat(e), eps

    def close(self):
        for e in self.solo:
            e.close()


def assert_same_run(engines, ref, what):
    got, exp = read_all(engines), read_all(ref.solo)
    assert_nets(got, exp, what)
    for r, (x, y) in enumerate(zip(engines, ref.solo)):
        sx, sy = x.stats(), y.stats()
        for k in STAT_KEYS:
            assert sx[k] == sy[k], (what, r, k, sx[k], sy[k])
    return got


STEP_CASES = [(slices, every, nm, gain)
              for slices, every in ((1, 1), (4, 1), (4, 2), (4, 3))
              for nm, gain in ((AR | BR, 2.0), (BR, 1.0))] + [(4, 3, AR | BR, 1.0), (4, 3, BR, 2.0)]


@pytest.mark.parametrize("slices,every,nets_mask,gain", STEP_CASES)
def test_group_steps_with_a_br_exchange(pkg, slices, every, nets_mask, gain):
    R, steps = 3, 3
    cfg = dict(SMALL, slices=slices)
    g = pkg.engine.EngineGroup(R, seed=99, init_seed=0, **cfg)
    g.set_exchange(nets_mask, every=every, scale=gain / R)
    model = X.GroupModel(R)
    model.set_exchange(nets_mask, every, F(gain / R))
    ref = Restated(pkg, R, model, seed=99, init_seed=0, **cfg)
    for step in range(steps):
        g.step()
        ref.step()
        got = assert_same_run(g.replicas, ref, f"step {step}")
    assert ref.due == steps * slices // every          # 4 slices, every 3: 3 steps give 4 exchanges
    assert model.exchanges == ref.due + 1 and ref.delta_checks >= ref.due
    # not vacuous: the BR nets are one net, the target nets each replica's own (its syncs fall at
    # its own update counts), and there were several syncs
    for r in range(1, R):
        assert X.same_bits(got[r, :, 1], got[0, :, 1])
        assert not X.same_bits(got[r, :, 2], got[0, :, 2])
        assert X.same_bits(got[r, :, 0], got[0, :, 0]) == bool(nets_mask & AR)
    for e in g.replicas:
        assert min(e.stats()["br_updates"]) > SMALL["target_every"]
    g.close()
    ref.close()


def test_serial_lag2_loop_with_a_br_exchange(pkg):
    """A pipelined group (slice_lag 2) exchanging BR nets runs nfsp_group_step's serial loop: the
    header's rule on standalone lag-1 engines -- slice j acts with snapshot j & 1 -- gives the same
    nets and counters."""
    R, K = 2, 4
    g = pkg.engine.EngineGroup(R, seed=313, init_seed=4, slices=K, slice_lag=2, **SMALL)
    g.set_exchange(AR | BR, every=1)
    model = X.GroupModel(R)
    model.set_exchange(AR | BR, 1, F(1.0 / R))
    ref = Restated(pkg, R, model, seed=313, init_seed=4, slices=K, slice_lag=1, **SMALL)
    for step in range(2):
        g.step()
        ref.step(lag2=True)
        got = assert_same_run(g.replicas, ref, f"step {step}")
    assert ref.due == 2 * K
    assert X.same_bits(got[0, :, :2], got[1, :, :2]) and not X.same_bits(got[0, :, 2], got[1, :, 2])
    # the lag matters: a lag-1 restatement ends elsewhere
    model1 = X.GroupModel(R)
    model1.set_exchange(AR | BR, 1, F(1.0 / R))
    ref1 = Restated(pkg, R, model1, seed=313, init_seed=4, slices=K, slice_lag=1, **SMALL)
    for step in range(2):
        ref1.step()
    assert not X.same_bits(read_all(ref1.solo), got)
    g.close()
    ref.close()
    ref1.close()


def test_serial_and_pipelined_lag2_loops_are_one_restatement(pkg):
    """nets = AR alone: the serial loop (sched serial) and the pipelined one both equal the same
    restatement on standalone engines."""
    R, K = 2, 4
    groups = []
    for serial in (1, 0):
        g = pkg.engine.EngineGroup(R, seed=313, init_seed=4, slices=K, slice_lag=2, **SMALL)
        if serial:
            g.set_sched(serial=1)
        g.set_exchange(AR, every=1)
        groups.append(g)
    model = X.GroupModel(R)
    model.set_exchange(AR, 1, F(1.0 / R))
    ref = Restated(pkg, R, model, seed=313, init_seed=4, slices=K, slice_lag=1, **SMALL)
    for step in range(2):
        ref.step(lag2=True)
        for g, name in zip(groups, ("serial", "pipelined")):
            g.step()
            g.check()
            got = assert_same_run(g.replicas, ref, f"{name} step {step}")
    assert X.same_bits(got[0, :, 0], got[1, :, 0]) and not X.same_bits(got[0, :, 1], got[1, :, 1])
    for g in groups:
        g.close()
    ref.close()


# ---- d. the shard kernels -------------------------------------------------------------------------
class OtherShards:
    """A host callback (nfsp_exchange_fn) that stands for the other shards: at call k it records
    the deltas D it is given and the AR nets as they are, and leaves S = f32(D + X_k) with a few
    entries forced to -0.0.  It never raises into its C caller."""
    NEG0 = (5, 700, X.NP + 9, 2 * X.NP - 1)          # into [2][NP]

    @classmethod
    def plant_neg0(cls, *engines):
        """-0.0 into the AR nets where S will be -0.0, before set_exchange takes them as W0: the
        first exchange must leave +0.0 there (W0 + (0 + S) * scale), not -0.0 (W0 + S * scale)."""
        for e in engines:
            for i in cls.NEG0:
                e.weights_tensor(i // X.NP, 0)[i % X.NP] = -0.0
        torch.cuda.synchronize()

    def __init__(self, pkg, eng, fail_at=None):
        self.pkg, self.eng, self.fail_at = pkg, eng, fail_at
        self.calls, self.error = [], None
        self.fn = pkg.native.EXCHANGE_FN(self)

    def __call__(self, _user, ptr, n):
        try:
            k = len(self.calls)
            if self.fail_at is not None and k >= self.fail_at:
                return 1
            assert n == 2 * X.NP, n
            t = self.pkg.native.wrap_device(ptr, n, torch.float32, self.eng.dev)
            D = t.cpu().numpy().copy().reshape(2, X.NP)
            W_pre = np.stack([self.eng.get_weights(a, 0) for a in (0, 1)])
            S = D + X.other_shards(k)
            S.reshape(-1)[list(self.NEG0)] = F(-0.0)
            t.copy_(torch.as_tensor(S.reshape(-1)))
            torch.cuda.synchronize()
            self.calls.append((D, W_pre, S))
            return 0
        except BaseException as ex:       # never unwind through the C caller
            self.error = ex
            return 1


def ar_nets(e):
    torch.cuda.synchronize()
    return np.stack([e.get_weights(a, 0) for a in (0, 1)])


def check_calls(shards, W0, scale, upto_checked=0):
    """Every recorded callback invocation from `upto_checked` on: D is the AR nets' delta against
    W0, and the next one's is taken against shard_apply of this one.  Returns the W0 now."""
    for k in range(upto_checked, len(shards.calls)):
        D, W_pre, S = shards.calls[k]
        d = X.first_diff(D, X.shard_delta(W_pre, W0))
        assert d is None, (f"call {k}: D", d)
        assert np.all(X.bits(S.reshape(-1)[list(shards.NEG0)]) == 0x80000000)
        new = X.shard_apply(W0, S, scale)
        was = X.bits(W0.reshape(-1)[list(shards.NEG0)])       # a -0 sum moves nothing but a -0.0 base
        assert np.all(X.bits(new.reshape(-1)[list(shards.NEG0)]) == np.where(was == 0x80000000, 0, was))
        if k == 0:
            assert np.all(was == 0x80000000)                  # (planted)
        W0 = new
    return W0


@pytest.mark.parametrize("every,scale", [(1, 0.5), (3, 2.0 / 3.0)])
def test_shard_kernels_slice_by_slice(pkg, every, scale):
    """slice_lag 1, driven by rollout / update: the exchange runs inside the due learner call, so
    the AR nets right after it are shard_apply's.  A twin without the exchange holds the same BR
    and target nets up to the call of the first exchange (they depend on the AR nets only
    through later rollouts)."""
    cfg = dict(SMALL, slices=4, seed=606, init_seed=8)
    e, twin = pkg.engine.SelfPlayEngine(**cfg), pkg.engine.SelfPlayEngine(**cfg)
    shards = OtherShards(pkg, e)
    shards.plant_neg0(e, twin)
    W0 = ar_nets(e)
    e.set_exchange(every, scale, fn=shards.fn)
    checked = 0
    for call in range(1, 13):
        e.rollout()
        e.update()
        twin.rollout()
        twin.update()
        assert shards.error is None, shards.error
        assert e.exchanges() == len(shards.calls) == call // every
        if call % every == 0:
            W0 = check_calls(shards, W0, scale, checked)
            checked = len(shards.calls)
            d = X.first_diff(ar_nets(e), W0)
            assert d is None, (f"after call {call}: AR nets", d)
        both = read_all([e, twin])
        if call <= every:
            assert X.same_bits(both[0, :, 1:], both[1, :, 1:]), call
    assert checked == 12 // every
    assert not X.same_bits(both[0, :, 0], both[1, :, 0])
    assert not X.same_bits(both[0, :, 1], both[1, :, 1])         # and it fed back into play
    e.close()
    twin.close()


@pytest.mark.parametrize("every,scale", [(1, 2.0 / 3.0), (3, 0.5)])
def test_shard_kernels_pipelined(pkg, every, scale):
    """slice_lag 2: an exchange is enqueued by the next learner call or at the step's end, so
    the assertions go per callback invocation; at a step's end the AR nets are shard_apply's when
    the step's last call exchanged."""
    K, steps = 4, 3
    cfg = dict(SMALL, slices=K, slice_lag=2, seed=606, init_seed=8)
    e, twin = pkg.engine.SelfPlayEngine(**cfg), pkg.engine.SelfPlayEngine(**cfg)
    shards = OtherShards(pkg, e)
    shards.plant_neg0(e, twin)
    W0 = ar_nets(e)
    e.set_exchange(every, scale, fn=shards.fn)
    checked = 0
    for step in range(1, steps + 1):
        e.step()
        twin.step()
        assert shards.error is None, shards.error
        assert e.exchanges() == len(shards.calls) == step * K // every
        W0 = check_calls(shards, W0, scale, checked)
        checked = len(shards.calls)
        if (step * K) % every == 0:
            d = X.first_diff(ar_nets(e), W0)
            assert d is None, (f"after step {step}: AR nets", d)
        both = read_all([e, twin])
        if step == 1 and every == 3:
            # the exchange after slice 2 (j = 2) would feed slice 4's snapshot: not in this step
            assert X.same_bits(both[0, :, 1:], both[1, :, 1:])
    assert checked == steps * K // every and checked >= 4
    assert not X.same_bits(both[0, :, 0], both[1, :, 0])
    assert not X.same_bits(both[0, :, 1], both[1, :, 1])
    e.close()
    twin.close()


def test_shard_callback_failure_fails_the_step(pkg):
    e = pkg.engine.SelfPlayEngine(**dict(SMALL, slices=4, seed=606, init_seed=8))
    shards = OtherShards(pkg, e, fail_at=1)
    e.set_exchange(1, 0.5, fn=shards.fn)
    e.rollout()
    e.update()
    assert e.exchanges() == 1 and shards.error is None
    e.rollout()
    with pytest.raises(pkg.native.NativeError, match=r"the exchange callback failed \(rc 1\)"):
        e.update()
    assert e.exchanges() == 1
    e.close()

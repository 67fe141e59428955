"""TEST INFRASTRUCTURE ONLY -- the exchange of nets between learners, restated in numpy.

The rule (include/nfsp.h nfsp_group_set_exchange, nfsp_engine_set_exchange):

    W = W0 + (sum_r (W_r - W0)) * scale,   W0 = W

summed in replica order from +0, every intermediate rounded to float32, nothing contracted.
The library implements it twice -- k_group_xchg (csrc/learner.hip, engine groups) and
k_xchg_delta / k_xchg_apply (csrc/exchange.hip, one engine per shard) -- and promises that the
two agree bit for bit.  Here it stands a third time, in plain numpy, with the state a group
keeps around it (GroupModel) and the inputs that tell a right kernel from a wrong one
(make_nets, WRONG).  No torch, no package import.

numpy's float32 array arithmetic rounds every operation once to float32 and never fuses a
multiply with an add, which is the rule's own arithmetic."""
import numpy as np

F = np.float32
NP = 30 * 64 + 64 + 64 * 3 + 3          # one packed net (include/nfsp.h)
XCHG_AR, XCHG_BR = 1, 2                 # NFSP_XCHG_*
NET_AR, NET_BR, NET_TARGET = 0, 1, 2


def bits(x):
    return np.ascontiguousarray(np.asarray(x, F)).view(np.uint32)


def same_bits(x, y):
    return np.array_equal(bits(x), bits(y))


def first_diff(x, y):
    """(flat index, x there, y there) of the first element whose bits differ, or None."""
    d = np.flatnonzero(bits(x).reshape(-1) != bits(y).reshape(-1))
    if not len(d):
        return None
    i = int(d[0])
    return i, float(np.asarray(x, F).reshape(-1)[i]), float(np.asarray(y, F).reshape(-1)[i])


# ---- the rule -----------------------------------------------------------------------------
def group_exchange(W, W0, scale):
    """W [R][...] f32, W0 [...]: W0 + f32(s * scale), s = 0; for r: s = f32(s + f32(W[r] - W0))."""
    W, W0, scale = np.asarray(W, F), np.asarray(W0, F), F(scale)
    s = np.zeros_like(W0)                                # +0
    for r in range(W.shape[0]):
        d = W[r] - W0
        s = s + d
    p = s * scale
    return W0 + p


def shard_delta(W, W0):
    return np.asarray(W, F) - np.asarray(W0, F)


def shard_apply(W0, S, scale):
    """f32(W0 + f32(f32(0 + S) * scale)): the sum over shards arrives as S; 0 + S makes a -0 sum
    the +0 that a sum started from +0 gives."""
    z = F(0) + np.asarray(S, F)
    p = z * F(scale)
    return np.asarray(W0, F) + p


def sum_in_rank_order(D):
    """An honest all-reduce as the rule counts it: from +0, rank 0 first."""
    s = np.zeros_like(np.asarray(D[0], F))
    for d in D:
        s = s + np.asarray(d, F)
    return s


# ---- wrong variants: what a subtly wrong kernel would compute --------------------------------
def wrong_fused(W, W0, scale):
    """(a) base + s * scale contracted: the product kept exact, one rounding (f64 holds the
    product of two f32 exactly, and its sum with an f32 to far more bits than f32's rounding
    can see at these magnitudes)."""
    W, W0 = np.asarray(W, F), np.asarray(W0, F)
    s = np.zeros_like(W0)
    for r in range(W.shape[0]):
        s = s + (W[r] - W0)
    return (W0.astype(np.float64) + s.astype(np.float64) * np.float64(F(scale))).astype(F)


def _pairwise(d):
    if len(d) == 1:
        return d[0]
    h = len(d) // 2                    # the smaller half first: at 3 terms d0 + (d1 + d2)
    return _pairwise(d[:h]) + _pairwise(d[h:])


def wrong_pairwise(W, W0, scale):
    """(b) the deltas summed as a tree instead of in replica order."""
    W, W0 = np.asarray(W, F), np.asarray(W0, F)
    s = np.zeros_like(W0) + _pairwise([W[r] - W0 for r in range(W.shape[0])])
    return W0 + s * F(scale)


def wrong_acc16(W, W0, scale):
    """(b') 16 accumulators (what an unrolled loop with split sums does), then those in order."""
    W, W0 = np.asarray(W, F), np.asarray(W0, F)
    acc = [np.zeros_like(W0) for _ in range(16)]
    for r in range(W.shape[0]):
        acc[r % 16] = acc[r % 16] + (W[r] - W0)
    s = np.zeros_like(W0)
    for a in acc:
        s = s + a
    return W0 + s * F(scale)


def wrong_sum_first(W, W0, scale):
    """(c) sum(W_r) - R * W0 instead of the sum of differences."""
    W, W0 = np.asarray(W, F), np.asarray(W0, F)
    t = np.zeros_like(W0)
    for r in range(W.shape[0]):
        t = t + W[r]
    s = t - F(W.shape[0]) * W0
    return W0 + s * F(scale)


def wrong_scale_per_term(W, W0, scale):
    """(d) every difference scaled before it is summed."""
    W, W0 = np.asarray(W, F), np.asarray(W0, F)
    s = np.zeros_like(W0)
    for r in range(W.shape[0]):
        s = s + (W[r] - W0) * F(scale)
    return W0 + s


def _pow2(x):
    m, _ = np.frexp(np.float64(F(x)))
    return m == 0.5


# name -> (variant, can it differ from the rule at (R, scale) at all?).  Where it cannot, the
# variant IS the rule by an identity of float arithmetic, whatever the inputs:
#   a product with a power of two is exact (no over- or underflow at these magnitudes), so
#   contracting it or applying it per term changes no rounding;
#   one or two terms can be summed in one order only (0 + d0 is exact), 16 accumulators hold
#   one term each up to R = 16 and are then added in replica order;
#   at R = 1, (0 + W_0) - 1 * W0 is W_0 - W0.
WRONG = {
    "fused": (wrong_fused, lambda R, scale: not _pow2(scale)),
    "pairwise": (wrong_pairwise, lambda R, scale: R >= 3),
    "acc16": (wrong_acc16, lambda R, scale: R >= 17),
    "sum_first": (wrong_sum_first, lambda R, scale: R >= 2),
    "scale_per_term": (wrong_scale_per_term, lambda R, scale: R >= 2 and not _pow2(scale)),
}


# ---- inputs ---------------------------------------------------------------------------------
# planted entries of every net (indices into NP), the same handful at every R and seed
PLANT_EQUAL = (0, 257, 2178)          # W_r == W0 for every r
PLANT_NEG0 = (1, 1500)                # W0 = -0.0, the replicas' values ordinary
PLANT_NEG0_EQUAL = (2, 2177)          # W0 = -0.0 and W_r = -0.0 for every r: the rule gives +0.0
PLANT_BIG = (3, 64, 1999)             # one replica far larger than the rest
SEED = 20260


def _signed_log_uniform(rng, shape, lo_exp, hi_exp):
    m = np.exp2(rng.uniform(lo_exp, hi_exp, size=shape))
    return (m * rng.choice([-1.0, 1.0], size=shape)).astype(F)


def make_nets(R, seed=SEED):
    """(W0 [2][3][NP], W [R][2][3][NP]) f32: a common base and R replicas' nets around it.

    |W0| in [2^-9, 2^-1] and W_r = W0 * (1 +- u), u in [2^-6, 2^-1] for half of the entries (an
    SGD step's size: W_r - W0 is exact) and in [1.5, 2.9] for the rest (W_r beyond [W0 / 2, 2 W0],
    where the difference rounds), so every magnitude lies in [2^-10, 2] and every
    |W_r - W0| >= 2^-15 > 2^-20: no difference, sum or product is subnormal (numpy keeps
    subnormals; whether the device does is not the subject).  The deltas are of the base's size,
    so the roundings of each sum, of s * scale and of base + that are visible in the result --
    what the wrong variants get wrong.  Then the planted entries (PLANT_*)."""
    rng = np.random.RandomState(seed * 1000 + R)
    W0 = _signed_log_uniform(rng, (2, 3, NP), -9.0, -1.0)
    shape = (R, 2, 3, NP)
    u = np.where(rng.rand(*shape) < 0.5, np.exp2(rng.uniform(-6.0, -1.0, size=shape)),
                 rng.uniform(1.5, 2.9, size=shape))
    sgn = rng.choice([-1.0, 1.0], size=shape)
    W = (W0.astype(np.float64) * (1.0 + sgn * u)).astype(F)
    for i in PLANT_EQUAL:
        W[..., i] = W0[..., i]
    for i in PLANT_NEG0:
        W0[..., i] = F(-0.0)
        W[..., i] = _signed_log_uniform(rng, (R, 2, 3), -9.0, 0.0)
    for i in PLANT_NEG0_EQUAL:
        W0[..., i] = F(-0.0)
        W[..., i] = F(-0.0)
    for k, i in enumerate(PLANT_BIG):
        W0[..., i] = F(2.0 ** -9) * F(1.0 + 0.125 * k)
        W[..., i] = W0[..., i] * (F(1.0) + _signed_log_uniform(rng, (R, 2, 3), -6.0, -1.0))
        W[(k * 7) % R, ..., i] = F(1.9) - F(0.01 * k)
    return W0, W


def check_nets(W0, W):
    """make_nets' promises, for the tests."""
    planted0 = PLANT_NEG0 + PLANT_NEG0_EQUAL
    keep = np.ones(NP, bool)
    keep[list(planted0)] = False
    for x in (W0[..., keep], W[..., keep]):
        a = np.abs(x)
        assert a.min() >= 2.0 ** -10 and a.max() <= 2.0, (a.min(), a.max())
    keep[list(PLANT_EQUAL)] = False
    d = np.abs(W[..., keep] - W0[..., keep])
    assert d.min() >= 2.0 ** -20, d.min()
    a = np.abs(W[..., list(PLANT_NEG0)])
    assert a.min() >= 2.0 ** -10 and a.max() <= 2.0
    tiny = np.finfo(F).tiny
    for x in (W - W0,):
        nz = np.abs(x[x != 0])
        assert nz.min() >= tiny


def other_shards(k, seed=SEED):
    """X_k [2][NP] f32: what the other shards' deltas sum to at the k-th exchange of a one-engine
    test (the host callback writes S = f32(D + X_k)): signed, 2^-12 .. 2^-3, an SGD step's size
    and more."""
    rng = np.random.RandomState(seed * 1000 + 500 + k)
    return _signed_log_uniform(rng, (2, NP), -12.0, -3.0)


# the (R, nets, scale) of the group kernel's cases (tests/test_gpu_exchange_ref.py a); the scale
# as the C ABI receives it (a double rounded to float)
def _kernel_cases():
    out = []
    for R in (1, 2, 3, 15, 16, 17, 33):
        out.append((R, XCHG_AR | XCHG_BR, F(2.0 / R)))
    for R in (3, 17):
        for nets in (XCHG_AR, XCHG_BR, XCHG_AR | XCHG_BR):
            for scale in (F(1.0 / R), F(2.0 / R), F(0.75)):
                if (R, nets, scale) not in out:
                    out.append((R, nets, scale))
    return out


KERNEL_CASES = _kernel_cases()
# every (R, scale) a GPU case exchanges at: the kernel's, whole steps (R 3 at gain 1 and 2; R 2
# at the mean) and the shard kernels' cross-check (R 3)
R_SCALES = sorted({(R, float(s)) for R, _, s in KERNEL_CASES} |
                  {(3, float(F(1.0 / 3))), (3, float(F(2.0 / 3))), (2, 0.5)})


# ---- a group's exchange state ---------------------------------------------------------------
class GroupModel:
    """The exchange of an engine group as include/nfsp.h and csrc/group.hip state it: which nets,
    how often, the scale, which nets have a W0 (w0_valid), the learner calls counted since
    set_exchange, and W0 [3 nets][2 agents][NP]."""

    def __init__(self, R, avg_ar_slices=None):
        self.R = int(R)
        self.nets, self.every, self.scale = 0, 0, F(1)
        self.w0_valid, self.calls = 0, 0
        self.w0_loaded = 0               # nets whose W0 a load restored, until the nets move on
        self.W0 = np.zeros((3, 2, NP), F)
        self.exchanges = 0
        self.last_broadcast = 0          # the nets (XCHG_*) the last exchange copied from replica 0
        if avg_ar_slices is not None:    # NFSP_GROUP_AVG_AR: AR, once per step, the mean
            self.nets, self.every, self.scale = XCHG_AR, int(avg_ar_slices), F(1) / F(self.R)

    def set_exchange(self, nets, every, scale):
        if nets & ~(XCHG_AR | XCHG_BR):
            raise ValueError("nets: NFSP_XCHG_AR | NFSP_XCHG_BR")
        if every < 0 or (every > 0 and not nets):
            raise ValueError("every >= 0 (and nets when on)")
        on = nets if every else 0
        # a net this call turns on starts over -- unless a load has just restored its W0 (the
        # cadence is not in a blob: a resumed run re-issues it and goes on)
        self.w0_valid &= ~(on & ~self.nets & ~self.w0_loaded)
        self.w0_loaded = 0
        self.nets, self.every, self.scale = on, int(every), F(scale)
        self.calls = 0

    def load(self, w0_valid, W0):
        """nfsp_group_load_state: the blob's flags and W0 [3][2][NP]."""
        self.w0_valid = self.w0_loaded = int(w0_valid)
        self.W0 = np.array(W0, F).reshape(3, 2, NP)
        self.calls = 0

    def begin_step(self):
        """nfsp_group_step's start: is a broadcast due before the first slice?"""
        self.w0_loaded = 0
        return self.needs_broadcast()

    def due(self):
        """After a learner call: is the exchange due?  (++calls % every == 0)"""
        if self.every <= 0:
            return False
        self.calls += 1
        return self.calls % self.every == 0

    def needs_broadcast(self):
        """nfsp_group_step makes the nets common before its first slice when a configured net
        has no W0 yet."""
        return bool(self.nets & ~self.w0_valid)

    def exchange(self, W):
        """W [R][2 agents][3 nets][NP] -> the replicas' nets after one exchange
        (nfsp_group_average_ar, or a due exchange inside nfsp_group_step)."""
        W = np.asarray(W, F)
        assert W.shape == (self.R, 2, 3, NP), W.shape
        nets = self.nets if self.nets else XCHG_AR
        scale = self.scale if self.nets else F(1) / F(self.R)
        out = W.copy()
        self.w0_loaded = 0
        self.last_broadcast = nets & ~self.w0_valid
        for n, bit in ((NET_AR, XCHG_AR), (NET_BR, XCHG_BR)):
            if not nets & bit:
                continue
            if not self.w0_valid & bit:          # replica 0's net everywhere, a BR net with its target
                for m in ((n, NET_TARGET) if n == NET_BR else (n,)):
                    self.W0[m] = W[0, :, m]
                    out[:, :, m] = W[0, :, m]
            else:
                new = group_exchange(W[:, :, n], self.W0[n], scale)
                self.W0[n] = new
                out[:, :, n] = new
        self.w0_valid |= nets
        self.exchanges += 1
        return out

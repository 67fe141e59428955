"""The exchange's numpy restatement (tests/exchange_ref.py) and its inputs, without a GPU: the
nets make_nets writes tell the rule from what a subtly wrong kernel would compute, at the R and
scale of every GPU case of tests/test_gpu_exchange_ref.py.  These are conditions on the
inputs: a GPU comparison on inputs that cannot tell the variants apart would prove nothing.

Share of elements (of 2 x 3 x 2,179) in which each wrong variant differs from the rule, as
measured (the test prints them; the bar is 1 %).  "=": the variant is the rule itself there by
an identity of float arithmetic (exchange_ref.WRONG), asserted as exact equality:

    R   scale        fused  pairwise  acc16  sum_first  scale_per_term
    1   2              =       =        =        =          =
    2   0.5            =       =        =      16.78 %      =
    2   1              =       =        =      32.03 %      =
    3   1/3          29.52 %  13.16 %   =      38.18 %    26.52 %
    3   2/3          31.83 %  16.41 %   =      45.86 %    32.38 %
    3   0.75         20.35 %  17.02 %   =      48.38 %    34.19 %
    15  2/15         27.64 %  40.99 %   =      69.93 %    49.07 %
    16  0.125          =      40.87 %   =      68.86 %      =
    17  1/17         13.45 %  27.81 %  25.86 % 57.79 %    34.50 %
    17  2/17         26.74 %  40.74 %  38.68 % 71.45 %    49.79 %
    17  0.75         22.48 %  56.70 %  53.91 % 80.50 %    68.62 %
    33  2/33         20.51 %  44.11 %  47.37 % 78.51 %    51.53 %"""
import numpy as np
import pytest

import exchange_ref as X

F = np.float32


def share(a, b):
    return float((X.bits(a) != X.bits(b)).mean())


@pytest.mark.parametrize("R", sorted({R for R, _ in X.R_SCALES}))
def test_make_nets_keeps_its_promises(R):
    W0, W = X.make_nets(R)
    assert W0.shape == (2, 3, X.NP) and W.shape == (R, 2, 3, X.NP) and W.dtype == W0.dtype == F
    X.check_nets(W0, W)
    for i in X.PLANT_EQUAL:
        assert all(X.same_bits(W[r, ..., i], W0[..., i]) for r in range(R))
    for i in X.PLANT_NEG0 + X.PLANT_NEG0_EQUAL:
        assert np.all(X.bits(W0[..., i]) == 0x80000000)
    for i in X.PLANT_NEG0_EQUAL:
        assert np.all(X.bits(W[..., i]) == 0x80000000)
    for i in X.PLANT_BIG:
        a = np.sort(np.abs(W[..., i]), axis=0)
        assert np.all(a[-1] > 1.5) and (R == 1 or np.all(a[-2] < 2.0 ** -7))
    W0b, Wb = X.make_nets(R)                          # the same nets for every test that asks
    assert X.same_bits(W0, W0b) and X.same_bits(W, Wb)
    # no intermediate of the rule is subnormal
    tiny = np.finfo(F).tiny
    s = np.zeros_like(W0)
    for r in range(R):
        s = s + (W[r] - W0)
        assert np.abs(s[s != 0]).min() >= tiny
    for scale in {sc for RR, sc in X.R_SCALES if RR == R}:
        p = s * F(scale)
        assert np.abs(p[p != 0]).min() >= tiny


@pytest.mark.parametrize("R,scale", X.R_SCALES)
def test_inputs_tell_the_rule_from_wrong_variants(R, scale):
    """Each wrong variant differs from the rule in at least 1 % of make_nets' elements -- wherever
    float arithmetic lets it differ at all (exchange_ref.WRONG says where and why); where it
    cannot, it IS the rule, bit for bit, which pins that list of exemptions too."""
    W0, W = X.make_nets(R)
    ref = X.group_exchange(W, W0, scale)
    for name, (fn, can_differ) in X.WRONG.items():
        sh = share(ref, fn(W, W0, scale))
        print(f"R {R} scale {scale:.9g} {name}: {100 * sh:.2f} % of elements differ")
        if can_differ(R, scale):
            assert sh >= 0.01, (name, R, scale, sh)
        else:
            assert sh == 0.0, (name, R, scale, sh)


def test_every_variant_is_caught_somewhere():
    """No variant is exempt at every GPU case, and R = 17 and 33 (the unrolled body plus a
    remainder) catch all of them."""
    for name, (_, can_differ) in X.WRONG.items():
        assert any(can_differ(R, s) for R, s in X.R_SCALES), name
        for R in (17, 33):
            assert any(can_differ(RR, s) for RR, s in X.R_SCALES if RR == R), (name, R)


def test_shard_apply_signed_zero_sum():
    """S = -0.0 (one shard whose nets did not move): 0 + S is +0, so W0 stays where it is not a
    signed zero and a -0.0 base becomes +0.0, as the group's sum from +0 gives."""
    W0, _ = X.make_nets(3)
    base = W0[:, 0]
    S = np.full_like(base, -0.0)
    for scale in (0.5, 2.0 / 3.0):
        out = X.shard_apply(base, S, scale)
        nz = X.bits(base) != 0x80000000
        assert nz.sum() > 0 and (~nz).sum() == 2 * len(X.PLANT_NEG0 + X.PLANT_NEG0_EQUAL)
        assert np.array_equal(X.bits(out)[nz], X.bits(base)[nz])
        assert np.all(X.bits(out)[~nz] == 0)
        # and the group rule agrees on equal nets: every delta +0
        grp = X.group_exchange(np.stack([base, base]), base, scale)
        assert X.same_bits(grp, out)


def test_one_replica_at_scale_one_is_not_the_identity():
    """W0 + (W - W0) is not W in f32; nothing here or on the GPU asserts that it is."""
    W0, W = X.make_nets(1)
    out = X.group_exchange(W, W0, 1.0)
    assert 0.0 < share(out, W[0]) < 1.0
    assert np.abs(out.astype(np.float64) - W[0]).max() <= 2.0 ** -23      # an ulp of the largest base


def test_shards_equal_the_group_on_the_same_nets():
    """nfsp.h's claim, on the restatements: shards that apply the honest sum of their deltas, in
    rank order, hold what a group's exchange gives."""
    for R, scale in X.R_SCALES:
        W0, W = X.make_nets(R)
        S = X.sum_in_rank_order([X.shard_delta(W[r], W0) for r in range(R)])
        assert X.same_bits(X.shard_apply(W0, S, scale), X.group_exchange(W, W0, scale)), (R, scale)


def test_group_model_bookkeeping():
    R = 3
    W0, W = X.make_nets(R)
    m = X.GroupModel(R)
    with pytest.raises(ValueError):
        m.set_exchange(4, 1, 0.5)
    with pytest.raises(ValueError):
        m.set_exchange(0, 1, 0.5)
    # nothing configured: AR at the mean, the first call a broadcast of replica 0
    a = m.exchange(W)
    assert m.last_broadcast == X.XCHG_AR and m.w0_valid == X.XCHG_AR
    assert all(X.same_bits(a[r, :, 0], W[0, :, 0]) for r in range(R))
    assert X.same_bits(a[:, :, 1:], W[:, :, 1:])
    b = m.exchange(W)
    assert m.last_broadcast == 0
    assert X.same_bits(b[1, :, 0], X.group_exchange(W[:, :, 0], W[0, :, 0], F(1) / F(3)))
    # the first set_exchange turns on whatever it names (nothing was configured): all broadcast
    m.set_exchange(X.XCHG_AR, 2, 0.75)
    assert m.w0_valid == 0 and m.needs_broadcast() and m.calls == 0
    assert [m.due() for _ in range(5)] == [False, True, False, True, False]
    b = m.exchange(W)
    assert m.last_broadcast == X.XCHG_AR
    # BR turned on next to AR: BR and its target broadcast, AR goes on against its W0
    m.set_exchange(X.XCHG_AR | X.XCHG_BR, 1, 0.75)
    assert m.w0_valid == X.XCHG_AR and m.needs_broadcast()
    c = m.exchange(W)
    assert m.last_broadcast == X.XCHG_BR and not m.needs_broadcast()
    assert all(X.same_bits(c[r, :, 1:], W[0, :, 1:]) for r in range(R))
    assert X.same_bits(c[0, :, 0], X.group_exchange(W[:, :, 0], b[0, :, 0], 0.75))
    # off keeps the flags; on again clears them for what was off
    m.set_exchange(X.XCHG_AR | X.XCHG_BR, 0, 1.0)
    assert m.nets == 0 and m.w0_valid == 3 and not m.due()
    m.set_exchange(X.XCHG_BR, 1, 1.0)
    assert m.w0_valid == X.XCHG_AR
    d = m.exchange(W)
    assert m.last_broadcast == X.XCHG_BR and X.same_bits(d[:, :, 0], W[:, :, 0])
    # a load restores W0 and its flags; the first set_exchange after it goes on from them ...
    saved = m.W0.copy()
    n = X.GroupModel(R)
    n.load(3, saved)
    n.set_exchange(X.XCHG_AR | X.XCHG_BR, 1, 0.75)
    assert n.w0_valid == 3 and not n.begin_step()
    e = n.exchange(W)
    assert n.last_broadcast == 0 and X.same_bits(e[0, :, 1], X.group_exchange(W[:, :, 1], saved[1], 0.75))
    assert X.same_bits(e[:, :, 2], W[:, :, 2])               # the target nets stay each replica's own
    n.set_exchange(X.XCHG_AR, 1, 0.75)                       # ... a later one starts over as ever
    n.set_exchange(X.XCHG_AR | X.XCHG_BR, 1, 0.75)
    assert n.w0_valid == X.XCHG_AR
    # ... and not once the nets moved on after the load
    n = X.GroupModel(R)
    n.load(3, saved)
    assert not n.begin_step()
    n.set_exchange(X.XCHG_AR | X.XCHG_BR, 1, 0.75)
    assert n.w0_valid == 0 and n.begin_step()
    # NFSP_GROUP_AVG_AR
    g = X.GroupModel(4, avg_ar_slices=2)
    assert (g.nets, g.every, g.scale) == (X.XCHG_AR, 2, F(0.25)) and g.needs_broadcast()

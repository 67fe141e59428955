"""Heterogeneous engine groups at the C-ABI boundary, without a device: the three entry points
are exported, and nfsp_group_cfgs_check (host only) accepts lists that differ in every field a
group's replicas may differ in and refuses, naming field and replica, those that differ in a
field the shared launches need equal (include/nfsp.h nfsp_group_create_v)."""
import ctypes as C

import pytest

# (field, a value unlike the default that nfsp_engine_create itself accepts)
UNIFORM_FIELDS = [("n_lanes", 2048), ("rl_capacity", 30_000), ("sl_capacity", 30_000),
                  ("batch", 64), ("inserts_per_update", 64), ("epochs", 1), ("slices", 2), ("slice_lag", 2),
                  ("sched", 1)]


@pytest.fixture(scope="module")
def L(pkg):
    return pkg.native.load()


def cfg_array(pkg, L, dicts):
    out = []
    for d in dicts:
        c = pkg.native.EngineCfg()
        assert L.nfsp_engine_default_cfg(C.byref(c)) == pkg.native.OK
        c.n_lanes = 1024
        c.sched = 0                      # (the default reads the environment)
        for k, v in d.items():
            assert hasattr(c, k), k
            setattr(c, k, v)
        out.append(c)
    return (pkg.native.EngineCfg * len(out))(*out)


def check(pkg, L, dicts, flags=0):
    arr = cfg_array(pkg, L, dicts)
    rc = L.nfsp_group_cfgs_check(arr, len(dicts), flags)
    return rc, L.nfsp_last_error().decode()


def test_symbols_exported_and_bound(pkg, L):
    so = C.CDLL(pkg.native.LIB_PATH)
    for name in ("nfsp_group_create_v", "nfsp_group_cfgs_check", "nfsp_group_replica_cfg"):
        getattr(so, name)
        assert name in pkg.native.SIGNATURES
    assert L.nfsp_version() == 1


def test_create_v_null_arguments(pkg, L):
    assert L.nfsp_group_create_v(None, None, 1, 0, None) == pkg.native.EINVAL
    assert b"null" in L.nfsp_last_error()
    assert L.nfsp_group_cfgs_check(None, 1, 0) == pkg.native.EINVAL
    assert L.nfsp_group_replica_cfg(None, 0, None) == pkg.native.EINVAL


def test_every_allowed_field_may_differ_at_once(pkg, L):
    nat = pkg.native
    other = dict(seed=99, eta=0.3, lr_br=0.01, lr_ar=0.02, gamma=0.9, epsilon=0.2, target_every=5,
                 quirks=nat.EXT_SL_ONEHOT | nat.EXT_RESERVOIR | nat.EXT_EPS_CONST | nat.EXT_SAMPLE_AR)
    rc, msg = check(pkg, L, [{}, other, {}])
    assert rc == nat.OK, msg
    # identical cfgs, seed included, are legal; so is a single replica
    assert check(pkg, L, [{}, {}])[0] == nat.OK
    assert check(pkg, L, [other])[0] == nat.OK


@pytest.mark.parametrize("field,value", UNIFORM_FIELDS)
@pytest.mark.parametrize("where", [1, 2])
def test_uniform_field_difference_is_refused(pkg, L, field, value, where):
    dicts = [{}, {}, {}]
    dicts[where] = {field: value}
    if field == "slice_lag":             # (slice_lag 2 is for sliced engines; all three sliced)
        dicts = [dict(d, slices=2) for d in dicts]
    rc, msg = check(pkg, L, dicts)
    assert rc == pkg.native.EINVAL
    assert field in msg and f"replica {where}" in msg, msg


def test_hidden_and_fit_batch_are_uniform_fields(pkg, L):
    """hidden and fit_batch have one legal value each (64, 32), so a list cannot differ in them
    and be valid; the difference is what the check reports, with the field and the replica."""
    for field, value in (("hidden", 32), ("fit_batch", 16)):
        rc, msg = check(pkg, L, [{}, {field: value}])
        assert rc == pkg.native.EINVAL and field in msg and "replica 1" in msg and "differs" in msg, msg


def test_linear_q_bits_are_uniform(pkg, L):
    nat = pkg.native
    rc, msg = check(pkg, L, [{}, {}, {"quirks": nat.QUIRKS_REFERENCE | nat.EXT_LINEAR_Q}])
    assert rc == nat.EINVAL and "quirks" in msg and "LINEAR_Q" in msg and "replica 2" in msg, msg
    rc, msg = check(pkg, L, [{"quirks": nat.TEXTBOOK}, {"quirks": nat.TEXTBOOK_MSE}])
    assert rc == nat.EINVAL and "quirks" in msg and "replica 1" in msg, msg
    # every replica textbook-MSE, differing elsewhere: legal
    rc, msg = check(pkg, L, [{"quirks": nat.TEXTBOOK_MSE}, {"quirks": nat.TEXTBOOK_MSE_DECAY, "gamma": 1.0}])
    assert rc == nat.OK, msg


def test_exchange_flag_needs_a_uniform_group(pkg, L):
    nat = pkg.native
    rc, msg = check(pkg, L, [{}, {"lr_ar": 0.02}], nat.GROUP_AVG_AR)
    assert rc == nat.EINVAL and "lr_ar" in msg and "replica 1" in msg, msg
    rc, msg = check(pkg, L, [{"seed": 5}, {"seed": 6}, {"seed": 5}], nat.GROUP_AVG_AR)
    assert rc == nat.OK, msg
    assert check(pkg, L, [{}, {}], 2)[0] == nat.EINVAL          # unknown flag


def test_replica_count_and_invalid_cfg(pkg, L):
    nat = pkg.native
    arr = cfg_array(pkg, L, [{}])
    assert L.nfsp_group_cfgs_check(arr, 0, 0) == nat.EINVAL
    assert b"replicas" in L.nfsp_last_error()
    assert L.nfsp_group_cfgs_check(arr, nat.GROUP_MAX_REPLICAS + 1, 0) == nat.EINVAL
    rc, msg = check(pkg, L, [{}, {"target_every": 0}])           # nfsp_engine_create refuses it
    assert rc == nat.EINVAL and "replica 1" in msg, msg

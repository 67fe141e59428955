"""sweep.expand_grid (CPU, pure): the replicas of a one-launch sweep -- the product of the grid
values x seeds, grid-major and seed-minor, with the seeds and initial nets paired across the
grid points."""
import pytest


@pytest.fixture(scope="module")
def sweep(pkg):
    return pkg.sweep


def test_order_labels_and_seeds(sweep):
    grid = {"lr_ar": [0.1, 0.02], "lr_br": [0.05, 0.01, 0.002]}
    base = dict(n_lanes=4096, seed=500, gamma=0.9)
    cfgs, init_seeds, labels = sweep.expand_grid(grid, seeds=2, base=base, paired_init=False)
    assert len(cfgs) == len(init_seeds) == len(labels) == 2 * 3 * 2
    # grid-major (the last key fastest), seed-minor
    want = [(a, b, s) for a in grid["lr_ar"] for b in grid["lr_br"] for s in range(2)]
    assert [(c["lr_ar"], c["lr_br"], c["seed"] - 500) for c in cfgs] == want
    for k, (c, lab) in enumerate(zip(cfgs, labels)):
        assert lab == {"point": k // 2, "seed_index": k % 2, "lr_ar": c["lr_ar"], "lr_br": c["lr_br"]}
        assert c["n_lanes"] == 4096 and c["gamma"] == 0.9            # the base rides along
    assert init_seeds == list(range(12))                             # unpaired: one per replica
    assert base == dict(n_lanes=4096, seed=500, gamma=0.9)           # pure: base untouched
    assert sweep.expand_grid(grid, 2, base, False) == (cfgs, init_seeds, labels)


def test_default_seed_and_single_point(sweep):
    cfgs, init_seeds, labels = sweep.expand_grid({}, seeds=3, base=None, paired_init=False)
    assert [c["seed"] for c in cfgs] == [1234, 1235, 1236]           # nfsp_engine_default_cfg's seed
    assert labels == [{"point": 0, "seed_index": s} for s in range(3)]
    # a grid over the seed itself: each point's seeds count on from its own value
    cfgs, _, _ = sweep.expand_grid({"seed": [10, 100]}, seeds=2, base={"seed": 7}, paired_init=False)
    assert [c["seed"] for c in cfgs] == [10, 11, 100, 101]


def test_paired_init_seeds(sweep):
    cfgs, init_seeds, _ = sweep.expand_grid({"eta": [0.1, 0.2, 0.3]}, seeds=4, base={"seed": 9}, paired_init=True)
    assert init_seeds == [0, 1, 2, 3] * 3
    assert [c["seed"] for c in cfgs] == [9, 10, 11, 12] * 3          # and the same hands streams


def test_refuses_a_uniform_field(sweep):
    for key in ("n_lanes", "batch", "slices", "rl_capacity", "no_such_field"):
        with pytest.raises(ValueError, match=key):
            sweep.expand_grid({key: [1, 2]}, 1, {}, False)
    with pytest.raises(ValueError, match="LINEAR_Q"):
        sweep.expand_grid({"quirks": [7, 7 | 32]}, 1, {}, False)
    # quirks outside the two chain-selecting bits may be swept
    assert len(sweep.expand_grid({"quirks": [7, 7 | 64]}, 1, {}, False)[0]) == 2


def test_refuses_too_many_replicas(sweep):
    assert sweep.GROUP_MAX_REPLICAS == 256
    vals = [0.001 * k for k in range(1, 17)]
    assert len(sweep.expand_grid({"lr_ar": vals, "lr_br": vals}, 1, {}, False)[0]) == 256
    with pytest.raises(ValueError, match="256"):
        sweep.expand_grid({"lr_ar": vals, "lr_br": vals}, 2, {}, False)
    with pytest.raises(ValueError):
        sweep.expand_grid({"lr_ar": []}, 1, {}, False)


def test_point_stats(sweep):
    st = sweep.point_stats([1.0, 3.0, 5.0, 5.0], seeds=2)
    assert st[0] == (2.0, 2.0 ** 0.5) and st[1] == (5.0, 0.0)
    assert sweep.point_stats([4.0, 6.0], seeds=1) == [(4.0, 0.0), (6.0, 0.0)]


def test_constants_match_the_binding(pkg, sweep):
    nat = pkg.native
    assert sweep.GROUP_MAX_REPLICAS == nat.GROUP_MAX_REPLICAS
    assert sweep.UNIFORM_QUIRKS == nat.EXT_LINEAR_Q | nat.EXT_MSE_Q
    assert set(sweep.MAY_DIFFER) <= {n for n, _ in nat.EngineCfg._fields_}

"""Hyperparameter sweeps as ONE engine group (``EngineGroup(cfgs=...)``, nfsp_group_create_v):
every grid point x seed is a replica, so a 16-point grid or 4 settings x 4 paired seeds costs
one run at a group's throughput instead of sixteen single engines.

``expand_grid`` is pure (no library, no GPU): it only lays the grid out.  ``tools/sweep.py``
runs one.
"""
from __future__ import annotations

import itertools

# include/nfsp.h NFSP_GROUP_MAX_REPLICAS, NFSP_EXT_LINEAR_Q | NFSP_EXT_MSE_Q (kept here so that
# laying out a grid needs neither ctypes nor the library)
GROUP_MAX_REPLICAS = 256
UNIFORM_QUIRKS = 32 | 256
# the cfg fields the replicas of a group may differ in (nfsp_group_create_v)
MAY_DIFFER = ("seed", "eta", "lr_br", "lr_ar", "gamma", "epsilon", "target_every", "quirks")
DEFAULT_SEED = 1234      # nfsp_engine_default_cfg's


def expand_grid(grid: dict, seeds: int = 1, base: dict | None = None, paired_init: bool = False):
    """The replicas of a sweep: ``(cfgs, init_seeds, labels)`` for ``EngineGroup(cfgs=cfgs,
    init_seeds=init_seeds)``.

    ``grid`` maps a cfg field to the values to try; the grid points are the product of the
    values, keys in the dict's order with the LAST key varying fastest (itertools.product).
    Order of the replicas: grid-major, seed-minor -- replica ``p * seeds + s`` is seed s of grid
    point p.  Its cfg is ``base`` updated with the point's values and ``seed = base_seed + s``,
    where base_seed is the point's own ``seed`` if the grid has that key, else ``base['seed']``
    (default 1234, nfsp_engine_default_cfg's): seed s is the same hands stream at every grid
    point.  ``labels[k]`` is ``{"point": p, "seed_index": s, **the point's values}``.

    ``init_seeds``: with ``paired_init`` seed s of every grid point starts from the same initial
    nets (``init_seed = s``), so the points differ only in the swept values; otherwise every
    replica has its own (``init_seed = replica index``, EngineGroup's default).

    ValueError: a grid key outside ``MAY_DIFFER`` (the other fields shape the group's shared
    launches), an empty value list, quirks values that differ in EXT_LINEAR_Q / EXT_MSE_Q, or
    more than ``GROUP_MAX_REPLICAS`` replicas."""
    base = dict(base or {})
    seeds = int(seeds)
    if seeds < 1:
        raise ValueError("seeds must be >= 1")
    for k, vals in grid.items():
        if k not in MAY_DIFFER:
            raise ValueError(f"grid key {k!r}: the replicas of a group may differ only in {', '.join(MAY_DIFFER)}")
        if len(vals) == 0:
            raise ValueError(f"grid key {k!r} has no values")
    if "quirks" in grid:
        bits = {int(q) & UNIFORM_QUIRKS for q in grid["quirks"]}
        if len(bits) > 1:
            raise ValueError("grid key 'quirks': the values differ in EXT_LINEAR_Q / EXT_MSE_Q, which a group shares")
    keys = list(grid)
    points = [dict(zip(keys, vals)) for vals in itertools.product(*(grid[k] for k in keys))]
    n = len(points) * seeds
    if n > GROUP_MAX_REPLICAS:
        raise ValueError(f"{len(points)} grid points x {seeds} seeds = {n} replicas: a group holds at most "
                         f"{GROUP_MAX_REPLICAS}")
    cfgs, init_seeds, labels = [], [], []
    for p, point in enumerate(points):
        base_seed = int(point.get("seed", base.get("seed", DEFAULT_SEED)))
        for s in range(seeds):
            c = dict(base)
            c.update(point)
            c["seed"] = base_seed + s
            cfgs.append(c)
            init_seeds.append(s if paired_init else p * seeds + s)
            labels.append({"point": p, "seed_index": s, **point})
    return cfgs, init_seeds, labels


def point_stats(values, seeds: int) -> list:
    """Per grid point (mean, sample standard deviation over its seeds; 0.0 with one seed) of
    per-replica ``values`` in ``expand_grid``'s order."""
    out = []
    for p in range(len(values) // seeds):
        v = [float(x) for x in values[p * seeds:(p + 1) * seeds]]
        m = sum(v) / len(v)
        sd = (sum((x - m) ** 2 for x in v) / (len(v) - 1)) ** 0.5 if len(v) > 1 else 0.0
        out.append((m, sd))
    return out

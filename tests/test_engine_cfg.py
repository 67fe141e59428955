"""What the host derives from an nfsp_engine_cfg (csrc/engine_cfg.h) on the CPU: a stand-alone
program (tests/cpp/engine_cfg_main.cpp, host compiler, AddressSanitizer + UBSan) prints the broken
rule or the sizes of every cfg it reads, and the field table.  The expected values are written here
from the rules as include/nfsp.h states them and from the Python side's own lists (the ctypes
mirror, sweep.MAY_DIFFER, checkpoint.apply_overrides, test_group_hetero_abi.UNIFORM_FIELDS), which
the table now has to agree with."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import test_group_hetero_abi as hetero_abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "neural-ficititious-self-play-in-imperfect-information-games_amd", "csrc")
SRC = os.path.join(REPO, "tests", "cpp", "engine_cfg_main.cpp")

# nfsp_engine_default_cfg's values (the reference's preset), the session fields off
PRESET = dict(n_lanes=65536, hidden=64, rl_capacity=40_000, sl_capacity=40_000, batch=128, inserts_per_update=128,
              target_every=150, epochs=2, fit_batch=32, quirks=7, eta=0.1, lr_br=0.05, lr_ar=0.1, gamma=0.95,
              epsilon=0.06, seed=1234, slices=1, slice_lag=1, sched=0)
EXT_LINEAR_Q, EXT_MSE_Q = 32, 256
SHAPE, HYPER, SESSION = 1, 2, 4

M_LANES = "n_lanes must be in [1, 2^24)"
M_SLICES = "slices must be >= 1 and divide n_lanes"
M_LAG = "slice_lag must be 1 or 2"
M_BATCH = "batch must be 32, 64, 96 or 128"
M_EPOCHS = "epochs must be in [1, 4]"
M_CAP = "capacities must exceed the batch"
M_2GIB = "one slice's step records exceed 2 GiB: use more slices (or more inserts per update)"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("engine_cfg") / "engine_cfg_main")
    # the sanitizer runtimes linked into the program: it needs nothing preloaded
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-I" + CSRC, "-I" + os.path.join(REPO, "include"), SRC, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


def cfg(**kw):
    assert set(kw) <= set(PRESET)
    return dict(PRESET, **kw)


def words(c):
    f32 = lambda x: "%x" % struct.unpack("<I", struct.pack("<f", x))[0]
    f64 = lambda x: "%x" % struct.unpack("<Q", struct.pack("<d", x))[0]
    return " ".join([str(c[k]) for k in ("n_lanes", "hidden", "rl_capacity", "sl_capacity", "batch",
                                         "inserts_per_update", "target_every", "epochs", "fit_batch", "quirks")] +
                    [f32(c["eta"]), f32(c["lr_br"]), f32(c["lr_ar"]), f64(c["gamma"]), f64(c["epsilon"])] +
                    [str(c[k]) for k in ("seed", "slices", "slice_lag", "sched")])


def run(exe, lines, *args):
    r = subprocess.run([exe, *args], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]          # no sanitizer report
    out = r.stdout.split("\n")[:-1]
    assert args or len(out) == len(lines)
    return out


def checks(exe, cfgs):
    """Per cfg: the rule's message (str), or the sizes (dict)."""
    out = []
    for ln in run(exe, ["c " + words(c) for c in cfgs]):
        tag, rest = ln.split(" ", 1)
        assert tag in ("ok", "err")
        out.append(rest if tag == "err" else {k: int(v) for k, v in (x.split("=") for x in rest.split(" "))})
    return out


def table(exe):
    return [(n, int(o), int(s), c) for n, o, s, c in (ln.split(" ") for ln in run(exe, [], "fields"))]


def test_sizes(exe):
    one, sliced = checks(exe, [cfg(n_lanes=1),
                               cfg(n_lanes=4096, slices=4, inserts_per_update=96, batch=64, epochs=3)])
    # one lane: <= 4 RL and <= 4 SL records of an agent per hand, so 4 rows of headroom in the log,
    # 4 pending SL records, 4 // 128 + 2 triggers; 2 epochs x 128 / 32 steps of 2,560 B per update
    assert one == dict(N=1, nblk=1, log_cap=40_004, pend_cap=4, umax=2, steps=8, rec_bytes=2 * 8 * 2560)
    # 1,024 lanes per slice in 4 blocks of 256; 4,096 // 96 + 2 = 44 triggers; 3 x 64 / 32 steps
    assert sliced == dict(N=1024, nblk=4, log_cap=44_096, pend_cap=4096, umax=44, steps=6, rec_bytes=44 * 6 * 2560)


# each rule at its boundary: (the cfg, None if accepted else the message)
RULES = [
    (dict(n_lanes=(1 << 24) - 1, inserts_per_update=1 << 16), None),      # (few updates: far below 2 GiB)
    (dict(n_lanes=1 << 24, inserts_per_update=1 << 16), M_LANES),
    (dict(n_lanes=0), M_LANES),
    (dict(hidden=32), "only hidden == 64 is built"),
    (dict(n_lanes=4096, slices=3), M_SLICES),
    (dict(n_lanes=4096, slices=0), M_SLICES),
    (dict(n_lanes=4096, slices=4), None),
    (dict(slice_lag=0), M_LAG),
    (dict(slice_lag=2), None),
    (dict(slice_lag=3), M_LAG),
    (dict(batch=32), None), (dict(batch=64), None), (dict(batch=96), None), (dict(batch=128), None),
    (dict(batch=0), M_BATCH), (dict(batch=16), M_BATCH), (dict(batch=160), M_BATCH),
    (dict(fit_batch=16), "the SGD chains are built for fit_batch == 32"),
    (dict(epochs=0), M_EPOCHS), (dict(epochs=1), None), (dict(epochs=4), None), (dict(epochs=5), M_EPOCHS),
    (dict(rl_capacity=128), M_CAP), (dict(rl_capacity=129), None),
    (dict(sl_capacity=128), M_CAP), (dict(sl_capacity=129), None),
    (dict(sl_capacity=(1 << 31) - 1), None), (dict(sl_capacity=1 << 31), "sl_capacity must be < 2^31"),
    (dict(rl_capacity=(1 << 40) - 1), None), (dict(rl_capacity=1 << 40), "rl_capacity too large"),
    (dict(inserts_per_update=0), "bad cadence"), (dict(inserts_per_update=1, n_lanes=1024), None),
    (dict(target_every=0), "bad cadence"),
    (dict(quirks=7 | 1 << 9), "unknown bits in quirks (NFSP_QUIRK_* | NFSP_EXT_*)"),
    (dict(quirks=7 | EXT_MSE_Q), "NFSP_EXT_MSE_Q requires NFSP_EXT_LINEAR_Q"),
    (dict(quirks=7 | EXT_MSE_Q | EXT_LINEAR_Q), None),
    # [4 N + 2 triggers][4 epochs][128 / 32] records of 2,560 B: 52,426 x 40,960 B = 2,147,368,960 < 2^31
    (dict(n_lanes=13_106, inserts_per_update=1, epochs=4, batch=128), None),
    (dict(n_lanes=13_107, inserts_per_update=1, epochs=4, batch=128), M_2GIB),
    (dict(n_lanes=4 * 13_106, slices=4, inserts_per_update=1, epochs=4, batch=128), None),    # per slice
    (dict(n_lanes=4 * 13_107, slices=4, inserts_per_update=1, epochs=4, batch=128), M_2GIB),
]


def test_rules_at_their_boundaries(exe):
    assert 52_426 * 40_960 == 2_147_368_960 < 1 << 31 <= 52_430 * 40_960
    got = checks(exe, [cfg(**kw) for kw, _ in RULES])
    for (kw, want), g in zip(RULES, got):
        if want is None:
            assert isinstance(g, dict), (kw, g)
        else:
            assert g == want, (kw, g)
    assert got[-4]["umax"] == 52_426 and got[-4]["rec_bytes"] == 2_147_368_960


def test_rules_are_checked_in_order(exe):
    # several broken rules: the first of them in the header's order
    got = checks(exe, [cfg(hidden=1, n_lanes=0), cfg(n_lanes=0, slices=0), cfg(slices=0, slice_lag=0),
                       cfg(batch=16, epochs=0), cfg(epochs=0, rl_capacity=1), cfg(inserts_per_update=0, quirks=1 << 9)])
    assert got == ["only hidden == 64 is built", M_LANES, M_SLICES, M_BATCH, M_EPOCHS, "bad cadence"]


def test_table_is_the_ctypes_struct(exe, pkg):
    E = pkg.native.EngineCfg
    want = [(n, getattr(E, n).offset, getattr(E, n).size) for n, _ in E._fields_]
    assert [(n, o, s) for n, o, s, _ in table(exe)] == want
    assert C.sizeof(E) == 104


def test_field_classes_are_the_python_lists(exe, pkg):
    cls = {k: {n for n, _, _, c in table(exe) if c == k} for k in ("shape", "hyper", "session")}
    assert cls["hyper"] == set(pkg.sweep.MAY_DIFFER)

    def overridable(name):
        try:
            pkg.checkpoint.apply_overrides(pkg.native.EngineCfg(), {name: 1})
            return True
        except TypeError:
            return False
    assert cls["session"] == {n for n, _ in pkg.native.EngineCfg._fields_ if overridable(n)}
    # hidden and fit_batch have one legal value each, so no second value to refuse
    shared = (cls["shape"] | cls["session"]) - {"hidden", "fit_batch"}
    assert shared == {n for n, _ in hetero_abi.UNIFORM_FIELDS}


OTHER = dict(n_lanes=2048, hidden=32, rl_capacity=30_000, sl_capacity=30_001, batch=64, inserts_per_update=64,
             target_every=7, epochs=1, fit_batch=16, quirks=3, eta=0.2, lr_br=0.01, lr_ar=0.02, gamma=0.9, epsilon=0.5,
             seed=(1 << 63) + 5, slices=2, slice_lag=2, sched=1)


def test_first_diff_and_stored(exe):
    tab = table(exe)
    bit = dict(shape=SHAPE, hyper=HYPER, session=SESSION)
    lines, want = [], []
    for n, _, _, c in tab:
        for mask in range(1, 8):         # one field differs: reported by the masks that hold its class
            lines.append("d %d %s %s" % (mask, words(cfg()), words(cfg(**{n: OTHER[n]}))))
            want.append(n if mask & bit[c] else "-")
    # -0.0 is not 0.0; the shared quirk bits are a shape, named as such unless the whole word is asked for
    lines += ["d %d %s %s" % (HYPER, words(cfg(gamma=0.0)), words(cfg(gamma=-0.0))),
              "d %d %s %s" % (SHAPE | SESSION, words(cfg()), words(cfg(quirks=7 | EXT_LINEAR_Q))),
              "d %d %s %s" % (SHAPE | HYPER, words(cfg()), words(cfg(quirks=7 | EXT_LINEAR_Q))),
              "d %d %s %s" % (SHAPE | SESSION, words(cfg()), words(cfg(quirks=3))),
              # several differ: the first in declaration order
              "d 7 %s %s" % (words(cfg()), words(cfg(sched=1, epsilon=0.5, batch=64))),
              "d %d %s %s" % (HYPER | SESSION, words(cfg()), words(cfg(sched=1, epsilon=0.5, batch=64))),
              "d 7 %s %s" % (words(cfg()), words(cfg()))]
    want += ["gamma", "quirks (NFSP_EXT_LINEAR_Q | NFSP_EXT_MSE_Q)", "quirks", "-", "batch", "epsilon", "-"]
    assert run(exe, lines) == want
    # what a blob stores: every field but the session ones, those 1, 1, 0, the padding zero
    raw = bytes.fromhex(run(exe, ["s " + words(OTHER)])[0])
    fmt = "<iiqqiiiiiIfff4xddQiiI4x"
    assert len(raw) == struct.calcsize(fmt) == 104 and raw[60:64] == raw[100:104] == b"\0" * 4
    vals = dict(zip([n for n, _, _, _ in tab], struct.unpack(fmt, raw)))
    f32 = lambda x: struct.unpack("<f", struct.pack("<f", x))[0]
    assert vals == dict(OTHER, eta=f32(0.2), lr_br=f32(0.01), lr_ar=f32(0.02), slices=1, slice_lag=1, sched=0)

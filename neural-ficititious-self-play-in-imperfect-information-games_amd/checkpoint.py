"""Checkpoint files of a ``SelfPlayEngine`` or an ``EngineGroup`` (``nfsp_*_state_*``,
include/nfsp.h; the format: DESIGN.md §10).

The file is the state blob libnfsp writes, byte for byte.  ``save`` / ``load`` need the
engine (and so a GPU); ``read`` and ``digest`` are CPU only: a trained average-policy net can
be pulled out of a file on a machine without a device::

    ck = checkpoint.read("run.nfsp")
    ar0 = ck["engines"][0]["nets"][0, 0]        # agent 0's AR net, packed as nfsp.h says
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import native

MAGIC = b"NFSPSTAT"
VERSION = 1
KIND_ENGINE, KIND_GROUP = 1, 2
SEC_HOST, SEC_ST, SEC_NETS, SEC_RL, SEC_SL, SEC_GROUP = 1, 2, 3, 4, 5, 6
# digest constants (csrc/state_blob.h)
C0, C1 = 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F
M1, M2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB

HEADER_DTYPE = np.dtype([
    ("magic", "S8"), ("version", "<u4"), ("kind", "<u4"), ("total_bytes", "<u8"),
    ("payload_offset", "<u8"), ("payload_bytes", "<u8"), ("digest", "<u8", (2,)),
    ("sz_cfg", "<u4"), ("sz_dev", "<u4"), ("sz_rl", "<u4"), ("sz_sl", "<u4"), ("sz_host", "<u4"),
    ("np", "<u4"), ("replicas", "<u4"), ("n_sections", "<u4"), ("slices", "<i4"),
    ("slice_lag", "<i4"), ("sched", "<u4"), ("reserved", "<u4")])
SECTION_DTYPE = np.dtype([("kind", "<u4"), ("replica", "<u4"), ("offset", "<u8"), ("bytes", "<u8")])
CFG_DTYPE = np.dtype([
    ("n_lanes", "<i4"), ("hidden", "<i4"), ("rl_capacity", "<i8"), ("sl_capacity", "<i8"),
    ("batch", "<i4"), ("inserts_per_update", "<i4"), ("target_every", "<i4"), ("epochs", "<i4"),
    ("fit_batch", "<i4"), ("quirks", "<u4"), ("eta", "<f4"), ("lr_br", "<f4"), ("lr_ar", "<f4"),
    ("pad0", "<u4"), ("gamma", "<f8"), ("epsilon", "<f8"), ("seed", "<u8"), ("slices", "<i4"),
    ("slice_lag", "<i4"), ("sched", "<u4"), ("pad1", "<u4")])
HOST_DTYPE = np.dtype([
    ("cfg", CFG_DTYPE), ("game", "<i4"), ("pad0", "<i4"), ("g", "<i8"), ("learn_tag", "<u4"),
    ("pad1", "<u4"), ("iteration", "<i8", (2,)), ("target_count", "<i8", (2,)),
    ("target_syncs", "<i8", (2,)), ("epsilon", "<f8", (2,))])
ST_DTYPE = np.dtype([
    ("rl_total", "<i8", (2,)), ("sl_total", "<i8", (2,)), ("sl_count", "<i8", (2,)),
    ("last_rl", "<i8", (2,)), ("last_sl", "<i8", (2,)), ("iteration", "<i8", (2,)),
    ("target_count", "<i8", (2,)), ("target_syncs", "<i8", (2,)), ("br_updates", "<i8", (2,)),
    ("ar_updates", "<i8", (2,)), ("hands", "<i8"), ("rollouts", "<i8"), ("actions", "<u8", (2, 3)),
    ("reward_half", "<i8", (2,)), ("epsilon", "<f8", (2,)), ("temp", "<f8", (2,)),
    ("expl", "<f8", (2,)), ("lr_br", "<f4", (2,))])
RL_DTYPE = np.dtype([("s", "<u4"), ("s2", "<u4"), ("meta", "<u4"), ("a", "<f4", (3,)), ("pad", "<u4", (2,))])
SL_DTYPE = np.dtype([("x", "<u4"), ("a", "<f4", (3,))])
GROUP_DTYPE = np.dtype([("R", "<i4"), ("flags", "<u4"), ("calls", "<i8"), ("w0_valid", "<u4"), ("pad", "<u4")])
assert (HEADER_DTYPE.itemsize, SECTION_DTYPE.itemsize, CFG_DTYPE.itemsize, HOST_DTYPE.itemsize,
        ST_DTYPE.itemsize, RL_DTYPE.itemsize, SL_DTYPE.itemsize, GROUP_DTYPE.itemsize) == (
            104, 24, 104, 192, 296, 32, 16, 24)


def _mix64(z: np.ndarray) -> np.ndarray:
    z = (z ^ (z >> np.uint64(30))) * np.uint64(M1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(M2)
    return z ^ (z >> np.uint64(31))


def digest(payload) -> tuple:
    """(D0, D1) of a payload (bytes-like, whole 8-byte words): the numpy restatement of
    csrc/state_blob.h -- D0 = sum mix64(w[i] ^ (i + 1) * C0), D1 = sum mix64(w[i] + (i + 1) * C1),
    mod 2^64, over the little-endian u64 words w[i]."""
    b = np.frombuffer(payload, np.uint8)
    if b.size % 8:
        raise ValueError("a payload is whole 8-byte words")
    w = b.view("<u8").astype(np.uint64)
    i1 = np.arange(1, w.size + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        d0 = _mix64(w ^ (i1 * np.uint64(C0))).sum(dtype=np.uint64)
        d1 = _mix64(w + i1 * np.uint64(C1)).sum(dtype=np.uint64)
    return int(d0), int(d1)


def _ptr(a: np.ndarray):
    return C.c_void_p(a.ctypes.data) if a.size else C.c_void_p(0)


def check(data) -> native.StateInfo:
    """nfsp_state_check on a blob in memory (host only): raises native.NativeError."""
    a = np.frombuffer(data, np.uint8)
    info = native.StateInfo()
    buf = a if a.size else np.zeros(1, np.uint8)
    native.check(native.load().nfsp_state_check(_ptr(buf), a.size, C.byref(info)), "nfsp_state_check")
    return info


def stored_cfg(data, replica: int = 0):
    """(native.EngineCfg with the saver's slicing, game) of a blob in memory (nfsp_state_cfg)."""
    a = np.frombuffer(data, np.uint8)
    cfg, game = native.EngineCfg(), C.c_int32()
    native.check(native.load().nfsp_state_cfg(_ptr(a), a.size, int(replica), C.byref(cfg), C.byref(game)),
                 "nfsp_state_cfg")
    return cfg, game.value


def _scalar(rec, name):
    v = rec[name]
    return v.tolist() if isinstance(v, np.ndarray) else v.item()


def parse(data) -> dict:
    """``read`` on a blob in memory."""
    a = np.frombuffer(data, np.uint8)
    check(a)
    hd = a[:HEADER_DTYPE.itemsize].view(HEADER_DTYPE)[0]
    nsec = int(hd["n_sections"])
    secs = a[HEADER_DTYPE.itemsize:HEADER_DTYPE.itemsize + nsec * SECTION_DTYPE.itemsize].view(SECTION_DTYPE)

    def body(k, dtype):
        o, n = int(secs[k]["offset"]), int(secs[k]["bytes"])
        return a[o:o + n].view(dtype)

    header = {k: _scalar(hd, k) for k in HEADER_DTYPE.names if k not in ("magic", "reserved")}
    header["digest"] = tuple(int(x) for x in hd["digest"])
    out = {"header": header, "group": None, "engines": [],
           "payload": a[int(hd["payload_offset"]):int(hd["total_bytes"])]}
    k = 0
    if int(hd["kind"]) == KIND_GROUP:
        raw = body(0, np.uint8)
        g = raw[:GROUP_DTYPE.itemsize].view(GROUP_DTYPE)[0]
        out["group"] = {"R": int(g["R"]), "flags": int(g["flags"]), "calls": int(g["calls"]),
                        "w0_valid": int(g["w0_valid"]),
                        "w0": raw[GROUP_DTYPE.itemsize:].view("<f4").reshape(3, 2, native.NP)}
        k = 1
    for r in range(int(hd["replicas"])):
        host = body(k, HOST_DTYPE)[0]
        st = body(k + 1, ST_DTYPE)[0]
        live = np.minimum(st["rl_total"], host["cfg"]["rl_capacity"])
        rl, sl = body(k + 3, RL_DTYPE), body(k + 4, SL_DTYPE)
        n0, c0 = int(live[0]), int(st["sl_count"][0])
        eng = {"cfg": {f: _scalar(host["cfg"], f) for f in CFG_DTYPE.names if not f.startswith("pad")},
               "game": int(host["game"]), "g": int(host["g"]), "learn_tag": int(host["learn_tag"]),
               "iteration": host["iteration"].tolist(), "target_count": host["target_count"].tolist(),
               "target_syncs": host["target_syncs"].tolist(), "epsilon": host["epsilon"].tolist(),
               "st": st, "nets": body(k + 2, "<f4").reshape(2, 3, native.NP),
               "rl": [rl[:n0], rl[n0:]], "sl": [sl[:c0], sl[c0:]]}
        out["engines"].append(eng)
        k += 5
    return out


def read(path) -> dict:
    """A checkpoint file, checked (nfsp_state_check) and taken apart, on the CPU:
    ``header`` (dict), ``payload`` (u8 view), ``group`` (None | R, flags, calls, w0_valid,
    w0 [3][2][NP]) and per replica in ``engines``: cfg, game, g, learn_tag, the schedules, ``st``
    (EngineDev as a numpy record), ``nets`` [2 agents][3 nets][NP] f32, and per agent the live
    M_RL records ``rl`` (RL_DTYPE, oldest first) and M_SL rows ``sl`` (SL_DTYPE)."""
    return parse(np.fromfile(path, dtype=np.uint8))


def _kind(obj) -> str:
    return "group" if hasattr(obj, "replicas") else "engine"


def _blob(obj) -> np.ndarray:
    """The object's state blob (nfsp_engine_save_state / nfsp_group_save_state)."""
    k = _kind(obj)
    n = native.I64()
    native.check(getattr(obj.L, f"nfsp_{k}_state_bytes")(obj.h, C.byref(n)), f"nfsp_{k}_state_bytes")
    buf = np.empty(n.value, np.uint8)
    w = native.I64()
    native.check(getattr(obj.L, f"nfsp_{k}_save_state")(obj.h, _ptr(buf), buf.size, C.byref(w)),
                 f"nfsp_{k}_save_state")
    return buf[:w.value]


def _write(f, data: np.ndarray):
    f.write(memoryview(data))


def save(obj, path):
    """Save an engine or a group at a step boundary: the blob goes to ``path + '.tmp'``, which
    then replaces ``path`` -- a failed or interrupted save never leaves a partial file there."""
    path = os.fspath(path)
    data = _blob(obj)
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            _write(f, data)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
    return int(data.size)


def load_bytes(obj, data):
    a = np.frombuffer(data, np.uint8)
    k = _kind(obj)
    native.check(getattr(obj.L, f"nfsp_{k}_load_state")(obj.h, _ptr(a), a.size), f"nfsp_{k}_load_state")


def load(obj, path):
    """Load a checkpoint file into an existing engine or group (same cfg but for slices,
    slice_lag and sched).  Refused (native.NativeError) before anything is written if the file
    is damaged or does not fit."""
    load_bytes(obj, np.fromfile(os.fspath(path), dtype=np.uint8))


def apply_overrides(cfg: native.EngineCfg, overrides: dict) -> dict:
    """The stored cfg as constructor keywords, with the fields a load may change."""
    for k in overrides:
        if k not in ("slices", "slice_lag", "sched"):
            raise TypeError(f"from_checkpoint: only slices, slice_lag and sched may be overridden, not {k!r}")
    kw = {name: getattr(cfg, name) for name, _ in cfg._fields_}
    kw.update(overrides)
    return kw

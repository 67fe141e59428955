"""CPU checks of the checkpoint format: the host parser nfsp_state_check /
nfsp_state_cfg / nfsp_state_digest and the package's checkpoint.py, without a device.

The blobs here come from a writer of this file's own, written from the documented byte
offsets alone (struct.pack_into at literal offsets, a pure-Python digest): that the library
accepts them is the check that the document and the code agree."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

NP = 30 * 64 + 64 + 64 * 3 + 3
MASK = (1 << 64) - 1
C0, C1 = 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def py_digest(payload: bytes):
    d0 = d1 = 0
    for i in range(len(payload) // 8):
        w = int.from_bytes(payload[8 * i:8 * i + 8], "little")
        d0 += mix64(w ^ (((i + 1) * C0) & MASK))
        d1 += mix64((w + (i + 1) * C1) & MASK)
    return d0 & MASK, d1 & MASK


CFG = dict(n_lanes=4, hidden=64, rl_capacity=5, sl_capacity=6, batch=128, inserts_per_update=128,
           target_every=7, epochs=2, fit_batch=32, quirks=7, eta=0.1, lr_br=0.05, lr_ar=0.1,
           gamma=0.95, epsilon=0.06, seed=77)


def engine_payload(rng, seed, rl_total=(7, 3), sl_total=(2, 9), g=3):
    """The five sections of one engine (HOST 192 B, ST 296 B, NETS, RL, SL) as bytes objects."""
    c = CFG
    host = bytearray(192)
    struct.pack_into("<iiqqiiiiiIfffI", host, 0, c["n_lanes"], c["hidden"], c["rl_capacity"], c["sl_capacity"],
                     c["batch"], c["inserts_per_update"], c["target_every"], c["epochs"], c["fit_batch"],
                     c["quirks"], c["eta"], c["lr_br"], c["lr_ar"], 0)
    struct.pack_into("<ddQiiI", host, 64, c["gamma"], c["epsilon"], seed, 1, 1, 0)   # slices, lag, sched
    struct.pack_into("<i", host, 104, 0)                  # game
    struct.pack_into("<q", host, 112, g)
    struct.pack_into("<I", host, 120, 11)                 # learn_tag
    struct.pack_into("<qqqqqqdd", host, 128, 8, 6, 4, 3, 1, 1, 0.01, 0.02)
    live = [min(t, c["rl_capacity"]) for t in rl_total]
    cnt = [min(t, c["sl_capacity"]) for t in sl_total]
    st = bytearray(296)
    struct.pack_into("<6q", st, 0, *rl_total, *sl_total, *cnt)
    struct.pack_into("<q", st, 160, g * c["n_lanes"])     # hands
    struct.pack_into("<q", st, 168, g)                    # rollouts: hands per lane in the payload
    struct.pack_into("<2f", st, 288, 0.05, 0.05)
    nets = rng.standard_normal(6 * NP).astype("<f4").tobytes()
    rl = rng.integers(0, 256, 32 * sum(live), dtype=np.uint8).tobytes()
    sl = rng.integers(0, 256, 16 * sum(cnt), dtype=np.uint8).tobytes()
    return [(1, bytes(host)), (2, bytes(st)), (3, nets), (4, rl), (5, sl)], live, cnt


def assemble(kind, replicas, sections, slices=4, slice_lag=2, sched=0):
    """Header (104 B) + section table (24 B each) + the sections back to back."""
    n = len(sections)
    off = 104 + 24 * n
    payload = b"".join(b for _, _, b in sections)
    total = off + len(payload)
    buf = bytearray(total)
    buf[0:8] = b"NFSPSTAT"
    struct.pack_into("<II", buf, 8, 1, kind)
    struct.pack_into("<QQQ", buf, 16, total, off, len(payload))
    struct.pack_into("<QQ", buf, 40, *py_digest(payload))
    struct.pack_into("<6I", buf, 56, 104, 296, 32, 16, 192, NP)
    struct.pack_into("<II", buf, 80, replicas, n)
    struct.pack_into("<iiII", buf, 88, slices, slice_lag, sched, 0)
    at = off
    for k, (sk, rep, b) in enumerate(sections):
        struct.pack_into("<IIQQ", buf, 104 + 24 * k, sk, rep, at, len(b))
        at += len(b)
    buf[off:] = payload
    return buf


def engine_blob(seed=1, **kw):
    rng = np.random.default_rng(seed)
    secs, live, cnt = engine_payload(rng, CFG["seed"], **kw)
    return assemble(1, 1, [(k, 0, b) for k, b in secs]), live, cnt


def group_blob(R=2):
    rng = np.random.default_rng(5)
    grp = bytearray(24)
    struct.pack_into("<iIqII", grp, 0, R, 1, 6, 1, 0)     # R, flags, calls, w0_valid, pad
    secs = [(6, 0, bytes(grp) + rng.standard_normal(6 * NP).astype("<f4").tobytes())]
    for r in range(R):
        es, _, _ = engine_payload(rng, CFG["seed"] + r)
        secs += [(k, r, b) for k, b in es]
    return assemble(2, R, secs)


@pytest.fixture(scope="module")
def L(pkg):
    import __graft_entry__
    __graft_entry__.build()
    return pkg.native.load()


def state_check(pkg, L, buf, n=None):
    a = np.frombuffer(bytes(buf), np.uint8)
    info = pkg.native.StateInfo()
    rc = L.nfsp_state_check(C.c_void_p(a.ctypes.data), len(a) if n is None else n, C.byref(info))
    return rc, info, L.nfsp_last_error().decode()


def test_check_accepts_a_blob_written_from_the_documented_layout(pkg, L):
    buf, _, _ = engine_blob()
    rc, info, msg = state_check(pkg, L, buf)
    assert rc == 0, msg
    assert (info.version, info.kind, info.replicas, info.n_sections) == (1, 1, 1, 5)
    assert (info.slices, info.slice_lag, info.sched) == (4, 2, 0)
    assert info.total_bytes == len(buf) and info.payload_offset == 104 + 24 * 5
    assert info.payload_bytes == len(buf) - info.payload_offset
    assert tuple(info.digest) == py_digest(bytes(buf[info.payload_offset:]))
    # a longer buffer than the blob is fine; both memories empty too (zero-length sections)
    assert state_check(pkg, L, buf + b"\0" * 16)[0] == 0
    rc, _, msg = state_check(pkg, L, engine_blob(rl_total=(0, 0), sl_total=(0, 0), g=0)[0])
    assert rc == 0, msg


def test_check_accepts_a_group_blob_and_cfg_reports_the_savers_slicing(pkg, L):
    buf = group_blob(2)
    rc, info, msg = state_check(pkg, L, buf)
    assert rc == 0, msg
    assert (info.kind, info.replicas, info.n_sections, info.group_flags) == (2, 2, 11, 1)
    a = np.frombuffer(bytes(buf), np.uint8)
    for r in (0, 1):
        cfg, game = pkg.native.EngineCfg(), C.c_int32(-1)
        assert L.nfsp_state_cfg(C.c_void_p(a.ctypes.data), len(a), r, C.byref(cfg), C.byref(game)) == 0
        assert (cfg.n_lanes, cfg.rl_capacity, cfg.sl_capacity, cfg.target_every) == (4, 5, 6, 7)
        assert cfg.seed == CFG["seed"] + r and game.value == 0
        assert (cfg.slices, cfg.slice_lag, cfg.sched) == (4, 2, 0)     # the header's, not the payload's 1, 1, 0
        assert cfg.eta == np.float32(0.1) and cfg.gamma == 0.95
    assert L.nfsp_state_cfg(C.c_void_p(a.ctypes.data), len(a), 2, None, None) == pkg.native.EINVAL


@pytest.mark.parametrize("nbytes", [0, 8, 24, 4096, 4096 + 8])
def test_numpy_digest_equals_the_host_c_digest(pkg, L, nbytes):
    payload = np.random.default_rng(nbytes).integers(0, 256, nbytes, dtype=np.uint8).tobytes()
    out = (C.c_uint64 * 2)()
    a = np.frombuffer(payload + b"\0", np.uint8)          # a valid pointer for n = 0 too
    assert L.nfsp_state_digest(C.c_void_p(a.ctypes.data), nbytes, out) == 0
    assert pkg.checkpoint.digest(payload) == (out[0], out[1]) == py_digest(payload)
    if nbytes == 0:
        assert (out[0], out[1]) == (0, 0)
    assert L.nfsp_state_digest(C.c_void_p(a.ctypes.data), nbytes + 4, out) == pkg.native.EINVAL


def test_digest_depends_on_word_order(pkg):
    w = np.random.default_rng(3).integers(0, 2**63, 64, dtype=np.uint64)
    base = pkg.checkpoint.digest(w.tobytes())
    sw = w.copy()
    sw[[5, 40]] = sw[[40, 5]]
    got = pkg.checkpoint.digest(sw.tobytes())
    assert got[0] != base[0] and got[1] != base[1]
    assert sorted(sw.tolist()) == sorted(w.tolist())


def _refused(pkg, L, buf, word, n=None):
    rc, _, msg = state_check(pkg, L, buf, n)
    assert rc == pkg.native.EINVAL, (rc, msg)
    assert word in msg, msg


def test_damaged_blobs_are_refused_with_a_message(pkg, L):
    good, _, _ = engine_blob()
    b = bytearray(good); b[0] ^= 1
    _refused(pkg, L, b, "magic")
    b = bytearray(good); struct.pack_into("<I", b, 8, 2)
    _refused(pkg, L, b, "version")
    # truncated at every section boundary (the section's first byte missing onwards), and one
    # byte short of the end
    for k in range(5):
        (off,) = struct.unpack_from("<Q", good, 104 + 24 * k + 8)
        _refused(pkg, L, good, "truncated", n=off)
    _refused(pkg, L, good, "truncated", n=len(good) - 1)
    _refused(pkg, L, good, "truncated", n=50)
    # a section table entry pointing past the end: by its size, and by its offset
    b = bytearray(good); struct.pack_into("<Q", b, 104 + 24 * 4 + 16, len(good))
    _refused(pkg, L, b, "past the end")
    b = bytearray(good); struct.pack_into("<Q", b, 104 + 24 * 3 + 8, len(good) + 8)
    _refused(pkg, L, b, "past the end")
    # one flipped bit anywhere in the payload: first byte, a net, the last byte
    off = 104 + 24 * 5
    for pos in (off, off + 192 + 296 + 1000, len(good) - 1):
        b = bytearray(good); b[pos] ^= 0x10
        _refused(pkg, L, b, "digest")
    # (a parser error is not a crash: the null buffer)
    assert L.nfsp_state_check(None, 100, None) == pkg.native.EINVAL


def test_read_returns_the_sections_with_their_shapes(pkg, tmp_path):
    ck = pkg.checkpoint
    buf, live, cnt = engine_blob()
    p = tmp_path / "e.nfsp"
    p.write_bytes(bytes(buf))
    d = ck.read(p)
    assert d["group"] is None and len(d["engines"]) == 1
    assert d["header"]["kind"] == 1 and d["header"]["slices"] == 4
    assert d["header"]["digest"] == ck.digest(d["payload"]) == py_digest(d["payload"].tobytes())
    e = d["engines"][0]
    assert e["cfg"]["n_lanes"] == 4 and e["cfg"]["seed"] == 77 and e["cfg"]["slices"] == 1
    assert e["g"] == 3 and e["learn_tag"] == 11 and e["iteration"] == [8, 6] and e["epsilon"] == [0.01, 0.02]
    assert e["nets"].shape == (2, 3, NP) and e["nets"].dtype == np.float32
    assert [len(x) for x in e["rl"]] == live == [5, 3] and e["rl"][0].dtype.itemsize == 32
    assert [len(x) for x in e["sl"]] == cnt == [2, 6] and e["sl"][0]["a"].shape == (2, 3)
    assert e["st"]["rl_total"].tolist() == [7, 3] and int(e["st"]["hands"]) == 12
    off = 104 + 24 * 5 + 192 + 296
    assert np.array_equal(e["nets"].ravel().view(np.uint8), np.frombuffer(bytes(buf[off:off + 24 * NP]), np.uint8))
    # a group
    p2 = tmp_path / "g.nfsp"
    p2.write_bytes(bytes(group_blob(2)))
    d = ck.read(p2)
    assert d["group"]["R"] == 2 and d["group"]["calls"] == 6 and d["group"]["w0"].shape == (3, 2, NP)
    assert [e["cfg"]["seed"] for e in d["engines"]] == [77, 78]
    # a damaged file is an error, not data
    bad = bytearray(buf); bad[-1] ^= 1
    p.write_bytes(bytes(bad))
    with pytest.raises(pkg.native.NativeError, match="digest"):
        ck.read(p)


def test_a_save_whose_write_raises_leaves_no_file(pkg, tmp_path, monkeypatch):
    ck = pkg.checkpoint
    blob = np.frombuffer(bytes(engine_blob()[0]), np.uint8)
    monkeypatch.setattr(ck, "_blob", lambda obj: blob)

    def failing(f, data):
        f.write(memoryview(data[:100]))
        raise OSError("disk full")
    path = tmp_path / "run.nfsp"
    monkeypatch.setattr(ck, "_write", failing)
    with pytest.raises(OSError, match="disk full"):
        ck.save(object(), path)
    assert os.listdir(tmp_path) == []                     # neither the file nor its .tmp
    # and an earlier checkpoint at `path` survives a failed save untouched
    path.write_bytes(b"previous")
    with pytest.raises(OSError):
        ck.save(object(), path)
    assert path.read_bytes() == b"previous" and os.listdir(tmp_path) == ["run.nfsp"]
    monkeypatch.undo()
    monkeypatch.setattr(ck, "_blob", lambda obj: blob)
    assert ck.save(object(), path) == blob.size
    assert path.read_bytes() == blob.tobytes() and os.listdir(tmp_path) == ["run.nfsp"]

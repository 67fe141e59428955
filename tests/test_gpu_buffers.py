"""The memories section of the C ABI (include/nfsp.h nfsp_buf_insert / nfsp_buf_sample) and the
Python buffers built on it, against plain restatements.  No tolerance anywhere: every assertion
is equality of raw bits.

A. The two entry points against tests/buffers_ref.py (checked by hand in test_buffers_ref.py),
   called through ``native`` exactly as buffers.py does.  Every cell of every table is distinct
   (``buffers_ref.table``), so a wrong word offset inside the 65-word row ``s[30] a[3] r s2[30] t``
   shows, and one row per table carries -0.0, denormals, infinities and NaNs with payloads.
   * Guard band: a table is rows G .. G + cap of an allocation of cap + 2 G rows per column whose
     other rows hold a sentinel.  A stray row within G = 8 rows of the table is seen, and lands in
     memory the test owns.  The out-of-range cases aim at exactly those rows.
   * Each case compares the whole allocation with the reference's, then separately asserts that
     the guard rows hold the sentinel and that every cell the reference did not write holds the
     bits it held before.
   * Shapes: the block edge of the one-lane-per-word grid (256 lanes: 3 records are 195 words, 4
     are 260), duplicate slots on both sides of the 4096-record size at which nfsp_buf_insert used
     to change method, every mix of M_RL and M_SL column sets, gathers with repeats, two inserts
     sharing the ctx's scratch with nothing between them, an engine's exported tables, and the
     host-side refusals.
B. pkg.buffers.ReplayBuffer / ReservoirBuffer against the deque model of oracle/nfsp_oracle.py on
   scripted sequences in the shape of the reference's env: one base array per hand that is
   rewritten in place (so pending records are read with their current values), at most 4 adds per
   base array, samples right after a rewrite, larger than the count, and across the wrap of the
   ring.  All 65 (33) columns of every sampled row and of the final table, bit for bit after the
   oracle's float64 is cast to float32.  NaNs in the script are quiet ones, so that the float32
   <-> float64 casts both sides make on the host keep every bit.
   * A condition on the inputs: cap exceeds the adds per base array.  Otherwise the drop-in's
     flush at len(pending) >= cap writes a record whose array the script still rewrites, the
     declared difference from a deque of views.

Measured (MI355X): the whole file (39 cases) takes 2.8 s, 1.7 s of them the first case's set-up
(torch's and the library's start); the slowest case takes 0.12 s.  On the library as it was before
the last writer was decided by an owner word, `4097-into-8-spread` and `9000-into-8-spread` fail
(all 8 rows wrong: 5 and 3 of them hold an earlier record, 3 and 5 mix words of several records)
and `4097-into-5000-pair` passes by the luck of the race.
"""
import numpy as np
import pytest

import buffers_ref as br
import nfsp_oracle as orc

pytestmark = pytest.mark.gpu

G = 8                      # guard rows on either side of every column
SENT = 0xFFC0DE00          # their words (a NaN no table holds), and their bytes in t
SENT_T = 0xA5
EINVAL = -1


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    torch.cuda.init()          # torch's runtime first, as everywhere in the package
    return pkg.native, torch, pkg.native.Context(1)


class Guarded:
    """A record table with the ids first_id .. first_id + cap - 1 inside its guard band.
    ``host[c]`` are the bits of the whole allocation [cap + 2 G, width] as uploaded."""

    def __init__(self, env, cap, first_id, cols=br.COLS):
        native, torch, _ = env
        self.native, self.cap, self.cols = native, cap, tuple(cols)
        inner = br.table(cap, first_id)
        self.host, self.dev = {}, {}
        for c in br.COLS:
            if c not in self.cols:
                self.host[c] = self.dev[c] = None
                continue
            b = br.bits(inner[c])
            full = np.full((cap + 2 * G,) + b.shape[1:], SENT_T if c == "t" else SENT, b.dtype)
            full[G:G + cap] = b
            self.host[c] = full
            self.dev[c] = torch.from_numpy(full.view(np.uint8 if c == "t" else np.int32)).cuda()
        self.rec = self.records(cap)

    def records(self, cap):
        """An nfsp_records over row G of every column, claiming ``cap`` rows."""
        p = [None if self.dev[c] is None else self.native.ptr(self.dev[c][G:]) for c in br.COLS]
        return self.native.Records(*p, cap)

    def inner(self, full):
        return {c: None if full[c] is None else full[c][G:G + self.cap] for c in br.COLS}

    def download(self):
        return {c: None if self.dev[c] is None
                else self.dev[c].cpu().numpy().view(self.host[c].dtype) for c in br.COLS}


def _torn(got, exp):
    """For a failure's message: of the rows of column s that differ from the reference, how many
    hold one (wrong) record throughout and how many mix words of several records."""
    if got["s"] is None:
        return ""
    bad = np.nonzero((got["s"] != exp["s"]).any(axis=1))[0]
    ids = (got["s"][bad] - np.uint32(br.EXP)) >> np.uint32(7)
    mixed = int(sum(len(set(r.tolist())) > 1 for r in ids))
    return f"column s: {len(bad)} rows differ, {len(bad) - mixed} hold another record, {mixed} mix records"


def check(dst, exp, rows, cols):
    """dst on the device against the reference's allocation ``exp``; ``rows`` (of the table) and
    ``cols`` are what the reference wrote."""
    got = dst.download()
    cap = dst.cap
    for c in dst.cols:
        sent = SENT_T if c == "t" else SENT
        assert np.array_equal(got[c], exp[c]), (c, _torn(got, exp))
        assert (got[c][:G] == sent).all() and (got[c][G + cap:] == sent).all(), c
        keep = np.ones(cap + 2 * G, bool)
        if c in cols:
            keep[G + np.array(sorted(rows), np.int64)] = False
        assert np.array_equal(got[c][keep], dst.host[c][keep]), c


def expected(dst, src, index, op, cap):
    """The reference's result on a copy of dst's allocation: (allocation, rows written, columns)."""
    exp = br.copy(dst.host)
    s = src.inner(src.host)
    if op == "insert":
        rows = br.insert(dst.inner(exp), s, index, cap)
    else:
        rows = br.sample(s, index, dst.inner(exp), cap)
    return exp, rows, br.both(dst.host, src.host)


def call(env, name, a, b, index, n=None, a_rec=None, b_rec=None):
    """nfsp_buf_insert(ctx, a = dst, b = src, slots, n) / nfsp_buf_sample(ctx, a = src, idx, k,
    b = dst), as buffers.py:80,88 call them.  Returns the status, after the stream has drained."""
    native, torch, ctx = env
    it = torch.as_tensor(np.asarray(index, np.int64), device="cuda")
    n = len(index) if n is None else n
    a_rec = a.rec if a_rec is None else a_rec
    b_rec = b.rec if b_rec is None else b_rec
    if name == "nfsp_buf_insert":
        rc = ctx.L.nfsp_buf_insert(ctx.h, native.C.byref(a_rec), native.C.byref(b_rec), native.ptr(it), n)
    else:
        rc = ctx.L.nfsp_buf_sample(ctx.h, native.C.byref(a_rec), native.ptr(it), n, native.C.byref(b_rec))
    torch.cuda.synchronize()
    return rc


def run_insert(env, dst, src, slots):
    assert call(env, "nfsp_buf_insert", dst, src, slots) == 0
    check(dst, *expected(dst, src, slots, "insert", dst.cap))


def run_sample(env, src, idx, dst):
    assert call(env, "nfsp_buf_sample", src, dst, idx) == 0
    check(dst, *expected(dst, src, idx, "sample", src.cap))


# ---------------------------------------------------------------- A. the two entry points
@pytest.mark.parametrize("n", [1, 3, 4, 63, 64, 65])
def test_insert_block_edges(env, n):
    slots = np.random.RandomState(n).permutation(97)[:n]
    run_insert(env, Guarded(env, 97, 30000), Guarded(env, n, 0), slots)


@pytest.mark.parametrize("k", [1, 3, 4, 63, 64, 65])
def test_sample_block_edges(env, k):
    idx = np.random.RandomState(100 + k).permutation(97)[:k]
    run_sample(env, Guarded(env, 97, 0), idx, Guarded(env, k + 3, 30000))


def _dup_slots(n, cap, kind):
    rs = np.random.RandomState(n + cap)
    if kind == "same":
        return np.full(n, 5 % cap, np.int64)
    if kind == "spread":                       # n / cap writers per slot, in a random order
        return rs.permutation(np.arange(n, dtype=np.int64) % cap)
    slots = rs.permutation(cap)[:n].astype(np.int64)      # "pair": distinct but for first == last
    slots[-1] = slots[0]
    return slots


DUPLICATES = [(2, 16, "same"), (64, 16, "same"), (4096, 8, "spread"), (4096, 5000, "pair"),
              (4097, 8, "spread"), (9000, 8, "spread"), (4097, 5000, "pair")]


@pytest.mark.parametrize("n,cap,kind", DUPLICATES, ids=[f"{n}-into-{c}-{k}" for n, c, k in DUPLICATES])
def test_insert_duplicate_slots_last_writer_wins(env, n, cap, kind):
    """The header's "duplicate slots: last i wins", below, at and above 4096 records.  With a
    duplicate, a plain scatter lets the lanes of two records race word by word: the surviving row
    can be an earlier record, or no record at all."""
    slots = _dup_slots(n, cap, kind)
    assert len(set(slots.tolist())) < n
    run_insert(env, Guarded(env, cap, 30000), Guarded(env, n, 0), slots)


RL, SL = br.COLS, ("s", "a")
COLUMN_SETS = [("rl-rl", RL, RL), ("sl-sl", SL, SL), ("rl-into-sl", RL, SL), ("sl-into-rl", SL, RL),
               ("rl-into-r-t", RL, ("r", "t"))]


@pytest.mark.parametrize("name,src_cols,dst_cols", COLUMN_SETS, ids=[c[0] for c in COLUMN_SETS])
@pytest.mark.parametrize("op", ["insert", "sample"])
def test_column_sets(env, op, name, src_cols, dst_cols):
    """NULL columns on either side: only the columns present in both tables are copied."""
    index = np.random.RandomState(7).permutation(97)[:65]
    if op == "insert":
        run_insert(env, Guarded(env, 97, 30000, dst_cols), Guarded(env, 65, 0, src_cols), index)
    else:
        run_sample(env, Guarded(env, 97, 0, src_cols), index, Guarded(env, 65, 30000, dst_cols))


def test_sample_repeats_and_permutations(env):
    rs = np.random.RandomState(11)
    run_sample(env, Guarded(env, 7, 0), rs.randint(7, size=300), Guarded(env, 300, 30000))
    src = Guarded(env, 97, 0)
    run_sample(env, src, np.arange(97), Guarded(env, 97, 30000))
    run_sample(env, src, np.arange(97)[::-1].copy(), Guarded(env, 97, 30000))


def test_empty_calls_succeed_and_write_nothing(env):
    dst, src = Guarded(env, 16, 30000), Guarded(env, 16, 0)
    assert call(env, "nfsp_buf_insert", dst, src, [3], n=0) == 0
    check(dst, br.copy(dst.host), set(), ())
    assert call(env, "nfsp_buf_sample", src, dst, [3], n=0) == 0
    check(dst, br.copy(dst.host), set(), ())


def test_two_inserts_share_the_scratch_without_a_synchronisation(env):
    """The ctx's de-duplication scratch serves both calls; the stream alone orders them."""
    native, torch, ctx = env
    rs = np.random.RandomState(5)
    d1, s1, d2, s2 = Guarded(env, 16, 30000), Guarded(env, 200, 0), Guarded(env, 16, 31000), Guarded(env, 150, 1000)
    sl1, sl2 = rs.randint(16, size=200), rs.randint(16, size=150)
    t1, t2 = (torch.as_tensor(x.astype(np.int64), device="cuda") for x in (sl1, sl2))
    ctx.call("nfsp_buf_insert", native.C.byref(d1.rec), native.C.byref(s1.rec), native.ptr(t1), 200)
    ctx.call("nfsp_buf_insert", native.C.byref(d2.rec), native.C.byref(s2.rec), native.ptr(t2), 150)
    torch.cuda.synchronize()
    check(d1, *expected(d1, s1, sl1, "insert", 16))
    check(d2, *expected(d2, s2, sl2, "insert", 16))


def test_sample_of_an_engines_exported_memories(pkg, env):
    """nfsp_records over the tensors eng.memories() returns: 128 rows, some repeated, of M_RL
    (cap = log_cap) and of M_SL, against torch indexing of the same tensors."""
    native, torch, _ = env
    eng = pkg.engine.SelfPlayEngine(n_lanes=256, rl_capacity=300, sl_capacity=150, seed=3, init_seed=1)
    eng.step()
    eng.step()
    rs = np.random.RandomState(2)
    for a in (0, 1):
        mem = eng.memories(a)
        for cap, cols in ((mem["log_cap"], [mem["rl_" + c] for c in br.COLS]),
                          (mem["sl_s"].shape[0], [mem["sl_s"], mem["sl_a"], None, None, None])):
            idx = rs.randint(cap, size=128)
            idx[100:] = idx[:28]
            assert any(float(x.abs().sum()) > 0 for x in cols[:2])
            src = native.Records(*[native.ptr(x) for x in cols], cap)
            dst = Guarded(env, 128, 30000, [c for c, x in zip(br.COLS, cols) if x is not None])
            assert call(env, "nfsp_buf_sample", None, dst, idx, a_rec=src) == 0
            got = dst.download()
            it = torch.as_tensor(idx, device="cuda")
            for c, x in zip(br.COLS, cols):
                if x is None:
                    continue
                want = x[it].cpu().numpy()
                want = want if c == "t" else want.view(np.uint32)
                assert np.array_equal(got[c][G:G + 128], want), c
                sent = SENT_T if c == "t" else SENT
                assert (got[c][:G] == sent).all() and (got[c][G + 128:] == sent).all(), c


def _out_of_range(cap, n):
    index = np.random.RandomState(13).permutation(cap)[:n].astype(np.int64)
    index[[2, 17, 40, n - 1]] = [-1, -G, cap, cap + G - 1]
    return index


def test_insert_skips_slots_outside_the_table(env):
    """Slots -1, -G, cap and cap + G - 1 in a batch of 65: a kernel that ignored cap would write
    the first and last guard rows and the two next to the table."""
    run_insert(env, Guarded(env, 97, 30000), Guarded(env, 65, 0), _out_of_range(97, 65))


def test_sample_skips_indices_outside_the_table(env):
    """The same four as indices: their rows of dst keep their bits (a kernel that ignored cap
    would copy src's guard rows there)."""
    run_sample(env, Guarded(env, 97, 0), _out_of_range(97, 65), Guarded(env, 65, 30000))


def test_host_side_refusals_launch_nothing(env):
    """Sizes the host knows: NFSP_EINVAL, and dst keeps every bit.  The allocations are large
    enough for every refused call (the guard rows), so a missing check is seen, not felt."""
    dst, src = Guarded(env, 97, 30000), Guarded(env, 97, 0)
    small_src, small_dst = Guarded(env, 64, 0), Guarded(env, 64, 30000)
    slots = np.arange(65)

    def refused(rc, table):
        assert rc == EINVAL
        check(table, br.copy(table.host), set(), ())

    refused(call(env, "nfsp_buf_insert", dst, small_src, slots), dst)               # n > src->cap
    refused(call(env, "nfsp_buf_sample", src, small_dst, slots), small_dst)         # k > dst->cap
    for bad in (0, -1):                                                             # cap <= 0
        refused(call(env, "nfsp_buf_insert", dst, src, slots[:3], a_rec=dst.records(bad)), dst)
        refused(call(env, "nfsp_buf_insert", dst, src, slots[:3], b_rec=src.records(bad)), dst)
        refused(call(env, "nfsp_buf_sample", src, dst, slots[:3], a_rec=src.records(bad)), dst)
        refused(call(env, "nfsp_buf_sample", src, dst, slots[:3], b_rec=dst.records(bad)), dst)
    refused(call(env, "nfsp_buf_insert", dst, src, slots, n=-1), dst)                # n < 0
    refused(call(env, "nfsp_buf_sample", src, dst, slots, n=-1), dst)
    native, _, ctx = env                                                           # NULL slots / idx
    refused(ctx.L.nfsp_buf_insert(ctx.h, native.C.byref(dst.rec), native.C.byref(src.rec), None, 3), dst)
    refused(ctx.L.nfsp_buf_sample(ctx.h, native.C.byref(src.rec), None, 3, native.C.byref(dst.rec)), dst)


# ---------------------------------------------------------------- B. the Python buffers
def _qbits(rs, n):
    """n random float32 bit patterns; a NaN gets its quiet bit (see the module docstring)."""
    b = rs.randint(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    nan = ((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0)
    b[nan] |= 0x00400000
    return b.view(np.float32)


def _replay_script(seed, adds, cap):
    """hand: the env's reset (new arrays); write: a step rewrites s[p] and the action vector in
    place; add: the record of that step; sample: a batch."""
    rs = np.random.RandomState(seed)
    ops, done = [], 0
    while done < adds:
        ops.append(("hand",))
        for _ in range(rs.randint(1, 5)):                       # at most 4 adds per base array
            p = int(rs.randint(2))
            ops.append(("write", p, _qbits(rs, 30), _qbits(rs, 3)))
            ops.append(("add", p, float(_qbits(rs, 1)[0]), _qbits(rs, 30), bool(rs.randint(2))))
            done += 1
            u = rs.rand()
            if u < 0.3:                                         # right after an in-place rewrite
                ops.append(("write", p, _qbits(rs, 30), _qbits(rs, 3)))
                ops.append(("sample", int(rs.choice([1, 4, cap, cap + 3]))))
            elif u < 0.45:
                ops.append(("sample", int(rs.choice([cap, cap + 3]))))
    return ops


def _play_replay(buf, ops, probe=None):
    out = []
    base = act = None
    for op in ops:
        if op[0] == "hand":
            base, act = np.zeros((2, 1, 30)), np.zeros((2, 1, 3))
        elif op[0] == "write":
            base[op[1]][0, :] = op[2]
            act[op[1]][0, :] = op[3]
        elif op[0] == "add":
            buf.add(base[op[1]], act[op[1]], op[2], np.array(op[3], np.float64).reshape(1, 30), op[4])
        else:
            if probe:
                probe(buf, op[1])
            out.append(buf.sample_batch(op[1]))
    return out


def _f32_bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64).astype(np.float32)).view(np.uint32)


def _same_batch(got, want, n_float):
    assert len(got) == len(want)
    for f in range(len(want)):
        assert np.shape(got[f]) == np.shape(want[f]), f
        if f < n_float:
            assert np.array_equal(_f32_bits(got[f]), _f32_bits(want[f])), f
        else:
            assert np.array_equal(np.asarray(got[f], bool), np.asarray(want[f], bool)), f


@pytest.mark.parametrize("cap", [7, 50])
def test_replay_buffer_matches_the_deque_model(pkg, env, cap):
    adds = 200
    ops = _replay_script(cap, adds, cap)
    ref = orc.ReplayBuffer(cap, 17)
    want = _play_replay(ref, ops)
    final = [np.array([rec[f] for rec in ref.items]) for f in range(5)]

    seen = dict(mixed=0, over=0)

    def probe(buf, k):
        seen["mixed"] += bool(buf.pending) and buf.flushed > 0
        seen["over"] += k > buf.count

    buf = pkg.buffers.ReplayBuffer(cap, 17, ctx=env[2])
    got = _play_replay(buf, ops, probe)
    assert len(got) == len(want) > 40
    for g, w in zip(got, want):
        _same_batch(g, w, 4)
    # the script reached what it is for: samples that mix device rows with pending host rows,
    # batches larger than the count, and a ring that wrapped many times
    assert seen["mixed"] > 10 and seen["over"] > 0 and buf.total == adds >= 4 * cap
    buf._flush()
    assert buf.flushed == adds and buf.count == cap == ref.count
    slot = env[1].as_tensor((adds - cap + np.arange(cap)) % cap, device="cuda")
    tb = buf.table
    table = [x[slot].cpu().numpy() for x in (tb.s, tb.a, tb.r, tb.s2, tb.t)]
    _same_batch([table[0].reshape(cap, 1, 30), table[1].reshape(cap, 1, 3), table[2],
                 table[3].reshape(cap, 1, 30), table[4]], final, 4)


def test_reservoir_buffer_matches_the_list_model(pkg, env):
    cap, adds = 40, 300
    rows = br.table(adds, rl=False)
    with np.errstate(invalid="ignore"):       # the table's signalling NaN turns quiet here, for both
        s64, a64 = rows["s"].astype(np.float64), rows["a"].astype(np.float64)

    def play(buf):
        out = []
        for i in range(adds):
            buf.add(s64[i].copy().reshape(1, 1, 30), a64[i].copy().reshape(1, 1, 3))
            if i % 23 == 5:
                out.append(buf.sample_batch(12 if i % 2 else 45))     # 45 > cap >= count
        return out

    ref = orc.ReservoirBuffer(cap, 19)
    want = play(ref)
    final = [np.array([rec[f] for rec in ref.items]) for f in range(2)]
    buf = pkg.buffers.ReservoirBuffer(cap, 19, ctx=env[2])
    got = play(buf)
    assert len(got) == len(want) == 13
    for g, w in zip(got, want):
        _same_batch(g, w, 2)
    assert buf.count == cap == len(ref.items)
    _same_batch([buf.table.s.cpu().numpy().reshape(cap, 1, 30),
                 buf.table.a.cpu().numpy().reshape(cap, 1, 3)], final, 2)

"""The memories section of the C ABI (include/nfsp.h nfsp_buf_insert, nfsp_buf_sample) restated
in numpy, and record tables in which every cell is recognisable.

Shares nothing with csrc/capi.hip: both operations are the sequential loop the header describes,
over the columns that are present (not ``None``) on both sides.

A table is a dict of column arrays, the 65 words of a record ``s[30] a[3] r s2[30] t``:

    s [cap, 30] float32   a [cap, 3] float32   r [cap] float32   s2 [cap, 30] float32   t [cap] uint8

An M_SL table has ``None`` for r, s2 and t.  Copies must preserve bits, so every comparison is on
``bits(x)`` (uint32 / uint8 views), never ``==`` on floats.
"""
import numpy as np

COLS = ("s", "a", "r", "s2", "t")
WIDTH = dict(s=30, a=3, r=1, s2=30, t=1)
FIRST_WORD = dict(s=0, a=30, r=33, s2=34, t=64)     # of a column in the 65-word row
EXP = 0x3F800000                                     # cell bits = EXP + ((k << 7) | w): a float in [1, 2)
MAX_ID = 1 << 16                                     # ((k << 7) | w) stays inside the mantissa
T_VALUES = (0, 1, 255)
# what a copy through float arithmetic would change: -0.0, a denormal, an infinity, a signalling
# NaN with a payload, and their negative / quiet variants in s2
SPECIAL_S = (0x80000000, 0x00000001, 0x7F800000, 0x7FA00000)
SPECIAL_S2 = (0x00000000, 0x80000001, 0xFF800000, 0xFFC00000)


def cell_bits(k, w):
    """uint32 bits of word w (0..64) of record k."""
    k = np.asarray(k, np.uint32)
    assert k.size == 0 or int(k.max()) < MAX_ID
    return ((k << np.uint32(7)) | np.uint32(w)) + np.uint32(EXP)


def table(n, first_id=0, rl=True, special=None):
    """n records with the ids first_id .. first_id + n - 1.  Row ``special`` (default n // 2)
    carries the special values in words 0..3 of s (and of s2), with the record's id in the low
    bits of the denormal and of the NaN payloads so that they too are distinct per record."""
    ids = np.arange(first_id, first_id + n, dtype=np.uint32)
    out = {}
    for c in COLS:
        if c == "t":
            out[c] = np.array(T_VALUES, np.uint8)[ids % 3] if rl else None
        elif c in ("r", "s2") and not rl:
            out[c] = None
        else:
            w = FIRST_WORD[c] + np.arange(WIDTH[c], dtype=np.uint32)
            b = cell_bits(ids[:, None], w[None, :])
            out[c] = (b[:, 0] if c == "r" else b).copy().view(np.float32)
    if n:
        row = n // 2 if special is None else special
        k = int(ids[row]) + 1                         # 1 .. 65536: below the NaN's quiet bit
        for c, vals in (("s", SPECIAL_S), ("s2", SPECIAL_S2)):
            if out[c] is not None:
                sp = np.array(vals, np.uint32)
                sp[1] += np.uint32(k << 1)            # still a denormal (< 2**23), still odd
                sp[3] += np.uint32(k)                 # NaN payload
                out[c].view(np.uint32)[row, :4] = sp
    return out


def bits(x):
    """The raw bits of a column: uint32 of float32, uint8 as it is."""
    x = np.ascontiguousarray(x)
    return x if x.dtype == np.uint8 else x.view(np.uint32)


def copy(tab):
    return {c: None if tab.get(c) is None else tab[c].copy() for c in COLS}


def both(dst, src):
    """The columns an operation copies: present on both sides."""
    return [c for c in COLS if dst.get(c) is not None and src.get(c) is not None]


def insert(dst, src, slots, cap):
    """dst[c][slots[i]] = src[c][i] for i = 0 .. n-1 in order (so the last i aimed at a slot
    wins), skipping every i whose slot lies outside [0, cap).  In place; returns the set of
    rows of dst that were written."""
    cols = both(dst, src)
    written = set()
    for i, j in enumerate(np.asarray(slots, np.int64).tolist()):
        if not 0 <= j < cap:
            continue
        for c in cols:
            dst[c][j] = src[c][i]
        written.add(j)
    return written


def sample(src, idx, dst, cap):
    """dst[c][i] = src[c][idx[i]]; a row whose index lies outside [0, cap) leaves dst untouched.
    In place; returns the set of rows of dst that were written."""
    cols = both(dst, src)
    written = set()
    for i, j in enumerate(np.asarray(idx, np.int64).tolist()):
        if not 0 <= j < cap:
            continue
        for c in cols:
            dst[c][i] = src[c][j]
        written.add(i)
    return written


def same_bits(a, b):
    """Tables equal bit for bit, column by column (None only equals None)."""
    for c in COLS:
        x, y = a.get(c), b.get(c)
        if (x is None) != (y is None):
            return False
        if x is not None and not np.array_equal(bits(x), bits(y)):
            return False
    return True

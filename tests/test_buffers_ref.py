"""tests/buffers_ref.py, the restatement tests/test_gpu_buffers.py compares the memories of the
C ABI with, checked by hand on cases small enough to write out.

Cells: word w of record k holds the float32 with the bits 0x3F800000 + ((k << 7) | w), so record
5's r (word 33) is 0x3F8002A1 and record 2's a[1] (word 31) is 0x3F80011F.  t cycles 0, 1, 255.
"""
import numpy as np

import buffers_ref as br


def test_cells_are_distinct_and_where_the_layout_says():
    tab = br.table(9000, first_id=100)
    assert br.bits(tab["r"])[5] == 0x3F800000 + ((105 << 7) | 33)
    assert br.bits(br.table(8)["r"])[5] == 0x3F8002A1
    assert br.bits(br.table(8)["a"])[2, 1] == 0x3F80011F
    assert br.bits(br.table(8)["s"])[7, 29] == 0x3F800000 + (7 << 7) + 29
    assert br.bits(br.table(8)["s2"])[7, 0] == 0x3F800000 + (7 << 7) + 34
    assert br.table(8)["t"].tolist() == [0, 1, 255, 0, 1, 255, 0, 1]
    words = np.concatenate([br.bits(tab[c]).reshape(-1) for c in ("s", "a", "r", "s2")])
    assert len(np.unique(words)) == 9000 * 64
    assert [tab[c].dtype for c in br.COLS] == [np.float32] * 4 + [np.uint8]
    assert [tab[c].shape for c in br.COLS] == [(9000, 30), (9000, 3), (9000,), (9000, 30), (9000,)]
    sl = br.table(3, rl=False)
    assert sl["r"] is None and sl["s2"] is None and sl["t"] is None and sl["a"].shape == (3, 3)


def test_special_values_sit_in_one_row_of_every_table():
    for n, row in ((1, 0), (2, 1), (97, 48)):
        tab = br.table(n, first_id=40)
        s, s2 = tab["s"][row, :4], tab["s2"][row, :4]
        assert br.bits(s)[0] == 0x80000000 and s[0] == 0 and np.signbit(s[0])
        assert 0 < s[1] < np.finfo(np.float32).tiny and s2[1] < 0 and -s2[1] < np.finfo(np.float32).tiny
        assert np.isposinf(s[2]) and np.isneginf(s2[2])
        assert np.isnan(s[3]) and np.isnan(s2[3])
        k = 40 + row + 1
        assert br.bits(s)[3] == 0x7FA00000 + k and br.bits(s2)[3] == 0xFFC00000 + k   # payloads
        assert br.bits(s)[3] != 0x7FC00000                                             # not the default NaN
    assert br.bits(br.table(5, special=4)["s"])[4, 0] == 0x80000000
    # == on floats would miss both a lost sign of zero and any NaN: bits() does not
    a, b = br.table(4), br.table(4)
    assert br.same_bits(a, b) and not np.array_equal(a["s"], b["s"])
    b["s"][2, 0] = 0.0
    assert a["s"][2, 0] == b["s"][2, 0] and not br.same_bits(a, b)


def test_insert_three_records_into_four_slots_last_writer_wins():
    dst, src = br.table(4, first_id=50), br.table(3, first_id=0)
    before = br.copy(dst)
    written = br.insert(dst, src, [2, 0, 2], 4)
    assert written == {0, 2}
    for c in br.COLS:
        d, s, b = br.bits(dst[c]), br.bits(src[c]), br.bits(before[c])
        assert np.array_equal(d[0], s[1])           # record 1 -> slot 0
        assert np.array_equal(d[2], s[2])           # slot 2: record 2, not record 0
        assert not np.array_equal(d[2], s[0])
        assert np.array_equal(d[1], b[1]) and np.array_equal(d[3], b[3])
    assert br.bits(dst["r"]).tolist() == [0x3F800000 + (1 << 7) + 33, 0x3F800000 + (51 << 7) + 33,
                                          0x3F800000 + (2 << 7) + 33, 0x3F800000 + (53 << 7) + 33]
    assert dst["t"].tolist() == [1, 0, 255, 255]    # ids 1, 51, 2, 53 mod 3 -> 1, 0, 2, 2


def test_sample_with_a_repeat():
    src, dst = br.table(4, first_id=0), br.table(5, first_id=50)
    before = br.copy(dst)
    written = br.sample(src, [3, 1, 3], dst, 4)
    assert written == {0, 1, 2}
    for c in br.COLS:
        d, s, b = br.bits(dst[c]), br.bits(src[c]), br.bits(before[c])
        assert np.array_equal(d[0], s[3]) and np.array_equal(d[1], s[1]) and np.array_equal(d[2], s[3])
        assert np.array_equal(d[3:], b[3:])
    assert br.bits(dst["a"])[2].tolist() == [0x3F800000 + (3 << 7) + w for w in (30, 31, 32)]


def test_null_column_on_either_side_is_skipped():
    # M_RL -> M_SL: only s and a exist in dst
    dst, src = br.table(4, first_id=50, rl=False), br.table(2, first_id=0)
    br.insert(dst, src, [3, 1], 4)
    assert dst["r"] is None and dst["s2"] is None and dst["t"] is None
    assert np.array_equal(br.bits(dst["s"])[3], br.bits(src["s"])[0])
    assert np.array_equal(br.bits(dst["a"])[1], br.bits(src["a"])[1])
    # M_SL -> M_RL: r, s2 and t of dst keep their bits, in the written rows too
    dst, src = br.table(4, first_id=50), br.table(2, first_id=0, rl=False)
    before = br.copy(dst)
    br.insert(dst, src, [3, 1], 4)
    assert np.array_equal(br.bits(dst["s"])[1], br.bits(src["s"])[1])
    for c in ("r", "s2", "t"):
        assert np.array_equal(br.bits(dst[c]), br.bits(before[c]))
    # a dst with r and t alone, for sample
    src, dst = br.table(4), br.table(2, first_id=50)
    dst["s"] = dst["a"] = dst["s2"] = None
    br.sample(src, [2, 0], dst, 4)
    assert br.bits(dst["r"]).tolist() == [0x3F800000 + (2 << 7) + 33, 0x3F800000 + 33]
    assert dst["t"].tolist() == [255, 0]
    assert br.both(dst, src) == ["r", "t"]


def test_out_of_range_rows_are_skipped():
    dst, src = br.table(4, first_id=50), br.table(4, first_id=0)
    before = br.copy(dst)
    written = br.insert(dst, src, [-1, 4, 1, 1 << 40], 4)
    assert written == {1}
    exp = br.copy(before)
    for c in br.COLS:
        exp[c][1] = src[c][2]
    assert br.same_bits(dst, exp)
    dst, src = br.table(4, first_id=50), br.table(3, first_id=0)
    before = br.copy(dst)
    written = br.sample(src, [3, 2, -1, 0], dst, 3)
    assert written == {1, 3}
    for c in br.COLS:
        d, s, b = br.bits(dst[c]), br.bits(src[c]), br.bits(before[c])
        assert np.array_equal(d[0], b[0]) and np.array_equal(d[2], b[2])
        assert np.array_equal(d[1], s[2]) and np.array_equal(d[3], s[0])

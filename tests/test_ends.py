"""Fixed trims and sliding-window quality cutting of both read ends, on the host: the rule's loop (tests/ends_expect.py), the
package's ends_cut and index.ends_rows against it, EndRules and the argument errors of the filters.

The expectation of every test is the loop of tests/ends_expect.py -- the rule as include/ffq.h states it, written out there --
never the package's own host implementation.  The device: tests/test_ends_device.py, tests/test_ends_stream.py.
"""
import io

import numpy as np
import pytest

import ends_expect as E


# ---- the loop -------------------------------------------------------------------------------------------------------------
def test_the_loop_gives_the_hand_values():
    assert E.hand_line("u2") == b"?#"                   # Q30 and Q2 with qual_base 33
    for text, r, want in E.HAND:
        assert E.loop_cut(E.hand_line(text), r) == want, (text, r)


def test_the_running_sums_are_the_sums():
    rng = np.random.default_rng(3)
    v = [int(x) for x in rng.integers(-40, 60, 150)]
    for a, b, W in ((0, 150, 4), (7, 93, 64), (10, 11, 1), (5, 5, 1), (0, 3, 4)):
        assert E.window_sums(v, a, b, W) == [sum(v[i:i + W]) for i in range(a, b - W + 1)]


def test_seeded_table_holds_what_it_should():
    buf, rows = E.seeded_table()
    assert 3900 <= len(rows) <= 4100 and len(buf) < 1 << 20
    for setting in ("front", "right", "tail", "all three"):
        _rows, stats, spans = E.seeded_want(setting)
        elig = len(spans)
        assert elig == len(rows) - stats[2] and stats[2] >= 40
        assert 4 * stats[0] >= elig, (setting, stats, elig)                       # at least a quarter are changed
        assert 4 * sum(1 for n, a, b in spans if b - a == n) >= elig, setting     # at least a quarter are not
        assert sum(1 for n, a, b in spans if n > 0 and b == a) >= 100, setting    # reads that go away
        assert any(0 < n < 4 for n, _a, _b in spans)                              # a row shorter than the window
        assert max(n for n, _a, _b in spans) <= 220 and min(n for n, _a, _b in spans) == 0
    for setting in ("window 64", "window 1", "fixed"):
        stats = E.seeded_want(setting)[1]
        assert stats[0] > 500, (setting, stats)
    # the fixed trims: 5 and 3 off every read that has them, 100 kept at the most
    for n, a, b in E.seeded_want("fixed")[2]:
        assert (a, b) == ((5, min(n - 3, 105)) if n > 8 else (0, 0))


@pytest.mark.parametrize("stage", ("front", "right", "tail"))
def test_the_edge_tables_cut_where_they_say(stage):
    buf, rows, what = E.edge_table(stage)
    assert len(what) == len(E.EDGE_OFFSETS) * len(E.EDGE_WINDOWS) * 2 and set(r[5] - r[4] for r in rows) == {E.EDGE_LEN}
    for r, (o, W, pattern) in zip(rows[::7], what[::7]):
        a, b = E.loop_cut(buf[r[4]:r[5]], E.edge_rules(stage, W))
        assert (a if stage == "front" else b) == o, (stage, o, W, pattern, a, b)


def test_long_table_holds_what_it_should():
    buf, rows, names = E.long_table()
    lengths = [r[5] - r[4] for r in rows]
    assert {E.LONG, E.LONG + 1, 5000, 20000} <= set(lengths) and len(buf) < 1 << 20
    want, stats, spans = E.loop_rows(buf, rows, E.ALL3)
    by = dict(zip(names, zip(rows, want)))
    assert stats[2] == 1 and (by["newline"][1] == by["newline"][0]).all()
    assert by["all bad"][1][3] == by["all bad"][1][2] and (by["all good"][1] == by["all good"][0]).all()
    for n in (E.LONG, E.LONG + 1, 5000, 20000):
        for edge in (1024, 2048):
            r, w = by["front %d %d" % (n, edge)]
            assert w[2] - r[2] == edge - 2 and w[3] == r[3]
            r, w = by["right %d %d" % (n, edge)]
            assert w[2] == r[2] and w[3] - r[2] == edge - 1
            r, w = by["island %d %d" % (n, edge)]
            assert w[2] - r[2] == edge - 2 and w[3] - r[2] == edge + 1
            r, w = E.loop_rows(buf, [by["tail %d %d" % (n, edge)][0]], E.TAIL)[0][0], None
            assert r[3] - r[2] == n - edge - 2


# ---- the host implementation against the loop ---------------------------------------------------------------------------------
def test_ends_cut_and_ends_rows_host(pkg):
    from fastqandfurious_amd import index as X, fastqandfurious as F
    for text, r, want in E.HAND:
        assert F.ends_cut(E.hand_line(text), E.pkg_rules(F, r)) == want, (text, r)
    buf, rows, names = E.hand_table()
    sbuf, srows = E.seeded_table()
    for setting, r in E.SETTINGS.items():
        want, stats, _spans = E.loop_rows(buf, rows, r)
        assert stats[2] == len(names)
        got = X.ends_rows(buf, np.array(rows, dtype=np.int64), E.pkg_rules(F, r))
        assert got.shape == want.shape and (got == want).all(), setting
        got = X.ends_rows(buf, np.array(rows, dtype=np.int64) + 1000, E.pkg_rules(F, r), shift=1000)
        assert (got == want + 1000).all()
        want = E.seeded_want(setting)[0]
        got = X.ends_rows(sbuf, np.array(srows, dtype=np.int64), E.pkg_rules(F, r))
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (setting, bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())
        got = X.ends_rows(sbuf, np.array(srows[:300], dtype=np.int64) + 77, E.pkg_rules(F, r), shift=77)
        assert (got == want[:300] + 77).all()
    # another qual_base: the values go negative
    r = E.Rules(front=(5, 3), right=(7, 2), tail=(3, 4))
    want = E.loop_rows(sbuf, srows[:600], r, qual_base=64)[0]
    assert (X.ends_rows(sbuf, np.array(srows[:600], dtype=np.int64), E.pkg_rules(F, r), qual_base=64) == want).all()
    for stage in ("front", "right", "tail"):
        ebuf, erows, what = E.edge_table(stage)
        for W in E.EDGE_WINDOWS:
            sub = [r for r, w in zip(erows, what) if w[1] == W]
            want = E.loop_rows(ebuf, sub, E.edge_rules(stage, W))[0]
            assert (X.ends_rows(ebuf, np.array(sub, dtype=np.int64), E.pkg_rules(F, E.edge_rules(stage, W))) == want).all(), (stage, W)
    for r in srows[:50] + srows[495:520]:
        assert F.ends_trimmable(sbuf, r) == F.trimmable(sbuf, r)
    assert sum(not F.ends_trimmable(sbuf, r) for r in srows) == E.seeded_want("front")[1][2]


def test_end_rules(pkg):
    from fastqandfurious_amd import fastqandfurious as F, hip
    r = F.EndRules(3, 2, 100, front=(4, 20), tail=(64, 93))
    assert (r.trim_front, r.trim_tail, r.keep_len, r.front, r.right, r.tail) == (3, 2, 100, (4, 20), None, (64, 93))
    s = hip.ends_rules_struct(r, 64)
    assert [getattr(s, n) for n, _t in s._fields_] == [3, 2, 100, 64, 4, 20, 0, 0, 64, 93]
    assert F.EndRules(keep_len=5).keep_len == 5 and F.EndRules(1, keep_len=0).keep_len is None
    for bad in (dict(), dict(trim_front=-1), dict(trim_tail=-1), dict(keep_len=-1), dict(trim_front=1.5), dict(trim_front=True),
                dict(front=(65, 20)), dict(front=(0, 20)), dict(right=(4, 0)), dict(right=(4, 94)), dict(tail=(4,)), dict(tail=4),
                dict(tail=(4.0, 20)), dict(front=(4, 20, 1)), dict(trim_front=1 << 31), dict(keep_len=0)):
        with pytest.raises(ValueError, match="ends"):
            F.EndRules(**bad)


def test_argument_errors_host(pkg):
    from fastqandfurious_amd import index as X, fastqandfurious as F
    good = F.EndRules(front=(4, 20))
    for bad in ((4, 20), "front", 4, dict(front=(4, 20))):
        with pytest.raises(ValueError):
            F.ends_cut(b"IIII", bad)
        with pytest.raises(ValueError):
            X.ends_rows(b"", np.zeros((0, 6), dtype=np.int64), bad)
    for base in (-1, 256):
        with pytest.raises(ValueError, match="qual_base"):
            F.ends_cut(b"IIII", good, base)
    # the filters name the setting, before anything is opened or read
    for bad in ((4, 20), "front", 4, E.FRONT, (good, good, good), [good]):
        fh = io.BytesIO(b"@a\nACGT\n+\nIIII\n")
        with pytest.raises(ValueError, match="ends"):
            F.filter_fastq(fh, io.BytesIO(), entrypos=F.entrypos, ends=bad)
        assert fh.tell() == 0
        fh1, fh2 = io.BytesIO(b"@a\nACGT\n+\nIIII\n"), io.BytesIO(b"@a\nACGT\n+\nIIII\n")
        with pytest.raises(ValueError, match="ends"):
            F.filter_fastq_paired(fh1, fh2, io.BytesIO(), io.BytesIO(), entrypos=F.entrypos, ends=bad)
        assert fh1.tell() == 0 and fh2.tell() == 0
    fh = io.BytesIO(b"@a\nACGT\n+\nIIII\n")
    with pytest.raises(ValueError, match="qual_base"):
        F.filter_fastq(fh, io.BytesIO(), entrypos=F.entrypos, ends=good, qual_base=300)
    assert fh.tell() == 0
    with pytest.raises(TypeError):
        F.filter_fastq(io.BytesIO(), io.BytesIO(), entrypos=F.entrypos, ends=good, ends_report=object())
    with pytest.raises(ValueError, match="ends"):
        F.filter_fastq(io.BytesIO(), io.BytesIO(), entrypos=F.entrypos, ends_report=F.EndsReport())

"""Quality trimming by editing rows of the offset table: ffq_table_trim_quality (device), index.trim_rows (host),
entryfunc_qualitytrim (per record).

The expectation of every test is the loop below -- the rule as include/ffq.h states it, written out here -- never the
package's own host implementation.  Coordinates: a row minus `add` indexes the buffer the scanner saw; with a sentinel
that buffer is b'\\n' + bytes.
"""
import functools
import io
import os

import numpy as np
import pytest

import grid_expect as GE

from conftest import GOLDEN_DIR, golden_file


# ---- the rule ------------------------------------------------------------------------------------------------------
def loop_span(q, cf, cb, base=33):
    n = len(q)
    start, stop = 0, n
    s = best = 0
    for i in range(n):
        s += cf - (q[i] - base)
        if s < 0:
            break
        if s > best:
            best, start = s, i + 1
    s = best = 0
    for i in range(n - 1, -1, -1):
        s += cb - (q[i] - base)
        if s < 0:
            break
        if s > best:
            best, stop = s, i
    if start >= stop:
        start = stop = 0
    return start, stop


def loop_rows(buf, rows, cf, cb, base=33, add=0):
    """(new rows, [changed, bases removed, skipped]) for rows (+ add) over `buf` (bytes: the buffer as the scanner saw it)."""
    out, stats = [], [0, 0, 0]
    for row in rows:
        row = [int(x) for x in row]
        p2, p3, p4, p5 = (x - add for x in row[2:])
        ok = min(p2, p3, p4, p5) >= 0 and p2 <= p3 <= len(buf) and p4 <= p5 <= len(buf) and p3 - p2 == p5 - p4
        if ok and 10 in buf[p4:p5]:
            ok = False
        if not ok:
            stats[2] += 1
            out.append(row)
            continue
        n = p5 - p4
        a, b = loop_span(buf[p4:p5], cf, cb, base)
        if (a, b) != (0, n):
            stats[0] += 1
            stats[1] += n - (b - a)
        out.append(row[:2] + [row[2] + a, row[2] + b, row[4] + a, row[4] + b])
    return np.array(out, dtype=np.int64).reshape(-1, 6), stats


# ---- hand vectors: (name, quality bytes, cf, cb, base, the span worked out by hand) ------------------------------------
def _q(vals, base=33):
    return bytes(v + base for v in vals)


HAND = [
    ("the issue's example", _q([42, 40, 26, 27, 8, 7, 11, 4, 2, 3]), 0, 10, 33, (0, 4)),
    ("n = 0", b"", 20, 20, 33, (0, 0)),
    ("n = 1, low", _q([5]), 0, 10, 33, (0, 0)),
    ("n = 1, high", _q([30]), 10, 10, 33, (0, 1)),
    ("all above the cutoff", _q([30] * 20), 20, 20, 33, (0, 20)),
    ("all below the cutoff", _q([2] * 20), 20, 20, 33, (0, 0)),
    ("3' tie: sums 5, 5, 5 keep the first maximum", _q([40, 40, 40, 10, 10, 5]), 0, 10, 33, (0, 5)),
    ("5' tie: sums 5, 5, 5 keep the first maximum", _q([5, 10, 10, 40, 40]), 10, 0, 33, (1, 5)),
    ("a run of exact zeros never beats best = 0", _q([10, 10, 10, 40]), 10, 10, 33, (0, 4)),
    ("zeros, then a rise behind them", _q([10, 10, 9, 40, 40]), 10, 0, 33, (3, 5)),
    ("bytes below the base with cutoff 0", bytes([30, 30, 70, 70, 70]), 0, 0, 33, (2, 5)),
    ("base 64", bytes([66, 66, 104, 104, 66]), 20, 20, 64, (2, 4)),
    ("front and back cross", _q([5, 5, 5, 12, 5, 5, 5]), 10, 10, 33, (0, 0)),
    ("front and back meet exactly", _q([2, 2, 2, 30, 2, 2]), 10, 10, 33, (3, 4)),
    ("front eats everything, back nothing", _q([2, 2, 2, 2, 19]), 20, 0, 33, (0, 0)),
]


def hand_table():
    """One buffer with a four-line record per hand vector, then the ineligible rows.  Returns (bytes, rows, names): rows
    index the bytes (no sentinel, add 0)."""
    buf, rows, names = bytearray(b"##"), [], []
    for i, (name, q, *_rest) in enumerate(HAND):
        p0 = len(buf)
        buf += b"@h%d\n" % i
        p1 = len(buf) - 1
        p2 = len(buf)
        buf += b"A" * len(q) + b"\n+\n"
        p4 = len(buf)
        buf += q + b"\n"
        rows.append([p0, p1, p2, p2 + len(q), p4, p4 + len(q)])
        names.append(name)
    # a quality with a newline in it (a wrapped record: the lengths agree)
    p0 = len(buf)
    buf += b"@w\nACGT\nAC\n+\n"
    p4 = len(buf)
    buf += b"!!!!\n!!\n"
    rows.append([p0, p0 + 2, p0 + 3, p0 + 10, p4, p4 + 7]); names.append("newline in the quality")
    p0 = len(buf)
    buf += b"@u\nACGTA\n+\n!!!!\n"
    rows.append([p0, p0 + 2, p0 + 3, p0 + 8, p0 + 11, p0 + 15]); names.append("unequal lengths")
    rows.append([p0, p0 + 2, p0 + 3, p0 + 8, -1, -1]); names.append("a FASTA row")
    rows.append([p0, p0 + 2, p0 + 3, p0 + 7, len(buf) - 3, len(buf) + 1]); names.append("past the buffer")
    rows.append([p0, p0 + 2, -5, -1, p0 + 11, p0 + 15]); names.append("in front of the buffer")
    return bytes(buf), rows, names


def test_the_loop_gives_the_hand_values():
    for name, q, cf, cb, base, want in HAND:
        assert loop_span(q, cf, cb, base) == want, name


def _groups():
    """the hand rows by (cf, cb, base): a call has one set of parameters"""
    buf, rows, names = hand_table()
    params = [(cf, cb, base) for _n, _q_, cf, cb, base, _w in HAND]
    out = {}
    for i, p in enumerate(params):
        out.setdefault(p, []).append(i)
    tail = list(range(len(HAND), len(rows)))
    return buf, rows, names, out, tail


def test_hand_vectors_host(pkg):
    """index.trim_rows and entryfunc_qualitytrim.__call__ against the loop, on the hand vectors and the ineligible rows"""
    from fastqandfurious_amd import index as X, fastqandfurious as F
    buf, rows, names, groups, tail = _groups()
    for (cf, cb, base), idx in groups.items():
        sub = [rows[i] for i in idx] + [rows[i] for i in tail]
        want, stats = loop_rows(buf, sub, cf, cb, base)
        for j, i in enumerate(idx):
            a, b = HAND[i][5]
            assert list(want[j]) == rows[i][:2] + [rows[i][2] + a, rows[i][2] + b, rows[i][4] + a, rows[i][4] + b], names[i]
        assert (want[len(idx):] == np.array([rows[i] for i in tail])).all() and stats[2] == len(tail)
        got = X.trim_rows(buf, np.array(sub, dtype=np.int64), cb, cf, base)
        assert got.shape == want.shape and (got == want).all(), (cf, cb, base)
        # shifted rows
        got = X.trim_rows(buf, np.array(sub, dtype=np.int64)[:len(idx)] + 1000, cb, cf, base, shift=1000)
        assert (got == want[:len(idx)] + 1000).all()
        for col in ("entry", "sequence", "quality", "header"):
            for lo, hi in ((None, None), (2, None), (None, 3)):
                ef = F.entryfunc_qualitytrim(cb, cf, base, min_len=lo, max_len=hi, column=col)
                for r, w in zip(sub, want):
                    pos = list(r)
                    item = ef(buf, pos, 0)
                    assert pos == list(r), "the caller's pos was modified"
                    ln = int(w[3] - w[2])
                    e = (buf[w[0] + 1:w[1]], buf[w[2]:w[3]], buf[w[4]:w[5]])
                    e = {"entry": e, "header": e[0], "sequence": e[1], "quality": e[2]}[col]
                    if (lo is not None and ln < lo) or (hi is not None and ln > hi):
                        e = None
                    assert item == e, (r, col, lo, hi)


def _python_rows(F, data):
    """rows of every record of `data` by the Python scanner (buffer = b'\\n' + data, as the iterator builds it)"""
    from array import array
    buf, rows, pos, offset = b"\n" + data, [], array("q", [-1] * 6), 0
    while F.entrypos(buf, offset, pos) == F.COMPLETE:
        rows.append(list(pos))
        offset = pos[5] - 1
    return buf, rows


def test_golden_file_host(pkg):
    """... and on tests/golden/data/test.fq scanned by the Python entrypos"""
    from fastqandfurious_amd import index as X, fastqandfurious as F
    buf, rows = _python_rows(F, golden_file("test.fq"))
    assert len(rows) >= 3
    for cf, cb in ((0, 10), (20, 20), (30, 30), (5, 0)):
        want, stats = loop_rows(buf, rows, cf, cb)
        got = X.trim_rows(buf, np.array(rows, dtype=np.int64), cb, cf)
        assert (got == want).all(), (cf, cb)
        ef = F.entryfunc_qualitytrim(cb, cf)
        for r, w in zip(rows, want):
            assert ef(buf, r, -1) == (buf[w[0] + 1:w[1]], buf[w[2]:w[3]], buf[w[4]:w[5]])
        assert (cf, cb) != (20, 20) or stats[0] >= 2


def expected_items(F, data, cf, cb, min_len=None, max_len=None, column="entry", fbufsize=20000):
    """What the iterator owes for entryfunc_qualitytrim: the default entryfunc's items, trimmed by the loop, None where
    the trimmed length is outside the bounds."""
    out = []
    for h, s, q in F.readfastq_iter(io.BytesIO(data), fbufsize, F.entryfunc, F.entrypos):
        if len(s) == len(q) and b"\n" not in q:
            a, b = loop_span(q, cf, cb)
            s, q = s[a:b], q[a:b]
        if (min_len is not None and len(s) < min_len) or (max_len is not None and len(s) > max_len):
            out.append(None)
        else:
            out.append({"entry": (h, s, q), "header": h, "sequence": s, "quality": q}[column])
    return out


def test_readfastq_iter_python_scanner(pkg):
    from fastqandfurious_amd import fastqandfurious as F
    data = golden_file("test.fq")
    want = expected_items(F, data, 20, 20, min_len=30)
    with open(os.path.join(GOLDEN_DIR, "data", "test.fq"), "rb") as fh:
        got = list(F.readfastq_iter(fh, 20000, F.entryfunc_qualitytrim(20, 20, min_len=30), F.entrypos))
    assert got == want and len(want) == 4 and want != list(F.readfastq_iter(io.BytesIO(data), 20000, F.entryfunc, F.entrypos))
    # (a cutoff that trims some of the reads away)
    want = expected_items(F, data, 30, 30, min_len=30)
    assert any(e is None for e in want) and any(e is not None for e in want)
    assert list(F.readfastq_iter(io.BytesIO(data), 20000, F.entryfunc_qualitytrim(30, 30, min_len=30), F.entrypos)) == want
    for col in ("sequence", "quality", "header"):
        got = list(F.readfastq_iter(io.BytesIO(data), 300, F.entryfunc_qualitytrim(20, 20, min_len=30, column=col), F.entrypos))
        assert got == expected_items(F, data, 20, 20, min_len=30, column=col)


def test_entryfunc_arguments(pkg):
    from fastqandfurious_amd import fastqandfurious as F
    for bad in (dict(cutoff_back=128), dict(cutoff_back=1, cutoff_front=-1), dict(cutoff_back=1, qual_base=256),
                dict(cutoff_back=1, column="nope")):
        with pytest.raises(ValueError):
            F.entryfunc_qualitytrim(**bad)


# ---- the device ------------------------------------------------------------------------------------------------------------
def device_trim(ctx, data, rows, cf, cb, base=33, sentinel=False, add=0, in_place=False):
    """rows (host int64[n][6]) trimmed by ffq_table_trim_quality over `data` (bytes / uint8 array) -> (rows, stats)"""
    import torch
    dbuf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda() if not hasattr(data, "data_ptr") else data
    t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 6)).cuda()
    out = t if in_place else torch.full_like(t, -77)
    stats = ctx.table_trim_quality(dbuf.data_ptr(), dbuf.numel(), t.data_ptr(), t.shape[0], cb, cf, base, d_out=out.data_ptr(),
                                   sentinel=sentinel, add=add)
    return out.cpu().numpy(), list(stats)


@pytest.mark.gpu
def test_hand_vectors_device(gpu_ctx):
    buf, rows, names, groups, tail = _groups()
    for (cf, cb, base), idx in groups.items():
        sub = np.array([rows[i] for i in idx] + [rows[i] for i in tail], dtype=np.int64)
        want, stats = loop_rows(buf, sub, cf, cb, base)
        got, gstats = device_trim(gpu_ctx, buf, sub, cf, cb, base)
        assert (got == want).all(), ((cf, cb, base), got.tolist(), want.tolist())
        assert gstats == stats
    # with a sentinel, coordinate 0 is the virtual newline: a quality that starts there is not trimmed
    sub = np.array([[0, 1, 2, 4, 0, 2], [0, 1, 2, 4, 1, 3]], dtype=np.int64)
    want, stats = loop_rows(b"\n" + buf, sub, 20, 20)
    got, gstats = device_trim(gpu_ctx, buf, sub, 20, 20, sentinel=True, add=0)
    assert (got == want).all() and gstats == stats and stats[2] == 1
    # no rows: nothing happens
    assert device_trim(gpu_ctx, buf, np.zeros((0, 6), dtype=np.int64), 20, 20)[1] == [0, 0, 0]


LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 4096, 4097, 70001)
REGIMES = ["uniform", "all-low"] + ["ends-%s" % k for k in (0, 1, 15, 16, 17, 64, 65, "n")]


def sweep_buffer(regime):
    """One buffer: for every residue r of 16 and every length, a record whose QUALITY starts at an address = r mod 16
    (sequence and quality lines of that length; '#' filler in between).  4096 / 4097 sit on either side of the length
    above which the library gives a row a wave of its own."""
    rng = np.random.default_rng(1234 + REGIMES.index(regime))
    parts, rows, at = [], [], 0

    def put(b):
        nonlocal at
        parts.append(b)
        at += len(b)
    put(b"#")
    for r in range(16):
        for n in LENGTHS:
            if regime == "uniform":
                q = rng.integers(0, 41, n)
            elif regime == "all-low":
                q = rng.integers(0, 6, n)
            else:
                k = regime.split("-")[1]
                k = n if k == "n" else min(int(k), n)
                q = rng.integers(30, 41, n)
                q[:k] = rng.integers(0, 6, k)
                q[n - k:] = rng.integers(0, 6, k)
            p0 = at
            put(b"@s\n")
            p2 = at
            put(b"A" * n + b"\n+\n")
            put(b"#" * ((r - at) % 16))
            p4 = at
            assert p4 % 16 == r
            put((q + 33).astype(np.uint8).tobytes() + b"\n")
            rows.append([p0, p0 + 2, p2, p2 + n, p4, p4 + n])
    return b"".join(parts), np.array(rows, dtype=np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("regime", REGIMES)
def test_length_and_alignment_sweep(gpu_ctx, regime):
    """every length on either side of a chunk, a group and the short / long split, at every residue of the quality's
    address, qualities that make the walks long, short, and complete; sentinel and add in every combination"""
    import torch
    buf, rows = sweep_buffer(regime)
    want, stats = loop_rows(buf, rows, 20, 20)
    if regime == "all-low":
        assert stats[0] == len(rows) and (want[:, 3] == want[:, 2]).all()
    dbuf = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).cuda()
    for sentinel in (0, 1):
        for add in (0, -1, (1 << 33) + 5):
            got, gstats = device_trim(gpu_ctx, dbuf, rows + sentinel + add, 20, 20, sentinel=bool(sentinel), add=add)
            bad = np.nonzero((got != want + sentinel + add).any(axis=1))[0]
            assert bad.size == 0, (sentinel, add, bad[:5], got[bad[:5]] - sentinel - add, want[bad[:5]])
            assert gstats == stats, (sentinel, add)


def table_of_quals(quals):
    """(bytes, rows) of four-line records with these quality values (arrays of Phred scores; the sequence is all 'A')"""
    buf, rows = bytearray(b"#"), []
    for q in quals:
        n = len(q)
        p0 = len(buf)
        buf += b"@h\n"
        p2 = len(buf)
        buf += b"A" * n + b"\n+\n"
        p4 = len(buf)
        buf += (np.asarray(q, dtype=np.int64) + 33).astype(np.uint8).tobytes() + b"\n"
        rows.append([p0, p0 + 2, p2, p2 + n, p4, p4 + n])
    return bytes(buf), np.array(rows, dtype=np.int64).reshape(-1, 6)


def check_device(ctx, buf, rows, cf=20, cb=20, combos=((0, 0, False),)):
    """the device against the loop, every row and the stats, for (sentinel, add, in place) combinations"""
    import torch
    want, stats = loop_rows(buf, rows, cf, cb)
    dbuf = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).cuda()
    for sentinel, add, in_place in combos:
        got, gstats = device_trim(ctx, dbuf, rows + sentinel + add, cf, cb, sentinel=bool(sentinel), add=add, in_place=in_place)
        bad = np.nonzero((got != want + sentinel + add).any(axis=1))[0]
        assert bad.size == 0, (sentinel, add, in_place, bad[:5], (got[bad[:5]] - sentinel - add).tolist(), want[bad[:5]].tolist())
        assert gstats == stats, (sentinel, add, in_place)
    return want, stats


def long_table(trimmed):
    """40 short reads and, at rows 13 and 31, one of 5000 and one of 70 000 quality bytes; trimmed: both ends of the long ones
    are low for more than the 1024 bytes of a chunk of the long rows' kernel, else the long ones are high throughout"""
    rng = np.random.default_rng(42)
    short = [rng.integers(0, 41, int(rng.integers(0, 101))) for _ in range(40)]
    longs = []
    for n, k in ((5000, 1100), (70000, 3000)):
        q = rng.integers(30, 41, n)
        if trimmed:
            q[:k] = rng.integers(0, 6, k)
            q[n - k:] = rng.integers(0, 6, k)
        longs.append(q)
    return table_of_quals(short[:13] + [longs[0]] + short[13:30] + [longs[1]] + short[30:])


def test_long_table_cuts_by_the_loop():
    """what test_long_reads_among_short_ones rests on, by the loop alone"""
    for trimmed in (True, False):
        buf, rows = long_table(trimmed)
        assert rows.shape[0] == 42 and [int(x) for x in (rows[:, 5] - rows[:, 4])[[13, 31]]] == [5000, 70000]
        assert ((rows[:, 5] - rows[:, 4])[[12, 14, 30, 32]] <= 100).all()
        want, stats = loop_rows(buf, rows, 20, 20)
        for i in (13, 31):
            front, back = want[i][4] - rows[i][4], rows[i][5] - want[i][5]
            if trimmed:
                assert front > 1024 and back > 1024 and want[i][5] > want[i][4]
            else:
                assert front == 0 and back == 0


@pytest.mark.gpu
@pytest.mark.parametrize("trimmed", (True, False))
def test_long_reads_among_short_ones(gpu_ctx, trimmed):
    """one read of 5000 and one of 70 000 quality bytes in a wave of short ones: either end of them is cut beyond the first
    chunk of the long rows' kernel; and the same reads with nothing to cut"""
    buf, rows = long_table(trimmed)
    want, stats = check_device(gpu_ctx, buf, rows, combos=((0, 0, False), (0, 0, True), (1, 7, False), (1, 7, True)))
    for i in (13, 31):
        front, back = want[i][4] - rows[i][4], rows[i][5] - want[i][5]
        assert (front > 1024 and back > 1024) if trimmed else (front == 0 and back == 0)


def idle_table(kind):
    """runs of 64, 65 and 300 rows that are empty (or ineligible) between ordinary rows, and 64 at the end -> (bytes, rows, idle mask)"""
    rng = np.random.default_rng(9)
    buf, rows = table_of_quals([rng.integers(0, 41, int(rng.integers(0, 151))) for _ in range(50)])
    p = int(rows[0][2])
    idle = [0, 1, p, p, p + 2, p + 2] if kind == "empty" else [0, 1, p, p + 30, -1, -1]
    table, mask, at = [], [], 0
    for run in (64, 65, 300):
        table += rows[at:at + 12].tolist() + [idle] * run
        mask += [False] * 12 + [True] * run
        at += 12
    table += rows[at:].tolist() + [idle] * 64
    mask += [False] * (50 - at) + [True] * 64
    return buf, np.array(table, dtype=np.int64), np.array(mask)


@pytest.mark.parametrize("kind", ("empty", "ineligible"))
def test_idle_table_by_the_loop(kind):
    buf, table, idle = idle_table(kind)
    want, stats = loop_rows(buf, table, 20, 20)
    assert idle.sum() == 64 + 65 + 300 + 64 and (want[idle] == table[idle]).all()
    assert stats[2] == (0 if kind == "empty" else idle.sum()) and stats[0] > 5


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("empty", "ineligible"))
def test_runs_of_rows_with_nothing_to_do(gpu_ctx, kind):
    """runs of 64, 65 and 300 consecutive rows that are empty (or ineligible) between ordinary rows, out of place and in place"""
    buf, table, idle = idle_table(kind)
    want, stats = check_device(gpu_ctx, buf, table, combos=((0, 0, False), (0, 0, True)))
    assert stats[2] == (0 if kind == "empty" else 64 + 65 + 300 + 64) and stats[0] > 5
    if kind == "ineligible":
        got, gstats = device_trim(gpu_ctx, buf, table, 20, 20)
        assert got[idle].tobytes() == table[idle].tobytes() and gstats[2] == idle.sum()


def many_rows_table():
    """140 000 rows of very short reads drawn from 3000 different ones"""
    rng = np.random.default_rng(3)
    pool = [rng.integers(0, 41, int(rng.integers(0, 13))) for _ in range(3000)]
    return table_of_quals([pool[i] for i in rng.integers(0, len(pool), 140000)])


@pytest.mark.gpu
def test_more_rows_than_one_pass_of_the_grid(gpu_ctx):
    """2048 workgroups of 32 rows: 65 536 rows a pass; 140 000 rows are a second and a third step, the last one with rows for
    some of the workgroups only"""
    buf, rows = many_rows_table()
    assert rows.shape[0] > 2 * 2048 * 32 and len(buf) < 6 << 20
    want, stats = check_device(gpu_ctx, buf, rows)
    assert stats[0] > 10000 and stats[2] == 0


# ---- more long rows than one pass of the long launch's grid (tests/grid_expect.py) ------------------------------------------------
TRIM_LONG = 4096                      # quality bytes above which the library gives a row a wave of its own (csrc/ffq_trim.h)


@functools.lru_cache(maxsize=None)
def long_list_pool():
    """(bytes, rows, long, rows out and [changed, removed, skipped] of every pool row ALONE, by the loop): 40 short reads, one of
    TRIM_LONG quality bytes, and six above it -- just above and up to 6000, low ends of several lengths, none, all low"""
    rng = np.random.default_rng(44)
    quals = [rng.integers(0, 41, int(rng.integers(0, 101))) for _ in range(40)] + [rng.integers(25, 41, TRIM_LONG)]
    for n, k in ((TRIM_LONG + 1, 0), (TRIM_LONG + 2, 7), (TRIM_LONG + 4, 1100), (4500, 300), (5200, 2000), (6000, 6000)):
        q = rng.integers(30, 41, n)
        q[:k] = rng.integers(0, 6, k)
        q[n - k:] = rng.integers(0, 6, k)
        quals.append(q)
    buf, rows = table_of_quals(quals)
    long = [i for i, q in enumerate(quals) if len(q) > TRIM_LONG]
    per = [loop_rows(buf, [r], 20, 20) for r in rows]
    return buf, rows, tuple(long), np.array([w[0] for w, _s in per], dtype=np.int64), np.array([st for _w, st in per], dtype=np.int64)


def long_list_table():
    """(rows in, rows out, stats, which rows are long) of pool[idx]"""
    _buf, rows, long, out, stats = long_list_pool()
    idx = GE.long_idx(long, [i for i in range(len(rows)) if i not in long], seed=45)
    return rows[idx], out[idx], stats[idx].sum(axis=0).tolist(), np.isin(idx, long)


def test_the_long_list_table_is_what_the_loop_says():
    buf, rows, long, out, stats = long_list_pool()
    n = rows[:, 5] - rows[:, 4]
    assert len(long) == 6 and sorted(n[list(long)])[:2] == [TRIM_LONG + 1, TRIM_LONG + 2] and max(n) == 6000 and (n == TRIM_LONG).any()
    assert (stats[list(long), 0] > 0).sum() == 5 and (stats[list(long), 0] == 0).sum() == 1
    rin, want, wstats, is_long = long_list_table()
    assert int(is_long.sum()) == GE.N_LONG > 2 * 1024 * 4 and len(rin) == 2 * GE.N_LONG >= 4096
    at = GE.sample_rows(len(rin), GE.P_LONG)
    loop, lstats = loop_rows(buf, rin[at], 20, 20)
    assert len(at) >= 2000 and (loop == want[at]).all()
    order = np.flatnonzero(is_long)
    for s in GE.passes(len(order), GE.P_LONG):                         # every long pool row in every pass over the list
        assert len({tuple(r) for r in rin[order[s]].tolist()}) == 6
    assert len(GE.passes(len(order), GE.P_LONG)) == 3


@pytest.mark.gpu
def test_more_long_rows_than_one_pass_of_the_grid(gpu_ctx):
    """9195 rows above TRIM_LONG among as many short ones: k_trim_long's 1024 workgroups of four waves take three steps over the
    list, the last for 1003 entries; out of place and in place, and with a sentinel and add = 7"""
    buf = long_list_pool()[0]
    rin, want, stats, is_long = long_list_table()
    assert int(is_long.sum()) > 2 * 1024 * 4 and len(rin) >= 4096
    for sentinel, add, in_place in ((0, 0, False), (0, 0, True), (1, 7, False)):
        got, gstats = device_trim(gpu_ctx, buf, rin + sentinel + add, 20, 20, sentinel=bool(sentinel), add=add, in_place=in_place)
        what = "sentinel %d, add %d, in place %s" % (sentinel, add, in_place)
        GE.same_rows(got[is_long], (want + sentinel + add)[is_long], GE.P_LONG, what + ": the long rows (list entries)")
        GE.same_rows(got, want + sentinel + add, GE.P_SHORT, what)
        assert gstats == stats, what


def scan_on_device(ctx, data):
    import torch
    dbuf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    cap = len(data) // 40 + 16
    table = torch.empty((cap, 6), dtype=torch.int64, device="cuda")
    rc, res = ctx.scan_device(dbuf.data_ptr(), len(data), table.data_ptr(), cap)
    assert rc == 0
    return dbuf, table[:int(res.n_records)]


@pytest.mark.gpu
def test_synth_single_every_row(gpu_ctx):
    import torch
    from fastqandfurious_amd import synth, index as X
    data = synth.single(0, 4096).tobytes()
    dbuf, table = scan_on_device(gpu_ctx, data)
    rows = table.cpu().numpy()
    assert rows.shape[0] == 4096
    for cf, cb in ((0, 10), (20, 20), (30, 30)):
        want, stats = loop_rows(data, rows, cf, cb)
        got, gstats = X.trim_rows_device(gpu_ctx, dbuf, table, cb, cf)
        got = got.cpu().numpy()
        assert (got == want).all(), (cf, cb, np.nonzero((got != want).any(axis=1))[0][:5])
        assert list(gstats) == stats, (cf, cb)
        front, back = want[:, 2] - rows[:, 2], rows[:, 3] - want[:, 3]
        empty = want[:, 3] == want[:, 2]
        if (cf, cb) == (20, 20):
            # the input covers the classes the kernel treats differently (by the loop's own result)
            assert ((back > 64) & ~empty).sum() >= 100 and ((front > 64) & ~empty).sum() >= 100
            assert ((back >= 1) & (back <= 15) & ~empty).sum() >= 1000
            assert empty.sum() >= 8
        if (cf, cb) == (30, 30):
            assert empty.sum() >= 1024          # the whole-read path
            # ... and the gather takes the table as the trim left it, the rows of length 0 among the others
            qual, off = X.select_column_device(gpu_ctx, dbuf, torch.from_numpy(want).cuda(), "quality", value_add=-33)
            exp = np.concatenate([np.frombuffer(data, dtype=np.uint8)[a:b] for a, b in want[:, 4:6]]).astype(np.int16) - 33
            assert (np.diff(off.cpu().numpy()) == want[:, 5] - want[:, 4]).all() and exp.size > 0
            assert (qual.cpu().numpy().astype(np.int16) == exp).all()
        if (cf, cb) == (0, 10):
            assert (front == 0).all() and back.max() <= 9 and ((back >= 1) & (back <= 9)).sum() >= 500
    # in place: the same rows
    want, stats = loop_rows(data, rows, 20, 20)
    t2 = table.clone()
    got, gstats = X.trim_rows_device(gpu_ctx, dbuf, t2, 20, 20, out=t2)
    assert got.data_ptr() == t2.data_ptr() and (t2.cpu().numpy() == want).all() and list(gstats) == stats
    # ... and what exists composes with it: the length filter drops what became too short, the gather returns the
    # trimmed quality, Phred-decoded
    kept = X.select_rows_device(gpu_ctx, t2, 30, None)
    wk = want[want[:, 3] - want[:, 2] >= 30]
    assert (kept.cpu().numpy() == wk).all()
    qual, off = X.select_column_device(gpu_ctx, dbuf, kept, "quality", value_add=-33)
    raw = np.frombuffer(data, dtype=np.uint8)
    exp = np.concatenate([raw[a:b] for a, b in wk[:, 4:6]]).astype(np.int16) - 33
    assert (qual.cpu().numpy().astype(np.int16) == exp).all() and (np.diff(off.cpu().numpy()) == wk[:, 5] - wk[:, 4]).all()


@pytest.mark.gpu
def test_synth_wrapped_rows_are_left_alone(gpu_ctx):
    """records wrapped over several lines come back byte-identical and counted; the single-line ones are trimmed"""
    from fastqandfurious_amd import synth, index as X
    data = synth.wrapped(0, 4096)[0].tobytes()
    dbuf, table = scan_on_device(gpu_ctx, data)
    rows = table.cpu().numpy()
    assert rows.shape[0] == 4096
    single = np.array([10 not in data[a:b] for a, b in rows[:, 4:6]])
    assert 100 < single.sum() < 1000 and ((rows[:, 3] - rows[:, 2])[single] <= 80).all()
    want, stats = loop_rows(data, rows, 20, 20)
    assert stats[2] == 4096 - single.sum() and (want[~single] == rows[~single]).all()
    got, gstats = X.trim_rows_device(gpu_ctx, dbuf, table, 20, 20)
    got = got.cpu().numpy()
    assert (got[~single] == rows[~single]).all()
    assert (got == want).all() and list(gstats) == stats
    assert (got[single] != rows[single]).any()


@pytest.mark.gpu
def test_errors(gpu_ctx):
    import torch
    from fastqandfurious_amd import hip, synth
    data = synth.single(0, 64).tobytes()
    dbuf, table = scan_on_device(gpu_ctx, data)
    n = table.shape[0]

    def call(t=table, out=None, cb=20, cf=20, base=33):
        return gpu_ctx.table_trim_quality(dbuf.data_ptr(), len(data), t.data_ptr(), n - 1, cb, cf, base,
                                          d_out=None if out is None else out.data_ptr())
    before = table.cpu().numpy().copy()
    for kw in (dict(cb=128), dict(cf=128), dict(cf=-1), dict(base=256), dict(t=table.view(-1)[1:]),
               dict(out=torch.empty_like(table).view(-1)[1:])):
        with pytest.raises(hip.FFQError) as e:
            call(**kw)
        assert e.value.code == hip.E_ARG, kw
    # a scan pending on the context
    t2 = torch.empty((n + 8, 6), dtype=torch.int64, device="cuda")
    gpu_ctx.scan_submit(dbuf.data_ptr(), len(data), t2.data_ptr(), n + 8)
    try:
        with pytest.raises(hip.FFQError) as e:
            call()
        assert e.value.code == hip.E_ARG
    finally:
        gpu_ctx.scan_wait()
    assert (table.cpu().numpy() == before).all()
    assert call() [2] == 0

"""FASTQ text from (buffer, table): ffq_table_render_fastq (device), index.render_rows (host).

The expectation of every test is the loop below -- the formula as include/ffq.h states it, over the three slices of the
reference's entryfunc -- never the package's own host implementation and never the device checking itself.  Coordinates:
a row minus `add` indexes the buffer the scanner saw; with a sentinel that buffer is b'\\n' + bytes, and its byte 0 is
never read.
"""
import functools
import io

import numpy as np
import pytest

import grid_expect as GE

from conftest import golden_file
from test_trim import loop_rows as loop_trim, scan_on_device

FILES = ("test.fq", "test_longqualityheader.fq", "test_multiline.fq")
GUARD = 0xEE


# ---- the rule ------------------------------------------------------------------------------------------------------
def loop_render(buf, rows, add=0, sentinel=False):
    """(text, offsets [n + 1], [bytes, rows rendered, rows skipped]) for rows (- add) over `buf` (bytes: the buffer as the
    scanner saw it, the sentinel's b'\\n' in front if there is one)"""
    out, off, stats = [], [0], [0, 0, 0]
    for row in rows:
        p0, p1, p2, p3, p4, p5 = (int(x) - add for x in row)
        ok = min(p0, p1, p2, p3, p4, p5) >= 0 and p0 + 1 <= p1 and p2 <= p3 and p4 <= p5 and max(p1, p3, p5) <= len(buf)
        if ok and sentinel and ((p2 == 0 and p3 > 0) or (p4 == 0 and p5 > 0)):
            ok = False                       # (a slice with the virtual newline in it is not inside the buffer)
        if ok:
            out.append(b"@" + buf[p0 + 1:p1] + b"\n" + buf[p2:p3] + b"\n+\n" + buf[p4:p5] + b"\n")
            stats[1] += 1
        else:
            out.append(b"")
            stats[2] += 1
        off.append(off[-1] + len(out[-1]))
    stats[0] = off[-1]
    return b"".join(out), off, stats


def entries_of(buf, rows, add=0):
    return [(buf[p0 + 1:p1], buf[p2:p3], buf[p4:p5]) for p0, p1, p2, p3, p4, p5 in (np.asarray(rows) - add).tolist()]


def golden_rows(golden, fn):
    return np.frombuffer(bytes.fromhex(golden["index"][fn]["index_hex"]), dtype=np.int64).reshape(-1, 6)


# ---- the host ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", FILES)
def test_render_rows_golden_files(pkg, golden, fn):
    from fastqandfurious_amd import index as X
    data, rows = golden_file(fn), golden_rows(golden, fn)
    want, _off, stats = loop_render(data, rows)
    assert stats[1] == len(rows) == 4 and want.count(b"\n+\n") >= 4
    assert X.render_rows(data, rows) == want
    assert X.render_rows(data, rows + 1000, shift=1000) == want
    assert X.render_rows(memoryview(data), rows[::-1]) == loop_render(data, rows[::-1])[0]
    # rows that are not renderable render as nothing
    odd = np.concatenate([rows[:1], [[5, 9, 12, 20, -1, -1]], rows[1:2], [[5, 9, 20, 12, 30, 40]],
                          [[5, 9, 12, 20, len(data) - 3, len(data) + 1]], [[5, 5, 12, 20, 30, 40]]])
    want2, _off, stats = loop_render(data, odd)
    assert stats[1:] == [2, 4] and X.render_rows(data, odd) == want2 == loop_render(data, rows[:2])[0]


@pytest.mark.parametrize("fn", FILES)
def test_rendered_golden_files_rescan_to_their_entries(pkg, golden, fn):
    from fastqandfurious_amd import index as X, fastqandfurious as F
    data, rows = golden_file(fn), golden_rows(golden, fn)
    text = X.render_rows(data, rows)
    got = list(F.readfastq_iter(io.BytesIO(text), 65536, F.entryfunc, F.entrypos))
    assert got == entries_of(data, rows)
    # (the entries the reference's own iterator gave for the file)
    assert [[h.hex(), s.hex(), q.hex()] for h, s, q in got] == golden["files"][fn]["tuples"]


# ---- the device ------------------------------------------------------------------------------------------------------
def device_render(ctx, data, rows, sentinel=False, add=0, misalign=0, cap=None, offsets=True):
    """rows (host int64[n][6]) rendered by ffq_table_render_fastq over `data` (bytes or a CUDA tensor) into an output that
    begins `misalign` bytes behind a 16-byte boundary and has `cap` bytes (None: what the loop needs is asked for first).
    Returns (rc, text bytes [cap], offsets or None, stats); asserts that no byte around the output was written."""
    import torch
    dbuf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda() if not hasattr(data, "data_ptr") else data
    t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 6)).cuda()
    n = t.shape[0]
    if cap is None:
        rc, st = ctx.table_render_fastq(dbuf.data_ptr(), dbuf.numel(), t.data_ptr(), n, None, 0, None, sentinel=sentinel, add=add)
        cap = st[0]
    out = torch.full((misalign + cap + 64,), GUARD, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda") if offsets else None
    rc, stats = ctx.table_render_fastq(dbuf.data_ptr(), dbuf.numel(), t.data_ptr(), n, out.data_ptr() + misalign, cap,
                                       off.data_ptr() if offsets else None, sentinel=sentinel, add=add)
    h = out.cpu().numpy()
    assert (h[:misalign] == GUARD).all() and (h[misalign + cap:] == GUARD).all(), "bytes outside the output were written"
    return rc, h[misalign:misalign + cap].tobytes(), (off.cpu().numpy() if offsets else None), list(stats)


def check(ctx, buf, rows, **kw):
    """device == loop, for rows over `buf` (no sentinel, add 0) handed over with the sentinel / add of kw"""
    s, add = int(bool(kw.get("sentinel", False))), kw.get("add", 0)
    want, off, stats = loop_render(buf, rows)
    rc, text, goff, gstats = device_render(ctx, kw.pop("dbuf", buf), np.asarray(rows, dtype=np.int64).reshape(-1, 6) + s + add, **kw)
    assert rc == 0 and gstats == stats, (gstats, stats, kw)
    assert goff is None or goff.tolist() == off, kw
    if text != want:
        bad = next(i for i in range(len(want)) if text[i] != want[i])
        raise AssertionError("first difference at output byte %d (row %d): %r != %r; %r"
                             % (bad, np.searchsorted(off, bad, side="right") - 1, text[bad - 8:bad + 24], want[bad - 8:bad + 24], kw))
    return want


def hand_buffer():
    """records by hand: (bytes, rows, names)"""
    buf, rows, names = bytearray(b"##"), [], []

    def rec(name, h, s, q, plus=b"+"):
        p0 = len(buf)
        buf.extend(b"@" + h + b"\n")
        p2 = len(buf)
        buf.extend(s + b"\n" + plus + b"\n")
        p4 = len(buf)
        buf.extend(q + b"\n")
        rows.append([p0, p0 + 1 + len(h), p2, p2 + len(s), p4, p4 + len(q)])
        names.append(name)
    rec("plain", b"read/1 x", b"ACGTACGTAC", b"IIIIIHHHH#")
    rec("an empty header", b"", b"ACG", b"III")
    rec("a read of length 0", b"e", b"", b"")
    rec("a read of length 1", b"one", b"A", b"!")
    rec("a repeated header on the + line", b"rep", b"ACGT", b"IIII", b"+rep")
    rec("a wrapped record", b"w", b"ACGT\nAC", b"IIII\nII")
    return buf, rows, names


@pytest.mark.gpu
def test_hand_vectors_device(gpu_ctx):
    buf, rows, names = hand_buffer()
    buf = bytes(buf)
    n = len(buf)
    # one row: the formula, spelled out
    rc, text, off, stats = device_render(gpu_ctx, buf, rows[:1])
    assert (rc, text, off.tolist(), stats) == (0, b"@read/1 x\nACGTACGTAC\n+\nIIIIIHHHH#\n", [0, 34], [34, 1, 0])
    # no rows: nothing, and off[0] = 0
    rc, text, off, stats = device_render(gpu_ctx, buf, np.zeros((0, 6), dtype=np.int64), cap=0)
    assert (rc, text, off.tolist(), stats) == (0, b"", [0], [0, 0, 0])
    for i, name in enumerate(names):
        want = check(gpu_ctx, buf, rows[i:i + 1])
        assert want.count(b"\n+\n") == 1, name
    assert check(gpu_ctx, buf, rows[1:2]) == b"@\nACG\n+\nIII\n"
    assert check(gpu_ctx, buf, rows[2:3]) == b"@e\n\n+\n\n"
    assert check(gpu_ctx, buf, rows[3:4]) == b"@one\nA\n+\n!\n"
    assert check(gpu_ctx, buf, rows[4:5]) == b"@rep\nACGT\n+\nIIII\n"
    assert check(gpu_ctx, buf, rows[5:6]) == b"@w\nACGT\nAC\n+\nIIII\nII\n"
    # rows that are not renderable render as nothing: off[i + 1] == off[i]
    r = rows[0]
    skipped = [[r[0], r[1], r[2], r[3], -1, -1],                 # a FASTA-style row
               [r[0], r[1], r[3], r[2], r[4], r[5]],             # p3 < p2
               [r[0], r[1], r[2], r[3], n - 3, n + 1],           # p5 past the buffer
               [r[0], r[0], r[2], r[3], r[4], r[5]],             # no room for the '@'
               [-1, r[1], r[2], r[3], r[4], r[5]],
               [r[0], n + 5, r[2], r[3], r[4], r[5]]]
    mixed = [rows[0], skipped[0], rows[1], skipped[1], skipped[2], rows[3]] + skipped[3:] + [rows[5]]
    want, off, stats = loop_render(buf, mixed)
    assert stats[1:] == [4, 6] and off[2] == off[1] and off[5] == off[3]
    check(gpu_ctx, buf, mixed)
    check(gpu_ctx, buf, skipped)                                   # nothing at all
    # a slice may end at the end of the buffer
    check(gpu_ctx, buf, [[r[0], r[1], r[2], r[3], n - 4, n]])
    # repeated, reversed, overlapping
    check(gpu_ctx, buf, rows[::-1])
    check(gpu_ctx, buf, [rows[0]] * 5 + rows + [rows[3]] * 40)
    check(gpu_ctx, buf, [[rows[0][0], rows[2][1], rows[0][2], rows[1][3], rows[0][4], rows[3][5]]])
    # with a sentinel, coordinate 0 is the virtual newline: a slice with a byte in it that begins there is outside
    sub = np.array([[2, 3, 0, 2, 4, 6], [2, 3, 1, 2, 4, 6], [2, 3, 0, 0, 4, 6]], dtype=np.int64)
    want, off, stats = loop_render(b"\n" + buf, sub, sentinel=True)
    rc, text, goff, gstats = device_render(gpu_ctx, buf, sub, sentinel=True, add=0)
    assert stats == gstats and stats[2] == 1 and text == want and goff.tolist() == off
    # without the offsets
    rc, text, goff, gstats = device_render(gpu_ctx, buf, rows, offsets=False)
    assert text == loop_render(buf, rows)[0] and goff is None


_SWEEP = {}
CORNERS = [(0, 0, 0), (40, 40, 40), (0, 40, 0), (40, 0, 40), (0, 0, 40), (10, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (16, 16, 16)]


def sweep():
    """A few thousand records whose header, sequence and quality lengths run over 0..40 independently (fixed seed), a
    row that is not renderable now and then.  Returns (bytes, rows, text, offsets, stats) -- computed once."""
    if not _SWEEP:
        rng = np.random.default_rng(20240607)
        parts, rows, at = [b"#"], [], 1
        letters = np.frombuffer(b"ACGTNacgtn0123456789:;<=>?@ABCDEFGHIJ", dtype=np.uint8)
        for i in range(3000):
            h, s, q = (int(x) for x in rng.integers(0, 41, 3))
            if i < len(CORNERS):
                h, s, q = CORNERS[i]
            hb, sb, qb = (letters[rng.integers(0, len(letters), k)].tobytes() for k in (h, s, q))
            rec = b"@" + hb + b"\n" + sb + b"\n+\n" + qb + b"\n"
            p0, p2 = at, at + h + 2
            p4 = p2 + s + 3
            rows.append([p0, p0 + 1 + h, p2, p2 + s, p4, p4 + q] if i % 97 != 50 else [p0, p0 + 1 + h, p2, p2 + s, -1, -1])
            parts.append(rec)
            at += len(rec)
        buf = b"".join(parts)
        rows = np.array(rows, dtype=np.int64)
        _SWEEP["v"] = (buf, rows) + loop_render(buf, rows)
    return _SWEEP["v"]


@pytest.mark.gpu
@pytest.mark.parametrize("sentinel", (False, True))
@pytest.mark.parametrize("add", (0, (1 << 32) + 5))
def test_length_and_alignment_sweep(gpu_ctx, sentinel, add):
    """every combination of three lengths 0..40 at every residue of the output address: d_out 0..15 bytes behind a
    16-byte boundary; 3000 rows are twelve workgroups of the copy kernel"""
    import torch
    buf, rows, want, off, stats = sweep()
    assert stats[2] == 31 and len(want) > 16 * 4096 and np.diff(off)[:2].tolist() == [6, 126]
    dbuf = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).cuda()
    shifted = rows + int(sentinel) + add
    shifted[rows < 0] = -1                        # (the -1 of a FASTA row is not a position: it does not move)
    for mis in range(16):
        rc, text, goff, gstats = device_render(gpu_ctx, dbuf, shifted, sentinel=sentinel, add=add, misalign=mis, cap=len(want))
        assert rc == 0 and gstats == stats and goff.tolist() == off, (mis, gstats)
        if text != want:
            bad = next(i for i in range(len(want)) if text[i] != want[i])
            raise AssertionError((mis, bad, np.searchsorted(off, bad, side="right") - 1, text[bad - 8:bad + 24], want[bad - 8:bad + 24]))


@pytest.mark.gpu
def test_one_long_row_among_short_ones(gpu_ctx):
    """a 100 kB row, and rows on either side of the output length above which the library gives a row a wave of its
    own (4096), among 600 short ones"""
    rng = np.random.default_rng(7)
    parts, rows, at = [b"##"], [], 2
    lens = [(5, 30, 30)] * 300 + [(10, 50000, 50000)] + [(5, 20, 20)] * 150 + [(2, 2044, 2044), (2, 2044, 2045), (2, 2045, 2045)] \
        + [(7, 33, 33)] * 150 + [(3000, 8000, 1)]
    for h, s, q in lens:
        hb, sb, qb = (rng.integers(65, 91, k, dtype=np.uint8).tobytes() for k in (h, s, q))
        rec = b"@" + hb + b"\n" + sb + b"\n+\n" + qb + b"\n"
        p0, p2 = at, at + h + 2
        p4 = p2 + s + 3
        rows.append([p0, p0 + 1 + h, p2, p2 + s, p4, p4 + q])
        parts.append(rec)
        at += len(rec)
    buf = b"".join(parts)
    want, off, stats = loop_render(buf, rows)
    assert want == buf[2:] and sorted(np.diff(off))[-5:] == [4096, 4097, 4098, 11007, 100016]
    for mis in (0, 5):
        check(gpu_ctx, buf, rows, misalign=mis)
    check(gpu_ctx, buf, rows[::-1], misalign=11, sentinel=True, add=-1)


@pytest.mark.gpu
def test_exact_capacity(gpu_ctx):
    from fastqandfurious_amd import hip
    buf, rows, want, off, stats = sweep()
    rows = rows[:700]
    want, off, stats = loop_render(buf, rows)
    total = len(want)
    for mis in (0, 3):
        rc, text, goff, gstats = device_render(gpu_ctx, buf, rows, misalign=mis, cap=total)     # (asserts the guard bytes)
        assert rc == 0 and text == want and gstats == stats
        rc, text, goff, gstats = device_render(gpu_ctx, buf, rows, misalign=mis, cap=total - 1)
        assert rc == hip.E_TABLE_FULL and gstats[0] == total and goff.tolist() == off
    # sizing call: no output at all
    rc, st = gpu_ctx.table_render_fastq(0, 0, 0, 0, None, 0, None)
    assert rc == 0 and st == (0, 0, 0)


# ---- more rows than one pass of the grid (tests/grid_expect.py) -------------------------------------------------------------
RENDER_LONG = 4096                    # output bytes above which the library gives a row a wave of its own (csrc/ffq_render.h)


@functools.lru_cache(maxsize=None)
def grid_pool():
    """(bytes, rows, idle, long, text of every pool row by the loop): the first 300 records of the sweep -- lengths 0..40, rows that
    render as nothing --, rows that point outside, records of RENDER_LONG - 1, RENDER_LONG output bytes and six above it"""
    sbuf, srows = sweep()[:2]
    parts, rows, at = [sbuf], srows[:300].tolist(), len(sbuf)
    r = rows[0]
    rows += [[r[0], r[1], r[2], r[3], len(sbuf) + (1 << 30), len(sbuf) + (1 << 30) + 4], [-5, r[1], r[2], r[3], r[4], r[5]],
             [r[0], r[0], r[2], r[3], r[4], r[5]]]
    rng = np.random.default_rng(71)
    for h, s, q in ((2, 2043, 2044), (2, 2044, 2044), (2, 2044, 2045), (2, 2045, 2045), (30, 2100, 2100), (2, 2500, 2500), (2, 1, 6000),
                    (3000, 600, 600)):
        hb, sb, qb = (rng.integers(65, 91, k, dtype=np.uint8).tobytes() for k in (h, s, q))
        rec = b"@" + hb + b"\n" + sb + b"\n+\n" + qb + b"\n"
        p0, p2 = at, at + h + 2
        p4 = p2 + s + 3
        rows.append([p0, p0 + 1 + h, p2, p2 + s, p4, p4 + q])
        parts.append(rec)
        at += len(rec)
    buf, rows = b"".join(parts), np.array(rows, dtype=np.int64)
    texts = [loop_render(buf, [r])[0] for r in rows]
    idle = [i for i, t in enumerate(texts) if not t]
    long = [i for i, t in enumerate(texts) if len(t) > RENDER_LONG]
    return buf, rows, tuple(idle), tuple(long), texts


def grid_want(idx):
    """(text, offsets, [bytes, rows rendered, rows skipped]) of pool[idx]"""
    texts = grid_pool()[4]
    lens = np.array([len(t) for t in texts], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens[idx])])
    return b"".join([texts[i] for i in idx.tolist()]), off, [int(off[-1]), int((lens[idx] > 0).sum()), int((lens[idx] == 0).sum())]


def grid_table(arrangement, long_rows=False):
    _buf, rows, idle, long, _texts = grid_pool()
    if long_rows:
        return GE.long_idx(long, [i for i in range(len(rows)) if i not in long], seed=73)
    # (of the rows around RENDER_LONG, the one at it and the one a byte above it: the text stays below 64 MiB)
    texts = grid_pool()[4]
    short = np.array([i for i in range(len(rows)) if i not in long[1:] and len(texts[i]) != RENDER_LONG - 1])
    idx = GE.table_idx(arrangement, GE.n_above(GE.P_WIDE), GE.P_WIDE, len(short), np.flatnonzero(np.isin(short, idle)), seed=73)
    return short[idx]


def check_above(ctx, dbuf, idx, P, what, sentinel=False, add=0, short_by_one=False):
    from fastqandfurious_amd import hip
    rows = grid_pool()[1]
    want, off, stats = grid_want(idx)
    moved = rows[idx] + int(sentinel) + add
    moved[rows[idx] < 0] = -1                     # (a negative entry is not a position: it does not move)
    rc, text, goff, gstats = device_render(ctx, dbuf, moved, sentinel=sentinel, add=add, misalign=3, cap=len(want) - int(short_by_one))
    GE.same_rows(goff, off, P, what + ": offsets")
    assert gstats == stats, (what, gstats, stats)
    got = np.frombuffer(text, dtype=np.uint8)
    if short_by_one:                                            # the need reported, nothing written, the offsets all the same
        assert rc == hip.E_TABLE_FULL and (got == GUARD).all(), what
        return
    assert rc == 0
    bad = np.flatnonzero(got != np.frombuffer(want, dtype=np.uint8))
    if bad.size:
        r = int(np.searchsorted(off, bad[0], side="right") - 1)
        raise AssertionError("%s: first difference at output byte %d: row %d, pass %d: %r != %r"
                             % (what, bad[0], r, r // P, text[bad[0] - 8:bad[0] + 24], want[bad[0] - 8:bad[0] + 24]))


@pytest.mark.parametrize("long_rows", (False, True))
def test_the_table_above_one_pass_is_what_the_loop_says(long_rows):
    buf, rows, idle, long, texts = grid_pool()
    lens = np.array([len(t) for t in texts])
    assert len(rows) < 400 and len(buf) < 1 << 20 and len(idle) >= 6 and len(long) == 6
    assert {RENDER_LONG - 1, RENDER_LONG, RENDER_LONG + 1, RENDER_LONG + 2} <= set(lens.tolist()) and max(lens) < 8000
    P = GE.P_LONG if long_rows else GE.P_WIDE
    for arrangement in ("random",) if long_rows else GE.ARRANGEMENTS:
        idx = grid_table(arrangement, long_rows)
        n = len(idx)
        assert (n == 2 * GE.N_LONG and int(np.isin(idx, long).sum()) == GE.N_LONG > 2 * 1024 * 4 and n >= 4096) if long_rows else n > 2048 * 256
        want, off, stats = grid_want(idx)
        assert len(want) == stats[0] < 64 << 20 and stats[1] + stats[2] == n
        at = GE.sample_rows(n, P)
        text, loff, lstats = loop_render(buf, rows[idx[at]])
        assert len(at) >= 2000 and (text, loff, lstats) == (grid_want(idx[at])[0], grid_want(idx[at])[1].tolist(), grid_want(idx[at])[2])
        assert all(want[off[i]:off[i + 1]] == texts[idx[i]] for i in at.tolist())
        order = np.flatnonzero(np.isin(idx, long)) if long_rows else np.arange(n)
        for k, s in enumerate(GE.passes(len(order), P)):
            part = idx[order[s]]
            if (arrangement, k > 0) in (("late work", False), ("early work", True)):
                assert set(part.tolist()) <= set(idle)
            elif long_rows:
                assert set(part.tolist()) == set(long)
            else:
                assert (lens[part] == 0).any() and (lens[part] == RENDER_LONG).any() and (lens[part] > RENDER_LONG).any() and \
                    (lens[part] == 6).any()


@pytest.mark.gpu
def test_more_rows_than_one_pass_of_the_grid(gpu_ctx):
    """two steps of every workgroup of k_render_sum and the copy behind it, the second for 301 of the 2048 with seven rows for the
    last of those: every byte, every offset, the three counts; "late work" with a sentinel and add; a capacity one byte short"""
    import torch
    dbuf = torch.from_numpy(np.frombuffer(grid_pool()[0], dtype=np.uint8).copy()).cuda()
    for arrangement in GE.ARRANGEMENTS:
        idx = grid_table(arrangement)
        assert len(idx) > 2048 * 256
        sentinel, add = (True, (1 << 32) + 5) if arrangement == "late work" else (False, 0)
        check_above(gpu_ctx, dbuf, idx, GE.P_WIDE, arrangement, sentinel, add)
        if arrangement == "random":
            check_above(gpu_ctx, dbuf, idx, GE.P_WIDE, arrangement + ", one byte short", short_by_one=True)


@pytest.mark.gpu
def test_more_long_rows_than_one_pass_of_the_grid(gpu_ctx):
    """9195 rows above RENDER_LONG output bytes among as many others: k_render_long's 1024 workgroups take three steps over the list"""
    import torch
    dbuf = torch.from_numpy(np.frombuffer(grid_pool()[0], dtype=np.uint8).copy()).cuda()
    idx = grid_table("random", long_rows=True)
    assert int(np.isin(idx, grid_pool()[3]).sum()) > 2 * 1024 * 4 and len(idx) >= 4096
    check_above(gpu_ctx, dbuf, idx, GE.P_WIDE, "long rows among short ones")
    check_above(gpu_ctx, dbuf, idx, GE.P_WIDE, "long rows, one byte short", short_by_one=True)


def _trim_filter_loop(data, rows, cf, cb, min_len):
    t, tstats = loop_trim(data, rows, cf, cb)
    return t[t[:, 3] - t[:, 2] >= min_len], tstats


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("single", "wrapped"))
def test_real_scans(gpu_ctx, kind):
    """scanned on the device, rendered untouched and after trim (20, 20) + filter (min 30); the text rescans, on the device,
    to rows whose slices are the rendered entries"""
    from fastqandfurious_amd import synth, index as X
    data = (synth.single(0, 20000) if kind == "single" else synth.wrapped(0, 5000)[0]).tobytes()
    dbuf, table = scan_on_device(gpu_ctx, data)
    rows = table.cpu().numpy()
    assert rows.shape[0] == (20000 if kind == "single" else 5000)

    def rendered_equals(tab, hrows):
        want, off, stats = loop_render(data, hrows)
        text, goff, gstats = X.render_rows_device(gpu_ctx, dbuf, tab)
        assert list(gstats) == stats and goff.cpu().numpy().tolist() == off
        got = text.cpu().numpy().tobytes()
        assert got == want
        # ... and back: the text scanned on the device
        d2, t2 = scan_on_device(gpu_ctx, got)
        assert entries_of(got, t2.cpu().numpy()) == entries_of(data, hrows)
        return got
    text = rendered_equals(table, rows)
    if kind == "single":
        assert text == data
    else:
        assert len(text) <= len(data) and text.count(b"\n") > 6 * 5000
    trimmed, tstats = X.trim_rows_device(gpu_ctx, dbuf, table, 20, 20)
    kept = X.select_rows_device(gpu_ctx, trimmed, 30, None)
    want_rows, want_tstats = _trim_filter_loop(data, rows, 20, 20, 30)
    assert list(tstats) == want_tstats and (kept.cpu().numpy() == want_rows).all()
    assert 0 < len(want_rows) < len(rows) or kind == "wrapped"
    text = rendered_equals(kept, want_rows)
    assert len(text) < len(data) or kind == "wrapped"


@pytest.mark.gpu
def test_errors(gpu_ctx):
    import torch
    from fastqandfurious_amd import hip, synth
    data = synth.single(0, 64).tobytes()
    dbuf, table = scan_on_device(gpu_ctx, data)
    n = table.shape[0]
    out = torch.empty(len(data) + 16, dtype=torch.uint8, device="cuda")

    def call(t=table, cap=len(data), rows=n):
        return gpu_ctx.table_render_fastq(dbuf.data_ptr(), len(data), t.data_ptr(), rows, out.data_ptr(), cap, None)
    for kw in (dict(t=table.view(-1)[1:], rows=n - 1), dict(cap=-1), dict(rows=-1)):
        with pytest.raises(hip.FFQError) as e:
            call(**kw)
        assert e.value.code == hip.E_ARG, kw
    # a scan pending on the context
    t2 = torch.empty((n + 8, 6), dtype=torch.int64, device="cuda")
    gpu_ctx.scan_submit(dbuf.data_ptr(), len(data), t2.data_ptr(), n + 8)
    try:
        with pytest.raises(hip.FFQError) as e:
            call()
        assert e.value.code == hip.E_ARG and "pending" in str(e.value)
    finally:
        gpu_ctx.scan_wait()
    rc, stats = call()
    assert rc == 0 and stats == (len(data), 64, 0) and out[:len(data)].cpu().numpy().tobytes() == data

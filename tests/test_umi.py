"""UMIs on the offset table: ffq_table_take_umi (the take: a row edit) and ffq_table_render_fastq_umi (the insert: the tag in the
rendered name), on the device.

The expectation of every test is a loop of tests/umi_expect.py -- the rule as include/ffq.h states it, written out there --,
never the package's own host implementation and never the device checking itself.
"""
import functools

import numpy as np
import pytest

import grid_expect as GE
import umi_expect as E

GUARD = 0xEE


# ---- the loop ----------------------------------------------------------------------------------------------------------
def test_the_loop_gives_the_hand_values():
    for seq, length, skip, tag, rest in E.HAND_TAKE:
        qual = bytes(33 + (j % 40) for j in range(len(seq)))
        assert E.loop_take(seq, qual, length, skip) == (tag, rest, qual[len(seq) - len(rest):]), seq
    for header, tags, prefix, delim, want in E.HAND_NAME:
        assert E.loop_name(header, tags, E.Rules(prefix=prefix, delim=delim)) == want, header
    buf, rows, n_bad = E.hand_table()
    want, stats = E.loop_take_rows(buf, rows, 8, 3)
    assert stats == [sum(1 for c in E.HAND_TAKE if len(c[0]) >= 8), sum(min(11, len(c[0])) for c in E.HAND_TAKE if len(c[0]) >= 8), n_bad]
    assert n_bad == 6 and (want[-n_bad:] == np.array(rows[-n_bad:])).all()
    # per_read with one mate too short: no tag at all
    b1, b2 = bytearray(b"#"), bytearray(b"#")
    r1, r2 = E.record(b1, b"p/1", b"ACGTACGTCC"), E.record(b2, b"p/2", b"ACG")
    t1, t2 = E.loop_take_rows(bytes(b1), [r1], 4, 0)[0], E.loop_take_rows(bytes(b2), [r2], 4, 0)[0]
    assert (t2 == [r2]).all() and t1[0, 2] == r1[2] + 4
    s1, s2 = E.Side(bytes(b1), t1), E.Side(bytes(b2), t2)
    for side, name in ((s1, b"p/1"), (s2, b"p/2")):
        text, _off, stats = E.loop_render(side, E.Rules("per_read", 4), s1, s2)
        assert stats[3] == 0 and text.startswith(b"@" + name + b"\n")
    text, _off, stats = E.loop_render(s2, E.Rules("read1", 4), s1, s2)
    assert text == b"@p/2:ACGT\nACG\n+\nIII\n" and stats == [len(text), 1, 0, 1]
    text, _off, stats = E.loop_render(s1, E.Rules("read1", 4, prefix=b"UMI"), s1, s2)
    assert text == b"@p/1:UMI_ACGT\nACGTCC\n+\nIIIIII\n"


def test_seeded_table_holds_what_it_should():
    buf, rows = E.seeded_table()
    assert 3900 <= len(rows) <= 4100 and len(buf) < 1 << 20
    lengths = [r[3] - r[2] for r in rows]
    assert min(lengths) == 0 and 200 < max(lengths) <= 221
    for length, skip in TAKES:
        want, stats = E.seeded_want(length, skip)
        assert stats[2] >= 40 and stats[0] > 400 and stats[0] + stats[2] < len(rows)
        assert any(w[3] == w[2] and r[3] > r[2] for w, r in zip(want.tolist(), rows))          # a read that is all tag


# ---- the take on the device ------------------------------------------------------------------------------------------------
TAKES = ((1, 0), (8, 3), (64, 64))


def device_take(ctx, data, rows, length, skip, sentinel=False, add=0, in_place=False):
    """rows (int64[n][6]) through ffq_table_take_umi over `data` (bytes) -> (rows, stats)"""
    import torch
    dbuf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 6)).cuda()
    out = t if in_place else torch.full_like(t, -77)
    stats = ctx.table_take_umi(dbuf.data_ptr(), dbuf.numel(), t.data_ptr(), t.shape[0], length, skip, d_out=out.data_ptr(),
                               sentinel=sentinel, add=add)
    return out.cpu().numpy(), list(stats)


def moved(rows, by):
    """rows + by; a negative entry is not a position and does not move"""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
    out = rows + by
    out[rows < 0] = -1
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("length,skip", TAKES)
def test_take_hand_table_device(gpu_ctx, length, skip):
    buf, rows, n_bad = E.hand_table()
    rows = np.array(rows, dtype=np.int64)
    want, stats = E.loop_take_rows(buf, rows, length, skip)
    assert stats[2] == n_bad
    for in_place in (False, True):
        got, gstats = device_take(gpu_ctx, buf, rows, length, skip, in_place=in_place)
        assert (got == want).all() and gstats == stats, (in_place, got.tolist(), want.tolist(), gstats, stats)
        # with a sentinel and add = 1000: the rows index b"\n" + bytes
        w2, s2 = E.loop_take_rows(b"\n" + buf, moved(rows, 1001), length, skip, add=1000, sentinel=True)
        assert s2 == stats and (w2 == moved(want, 1001)).all()
        got, gstats = device_take(gpu_ctx, buf, moved(rows, 1001), length, skip, sentinel=True, add=1000, in_place=in_place)
        assert (got == w2).all() and gstats == stats
    # with a sentinel, coordinate 0 is the virtual newline: a line with bytes in it that begins there is left alone
    data = b"ACGTACGTAC\n+\nIIIIIIIIII\n"
    sub = np.array([[-1, -1, 0, 10, 14, 24], [0, 0, 1, 11, 14, 24], [0, 0, 1, 1, 0, 0]], dtype=np.int64)
    want, stats = E.loop_take_rows(b"\n" + data, sub, 1, 0, sentinel=True)
    assert stats[2] == 1 and (want[0] == sub[0]).all()
    got, gstats = device_take(gpu_ctx, data, sub, 1, 0, sentinel=True, add=0)
    assert (got == want).all() and gstats == stats
    assert device_take(gpu_ctx, buf, np.zeros((0, 6), dtype=np.int64), length, skip)[1] == [0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("length,skip", TAKES)
def test_take_seeded_table_device(gpu_ctx, length, skip):
    buf, rows = E.seeded_table()
    want, stats = E.seeded_want(length, skip)
    for in_place in (False, True):
        got, gstats = device_take(gpu_ctx, buf, rows, length, skip, in_place=in_place)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (in_place, bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())
        assert gstats == stats
    w2, s2 = E.loop_take_rows(b"\n" + buf, moved(rows, 1001), length, skip, add=1000, sentinel=True)
    got, gstats = device_take(gpu_ctx, buf, moved(rows, 1001), length, skip, sentinel=True, add=1000)
    assert (got == w2).all() and gstats == s2 == stats


@functools.lru_cache(maxsize=None)
def take_pool():
    """(bytes, rows, idle, long): the pool of the take's tables above one pass of the grid -- the hand table, 260 seeded rows,
    empty rows, and rows around TAKE_LONG, one of them with a newline far inside its quality.  idle: nothing to do."""
    hbuf, hrows, n_bad = E.hand_table()
    buf, rows = bytearray(hbuf), [list(r) for r in hrows[:-1]]            # (without "past the buffer": the buffer grows)
    sbuf, srows = E.seeded_table()
    for i, r in enumerate(srows[:260]):
        rows.append(E.record(buf, b"s%d" % i, sbuf[r[2]:r[3]]))
    for i in range(8):
        rows.append(E.record(buf, b"e%d" % i, b""))
        rows.append(E.record(buf, b"f%d" % i, b"ACGTACGTACGT")[:4] + [-1, -1])
    rng = np.random.default_rng(23)
    long = []
    for i, n in enumerate((E.TAKE_LONG, E.TAKE_LONG + 1, 5000, 6000, 4500, 4100, 4097)):
        q = bytearray(b"I" * n)
        if n == 4500:
            q[4400] = 10
        if n > E.TAKE_LONG:
            long.append(len(rows))
        rows.append(E.record(buf, b"l%d" % i, E.body_of(rng, n), bytes(q)))
    rows.append([0, 1, len(buf) - 12, len(buf) + 1, 2, 15])              # past the buffer
    data = bytes(buf)
    idle = [i for i, r in enumerate(rows) if E.loop_take_rows(data, [r], 8, 3)[1][0] == 0]
    return data, tuple(tuple(r) for r in rows), tuple(idle), tuple(long)


@functools.lru_cache(maxsize=None)
def take_parts(sentinel=False, add=0):
    """the loop's answer for every pool row ALONE: (rows in, rows out, [changed, bases removed, skipped] each)"""
    buf, rows, _idle, _long = take_pool()
    seen = (b"\n" if sentinel else b"") + buf
    rin = moved(rows, add + int(sentinel))
    per = [E.loop_take_rows(seen, [r], 8, 3, add=add, sentinel=sentinel) for r in rin]
    return rin, np.array([w[0] for w, _s in per], dtype=np.int64), np.array([s for _w, s in per], dtype=np.int64)


def test_the_takes_pool_is_what_the_loop_says():
    buf, rows, idle, long = take_pool()
    assert len(rows) < 400 and len(buf) < 1 << 20 and len(long) == 6 and len(idle) > 20
    rin, rout, stats = take_parts()
    assert stats[list(long)][:, 0].sum() == 5 and stats[list(long)][:, 2].sum() == 1          # (the newline far inside a long quality)
    want, wstats = E.loop_take_rows(buf, rows, 8, 3)
    assert (want == rout).all() and stats.sum(axis=0).tolist() == wstats
    r2, o2, s2 = take_parts(True, 500)
    assert (o2 == moved(rout, 501)).all() and (s2 == stats).all()


@pytest.mark.gpu
def test_take_more_rows_than_one_pass_of_the_grid(gpu_ctx):
    """three steps of every workgroup of k_umi_take (2048 workgroups of 32 rows), the last one partial: every row and the three
    counts, out of place and in place; "late work" with a sentinel and add = 500"""
    buf, rows, idle, _long = take_pool()
    for arrangement in GE.ARRANGEMENTS:
        sentinel, add = (True, 500) if arrangement == "late work" else (False, 0)
        idx = GE.table_idx(arrangement, GE.n_above(GE.P_SHORT), GE.P_SHORT, len(rows), idle, seed=43)
        rin, rout, stats = take_parts(sentinel, add)
        for in_place in (False, True):
            got, gstats = device_take(gpu_ctx, buf, rin[idx], 8, 3, sentinel=sentinel, add=add, in_place=in_place)
            GE.same_rows(got, rout[idx], GE.P_SHORT, "%s, in place %s" % (arrangement, in_place))
            assert gstats == stats[idx].sum(axis=0).tolist(), (arrangement, in_place)


@pytest.mark.gpu
def test_take_more_long_rows_than_one_pass_of_the_grid(gpu_ctx):
    """9195 rows above TAKE_LONG among as many short ones: the long launch's 1024 workgroups take three steps over the list"""
    buf, rows, _idle, long = take_pool()
    idx = GE.long_idx(long, [i for i in range(len(rows)) if i not in long], seed=43)
    rin, rout, stats = take_parts()
    is_long = np.isin(idx, long)
    assert int(is_long.sum()) > 2 * 1024 * 4 and len(idx) >= 4096
    for in_place in (False, True):
        got, gstats = device_take(gpu_ctx, buf, rin[idx], 8, 3, in_place=in_place)
        GE.same_rows(got[is_long], rout[idx][is_long], GE.P_LONG, "long rows (list entries), in place %s" % in_place)
        GE.same_rows(got, rout[idx], GE.P_SHORT, "all rows, in place %s" % in_place)
        assert gstats == stats[idx].sum(axis=0).tolist()


# ---- the insert on the device ------------------------------------------------------------------------------------------------
def view_of(hip, dbuf, t, side):
    return hip.table_view(dbuf.data_ptr() if dbuf.numel() else 0, dbuf.numel(), t.data_ptr(), sentinel=side.sentinel, add=side.add)


def on_device(side):
    """(buffer, table) tensors of a Side: the buffer without its sentinel byte"""
    import torch
    data = side.seen[1:] if side.sentinel else side.seen
    dbuf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    t = torch.from_numpy(np.ascontiguousarray(side.rows, dtype=np.int64).reshape(-1, 6)).cuda()
    return dbuf, t


def device_render(ctx, side, rules, src1=None, src2=None, misalign=0, cap=None, keep=None):
    """side.rows rendered by ffq_table_render_fastq_umi into an output that begins `misalign` bytes behind a 16-byte boundary and
    has `cap` bytes (None: the sizing call says).  src1 / src2: Sides, or "self".  Returns (rc, text [cap], offsets, stats);
    asserts that no byte around the output was written.  keep: a dict that holds the tensors of a Side between calls."""
    import torch
    from fastqandfurious_amd import hip
    keep = {} if keep is None else keep

    def dev(s):
        if id(s) not in keep:
            keep[id(s)] = (s,) + on_device(s)
        return keep[id(s)][1:]
    dbuf, t = dev(side)
    views = [view_of(hip, dbuf, t, side)]
    for s in (src1, src2):
        views.append(None if s is None else views[0] if s is side else view_of(hip, *dev(s), s))
    n = t.shape[0]
    if cap is None:
        rc, st = ctx.table_render_fastq_umi(views[0], n, rules, None, 0, None, views[1], views[2])
        cap = st[0]
    out = torch.full((misalign + cap + 64,), GUARD, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    rc, stats = ctx.table_render_fastq_umi(views[0], n, rules, out.data_ptr() + misalign, cap, off.data_ptr(), views[1], views[2])
    h = out.cpu().numpy()
    assert (h[:misalign] == GUARD).all() and (h[misalign + cap:] == GUARD).all(), "bytes outside the output were written"
    return rc, h[misalign:misalign + cap].tobytes(), off.cpu().numpy(), list(stats)


def same_text(text, want, off, what):
    if text != want:
        n = min(len(text), len(want))
        bad = next((i for i in range(n) if text[i] != want[i]), n)
        raise AssertionError("%s: first difference at output byte %d (row %d): %r != %r"
                             % (what, bad, np.searchsorted(off, bad, side="right") - 1, text[max(bad - 8, 0):bad + 24], want[max(bad - 8, 0):bad + 24]))


def check(ctx, side, rules, src1=None, src2=None, **kw):
    want, off, stats = E.loop_render(side, rules, src1, src2)
    rc, text, goff, gstats = device_render(ctx, side, rules, src1, src2, **kw)
    assert rc == 0 and gstats == stats, (gstats, stats, rules)
    assert goff.tolist() == off, rules
    same_text(text, want, off, str(rules))
    return want, stats


@pytest.mark.gpu
def test_render_hand_names_device(gpu_ctx):
    for header, tags, prefix, delim, name in E.HAND_NAME:
        b1, b2 = bytearray(b"#"), bytearray(b"\n")
        r1 = E.record(b1, header, tags[0] + b"ACGTAC")
        r1 = [r1[0], r1[1], r1[2] + len(tags[0]), r1[3], r1[4] + len(tags[0]), r1[5]]
        s1 = E.Side(bytes(b1), [r1])
        if len(tags) == 1:
            want, stats = check(gpu_ctx, s1, E.Rules("read1", len(tags[0]), 0, prefix, delim), s1)
        else:
            r2 = E.record(b2, b"other", tags[1] + b"TT")
            r2 = [r2[0], r2[1], r2[2] + len(tags[1]), r2[3], r2[4] + len(tags[1]), r2[5]]
            s2 = E.Side(bytes(b2), [[x + 70 for x in r2]], 70, True)
            want, stats = check(gpu_ctx, s1, E.Rules("per_read", len(tags[0]), 0, prefix, delim), s1, s2)
        assert want == b"@" + name + b"\nACGTAC\n+\nIIIIII\n" and stats[3] == 1


@functools.lru_cache(maxsize=None)
def sweep(length, prefix):
    """Records whose header lengths run over 1..40 with the blank at {none, 0, the middle, the last byte} and whose reads -- behind
    a tag of `length` bases that the row has had taken off -- over 0..40; one row in 23 has a read shorter than the tag and
    carries none, one in 97 is a FASTA row.  Returns (Side, text, offsets, stats) by the loop -- computed once."""
    rng = np.random.default_rng([length, len(prefix)])
    letters = np.frombuffer(b"ACGTNacgtn0123456789:;<=>?@ABCDEFGHIJ", dtype=np.uint8)
    buf, rows, i = bytearray(b"#"), [], 0
    for h in range(1, 41):
        for blank in ("none", 0, "middle", "last"):
            for s in range(0, 41):
                hb = bytearray(letters[rng.integers(0, len(letters), h)].tobytes())
                if blank != "none":
                    hb[{0: 0, "middle": h // 2, "last": h - 1}[blank]] = (32, 9)[i % 2]
                short = i % 23 == 11
                tag = letters[rng.integers(0, 5, length if not short else length - 1)].tobytes()
                body = letters[rng.integers(0, len(letters), 0 if short else s)].tobytes()
                r = E.record(buf, bytes(hb), tag + body, bytes(rng.integers(33, 74, len(tag) + len(body), dtype=np.uint8)))
                if not short:
                    r = [r[0], r[1], r[2] + length, r[3], r[4] + length, r[5]]
                rows.append(r[:4] + [-1, -1] if i % 97 == 50 else r)
                i += 1
    side = E.Side(bytes(buf), np.array(rows, dtype=np.int64))
    return (side,) + E.loop_render(side, E.Rules("read1", length, 0, prefix), side)


@pytest.mark.gpu
@pytest.mark.parametrize("prefix", (b"", b"UMI"))
@pytest.mark.parametrize("length", (1, 7, 16, 17))
def test_render_chunk_sweep(gpu_ctx, length, prefix):
    """every header length 1..40 x blank place x read length 0..40, rows at every residue of the output address, d_out 3 bytes
    behind a 16-byte boundary: every way the pieces of a tagged row share or straddle a 16-byte chunk"""
    side, want, off, stats = sweep(length, prefix)
    n = len(side.rows)
    assert n == 40 * 4 * 41 and stats[3] > n * 9 // 10 and stats[2] > 50 and stats[1] - stats[3] > 200
    starts = np.array(off[:-1])[np.diff(off) > 0]
    assert set(((starts + 3) % 16).tolist()) == set(range(16))
    rc, text, goff, gstats = device_render(gpu_ctx, side, E.Rules("read1", length, 0, prefix), side, misalign=3, cap=len(want))
    assert rc == 0 and gstats == stats and goff.tolist() == off
    same_text(text, want, off, "sweep")


def two_buffers(n=600, length=6, seed=3):
    """mates in two buffers: (Side 1: no sentinel, add 0; Side 2: a sentinel and add = 1 << 33).  Mate 1 of pair i has had its
    tag taken if i % 5 != 1, mate 2 if i % 7 != 2; other source rows are too short, have a newline in the tag, are FASTA rows
    or point outside"""
    rng = np.random.default_rng(seed)
    bufs, rows = (bytearray(b"#"), bytearray(b"\n")), ([], [])
    for i in range(n):
        for k in (0, 1):
            took = (i % 5 != 1) if k == 0 else (i % 7 != 2)
            m = int(rng.integers(length, 60)) if took else int(rng.integers(0, length))
            s = E.body_of(rng, m)
            r = E.record(bufs[k], b"P%d%s/%d" % (i, (b" c", b"")[i % 2], k + 1), s)
            if took:
                r = [r[0], r[1], r[2] + length, r[3], r[4] + length, r[5]]
            odd = (i * 2 + k) % 61
            if odd == 3:
                r = [r[0], r[1] - 2, r[2], r[3], r[4], r[5]]               # "\n" inside [pos1 + 1, pos1 + 1 + len): the header's own
            elif odd == 9:
                r = [-1] * 6
            elif odd == 17:
                r = [r[0], (1 << 40), (1 << 40) + 30, r[3], r[4], r[5]]
            rows[k].append(r)
    add2 = 1 << 33
    t2 = np.array(rows[1], dtype=np.int64)
    m2 = t2 + add2
    m2[t2 < 0] = -1
    return E.Side(bytes(bufs[0]), np.array(rows[0], dtype=np.int64)), E.Side(bytes(bufs[1]), m2, add2, True)


@pytest.mark.gpu
@pytest.mark.parametrize("loc", ("read1", "read2", "per_read"))
def test_render_sources_in_two_buffers(gpu_ctx, loc):
    s1, s2 = two_buffers()
    keep = {}
    for side in (s1, s2):
        for prefix in (b"", b"Ab0"):
            rules = E.Rules(loc, 6, 0, prefix, b"+")
            want, stats = check(gpu_ctx, side, rules, s1 if loc != "read2" else None, s2 if loc != "read1" else None, misalign=5, keep=keep)
            assert 0 < stats[3] < stats[1] < len(side.rows)
    # no carrier anywhere: the output is ffq_table_render_fastq's, byte for byte
    import torch
    none = E.Side(s1.seen, np.array([[r[0], r[1], r[1] + 1, r[3], r[4], r[5]] for r in s1.rows.tolist()], dtype=np.int64))
    rc, text, goff, gstats = device_render(gpu_ctx, s1, E.Rules(loc, 6), none, none)
    assert gstats[3] == 0
    dbuf, t = on_device(s1)
    plain = torch.zeros(len(text) + 1, dtype=torch.uint8, device="cuda")
    rc2, st2 = gpu_ctx.table_render_fastq(dbuf.data_ptr(), dbuf.numel(), t.data_ptr(), t.shape[0], plain.data_ptr(), len(text),
                                          sentinel=False, add=0)
    assert rc == rc2 == 0 and list(st2) == gstats[:3] and plain.cpu().numpy()[:len(text)].tobytes() == text
    assert text == E.loop_render(s1, None)[0]


@functools.lru_cache(maxsize=None)
def long_side(length=12):
    """short rows, a 3000-byte header with its blank at 2900 (once below, once above RENDER_LONG output bytes), a 1-byte header
    in front of a 6000-base read, rows of RENDER_LONG - 1 .. + 2 output bytes (prefix b"UMI"); every read behind a taken tag of
    `length`"""
    rng = np.random.default_rng(9)
    buf, rows = bytearray(b"##"), []
    around = []
    for total in range(E.RENDER_LONG - 1, E.RENDER_LONG + 3):              # total = h + 2 s + 6 + (1 + 4 + length)
        h = 2 + (total - 11 - length) % 2
        around.append((h, (total - 11 - length - h) // 2))
    shapes = [(5, 30)] * 40 + [(3000, 100), (3000, 900)] + [(7, 33)] * 20 + [(1, 6000)] + around + [(40, 2500)] + \
        [(9, 20)] * 30 + [(5000, 5), (4089, 0)]
    for h, s in shapes:
        hb = bytearray(rng.integers(65, 91, h, dtype=np.uint8).tobytes())
        if h == 3000:
            hb[2900] = 32
        if h == 5000:
            hb[4999] = 9
        r = E.record(buf, bytes(hb), E.body_of(rng, length + s))
        rows.append([r[0], r[1], r[2] + length, r[3], r[4] + length, r[5]])
    return E.Side(bytes(buf), np.array(rows, dtype=np.int64))


@pytest.mark.gpu
def test_render_long_rows(gpu_ctx):
    side = long_side()
    rules = E.Rules("read1", 12, 0, b"UMI")
    want, off, stats = E.loop_render(side, rules, side)
    lens = np.diff(off)
    assert {E.RENDER_LONG - 1, E.RENDER_LONG, E.RENDER_LONG + 1, E.RENDER_LONG + 2} <= set(lens.tolist()) and stats[3] == len(side.rows)
    assert want.count(b":UMI_") == len(side.rows) and (lens > E.RENDER_LONG).sum() >= 6
    for mis in (0, 5):
        check(gpu_ctx, side, rules, side, misalign=mis)
    rev = E.Side(side.seen, side.rows[::-1].copy())
    check(gpu_ctx, rev, rules, rev, misalign=11)


@pytest.mark.gpu
def test_render_exact_capacity(gpu_ctx):
    from fastqandfurious_amd import hip
    side, _want, _off, _stats = sweep(7, b"UMI")
    side = E.Side(side.seen, side.rows[:700])
    rules = E.Rules("read1", 7, 0, b"UMI")
    want, off, stats = E.loop_render(side, rules, side)
    for mis in (0, 3):
        rc, text, goff, gstats = device_render(gpu_ctx, side, rules, side, misalign=mis, cap=len(want))      # (asserts the guard bytes)
        assert rc == 0 and text == want and gstats == stats
        rc, text, goff, gstats = device_render(gpu_ctx, side, rules, side, misalign=mis, cap=len(want) - 1)
        assert rc == hip.E_TABLE_FULL and gstats[0] == len(want) and goff.tolist() == off
        assert set(text) == {GUARD}                                      # the output is not touched


# ---- more rows than one pass of the capped grids (tests/grid_expect.py) ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def render_pool():
    """(Side of the pool, idle, long, text of every pool row by the loop): 300 rows of a sweep -- tagged rows, rows without a
    tag, rows that render as nothing --, rows that point outside, and the long side's rows"""
    sw = sweep(7, b"UMI")[0]
    buf, rows = bytearray(sw.seen), sw.rows[::22][:300].tolist()
    r = rows[0]
    rows += [[r[0], r[1], r[2], r[3], len(buf) + (1 << 30), len(buf) + (1 << 30) + 4], [-5, r[1], r[2], r[3], r[4], r[5]],
             [r[0], r[0], r[2], r[3], r[4], r[5]]]
    ls = long_side(7)
    at = len(buf)
    buf += ls.seen
    rows += (ls.rows[40:] + at).tolist()
    side = E.Side(bytes(buf), np.array(rows, dtype=np.int64))
    rules = E.Rules("read1", 7, 0, b"UMI")
    texts = [E.loop_render(E.Side(side.seen, side.rows[i:i + 1]), rules, E.Side(side.seen, side.rows[i:i + 1]))[0] for i in range(len(rows))]
    idle = [i for i, t in enumerate(texts) if not t]
    long = [i for i, t in enumerate(texts) if len(t) > E.RENDER_LONG]
    return side, tuple(idle), tuple(long), texts


def render_want(idx):
    texts = render_pool()[3]
    lens = np.array([len(t) for t in texts], dtype=np.int64)
    tagged = np.array([b":UMI_" in t for t in texts])
    off = np.concatenate([[0], np.cumsum(lens[idx])])
    return b"".join([texts[i] for i in idx.tolist()]), off, [int(off[-1]), int((lens[idx] > 0).sum()), int((lens[idx] == 0).sum()),
                                                             int(tagged[idx].sum())]


def render_above(ctx, idx, P, what, sentinel=False, add=0, short_by_one=False):
    from fastqandfurious_amd import hip
    pool = render_pool()[0]
    want, off, stats = render_want(idx)
    rows = pool.rows[idx] + int(sentinel) + add
    rows[pool.rows[idx] < 0] = -1
    side = E.Side((b"\n" if sentinel else b"") + pool.seen, rows, add, sentinel)
    rc, text, goff, gstats = device_render(ctx, side, E.Rules("read1", 7, 0, b"UMI"), side, misalign=3, cap=len(want) - int(short_by_one))
    GE.same_rows(goff, off, P, what + ": offsets")
    assert gstats == stats, (what, gstats, stats)
    if short_by_one:
        assert rc == hip.E_TABLE_FULL and set(text) == {GUARD}, what
        return
    assert rc == 0
    got = np.frombuffer(text, dtype=np.uint8)
    bad = np.flatnonzero(got != np.frombuffer(want, dtype=np.uint8))
    if bad.size:
        r = int(np.searchsorted(off, bad[0], side="right") - 1)
        raise AssertionError("%s: first difference at output byte %d: row %d, pass %d: %r != %r"
                             % (what, bad[0], r, r // P, text[bad[0] - 8:bad[0] + 24], want[bad[0] - 8:bad[0] + 24]))


def render_idx(arrangement, long_rows=False):
    side, idle, long, texts = render_pool()
    if long_rows:
        return GE.long_idx(long, [i for i in range(len(side.rows)) if i not in long], seed=79)
    # (of the rows of a thousand bytes and more, the one at RENDER_LONG and the one a byte above it: the text stays below 64 MiB)
    short = np.array([i for i, x in enumerate(texts) if len(x) < 1000 or len(x) in (E.RENDER_LONG, E.RENDER_LONG + 1)])
    assert len(short) > 300 and sum(1 for i in short if i in long) == 1
    idx = GE.table_idx(arrangement, GE.n_above(GE.P_WIDE), GE.P_WIDE, len(short), np.flatnonzero(np.isin(short, idle)), seed=79)
    return short[idx]


def test_the_renders_pool_is_what_the_loop_says():
    side, idle, long, texts = render_pool()
    assert len(side.rows) < 400 and len(side.seen) < 1 << 20 and len(idle) >= 6 and len(long) >= 6
    for arrangement in GE.ARRANGEMENTS:
        idx = render_idx(arrangement)
        want, off, stats = render_want(idx)
        assert len(idx) > 2048 * 256 and stats[0] < 64 << 20 and stats[3] > 0
        at = GE.sample_rows(len(idx), GE.P_WIDE, 300)
        sub = E.Side(side.seen, side.rows[idx[at]])
        assert E.loop_render(sub, E.Rules("read1", 7, 0, b"UMI"), sub)[0] == render_want(idx[at])[0]


@pytest.mark.gpu
def test_render_more_rows_than_one_pass_of_the_grid(gpu_ctx):
    """two steps of every workgroup of k_umi_render_sum (2048 workgroups of 256 rows) and the copy behind it: every byte, every
    offset, the four counts; "late work" with a sentinel and add; a capacity one byte short"""
    for arrangement in GE.ARRANGEMENTS:
        idx = render_idx(arrangement)
        sentinel, add = (True, (1 << 32) + 5) if arrangement == "late work" else (False, 0)
        render_above(gpu_ctx, idx, GE.P_WIDE, arrangement, sentinel, add)
        if arrangement == "random":
            render_above(gpu_ctx, idx, GE.P_WIDE, arrangement + ", one byte short", short_by_one=True)


@pytest.mark.gpu
def test_render_more_long_rows_than_one_pass_of_the_grid(gpu_ctx):
    """9195 rows above RENDER_LONG output bytes among as many others: k_umi_render_long's 1024 workgroups take three steps"""
    idx = render_idx("random", long_rows=True)
    assert int(np.isin(idx, render_pool()[2]).sum()) > 2 * 1024 * 4 and len(idx) >= 4096
    render_above(gpu_ctx, idx, GE.P_WIDE, "long rows among short ones")


# ---- errors ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors_device(gpu_ctx):
    import torch
    from fastqandfurious_amd import hip
    buf, rows, _n = E.hand_table()
    side = E.Side(buf, np.array(rows, dtype=np.int64))
    dbuf, t = on_device(side)
    raw = torch.zeros(t.numel() + 1, dtype=torch.int64, device="cuda")
    for length, skip in ((0, 0), (65, 0), (8, -1), (8, 65)):
        with pytest.raises(hip.FFQError, match="ffq_table_take_umi"):
            gpu_ctx.table_take_umi(dbuf.data_ptr(), dbuf.numel(), t.data_ptr(), t.shape[0], length, skip)
    with pytest.raises(hip.FFQError, match="16-byte aligned"):
        gpu_ctx.table_take_umi(dbuf.data_ptr(), dbuf.numel(), t.data_ptr(), t.shape[0], 8, 0, d_out=raw.data_ptr() + 8)
    v = view_of(hip, dbuf, t, side)
    for bad in (E.Rules("nowhere"), E.Rules(length=0), E.Rules(length=65), E.Rules(skip=65), E.Rules(prefix=b"A" * 17), E.Rules(prefix=b"a-b"),
                E.Rules(delim=b" "), E.Rules(delim=b"\x7f"), E.Rules(delim=b"::")):
        with pytest.raises(hip.FFQError, match="ffq_table_render_fastq_umi"):
            gpu_ctx.table_render_fastq_umi(v, t.shape[0], bad, None, 0, None, v, v)
    for loc, s1, s2 in (("read1", None, v), ("read2", v, None), ("per_read", v, None), ("per_read", None, v)):
        with pytest.raises(hip.FFQError, match="source"):
            gpu_ctx.table_render_fastq_umi(v, t.shape[0], E.Rules(loc), None, 0, None, s1, s2)
    # no rows: nothing, and off[0] = 0
    off = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    rc, st = gpu_ctx.table_render_fastq_umi(v, 0, E.Rules(), None, 0, off.data_ptr(), v, None)
    assert rc == 0 and st == (0, 0, 0, 0) and off.item() == 0

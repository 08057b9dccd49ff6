"""Per-cycle base and quality statistics of a table: ffq_table_stats (device), FastqStats / index.stats_rows (host).

The expectation of every test is the plain loop below -- the table of include/ffq.h written out here, byte by byte -- never
FastqStats itself.  Bulk cases use a numpy form of that loop (np_words), which is checked against the plain loop on the
hand vectors.  Every comparison is exact equality over every word.  Coordinates: a row minus `add` indexes the buffer the
scanner saw; with a sentinel that buffer is b'\\n' + bytes.
"""
import functools
import io

import numpy as np
import pytest

import grid_expect as GE

TILE = 152              # cycles per LDS tile, and the bases above which a row gets a wave of its own (csrc/ffq_stats.h: STATS_TILE)
GROUP_BYTES = 32        # bytes of a row that its 8 lanes take per step (STATS_G * 4)
WAVE_BYTES = 256        # ... and the 64 lanes of the long rows' kernels


def n_words(C):
    return 8 + C * 101 + (C + 1) + 96 + 101


# ---- the rule ------------------------------------------------------------------------------------------------------
def loop_words(records, C, qbase=33):
    """records: (sequence, quality) of an eligible row, None for any other row -> the words, by a plain loop over bytes"""
    w = [0] * n_words(C)
    for rec in records:
        if rec is None:
            w[1] += 1
            continue
        seq, q = rec
        n = len(seq)
        w[0] += 1
        w[2] += n
        w[8 + 101 * C + min(n, C)] += 1
        sv = gc = 0
        for i in range(n):
            v = min(max(q[i] - qbase, 0), 95)
            b = seq[i]
            cls = 0 if b in b"Aa" else 1 if b in b"Cc" else 2 if b in b"Gg" else 3 if b in b"Tt" else 4
            sv += v
            if cls in (1, 2):
                gc += 1
            if cls == 4:
                w[6] += 1
            if i < C:
                w[8 + i * 5 + cls] += 1
                w[8 + 5 * C + i * 96 + v] += 1
            else:
                w[3] += 1
        w[4] += sv
        w[5] += gc
        if n > 0:
            w[8 + 102 * C + 1 + sv // n] += 1
            w[8 + 102 * C + 97 + (100 * gc) // n] += 1
    return np.array(w, dtype=np.uint64)


_CLS = np.full(256, 4, dtype=np.int64)
_CLS[[65, 97]], _CLS[[67, 99]], _CLS[[71, 103]], _CLS[[84, 116]] = 0, 1, 2, 3


def np_words(records, C, qbase=33):
    """the same loop, a record at a time; equal records are counted once and multiplied"""
    w = np.zeros(n_words(C), dtype=np.int64)
    mult = {}
    for rec in records:
        mult[rec] = mult.get(rec, 0) + 1
    for rec, k in mult.items():
        if rec is None:
            w[1] += k
            continue
        seq, q = rec
        n = len(seq)
        w[0] += k
        w[2] += k * n
        w[8 + 101 * C + min(n, C)] += k
        if n == 0:
            continue
        cls = _CLS[np.frombuffer(seq, dtype=np.uint8)]
        v = np.clip(np.frombuffer(q, dtype=np.uint8).astype(np.int64) - qbase, 0, 95)
        m = min(n, C)
        i = np.arange(m)
        w[8 + i * 5 + cls[:m]] += k                      # (one cycle each: no index twice)
        w[8 + 5 * C + i * 96 + v[:m]] += k
        sv, gc = int(v.sum()), int(((cls == 1) | (cls == 2)).sum())
        w[3] += k * (n - m)
        w[4] += k * sv
        w[5] += k * gc
        w[6] += k * int((cls == 4).sum())
        w[8 + 102 * C + 1 + sv // n] += k
        w[8 + 102 * C + 97 + (100 * gc) // n] += k
    return w.astype(np.uint64)


def records_of(buf, rows, add=0):
    """(sequence, quality) or None for every row (+ add) over `buf` (bytes: the buffer as the scanner saw it)"""
    out = []
    for row in np.asarray(rows, dtype=np.int64).reshape(-1, 6).tolist():
        p2, p3, p4, p5 = (x - add for x in row[2:])
        ok = min(p2, p3, p4, p5) >= 0 and p2 <= p3 <= len(buf) and p4 <= p5 <= len(buf) and p3 - p2 == p5 - p4
        if ok and (10 in buf[p2:p3] or 10 in buf[p4:p5]):
            ok = False
        out.append((buf[p2:p3], buf[p4:p5]) if ok else None)
    return out


def check_invariants(w, C):
    w = w.astype(np.int64)
    cb, cq = w[8:8 + 5 * C].sum(), w[8 + 5 * C:8 + 101 * C].sum()
    lh = w[8 + 101 * C:8 + 102 * C + 1]
    rq, gh = w[8 + 102 * C + 1:8 + 102 * C + 97], w[8 + 102 * C + 97:]
    assert cb == cq == w[2] - w[3]
    assert lh.sum() == w[0]
    assert rq.sum() == gh.sum() == w[0] - lh[0]
    assert w[7] == 0


# ---- tables by hand ------------------------------------------------------------------------------------------------
def record(buf, rows, seq, qual=None, header=b"@h", last=False):
    """append a four-line record to `buf` (bytearray) and its row to `rows`; last: without the newline behind the quality"""
    qual = b"I" * len(seq) if qual is None else qual
    p0 = len(buf)
    buf += header + b"\n"
    p2 = len(buf)
    buf += seq + b"\n+\n"
    p4 = len(buf)
    buf += qual + (b"" if last else b"\n")
    rows.append([p0, p2 - 1, p2, p2 + len(seq), p4, p4 + len(qual)])


def one_read(rng, n, alphabet=b"ACGTNacgtn.", qlo=33, qhi=75):
    alpha = np.frombuffer(alphabet, dtype=np.uint8)
    return alpha[rng.integers(0, len(alpha), n)].tobytes(), rng.integers(qlo, qhi, n, dtype=np.uint8).tobytes()


def table_of(reads, start_mod16=None, last=False):
    """(bytes, rows) of four-line records; start_mod16: the sequence of record i starts at an address = start_mod16[i] mod 16"""
    buf, rows = bytearray(b"#"), []
    for i, (s, q) in enumerate(reads):
        if start_mod16 is not None:
            buf += b"#" * ((start_mod16[i] - (len(buf) + 3)) % 16)
        record(buf, rows, s, q, last=last and i == len(reads) - 1)
    return bytes(buf), np.array(rows, dtype=np.int64).reshape(-1, 6)


def lengths_for(C):
    """0..9 and the powers of two around a group's and a wave's step, one below, at and above the tile (= the long-row
    threshold) and its multiples, and the same around C"""
    base = [0, 1, 3, 4, 5, 7, 8, 9, GROUP_BYTES - 1, GROUP_BYTES, GROUP_BYTES + 1, 63, 64, 65, TILE - 1, TILE, TILE + 1,
            5 * GROUP_BYTES - 1, 5 * GROUP_BYTES, 5 * GROUP_BYTES + 1, WAVE_BYTES - 1, WAVE_BYTES, WAVE_BYTES + 1, 2 * TILE - 1,
            2 * TILE, 2 * TILE + 1, TILE + WAVE_BYTES - 1, TILE + WAVE_BYTES, TILE + WAVE_BYTES + 1, 2 * WAVE_BYTES + 3]
    return base + [max(C - 1, 0), C, C + 1, 3 * C + 5]


HAND = [(b"", b""), (b"A", b"!"), (b"ACGTN", b"I5?#~"), (b"acgtnACGTN", b"IIIII!!!!~"), (b"GGGCCC", b"++++++"),
        (b"N" * 9, b"J" * 9), (b"ACGT" * 40, bytes(range(33, 73)) * 4)]


def ineligible_rows(buf, rows):
    """appends the rows the rule does not apply to; returns how many"""
    n0 = len(rows)
    record(buf, rows, b"ACGTAC\nGTACGT", b"IIIIII\nIIIIII")           # a wrapped record
    record(buf, rows, b"ACGTAC\nGTACGT", b"IIIIIIIIIIIII")             # a newline in the sequence only
    record(buf, rows, b"ACGTACGGTACGT", b"IIIIII\nIIIIII")             # ... in the quality only
    record(buf, rows, b"A" * 200 + b"\n" + b"C" * 99, b"I" * 300)       # ... in a long row's sequence
    record(buf, rows, b"A" * 300, b"I" * 299 + b"\n")                   # ... as a long row's last quality byte
    record(buf, rows, b"ACGTACGT", b"IIII")                             # unequal lengths
    p0 = rows[-1][0]
    rows.append(rows[-1][:4] + [-1, -1])                                # a FASTA row
    rows.append([p0, p0 + 2, p0 + 3, p0 + 7, len(buf) - 3, len(buf) + 1])   # past the buffer
    rows.append([p0, p0 + 2, len(buf) - 3, len(buf) + 1, p0 + 3, p0 + 7])
    rows.append([p0, p0 + 2, -5, -1, p0 + 11, p0 + 15])                 # in front of the buffer
    rows.append([p0, p0 + 2, p0 + 7, p0 + 3, p0 + 15, p0 + 11])         # ends in front of starts
    return len(rows) - n0


def hand_table():
    buf, rows = bytearray(b"##"), []
    for i, (s, q) in enumerate(HAND):
        record(buf, rows, s, q, header=b"@h%d" % i)
    tail = len(rows)
    n_bad = ineligible_rows(buf, rows)
    return bytes(buf), np.array(rows, dtype=np.int64), tail, n_bad


# ---- mixed reads as files hold them (the generator of tests/test_stream_pipeline.py, copied: that file is not edited) ---
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_NOISE = np.frombuffer(b"@+#5?I", dtype=np.uint8)
LONG_LENGTHS = (4095, 4096, 4097, 9000, 70000)


def _quality(rng, n, kind):
    if kind == 3:
        return b"#" * n
    if kind == 4:
        return _NOISE[rng.integers(0, len(_NOISE), n)].tobytes()
    q = rng.integers(33 + 25, 33 + 41, n, dtype=np.uint8)
    if kind in (1, 2):
        k = int(rng.integers(1, n + 1))
        bad = rng.integers(33 + 2, 33 + 16, k, dtype=np.uint8)
        if kind == 1:
            q[n - k:] = bad
        else:
            q[:k] = bad
    return q.tobytes()


def _wrap(b, w):
    return b"\n".join(b[i:i + w] for i in range(0, len(b), w))


def mixed_corpus(count, seed, long_every=0, wrap=True, adapter=None):
    """wrap: every seventh record or so is wrapped over several lines; adapter: implanted into a third of the reads"""
    rng = np.random.default_rng(seed)
    parts = []
    for i in range(count):
        n = int(rng.integers(1, 40)) if rng.random() < 0.2 else int(rng.integers(40, 321))
        wrapped = rng.random() < 0.15 and n >= 2 and wrap
        if long_every and i % long_every == long_every // 2:
            n, wrapped = LONG_LENGTHS[(i // long_every) % len(LONG_LENGTHS)], False
        head = b"" if rng.random() < 0.03 else b"r%d:%d/%d" % (i, int(rng.integers(0, 10 ** int(rng.integers(1, 9)))), i % 2 + 1)
        plus = b"+" + head if rng.random() < 0.2 else b"+"
        seq = _ACGT[rng.integers(0, 4, n)].tobytes()
        if rng.random() < 0.1:
            seq = seq.replace(b"A", b"N", 3).lower() if rng.random() < 0.5 else seq.replace(b"G", b"N", 2)
        if adapter is not None and rng.random() < 0.33:
            p = int(rng.integers(0, n))
            seq = (seq[:p] + adapter + seq[p:])[:n]
        qual = _quality(rng, n, int(rng.choice(5, p=(0.35, 0.25, 0.15, 0.1, 0.15))))
        if wrapped:
            w = int(rng.integers(7, 91))
            if w >= n:
                w = max(1, n // 2)
            seq, qual = _wrap(seq, w), _wrap(qual, w)
        parts.append(b"@" + head + b"\n" + seq + b"\n" + plus + b"\n" + qual + b"\n")
    return b"".join(parts)


def file_records(F, data):
    """(sequence, quality) or None for every record of a file, read with the Python scanner"""
    out = []
    for _h, s, q in F.readfastq_iter(io.BytesIO(data), 1 << 20, F.entryfunc, F.entrypos):
        out.append((s, q) if len(s) == len(q) and b"\n" not in s and b"\n" not in q else None)
    return out


# ---- the host ------------------------------------------------------------------------------------------------------------
def test_the_loop_gives_the_hand_values():
    C = 7
    w = loop_words([(b"acgtnACGTN", b"IIIII!!!!~")], C)
    assert w[:8].tolist() == [1, 0, 10, 3, 5 * 40 + 93, 4, 2, 0]
    cb = w[8:8 + 5 * C].reshape(C, 5)
    assert cb.tolist() == [[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 1, 0], [0, 0, 0, 0, 1], [1, 0, 0, 0, 0],
                           [0, 1, 0, 0, 0]]
    cq = w[8 + 5 * C:8 + 101 * C].reshape(C, 96)
    assert [int(np.flatnonzero(r)[0]) for r in cq] == [40] * 5 + [0, 0] and cq.sum() == 7
    assert w[8 + 101 * C:8 + 102 * C + 1].tolist() == [0] * 7 + [1]
    assert np.flatnonzero(w[8 + 102 * C + 1:8 + 102 * C + 97]).tolist() == [29]          # 293 // 10
    assert np.flatnonzero(w[8 + 102 * C + 97:]).tolist() == [40]
    check_invariants(w, C)
    # an empty read, a skipped row, clamping on both sides
    w = loop_words([(b"", b""), None, (b"GC", bytes([0, 255]))], 3, 64)
    assert w[:8].tolist() == [2, 1, 2, 0, 95, 2, 0, 0] and w[8 + 101 * 3] == 1 and w[8 + 102 * 3 + 97 + 100] == 1
    check_invariants(w, 3)


def test_the_numpy_form_is_the_loop():
    rng = np.random.default_rng(7)
    buf, rows, _tail, n_bad = hand_table()
    recs = records_of(buf, rows)
    assert sum(r is None for r in recs) == n_bad == 11
    reads = [one_read(rng, int(rng.integers(0, 400))) for _ in range(60)]
    every = bytes(b for b in range(256) if b != 10)
    recs += reads + reads[:7] + [(every, b"I" * 255), (b"A" * 255, every)]
    for C, qbase in ((1, 33), (7, 33), (150, 64), (200, 0), (512, 255)):
        want = loop_words(recs, C, qbase)
        assert (np_words(recs, C, qbase) == want).all(), (C, qbase)
        check_invariants(want, C)


def test_host_rule(pkg):
    """FastqStats.add_rows, index.stats_rows, from_words and += against the loop"""
    from fastqandfurious_amd import fastqandfurious as F, index as X, hip
    buf, rows, _tail, n_bad = hand_table()
    rng = np.random.default_rng(3)
    buf2, rows2 = table_of([one_read(rng, n) for n in lengths_for(150)])
    for C, qbase in ((1, 33), (7, 33), (150, 64), (200, 0), (512, 255)):
        assert hip.stats_words(C) == n_words(C)
        want = loop_words(records_of(buf, rows), C, qbase)
        s = X.stats_rows(buf, rows, qbase, C)
        assert (s.words == want).all() and s.head[1] == n_bad
        assert (X.stats_rows(buf, rows + 1000, qbase, C, shift=1000).words == want).all()
        assert (F.FastqStats(C, qbase).add_rows(bytearray(buf), rows.tolist()).words == want).all()
        # the named views are the words
        assert (np.concatenate([s.head, s.cycle_base.ravel(), s.cycle_qual.ravel(), s.len_hist, s.readq_hist, s.gc_hist]) == want).all()
        assert s.cycle_base.shape == (C, 5) and s.cycle_qual.shape == (C, 96) and s.len_hist.shape == (C + 1,)
        assert s.readq_hist.shape == (96,) and s.gc_hist.shape == (101,)
        # from_words round trip
        r = F.FastqStats.from_words(want, C, qbase)
        assert r == s and (r.words == want).all() and r.words is not want
        assert (F.FastqStats.from_words(want.tolist(), C, qbase).words == want).all()
        # += is counting the concatenation
        want2 = loop_words(records_of(buf2, rows2), C, qbase)
        both = loop_words(records_of(buf, rows) + records_of(buf2, rows2), C, qbase)
        t = X.stats_rows(buf2, rows2, qbase, C)
        assert (t.words == want2).all()
        s += t
        assert (s.words == both).all() and (s.head == both[:8]).all() and (t.words == want2).all()
        # derived values
        assert s.reads == int(both[0]) and s.bases == int(both[2])
        assert s.gc_fraction == int(both[5]) / int(both[2])
        cq = both[8 + 5 * C:8 + 101 * C].reshape(C, 96).astype(np.int64)
        assert s.q20_rate == cq[:, 20:].sum() / cq.sum() and s.q30_rate == cq[:, 30:].sum() / cq.sum()
        mq = s.mean_quality_per_cycle
        assert mq.shape == (C,) and mq[0] == (cq[0] * np.arange(96)).sum() / cq[0].sum()
    e = F.FastqStats(5)
    assert e.reads == 0 and np.isnan(e.gc_fraction) and np.isnan(e.q20_rate) and np.isnan(e.mean_quality_per_cycle).all()


def test_add_record(pkg):
    from fastqandfurious_amd import fastqandfurious as F
    s = F.FastqStats(7)
    for seq, q in HAND:
        s.add_record(seq, q)
    assert (s.words == loop_words(HAND, 7)).all()
    with pytest.raises(ValueError):
        s.add_record(b"ACGT", b"III")


def test_python_scanner_branches(pkg):
    """fastq_stats and filter_fastq(report=) with the Python scanner against the loop over the file and over the output"""
    from fastqandfurious_amd import fastqandfurious as F
    from test_trim import loop_span
    data = mixed_corpus(400, 11)
    recs = file_records(F, data)
    assert 20 < sum(r is None for r in recs) < 120
    for fbufsize in (3000, 1 << 20):
        s = F.fastq_stats(io.BytesIO(data), fbufsize, 33, 100, entrypos=F.entrypos)
        assert (s.words == np_words(recs, 100)).all()
    assert (F.fastq_stats(io.BytesIO(data), 5000, 64, 512, entrypos=F.entrypos).words == np_words(recs, 512, 64)).all()
    # the report
    plain = io.BytesIO()
    res0 = F.filter_fastq(io.BytesIO(data), plain, 4000, quality_cutoff=(20, 20), min_len=30, entrypos=F.entrypos)
    rep, out = F.FilterReport(200), io.BytesIO()
    res = F.filter_fastq(io.BytesIO(data), out, 4000, quality_cutoff=(20, 20), min_len=30, entrypos=F.entrypos, report=rep)
    assert res == res0 and out.getvalue() == plain.getvalue() and tuple(res._fields) == ("records_in", "records_out", "bases_removed", "bytes_out")
    assert (rep.before.words == np_words(recs, 200)).all()
    after = file_records(F, out.getvalue())
    assert (rep.after.words == np_words(after, 200)).all()
    assert rep.after.reads + int(rep.after.head[1]) == res.records_out
    dropped = 0
    for r in recs:
        if r is not None:
            a, b = loop_span(r[1], 20, 20)
            if b - a < 30:
                dropped += b - a
    assert rep.before.bases - rep.after.bases == res.bases_removed + dropped
    # qual_base follows
    rep = F.FilterReport(50)
    F.filter_fastq(io.BytesIO(data), io.BytesIO(), 4000, qual_base=64, entrypos=F.entrypos, report=rep)
    assert rep.before.qual_base == 64 and (rep.before.words == np_words(recs, 50, 64)).all() and rep.after == rep.before
    with pytest.raises(ValueError):
        F.fastq_stats(io.BytesIO(b"@a\nACGT\n+\nII"), 100, entrypos=F.entrypos)


def test_argument_errors(pkg):
    from fastqandfurious_amd import fastqandfurious as F, index as X
    for bad in (dict(max_cycles=0), dict(max_cycles=4097), dict(qual_base=-1), dict(qual_base=256)):
        with pytest.raises(ValueError):
            F.FastqStats(**bad)
        with pytest.raises(ValueError):
            X.stats_rows(b"ACGT", np.zeros((0, 6), dtype=np.int64), **bad)
        with pytest.raises(ValueError):
            F.fastq_stats(io.BytesIO(b""), entrypos=F.entrypos, **bad)
    with pytest.raises(ValueError):
        F.FilterReport(0)
    with pytest.raises(ValueError):
        F.FastqStats.from_words(np.zeros(10, dtype=np.uint64), 7)
    a, b = F.FastqStats(7), F.FastqStats(8)
    with pytest.raises(ValueError):
        a += b
    with pytest.raises(ValueError):
        a += F.FastqStats(7, 64)


# ---- the device ------------------------------------------------------------------------------------------------------------
def device_words(ctx, data, rows, C, qbase=33, sentinel=False, add=0, accumulate=False, into=None, wait=True, fill=-1):
    """ffq_table_stats over `data` (bytes / CUDA tensor) and rows (host int64[n][6]) -> (words, head, the device block);
    into: the block to count into (None: a new one filled with `fill`)"""
    import torch
    dbuf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda() if not hasattr(data, "data_ptr") else data
    t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 6)).cuda() if not hasattr(rows, "data_ptr") else rows
    out = torch.full((n_words(C) + 2,), fill, dtype=torch.int64, device="cuda") if into is None else into
    torch.cuda.synchronize()
    head = ctx.table_stats(dbuf.data_ptr(), dbuf.numel(), t.data_ptr(), t.shape[0], out.data_ptr(), qbase, C, accumulate=accumulate,
                           sentinel=sentinel, add=add, wait=wait)
    if not wait:
        assert head is None
        ctx.sync()
    got = out.cpu().numpy().view(np.uint64)
    if into is None:
        assert (got.view(np.int64)[n_words(C):] == fill).all(), "words behind the block were written"
    return got[:n_words(C)].copy(), head, out


def check_device(ctx, buf, rows, C, qbase=33, combos=((0, 0),), dbuf=None, want=None):
    """the device against the loop over every word, head and invariants, for (sentinel, add) combinations"""
    import torch
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
    if want is None:
        want = np_words(records_of(buf, rows), C, qbase)
    check_invariants(want, C)
    if dbuf is None:
        dbuf = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).cuda()
    for sentinel, add in combos:
        got, head, _ = device_words(ctx, dbuf, rows + sentinel + add, C, qbase, sentinel=bool(sentinel), add=add)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (C, qbase, sentinel, add, bad[:8], got[bad[:8]], want[bad[:8]])
        assert head == want[:8].tolist()
    return want


ALL_COMBOS = tuple((s, a) for s in (0, 1) for a in (0, -1, (1 << 33) + 5))
CYCLES = (1, 7, 150, TILE, TILE + 1, 200, 2 * TILE, 2 * TILE + 1, 512)      # (200: not a multiple of the tile)


@pytest.mark.gpu
def test_hand_vectors_device(gpu_ctx):
    buf, rows, tail, n_bad = hand_table()
    for C in (7, 150, 512):
        want = check_device(gpu_ctx, buf, rows, C, combos=ALL_COMBOS, want=loop_words(records_of(buf, rows), C))
        assert want[1] == n_bad and want[0] == tail
    # every ineligible row alone: it counts in head[1] only
    for i in range(tail, len(rows)):
        want = check_device(gpu_ctx, buf, rows[i:i + 1], 150)
        assert want[1] == 1 and want.sum() == 1
    # with a sentinel, coordinate 0 is the virtual newline: a row that touches it is skipped, one of length 0 there counts
    r = rows[2] + 1                                          # (a hand row in the coordinates of b"\n" + buf)
    n = int(r[3] - r[2])
    sub = np.array([[0, 1, 0, n, r[4], r[5]], r.tolist(), [0, 1, 0, 0, 0, 0], [r[0], r[1], r[2], r[3], 0, n]], dtype=np.int64)
    want = loop_words(records_of(b"\n" + buf, sub), 150)
    got, head, _ = device_words(gpu_ctx, buf, sub, 150, sentinel=True, add=0)
    assert (got == want).all() and want[:2].tolist() == [2, 2] and head == want[:8].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("C", CYCLES)
def test_read_lengths(gpu_ctx, C):
    """every length on either side of a step, of the tile / long-row threshold and of max_cycles, at every residue of 16"""
    import torch
    rng = np.random.default_rng(100 + C)
    reads, mods = [], []
    for i, n in enumerate(lengths_for(C) + lengths_for(150)):
        for r in (i % 16, (i * 7 + 3) % 16):
            reads.append(one_read(rng, n))
            mods.append(r)
    buf, rows = table_of(reads, mods)
    want = check_device(gpu_ctx, buf, rows, C, combos=ALL_COMBOS if C in (150, 200) else ((0, 0),))
    assert want[1] == 0 and want[3] > 0 and want[8 + 101 * C + C] >= 4
    # one row alone for every length
    dbuf = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).cuda()
    for i in range(0, len(reads), 2):
        check_device(gpu_ctx, buf, rows[i:i + 1], C, dbuf=dbuf)


@pytest.mark.gpu
def test_the_largest_max_cycles(gpu_ctx):
    rng = np.random.default_rng(4096)
    buf, rows = table_of([one_read(rng, 5000), one_read(rng, 3), one_read(rng, 4097)])
    want = check_device(gpu_ctx, buf, rows[:1], 4096)
    assert want[3] == 5000 - 4096
    check_device(gpu_ctx, buf, rows, 4096)


@pytest.mark.gpu
@pytest.mark.parametrize("qbase", (33, 64, 0, 255))
def test_every_byte_value(gpu_ctx, qbase):
    """a sequence and a quality that run through every byte but the newline: clamping on both sides, case folding, class 4"""
    every = bytes(b for b in range(256) if b != 10)
    reads = [(every, b"I" * 255), (b"A" * 255, every), (every[:TILE], every[-TILE:]), (every[100:150], every[:50])]
    buf, rows = table_of(reads)
    for C in (150, 512):
        want = check_device(gpu_ctx, buf, rows, C, qbase, want=loop_words(records_of(buf, rows), C, qbase))
        assert want[6] == 247 + 0 + (TILE - 8) + 48       # (the eight letters are all below 152; 'g' and 't' lie in 101..150)


@pytest.mark.gpu
def test_contention(gpu_ctx):
    """every lane on the same counters: 4096 copies of one 150-base row of constant quality; then 70 000 rows of 5 bases --
    more than 256 workgroups of 64 rows take in one step -- in order and reversed"""
    buf, rows = table_of([(b"ACGGT" * 30, b"F" * 150), (b"G" * 400, b"F" * 400)])
    want = check_device(gpu_ctx, buf, np.repeat(rows[:1], 4096, axis=0), 150)
    assert want[0] == 4096 and want[8 + 5 * 150 + 37] == 4096
    # (the same on the long rows' kernels)
    want = check_device(gpu_ctx, buf, np.repeat(rows[1:], 3000, axis=0), 512)
    assert want[0] == 3000 and want[8 + 399 * 5 + 2] == 3000
    rng = np.random.default_rng(5)
    pool = [one_read(rng, 5, qlo=33, qhi=45) for _ in range(300)]
    buf, rows = table_of(pool)
    table = rows[rng.integers(0, len(pool), 70000)]
    assert table.shape[0] > 4 * 256 * 64
    want = check_device(gpu_ctx, buf, table, 150)
    check_device(gpu_ctx, buf, table[::-1], 150, want=want)
    assert want[0] == 70000 and want[2] == 350000


# ---- more long rows than one pass of the long launches' grids (tests/grid_expect.py) ----------------------------------------------
LONG_LIST_CYCLES = (512, 200)         # four cycle tiles, the last one of 56 cycles; two, the last one of 48


@functools.lru_cache(maxsize=None)
def long_list_table():
    """(bytes, rows of the table, which of them go onto the long list, the long pool rows): short reads up to TILE bases and the
    rows the rule does not apply to; eight rows above TILE -- one, two and eight bases above it, 700, 1500 and 2500 bases, and
    two with a newline in a line, which the check strikes off the list -- drawn 9195 times among as many of the others"""
    rng = np.random.default_rng(48)
    buf, rows = bytearray(b"#"), []
    for n in [0, 1, 5, TILE - 1, TILE, TILE] + [int(x) for x in rng.integers(0, TILE + 1, 30)]:
        record(buf, rows, *one_read(rng, n))
    ineligible_rows(buf, rows)
    for n in (TILE + 1, TILE + 2, TILE + 8, 700, 1500, 2500):
        record(buf, rows, *one_read(rng, n))
    rows = np.array(rows, dtype=np.int64)
    n = rows[:, 3] - rows[:, 2]
    ok = (rows[:, 2:] >= 0).all(axis=1) & (rows[:, 3] <= len(buf)) & (rows[:, 5] <= len(buf)) & (n == rows[:, 5] - rows[:, 4])
    long = np.flatnonzero(ok & (n > TILE))
    idx = GE.long_idx(long, [i for i in range(len(rows)) if i not in long], seed=49)
    return bytes(buf), rows[idx], np.isin(idx, long), rows[long]


def test_the_long_list_table_is_what_the_loop_says():
    buf, table, is_long, long_rows = long_list_table()
    n = long_rows[:, 3] - long_rows[:, 2]
    recs = records_of(buf, long_rows)
    assert len(n) == 8 and sorted(n)[:2] == [TILE + 1, TILE + 2] and max(n) == 2500 and sum(r is None for r in recs) == 2
    assert int(is_long.sum()) == GE.N_LONG > 2 * 512 * 8 and len(table) == 2 * GE.N_LONG >= 4096
    order = np.flatnonzero(is_long)
    assert len(GE.passes(len(order), GE.P_LONG)) == 3
    for s in GE.passes(len(order), GE.P_LONG):                 # every long pool row, the two struck off among them, in every pass
        assert len({tuple(r) for r in table[order[s]].tolist()}) == 8
    at = GE.sample_rows(len(table), GE.P_LONG)
    recs = records_of(buf, table[at])
    for C in LONG_LIST_CYCLES:
        assert -(-C // TILE) >= 2 and C % TILE != 0
        want = np_words(recs, C)
        assert len(at) >= 2000 and (want == loop_words(recs, C)).all()
        check_invariants(want, C)
        assert want[1] > 100 and want[3] > 0 and want[8 + 101 * C + C] > 100


@pytest.mark.gpu
@pytest.mark.parametrize("C", LONG_LIST_CYCLES)
def test_more_long_rows_than_one_pass_of_the_grid(gpu_ctx, C):
    """9195 rows above TILE among as many others: k_stats_long_check's 512 workgroups of eight waves take three steps over the
    list and strike entries off it in each, k_stats_long_count's 128 take nine per cycle tile; every word of the block"""
    buf, table, is_long, _long_rows = long_list_table()
    assert int(is_long.sum()) > 2 * 512 * 8 and int(is_long.sum()) > 8 * 128 * 8 and len(table) >= 4096
    check_device(gpu_ctx, buf, table, C, combos=((0, 0), (1, (1 << 33) + 5)))


@pytest.mark.gpu
def test_alignment_and_the_end_of_the_buffer(gpu_ctx):
    """one record at every residue of 16; the last record's quality ends exactly at n_bytes"""
    rng = np.random.default_rng(16)
    for n in (150, 151, 5, 3, 300):
        rd = one_read(rng, n)
        buf, rows = table_of([rd] * 16 + [rd], list(range(16)) + [7], last=True)
        assert rows[-1][5] == len(buf)
        want = check_device(gpu_ctx, buf, rows, 150, combos=((0, 0), (1, 3)))
        assert want[0] == 17
        check_device(gpu_ctx, buf, rows[-1:], 150)
        # ... and a sequence that ends there
        swapped = rows[-1:, [0, 1, 4, 5, 2, 3]]
        check_device(gpu_ctx, buf, swapped, 150)


@pytest.mark.gpu
def test_ineligible_rows_among_others(gpu_ctx):
    rng = np.random.default_rng(8)
    buf, rows = bytearray(b"#"), []
    n_bad = 0
    for k in range(6):
        for _ in range(37):
            s, q = one_read(rng, int(rng.integers(0, 330)))
            record(buf, rows, s, q)
        n_bad += ineligible_rows(buf, rows)
    rows = np.array(rows, dtype=np.int64)
    # (a row that pointed past the buffer when it was appended may lie inside it now: the loop says what it is)
    want = check_device(gpu_ctx, bytes(buf), rows, 200, combos=ALL_COMBOS)
    assert want[1] >= n_bad - 12 and want[0] >= 6 * 37
    # runs of rows with nothing to do between ordinary rows: empty ones and ineligible ones
    p = int(rows[0][2])
    for idle in ([0, 1, p, p, p + 2, p + 2], [0, 1, p, p + 30, -1, -1]):
        table = np.concatenate([rows[:12], [idle] * 64, rows[12:24], [idle] * 65, rows[24:40], [idle] * 600, rows[40:], [idle] * 64])
        check_device(gpu_ctx, bytes(buf), table, 150)


@pytest.mark.gpu
def test_accumulate(gpu_ctx):
    import torch
    rng = np.random.default_rng(21)
    buf, rows = table_of([one_read(rng, int(rng.integers(0, 400))) for _ in range(500)])
    C = 150
    want = np_words(records_of(buf, rows), C)
    # over a block filled with 0xFF: a fresh count
    got, head, blk = device_words(gpu_ctx, buf, rows, C, fill=-1)
    assert (got == want).all() and head == want[:8].tolist()
    # twice more, accumulating: three times the table
    for k in (2, 3):
        got, head, _ = device_words(gpu_ctx, buf, rows, C, accumulate=True, into=blk)
        assert (got == want * np.uint64(k)).all() and head == (want[:8] * np.uint64(k)).tolist()
    # no rows: nothing is added; without accumulate the block is zeroed
    got, head, _ = device_words(gpu_ctx, buf, np.zeros((0, 6), dtype=np.int64), C, accumulate=True, into=blk)
    assert (got == want * np.uint64(3)).all() and head == (want[:8] * np.uint64(3)).tolist()
    got, head, _ = device_words(gpu_ctx, buf, np.zeros((0, 6), dtype=np.int64), C, into=blk)
    assert not got.any() and head == [0] * 8
    # head = NULL: enqueued only; the copy behind it has the same words
    got, head, _ = device_words(gpu_ctx, buf, rows, C, wait=False)
    assert head is None and (got == want).all()
    got, _, _ = device_words(gpu_ctx, buf, rows, C, accumulate=True, into=torch.zeros(n_words(C), dtype=torch.int64, device="cuda"), wait=False)
    assert (got == want).all()


@pytest.mark.gpu
def test_after_a_real_scan(gpu_ctx):
    """mixed reads as files hold them, scanned on the device: the count over the scanned rows, and index.stats_rows_device"""
    import torch
    from fastqandfurious_amd import index as X, fastqandfurious as F
    data = mixed_corpus(3000, 20242, long_every=150)
    dbuf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    table = torch.empty((4000, 6), dtype=torch.int64, device="cuda")
    rc, res = gpu_ctx.scan_device(dbuf.data_ptr(), len(data), table.data_ptr(), 4000)
    assert rc == 0 and int(res.n_records) == 3000
    table = table[:3000]
    rows = table.cpu().numpy()
    recs = records_of(data, rows)                           # (scan_device's rows index the bytes it was given)
    assert recs == file_records(F, data) and 200 < sum(r is None for r in recs) < 800
    for C, qbase in ((150, 33), (512, 33), (4096, 64)):
        want = np_words(recs, C, qbase)
        check_invariants(want, C)
        got, head, _ = device_words(gpu_ctx, dbuf, table, C, qbase, sentinel=True, add=-1)
        assert (got == want).all() and head == want[:8].tolist()
        s, out = X.stats_rows_device(gpu_ctx, dbuf, table, qbase, C)
        assert (s.words == want).all() and s.max_cycles == C and s.qual_base == qbase
        s2, out2 = X.stats_rows_device(gpu_ctx, dbuf, table, qbase, C, out=out, accumulate=True)
        assert out2 is out and (s2.words == want * np.uint64(2)).all()


@pytest.mark.gpu
def test_errors(gpu_ctx):
    import torch
    from fastqandfurious_amd import hip
    rng = np.random.default_rng(1)
    buf, rows = table_of([one_read(rng, 100) for _ in range(64)])
    dbuf = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).cuda()
    table = torch.from_numpy(rows).cuda()
    blk = torch.zeros(n_words(150) + 2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def call(out=blk.data_ptr(), C=150, qbase=33, t=table):
        return gpu_ctx.table_stats(dbuf.data_ptr(), len(buf), t.data_ptr(), 63, out, qbase, C, sentinel=False)
    for kw in (dict(C=0), dict(C=4097), dict(C=-1), dict(qbase=-1), dict(qbase=256), dict(out=0), dict(out=blk.data_ptr() + 8)):
        with pytest.raises(hip.FFQError) as e:
            call(**kw)
        assert e.value.code == hip.E_ARG, kw
    assert not blk.cpu().numpy().any()
    # a scan pending on the context
    data = mixed_corpus(50, 2)
    d2 = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    t2 = torch.empty((64, 6), dtype=torch.int64, device="cuda")
    gpu_ctx.scan_submit(d2.data_ptr(), len(data), t2.data_ptr(), 64)
    try:
        with pytest.raises(hip.FFQError) as e:
            call()
        assert e.value.code == hip.E_ARG
    finally:
        gpu_ctx.scan_wait()
    assert call()[0] == 63

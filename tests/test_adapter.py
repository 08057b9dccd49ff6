"""3' adapter trimming by editing rows of the offset table: ffq_table_trim_adapter (device), index.trim_adapter_rows (host),
adapter_cut / entryfunc_adaptertrim (per record), filter_fastq(adapter=...).

The expectation of every test is the loop below -- the rule as include/ffq.h states it, written out here -- never the
package's own host implementation.  Bulk cases use a per-row numpy form of the same loop (np_cut), which is checked against
the plain loop on the hand vectors and on random reads.  Coordinates: a row minus `add` indexes the buffer the scanner saw;
with a sentinel that buffer is b'\\n' + bytes.
"""
import functools
import io

import numpy as np
import pytest

import grid_expect as GE

from test_trim import loop_span, loop_rows as quality_loop_rows

AD = b"AGATCGGAAGAGC"
LONG = 2048             # bases above which the library gives a row a wave of its own (csrc/ffq_adapter.h: ADAPTER_LONG)
CHUNK_LONG = 512        # candidates per chunk of that kernel


# ---- the rule ------------------------------------------------------------------------------------------------------
def loop_cut(seq, ad=AD, err=100, mo=3):
    n, m = len(seq), len(ad)
    for p in range(0, n - mo + 1):
        ov = min(m, n - p)
        mm = sum(1 for j in range(ov) if ad[j] != 0x4E and seq[p + j] != ad[j])
        if mm <= (ov * err) // 1000:
            return p
    return n


def np_cut(seq, ad=AD, err=100, mo=3):
    """the same loop, every candidate at once"""
    n, m = len(seq), len(ad)
    if n < mo:
        return n
    ncand = n - mo + 1
    s = np.concatenate((np.frombuffer(seq, dtype=np.uint8), np.zeros(m, dtype=np.uint8)))
    a = np.frombuffer(ad, dtype=np.uint8)
    p = np.arange(ncand)[:, None]
    j = np.arange(m)[None, :]
    mism = (np.lib.stride_tricks.sliding_window_view(s, m)[:ncand] != a) & (a != 0x4E) & (p + j < n)
    ok = mism.sum(axis=1) <= (np.minimum(m, n - p[:, 0]) * err) // 1000
    hit = np.flatnonzero(ok)
    return int(hit[0]) if hit.size else n


def loop_rows(buf, rows, ad=AD, err=100, mo=3, add=0, cut=np_cut):
    """(new rows, [changed, bases removed, skipped]) for rows (+ add) over `buf` (bytes: the buffer as the scanner saw it)"""
    out, stats, cache = [], [0, 0, 0], {}
    for row in rows:
        row = [int(x) for x in row]
        p2, p3, p4, p5 = (x - add for x in row[2:])
        ok = min(p2, p3, p4, p5) >= 0 and p2 <= p3 <= len(buf) and p4 <= p5 <= len(buf) and p3 - p2 == p5 - p4
        if ok and 10 in buf[p2:p3]:
            ok = False
        if not ok:
            stats[2] += 1
            out.append(row)
            continue
        seq = buf[p2:p3]
        c = cache.get(seq)
        if c is None:
            c = cache[seq] = cut(seq, ad, err, mo)
        if c != len(seq):
            stats[0] += 1
            stats[1] += len(seq) - c
        out.append(row[:3] + [row[2] + c, row[4], row[4] + c])
    return np.array(out, dtype=np.int64).reshape(-1, 6), stats


# ---- hand vectors: (sequence, adapter, err_permille, min_overlap, cut) -------------------------------------------------
HAND = [
    (b"ACGTACGTAC" + AD + b"TTTT", AD, 100, 3, 10),
    (AD + b"ACGT", AD, 100, 3, 0),
    (b"CCCCCCCC" + AD, AD, 100, 3, 8),
    (b"ACGTACGTACAGATC", AD, 100, 3, 10),
    (b"CCCCCCCCCCAGA", AD, 100, 3, 10),
    (b"CCCCCCCCCCAG", AD, 100, 3, 12),
    (b"CCCCCAGATCGGTAGAGCCC", AD, 100, 3, 5),
    (b"CCCCCAGTTCGGTAGAGCCC", AD, 100, 3, 20),
    (b"CCCCCAGATCGGTA", AD, 100, 3, 14),
    (b"CCCCCAGATCGGTAG", AD, 100, 3, 5),
    (b"CCAGATCGGTAGAGCCCAGATCGGAAGAGC", AD, 100, 3, 2),
    (b"CCAGATCGGTAGAGCCCAGATCGGAAGAGC", AD, 0, 3, 17),
    (b"CCCCAGATCTTAAGAGC", b"AGATCNNAAGAGC", 0, 3, 4),
    (b"CCCCAGATCNNAAGAGC", AD, 100, 3, 17),
    (b"", AD, 100, 3, 0),
    (b"AG", AD, 100, 3, 2),
    (b"AGA", AD, 100, 3, 0),
    (b"AGATCGG", AD, 100, 3, 0),
    (b"CCCTCC", b"T", 0, 1, 3),
    (b"CCCCagatcggaagagc", AD, 100, 3, 17),
    (b"CCCCAGATCGGAAGAG", AD, 100, 13, 16),
]


def record(buf, rows, seq, qual=None, header=b"@h"):
    """append a four-line record to `buf` (bytearray) and its row to `rows`"""
    qual = b"I" * len(seq) if qual is None else qual
    p0 = len(buf)
    buf += header + b"\n"
    p2 = len(buf)
    buf += seq + b"\n+\n"
    p4 = len(buf)
    buf += qual + b"\n"
    rows.append([p0, p2 - 1, p2, p2 + len(seq), p4, p4 + len(qual)])


def hand_table():
    """One buffer with a four-line record per hand vector, then the ineligible rows.  Returns (bytes, rows, first ineligible)"""
    buf, rows = bytearray(b"##"), []
    for i, (seq, *_rest) in enumerate(HAND):
        record(buf, rows, seq, header=b"@h%d" % i)
    tail = len(rows)
    record(buf, rows, b"CCCC\nCC" + AD + b"CC")                  # a newline in front of a hit
    record(buf, rows, b"CC" + AD + b"CC\nCCCC")                  # ... and behind one
    record(buf, rows, b"CC" + AD + b"CC", qual=b"IIII")           # unequal lengths
    p0 = rows[-1][0]
    rows.append(rows[-1][:4] + [-1, -1])                          # a FASTA row
    rows.append([p0, p0 + 2, p0 + 3, p0 + 7, len(buf) - 3, len(buf) + 1])   # past the buffer
    rows.append([p0, p0 + 2, len(buf) - 3, len(buf) + 1, p0 + 3, p0 + 7])
    rows.append([p0, p0 + 2, -5, -1, p0 + 11, p0 + 15])           # in front of the buffer
    return bytes(buf), rows, tail


def _groups():
    """the hand rows by (adapter, err, min_overlap): a call has one set of parameters"""
    buf, rows, tail = hand_table()
    out = {}
    for i, (_s, ad, err, mo, _c) in enumerate(HAND):
        out.setdefault((ad, err, mo), []).append(i)
    return buf, rows, out, list(range(tail, len(rows)))


def one_read(rng, n, ad=AD, alphabet=b"ACGT", implant=True):
    """a read of length n over `alphabet`; implant: the adapter at a uniform position, cut off by the read's end, with 0-2
    random substitutions from ACGTN"""
    alpha = np.frombuffer(alphabet, dtype=np.uint8)
    s = alpha[rng.integers(0, len(alpha), n)].copy()
    if implant and n > 0:
        a = np.frombuffer(ad, dtype=np.uint8).copy()
        for _ in range(int(rng.integers(0, 3))):
            a[int(rng.integers(0, len(a)))] = np.frombuffer(b"ACGTN", dtype=np.uint8)[int(rng.integers(0, 5))]
        p = int(rng.integers(0, n))
        k = min(len(a), n - p)
        s[p:p + k] = a[:k]
    return s.tobytes()


def random_reads(rng, n_rows, max_len, ad=AD, alphabet=b"ACGT", every=2):
    """reads of length 0..max_len; every `every`-th has the adapter implanted (one_read)"""
    return [one_read(rng, int(rng.integers(0, max_len + 1)), ad, alphabet, i % every == 0) for i in range(n_rows)]


def table_of(reads, start_mod16=None):
    """(bytes, rows) of four-line records; start_mod16: the sequence of record i starts at an address = start_mod16[i] mod 16"""
    buf, rows = bytearray(b"#"), []
    for i, s in enumerate(reads):
        if start_mod16 is not None:
            buf += b"#" * ((start_mod16[i] - (len(buf) + 3)) % 16)
        record(buf, rows, s)
        assert start_mod16 is None or rows[-1][2] % 16 == start_mod16[i]
    return bytes(buf), np.array(rows, dtype=np.int64).reshape(-1, 6)


# ---- the host --------------------------------------------------------------------------------------------------------------
def test_the_loop_gives_the_hand_values():
    for seq, ad, err, mo, want in HAND:
        assert loop_cut(seq, ad, err, mo) == want, (seq, ad, err, mo)
        assert np_cut(seq, ad, err, mo) == want, (seq, ad, err, mo)


def test_the_numpy_form_is_the_loop():
    rng = np.random.default_rng(7)
    for ad, err, mo in ((AD, 100, 3), (AD, 200, 1), (b"T", 0, 1), (b"ACGTNACGTTGCA" * 5, 200, 20), (AD, 0, 13)):
        for s in random_reads(rng, 150, 90, ad):
            assert np_cut(s, ad, err, mo) == loop_cut(s, ad, err, mo), (s, ad, err, mo)


def test_hand_vectors_host(pkg):
    """index.trim_adapter_rows, adapter_cut and entryfunc_adaptertrim against the loop, on the hand rows and the ineligible rows"""
    from fastqandfurious_amd import index as X, fastqandfurious as F
    buf, rows, groups, tail = _groups()
    for (ad, err, mo), idx in groups.items():
        sub = [rows[i] for i in idx] + [rows[i] for i in tail]
        want, stats = loop_rows(buf, sub, ad, err, mo, cut=loop_cut)
        for j, i in enumerate(idx):
            c = HAND[i][4]
            assert list(want[j]) == rows[i][:3] + [rows[i][2] + c, rows[i][4], rows[i][4] + c], HAND[i]
            assert F.adapter_cut(HAND[i][0], ad, err, mo) == c
        assert (want[len(idx):] == np.array([rows[i] for i in tail])).all() and stats[2] == len(tail)
        got = X.trim_adapter_rows(buf, np.array(sub, dtype=np.int64), ad, err, mo)
        assert got.shape == want.shape and (got == want).all(), (ad, err, mo)
        got = X.trim_adapter_rows(buf, np.array(sub, dtype=np.int64)[:len(idx)] + 1000, ad, err, mo, shift=1000)
        assert (got == want[:len(idx)] + 1000).all()
        for col in ("entry", "sequence", "quality", "header"):
            for lo, hi in ((None, None), (2, None), (None, 3)):
                ef = F.entryfunc_adaptertrim(ad, err, mo, min_len=lo, max_len=hi, column=col)
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


def test_random_reads_host(pkg):
    from fastqandfurious_amd import index as X, fastqandfurious as F
    rng = np.random.default_rng(11)
    reads = random_reads(rng, 300, 120)
    buf, rows = table_of(reads)
    for ad, err, mo in ((AD, 100, 3), (AD, 200, 1), (AD, 0, 13)):
        want, _ = loop_rows(buf, rows, ad, err, mo)
        assert (X.trim_adapter_rows(buf, rows, ad, err, mo) == want).all()
        assert [F.adapter_cut(s, ad, err, mo) for s in reads] == [int(x) for x in want[:, 3] - want[:, 2]]


def test_argument_errors(pkg):
    from fastqandfurious_amd import index as X, fastqandfurious as F
    for bad in (dict(adapter=b""), dict(adapter=b"A" * 65), dict(adapter=AD, min_overlap=0), dict(adapter=AD, min_overlap=14),
                dict(adapter=AD, err_permille=-1), dict(adapter=AD, err_permille=1001)):
        with pytest.raises(ValueError):
            F.adapter_cut(b"ACGT", **bad)
        with pytest.raises(ValueError):
            F.entryfunc_adaptertrim(**bad)
        with pytest.raises(ValueError):
            X.trim_adapter_rows(b"ACGT", np.zeros((0, 6), dtype=np.int64), **bad)
        with pytest.raises(ValueError):
            F.filter_fastq(io.BytesIO(b""), io.BytesIO(), entrypos=F.entrypos, **bad)
    for bad in (dict(column="nope"), dict(quality_cutoff=128), dict(quality_cutoff=(1, -1)), dict(quality_cutoff=3, qual_base=256)):
        with pytest.raises(ValueError):
            F.entryfunc_adaptertrim(AD, **bad)


# ---- a file of mixed records, and what the iterator and filter_fastq owe for it ---------------------------------------------
def mixed_file(n_records, seed=5):
    """four-line records with and without adapters and qualities that the quality rule trims, and -- every seventh -- a record
    wrapped over several lines (its first line holds an adapter: it is left alone all the same)"""
    rng = np.random.default_rng(seed)
    reads = random_reads(rng, n_records, 160)
    out = []
    for i, s in enumerate(reads):
        n = len(s)
        q = rng.integers(25, 41, n)
        k = int(rng.integers(0, 12))
        if k and n:
            q[n - min(k, n):] = rng.integers(2, 12, min(k, n))
        q = (q + 33).astype(np.uint8).tobytes()
        if n == 0:
            s, q = b"A", b"I"          # (the scanners do not read an empty record back record for record)
        if i % 7 == 3 and len(s) > 40:
            s = s[:20] + b"\n" + s[20:]
            q = q[:20] + b"\n" + q[20:]
        out.append(b"@r%d x\n" % i + s + b"\n+\n" + q + b"\n")
    return b"".join(out)


def expected_records(F, data, ad=AD, err=100, mo=3, quality=None):
    """[(header, sequence, quality, bases the quality rule removed, bases the adapter removed, adapter rule skipped)] by the loops"""
    out = []
    for h, s, q in F.readfastq_iter(io.BytesIO(data), 1 << 20, F.entryfunc, F.entrypos):
        rq = ra = 0
        if quality is not None and len(s) == len(q) and b"\n" not in q:
            a, b = loop_span(q, *quality)
            rq = len(s) - (b - a)
            s, q = s[a:b], q[a:b]
        skipped = not (len(s) == len(q) and b"\n" not in s)
        if ad is not None and not skipped:
            c = np_cut(s, ad, err, mo)
            ra = len(s) - c
            s, q = s[:c], q[:c]
        out.append((h, s, q, rq, ra, skipped))
    return out


def expected_items(recs, min_len=None, max_len=None, column="entry"):
    out = []
    for h, s, q, *_ in recs:
        if (min_len is not None and len(s) < min_len) or (max_len is not None and len(s) > max_len):
            out.append(None)
        else:
            out.append({"entry": (h, s, q), "header": h, "sequence": s, "quality": q}[column])
    return out


def expected_output(recs, min_len=None, max_len=None):
    """(text, (records_in, records_out, bases_removed, bytes_out))"""
    kept = [e for e in expected_items(recs, min_len, max_len) if e is not None]
    text = b"".join(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n" for h, s, q in kept)
    return text, (len(recs), len(kept), sum(r[3] + r[4] for r in recs), len(text))


@pytest.fixture(scope="module")
def mixed(pkg):
    from fastqandfurious_amd import fastqandfurious as F
    data = mixed_file(1500)
    return data, expected_records(F, data, quality=(0, 20)), expected_records(F, data)


def test_mixed_file_has_every_kind(mixed):
    data, recs, plain = mixed
    assert len(recs) == 1500
    assert sum(1 for r in recs if r[5]) > 100                               # wrapped
    assert sum(1 for r in recs if r[4] > 0) > 300 and sum(1 for r in recs if r[3] > 0) > 300
    assert sum(1 for r in recs if r[3] > 0 and r[4] > 0) > 100              # both rules on one read
    assert sum(1 for r in recs if not r[5] and r[4] == 0) > 300
    assert [r[:3] for r in recs] != [r[:3] for r in plain]


@pytest.mark.parametrize("fbufsize", (3000, 1 << 20))
def test_readfastq_iter_python_scanner(pkg, mixed, fbufsize):
    from fastqandfurious_amd import fastqandfurious as F
    data, recs, plain = mixed
    got = list(F.readfastq_iter(io.BytesIO(data), fbufsize, F.entryfunc_adaptertrim(AD, quality_cutoff=20, min_len=30), F.entrypos))
    want = expected_items(recs, min_len=30)
    assert got == want and any(e is None for e in want) and any(e is not None for e in want)
    for col in ("sequence", "quality", "header"):
        got = list(F.readfastq_iter(io.BytesIO(data), fbufsize, F.entryfunc_adaptertrim(AD, 100, 3, max_len=100, column=col), F.entrypos))
        assert got == expected_items(plain, max_len=100, column=col)


@pytest.mark.parametrize("fbufsize", (3000, 1 << 20))
def test_filter_fastq_python_scanner(pkg, mixed, fbufsize):
    from fastqandfurious_amd import fastqandfurious as F
    data, recs, plain = mixed
    for kw, rr, bounds in ((dict(adapter=AD, quality_cutoff=20, min_len=30), recs, dict(min_len=30)),
                           (dict(adapter=AD), plain, {}),
                           (dict(adapter=AD, err_permille=100, min_overlap=3, max_len=120), plain, dict(max_len=120))):
        out = io.BytesIO()
        res = F.filter_fastq(io.BytesIO(data), out, fbufsize, entrypos=F.entrypos, **kw)
        want, counters = expected_output(rr, **bounds)
        assert out.getvalue() == want and tuple(res) == counters, kw
    # adapter=None: what it was
    out = io.BytesIO()
    res = F.filter_fastq(io.BytesIO(data), out, fbufsize, entrypos=F.entrypos)
    assert tuple(res)[:3] == (1500, 1500, 0)


# ---- the device ------------------------------------------------------------------------------------------------------------
def device_cut(ctx, data, rows, ad=AD, err=100, mo=3, sentinel=False, add=0, in_place=False):
    """rows (host int64[n][6]) trimmed by ffq_table_trim_adapter over `data` (bytes / CUDA tensor) -> (rows, stats)"""
    import torch
    dbuf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda() if not hasattr(data, "data_ptr") else data
    t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 6)).cuda()
    out = t if in_place else torch.full_like(t, -77)
    stats = ctx.table_trim_adapter(dbuf.data_ptr(), dbuf.numel(), t.data_ptr(), t.shape[0], ad, err, mo, d_out=out.data_ptr(),
                                   sentinel=sentinel, add=add)
    return out.cpu().numpy(), list(stats)


def check_device(ctx, buf, rows, ad=AD, err=100, mo=3, combos=((0, 0, False),), dbuf=None):
    """the device against the loop, every row and the stats, for (sentinel, add, in place) combinations"""
    import torch
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
    want, stats = loop_rows(buf, rows, ad, err, mo)
    if dbuf is None:
        dbuf = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).cuda()
    for sentinel, add, in_place in combos:
        got, gstats = device_cut(ctx, dbuf, rows + sentinel + add, ad, err, mo, sentinel=bool(sentinel), add=add, in_place=in_place)
        bad = np.nonzero((got != want + sentinel + add).any(axis=1))[0]
        assert bad.size == 0, ((ad, err, mo), sentinel, add, bad[:5], (got[bad[:5]] - sentinel - add).tolist(), want[bad[:5]].tolist())
        assert gstats == stats, ((ad, err, mo), sentinel, add)
    return want, stats


ALL_COMBOS = tuple((s, a, ip) for s in (0, 1) for a, ip in ((0, False), (-1, True), ((1 << 33) + 5, False)))


@pytest.mark.gpu
def test_hand_vectors_device(gpu_ctx):
    buf, rows, groups, tail = _groups()
    for (ad, err, mo), idx in groups.items():
        sub = np.array([rows[i] for i in idx] + [rows[i] for i in tail], dtype=np.int64)
        want, stats = check_device(gpu_ctx, buf, sub, ad, err, mo, combos=ALL_COMBOS)
        assert stats[2] == len(tail)
        for j, i in enumerate(idx):
            assert want[j][3] - want[j][2] == HAND[i][4]
    # with a sentinel, coordinate 0 is the virtual newline: a sequence that starts there is not trimmed; one of length 0 is
    # eligible and unchanged; a quality that starts there is never read
    r = np.array(rows[0]) + 1                               # (the first hand row in the coordinates of b"\n" + buf)
    n = int(r[3] - r[2])
    sub = np.array([[0, 1, 0, n, r[4], r[5]], r.tolist(), [0, 1, 0, 0, 0, 0], [r[0], r[1], r[2], r[3], 0, n]], dtype=np.int64)
    want, stats = loop_rows(b"\n" + buf, sub)
    got, gstats = device_cut(gpu_ctx, buf, sub, sentinel=True, add=0)
    assert (got == want).all() and gstats == stats and stats[2] == 1 and stats[0] == 2
    # no rows: nothing happens
    assert device_cut(gpu_ctx, buf, np.zeros((0, 6), dtype=np.int64))[1] == [0, 0, 0]


SWEEP_LENGTHS = tuple(range(0, 71)) + (127, 128, 129, 130, 255, 256, 257, 258, LONG - 1, LONG, LONG + 1)


def sweep_adapter(m):
    rng = np.random.default_rng(100 + m)
    ad = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, m)].copy()
    if m >= 13:
        ad[m // 2] = 0x4E
    return (AD if m == 13 else ad.tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("m", (1, 13, 33, 64))
def test_length_and_alignment_sweep(gpu_ctx, m):
    """every length on either side of a chunk and of the short / long split, the sequence at every residue of 16, for every
    (min_overlap, err_permille); sentinel, add and in place in every combination for one of them"""
    import torch
    ad = sweep_adapter(m)
    rng = np.random.default_rng(200 + m)
    reads, mods = [], []
    for r in range(16):
        for n in SWEEP_LENGTHS:
            reads.append(one_read(rng, n, ad, implant=bool(rng.integers(0, 3))))
            mods.append(r)
    buf, rows = table_of(reads, mods)
    dbuf = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).cuda()
    seen = set()
    for mo in sorted({1, min(3, m), m}):
        for err in (0, 100, 200):
            first = not seen
            want, stats = check_device(gpu_ctx, buf, rows, ad, err, mo, combos=ALL_COMBOS if first else ((0, 0, False),), dbuf=dbuf)
            seen.add((mo, err))
            if (mo, err) == (min(3, m), 200) and m >= 13:
                cut = want[:, 3] - rows[:, 2]
                n = rows[:, 3] - rows[:, 2]
                # (the table has partial hits, full ones and reads without a hit, by the loop)
                assert ((cut < n) & (n - cut < m)).sum() >= 20 and ((cut < n) & (n - cut >= m)).sum() >= 50 and (cut == n).sum() >= 100


@pytest.mark.gpu
def test_long_reads_among_short_ones(gpu_ctx):
    """one read of 5000 and one of 70 000 bases in a wave of short ones: the only hit lies beyond the short / long threshold
    and straddles a chunk boundary of the long rows' kernel; and the same reads with no hit"""
    rng = np.random.default_rng(42)
    alpha = np.frombuffer(b"CGT", dtype=np.uint8)           # (no 'A': no place of such a read matches AGATCGGAAGAGC)
    short = random_reads(rng, 40, 100)
    for hit in (True, False):
        longs = []
        for n, p in ((5000, CHUNK_LONG * 5 - 5), (70000, CHUNK_LONG * 100 - 5)):
            s = alpha[rng.integers(0, 3, n)].copy()
            if hit:
                s[p:p + len(AD)] = np.frombuffer(AD, dtype=np.uint8)
            longs.append((s.tobytes(), p))
        reads = short[:13] + [longs[0][0]] + short[13:30] + [longs[1][0]] + short[30:]
        buf, rows = table_of(reads)
        want, stats = check_device(gpu_ctx, buf, rows, combos=((0, 0, False), (1, 7, True)))
        for i, (s, p) in zip((13, 31), longs):
            assert p > LONG and p // CHUNK_LONG != (p + len(AD) - 1) // CHUNK_LONG
            assert want[i][3] - want[i][2] == (p if hit else len(s))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("empty", "ineligible"))
def test_runs_of_rows_with_nothing_to_do(gpu_ctx, kind):
    """runs of 64, 65 and 300 consecutive rows that are empty (or ineligible) between ordinary rows"""
    rng = np.random.default_rng(9)
    buf, rows = table_of(random_reads(rng, 50, 150))
    p = int(rows[0][2])
    idle = [0, 1, p, p, p + 2, p + 2] if kind == "empty" else [0, 1, p, p + 30, -1, -1]
    table, at = [], 0
    for run in (64, 65, 300):
        table += rows[at:at + 12].tolist() + [idle] * run
        at += 12
    table += rows[at:].tolist() + [idle] * 64
    table = np.array(table, dtype=np.int64)
    want, stats = check_device(gpu_ctx, buf, table, combos=((0, 0, False), (0, 0, True)))
    assert stats[2] == (0 if kind == "empty" else 64 + 65 + 300 + 64) and stats[0] > 5


@pytest.mark.gpu
def test_more_rows_than_one_pass_of_the_grid(gpu_ctx):
    """2048 workgroups of 32 rows: 65 536 rows a pass; 140 000 very short reads (drawn from 3000 different ones)"""
    rng = np.random.default_rng(3)
    pool = random_reads(rng, 3000, 12, every=3)
    buf, rows = table_of([pool[i] for i in rng.integers(0, len(pool), 140000)])
    assert rows.shape[0] > 2 * 2048 * 32 and len(buf) < 6 << 20
    want, stats = check_device(gpu_ctx, buf, rows)
    assert stats[0] > 10000 and stats[2] == 0


# ---- more long rows than one pass of the long launch's grid (tests/grid_expect.py) ------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_list_table():
    """(bytes, rows of the table, which of them are long, the long pool rows): 40 short reads, one of LONG bases and six above it
    -- just above and up to 5000, the only hit in front of, across and far behind the threshold, or none --, drawn 9195 times
    among as many short ones"""
    rng = np.random.default_rng(46)
    alpha = np.frombuffer(b"CGT", dtype=np.uint8)           # (no 'A': no place of such a read matches AGATCGGAAGAGC)
    reads = random_reads(rng, 40, 100)
    for n, p in ((LONG, LONG - 5), (LONG + 1, None), (LONG + 2, LONG - 3), (LONG + 3, 100), (3000, CHUNK_LONG * 5 - 5), (4000, None), (5000, 4995)):
        s = alpha[rng.integers(0, 3, n)].copy()
        if p is not None:
            k = min(len(AD), n - p)
            s[p:p + k] = np.frombuffer(AD, dtype=np.uint8)[:k]
        reads.append(s.tobytes())
    buf, rows = table_of(reads)
    long = [i for i, s in enumerate(reads) if len(s) > LONG]
    idx = GE.long_idx(long, [i for i in range(len(reads)) if i not in long], seed=47)
    return buf, rows[idx], np.isin(idx, long), rows[long]


def test_the_long_list_table_is_what_the_loop_says():
    buf, table, is_long, long_rows = long_list_table()
    n = long_rows[:, 3] - long_rows[:, 2]
    assert len(n) == 6 and sorted(n)[:3] == [LONG + 1, LONG + 2, LONG + 3] and max(n) == 5000
    assert int(is_long.sum()) == GE.N_LONG > 2 * 1024 * 4 and len(table) == 2 * GE.N_LONG >= 4096
    want, stats = loop_rows(buf, table)
    cut = (want[:, 3] - want[:, 2])[is_long]
    full = (table[:, 3] - table[:, 2])[is_long]
    assert (cut == full).sum() > 1000 and (cut < LONG).sum() > 1000 and ((cut > LONG) & (cut < full)).sum() > 1000
    at = GE.sample_rows(len(table), GE.P_LONG)
    assert len(at) >= 2000 and (loop_rows(buf, table[at], cut=loop_cut)[0] == want[at]).all()
    order = np.flatnonzero(is_long)
    assert len(GE.passes(len(order), GE.P_LONG)) == 3
    for s in GE.passes(len(order), GE.P_LONG):
        assert len({tuple(r) for r in table[order[s]].tolist()}) == 6


@pytest.mark.gpu
def test_more_long_rows_than_one_pass_of_the_grid(gpu_ctx):
    """9195 rows above LONG among as many short ones: k_adapter_long's 1024 workgroups of four waves take three steps over the
    list, the last for 1003 entries; out of place, in place, with a sentinel and add = 7"""
    buf, table, is_long, _long_rows = long_list_table()
    assert int(is_long.sum()) > 2 * 1024 * 4 and len(table) >= 4096
    want, stats = loop_rows(buf, table)
    for sentinel, add, in_place in ((0, 0, False), (0, 0, True), (1, 7, True)):
        got, gstats = device_cut(gpu_ctx, buf, table + sentinel + add, sentinel=bool(sentinel), add=add, in_place=in_place)
        what = "sentinel %d, add %d, in place %s" % (sentinel, add, in_place)
        GE.same_rows(got[is_long], (want + sentinel + add)[is_long], GE.P_LONG, what + ": the long rows (list entries)")
        GE.same_rows(got, want + sentinel + add, GE.P_SHORT, what)
        assert gstats == stats, what


@pytest.mark.gpu
def test_seeded_random_table_every_row(gpu_ctx):
    rng = np.random.default_rng(2024)
    reads = random_reads(rng, 4000, 300)
    buf, rows = table_of(reads)
    want, stats = check_device(gpu_ctx, buf, rows, combos=((0, 0, False), (1, -3, True)))
    n, cut = rows[:, 3] - rows[:, 2], want[:, 3] - rows[:, 2]
    hit = cut < n
    assert hit.mean() >= 0.25 and (~hit).mean() >= 0.25 and (hit & (n - cut < len(AD))).mean() >= 0.03


@pytest.mark.gpu
def test_adapter_after_quality_trim(gpu_ctx):
    """quality trim, then adapter trim on one table = the two loops in that order; the column gather and the render on the
    result are slices cut by the loops"""
    import torch
    from fastqandfurious_amd import index as X
    data = mixed_file(1500)
    dbuf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    cap = 2000
    table = torch.empty((cap, 6), dtype=torch.int64, device="cuda")
    rc, res = gpu_ctx.scan_device(dbuf.data_ptr(), len(data), table.data_ptr(), cap)
    assert rc == 0 and int(res.n_records) == 1500
    table = table[:1500]
    rows = table.cpu().numpy()
    sbuf = data                                             # (scan_device's rows index the bytes it was given)
    w1, s1 = quality_loop_rows(sbuf, rows, 0, 20)
    w2, s2 = loop_rows(sbuf, w1)
    assert s1[0] > 300 and s2[0] > 300 and s2[2] > 100
    t1, g1 = X.trim_rows_device(gpu_ctx, dbuf, table, 20, 0)
    t2, g2 = X.trim_adapter_rows_device(gpu_ctx, dbuf, t1, AD, out=t1)
    assert t2.data_ptr() == t1.data_ptr() and list(g1) == s1 and list(g2) == s2
    assert (t2.cpu().numpy() == w2).all()
    seq, off = X.select_column_device(gpu_ctx, dbuf, t2, "sequence")
    exp = b"".join(sbuf[a:b] for a, b in w2[:, 2:4])
    assert seq.cpu().numpy().view(np.uint8).tobytes() == exp and (np.diff(off.cpu().numpy()) == w2[:, 3] - w2[:, 2]).all()
    text, toff, tstats = X.render_rows_device(gpu_ctx, dbuf, t2)
    exp = b"".join(b"@" + sbuf[r[0] + 1:r[1]] + b"\n" + sbuf[r[2]:r[3]] + b"\n+\n" + sbuf[r[4]:r[5]] + b"\n" for r in w2.tolist())
    assert text.cpu().numpy().tobytes() == exp and tstats[1] == 1500


@pytest.mark.gpu
def test_errors(gpu_ctx):
    import torch
    from fastqandfurious_amd import hip
    buf, rows = table_of(random_reads(np.random.default_rng(1), 64, 100))
    dbuf = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).cuda()
    table = torch.from_numpy(rows).cuda()
    n = table.shape[0]

    def call(t=table, out=None, ad=AD, err=100, mo=3):
        return gpu_ctx.table_trim_adapter(dbuf.data_ptr(), len(buf), t.data_ptr(), n - 1, ad, err, mo,
                                          d_out=None if out is None else out.data_ptr(), sentinel=False)
    for kw in (dict(ad=b""), dict(ad=b"A" * 65), dict(mo=0), dict(mo=14), dict(err=-1), dict(err=1001), dict(t=table.view(-1)[1:]),
               dict(out=torch.empty_like(table).view(-1)[1:])):
        with pytest.raises(hip.FFQError) as e:
            call(**kw)
        assert e.value.code == hip.E_ARG, kw
    # a scan pending on the context
    data = mixed_file(50)
    d2 = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    t2 = torch.empty((64, 6), dtype=torch.int64, device="cuda")
    gpu_ctx.scan_submit(d2.data_ptr(), len(data), t2.data_ptr(), 64)
    try:
        with pytest.raises(hip.FFQError) as e:
            call()
        assert e.value.code == hip.E_ARG
    finally:
        gpu_ctx.scan_wait()
    assert (table.cpu().numpy() == rows).all()
    assert call(out=torch.empty_like(table))[2] == 0

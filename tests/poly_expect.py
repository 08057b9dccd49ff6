"""What the poly-tail tests share (tests/test_poly.py, test_poly_iter.py): the rule of ffq_table_trim_poly (include/ffq.h) as
a plain loop over bytes -- never the package's own poly_tail_cut --, the hand vectors of the issue, a seeded table with planted
tails, generated files whose reads end in G tails behind an adapter, and the expectation of filter_fastq / filter_fastq_paired
on them.  Computed once per set of parameters and left unchanged."""
import functools

import numpy as np

import merge_expect as M
import overlap_expect as X
import pairs_expect as P

LETTERS = b"ACGT"
BASES = (b"A", b"C", b"G", b"T", None)          # the five `base` values: a fixed base, or any (poly-X)
LONG = 4096                                     # bases above which the library gives a row a wave of its own (csrc/ffq_poly.h)


# ---- the rule --------------------------------------------------------------------------------------------------------
def loop_cut(seq, base, min_len=10):
    """the new length of seq; base: 0..3, or None for the set of all four"""
    n = len(seq)
    S = tuple(range(4)) if base is None else (base,)
    mm = dict.fromkeys(S, 0)
    hit = dict.fromkeys(S, 0)
    last = dict.fromkeys(S, -1)
    stop = n
    for i in range(n):
        k = X.cls(seq[n - 1 - i])
        t = {b: mm[b] + (k != b) for b in S}
        if i >= min_len - 1 and all(t[b] > min(5, (i + 1) // 8) for b in S):
            stop = i
            break
        mm = t
        if k in S:
            hit[k] += 1
            last[k] = i
    if stop < min_len:
        return n
    best = max(S, key=lambda b: (hit[b], -b))          # (ties: the lowest class)
    return n - 1 - last[best]


def base_of(b):
    return None if b is None else LETTERS.index(b)


def loop_rows(seen, rows, base, min_len=10, add=0):
    """(new rows, [changed, bases removed, skipped], new lengths of the eligible rows) for rows (+ add) over `seen` (bytes: the
    buffer as the scanner saw it, with its sentinel if it has one)"""
    out, stats, lens = [], [0, 0, 0], []
    for row in rows:
        row = [int(x) for x in row]
        p2, p3, p4, p5 = (x - add for x in row[2:])
        ok = min(p2, p3, p4, p5) >= 0 and p2 <= p3 <= len(seen) and p4 <= p5 <= len(seen) and p3 - p2 == p5 - p4
        if ok and 10 in seen[p2:p3]:
            ok = False
        if not ok:
            stats[2] += 1
            out.append(row)
            continue
        n = p3 - p2
        c = loop_cut(seen[p2:p3], base_of(base), min_len)
        lens.append((n, c))
        if c != n:
            stats[0] += 1
            stats[1] += n - c
        out.append(row[:3] + [row[2] + c, row[4], row[4] + c])
    return np.array(out, dtype=np.int64).reshape(-1, 6), stats, lens


# ---- the issue's hand vectors: (sequence, base, min_len, new length) ------------------------------------------------------
B10 = b"ACGTACGTAC"
T10 = b"ACGTACGTAT"
HAND = [
    (B10 + b"G" * 10, b"G", 10, 10),
    (B10 + b"G" * 9, b"G", 10, 10),             # the C is the one allowed mismatch of ten positions
    (B10 + b"G" * 8, b"G", 10, 18),
    (b"G" * 10, b"G", 10, 0),
    (b"G" * 9, b"G", 10, 9),
    (T10 + b"GGGAGGGGGGGGGGAG", b"G", 10, 14),
    (T10 + b"GAGAGGGGGGGGGGGG", b"G", 10, 12),
    (T10 + b"GGG" + b"A" * 5 + b"G" * 40, b"G", 10, 10),
    (T10 + b"GGG" + b"A" * 6 + b"G" * 48, b"G", 10, 19),
    (B10 + b"TTTTNTTTTTTT", None, 10, 10),
    (B10 + b"N" * 12, None, 10, 22),
    (b"ACGTTTTTTT" + b"A" * 10, None, 10, 10),
    (b"ACGTTTTTTTT" + b"A" * 10, None, 10, 11),
    (b"acgtacgtac" + b"g" * 12, b"G", 10, 10),
]


def record(buf, header, seq, qual=None):
    """a four-line record appended to buf (a bytearray); its row"""
    p0 = len(buf)
    buf += b"@" + header + b"\n"
    p2 = len(buf)
    buf += seq + b"\n+\n"
    p4 = len(buf)
    buf += (b"I" * len(seq) if qual is None else qual) + b"\n"
    return [p0, p2 - 1, p2, p2 + len(seq), p4, p4 + len(seq)]


def hand_table():
    """One buffer with a four-line record per hand vector, then the ineligible rows.  Returns (bytes, rows, names of the
    ineligible rows): rows index the bytes (no sentinel, add 0)."""
    buf, rows = bytearray(b"##"), []
    for i, (seq, *_rest) in enumerate(HAND):
        rows.append(record(buf, b"h%d" % i, seq))
    names = []
    p0 = len(buf)
    buf += b"@w\nACGT\nAC\n+\n"
    p4 = len(buf)
    buf += b"!!!!\n!!\n"
    rows.append([p0, p0 + 2, p0 + 3, p0 + 10, p4, p4 + 7]); names.append("a newline in the sequence, the lengths agree")
    p0 = len(buf)
    buf += b"@x\n" + B10 + b"\n" + b"G" * 12 + b"\n+\n"
    p4 = len(buf)
    buf += b"I" * 10 + b"\n" + b"I" * 12 + b"\n"
    rows.append([p0, p0 + 2, p0 + 3, p0 + 26, p4, p4 + 23]); names.append("a wrapped record whose last line is all G")
    p0 = len(buf)
    buf += b"@u\n" + b"A" + b"G" * 12 + b"\n+\n" + b"I" * 12 + b"\n"
    rows.append([p0, p0 + 2, p0 + 3, p0 + 16, p0 + 19, p0 + 31]); names.append("unequal lengths")
    rows.append([p0, p0 + 2, p0 + 3, p0 + 16, -1, -1]); names.append("a FASTA row")
    rows.append([p0, p0 + 2, len(buf) - 12, len(buf) + 1, p0 + 18, p0 + 31]); names.append("past the buffer")
    return bytes(buf), rows, names


# ---- a seeded table with planted tails -----------------------------------------------------------------------------------
TAIL_LENGTHS = tuple(range(7, 18)) + tuple(range(40, 51)) + tuple(range(62, 67)) + tuple(range(126, 131))


def body_of(rng, n):
    """n bytes: bases, a few of them lower-case, N or no base at all"""
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
    r = rng.random(n)
    s[r < 0.04] |= 0x20
    s[(r >= 0.04) & (r < 0.05)] = ord("N")
    s[(r >= 0.05) & (r < 0.055)] = ord(".")
    return s.tobytes()


def tail_of(rng, b, length, mismatches, grace):
    """a tail of `length` copies of base b (either case), read 5' to 3', with `mismatches` other bytes in it: in the first
    nine walk positions (grace) or anywhere"""
    t = bytearray(bytes([LETTERS[b] | (0x20 if rng.integers(0, 8) == 0 else 0)]) * length)
    others = bytes(x for x in b"ACGTN*" if x != LETTERS[b])
    for _ in range(mismatches):
        i = int(rng.integers(0, min(9, length) if grace else length))       # a walk position
        t[length - 1 - i] = others[int(rng.integers(0, len(others)))]
    return bytes(t)


@functools.lru_cache(maxsize=None)
def seeded_table(n_rows=4000, seed=7):
    """(bytes, rows): lengths 0..220; four rows in five end in a planted tail (five in eight of them G), every tail length of
    TAIL_LENGTHS with 0..7 mismatches in the grace zone or beyond; some reads are all tail; runs of 40 empty rows and of 40
    ineligible rows lie between rows with 130-base tails"""
    rng = np.random.default_rng(seed)
    buf, rows = bytearray(b"#"), []
    i = 0
    while len(rows) < n_rows:
        if len(rows) in (500, 1500, 2500):
            empty = len(rows) != 1500
            rows.append(record(buf, b"edge%d" % i, body_of(rng, 20) + b"G" * 130))
            for _ in range(40):
                r = record(buf, b"run%d" % i, b"" if empty else b"ACGTGGGGGGGGGGGG")
                rows.append(r if empty else r[:4] + [-1, -1])
            rows.append(record(buf, b"edge%d" % i, body_of(rng, 5) + b"T" * 128 + b"AT"))
        kind = int(rng.integers(0, 10))
        if kind < 8:
            b = 2 if kind < 5 else (0, 1, 3)[kind - 5]
            length = TAIL_LENGTHS[i % len(TAIL_LENGTHS)]
            mism = (0, 0, 1, 1, 2, 3, 4, 5, 6, 7)[int(rng.integers(0, 10))]
            tail = tail_of(rng, b, length, mism, bool(rng.integers(0, 2)))
            n_body = 0 if rng.integers(0, 25) == 0 else int(rng.integers(0, 221 - length))
            seq = body_of(rng, n_body) + tail
        else:
            seq = body_of(rng, int(rng.integers(0, 221)))
        rows.append(record(buf, b"r%d" % i, seq))
        i += 1
    return bytes(buf), tuple(tuple(r) for r in rows[:n_rows])


@functools.lru_cache(maxsize=None)
def seeded_want(base, min_len=10):
    buf, rows = seeded_table()
    return loop_rows(buf, rows, base, min_len)


@functools.lru_cache(maxsize=None)
def long_table(seed=3):
    """(bytes, rows): a 5000-base row whose tail is 4300 G with five mismatches, a 5000-base row of random bases, a row at the
    long threshold and one a byte above it, among short rows of the seeded kind"""
    rng = np.random.default_rng(seed)
    buf, rows = bytearray(b"#"), []
    sbuf, srows = seeded_table()

    def some_short(k):
        for r in srows[k:k + 12]:
            rows.append(record(buf, b"s", sbuf[r[2]:r[3]]))

    some_short(0)
    tail = bytearray(b"G" * 4300)
    for i in (12, 30, 1000, 3000, 4290):                # (walk positions: each within what is allowed there)
        tail[4299 - i] = ord("A")
    rows.append(record(buf, b"long-tail", body_of(rng, 699) + b"A" + bytes(tail)))
    some_short(600)
    rows.append(record(buf, b"long-random", body_of(rng, 5000)))
    rows.append(record(buf, b"at", body_of(rng, 95) + b"C" + b"G" * (LONG - 96)))
    some_short(1200)
    tail = bytearray(b"g" * 4000)
    tail[10] = tail[2000] = tail[3990] = ord("N")
    rows.append(record(buf, b"above", body_of(rng, LONG - 4000) + b"T" + bytes(tail)))
    rows.append(record(buf, b"long-all-tail", b"T" * 6000))
    some_short(2000)
    return bytes(buf), tuple(tuple(r) for r in rows)


@functools.lru_cache(maxsize=None)
def grid_pool():
    """(bytes, rows, idle, long): the pool of the tables above one pass of the grid (tests/grid_expect.py) -- every row of the
    hand table, 260 of the seeded table's, empty and ineligible rows, the long table's long rows and two more just above LONG.
    idle: the pool rows with nothing to do (empty or ineligible); long: those above LONG.  No sentinel, add 0."""
    hbuf, hrows, names = hand_table()
    assert names[-1] == "past the buffer"
    buf, rows = bytearray(hbuf), [list(r) for r in hrows[:-1]]
    idle = list(range(len(HAND), len(rows)))
    sbuf, srows = seeded_table()
    for i, r in enumerate(srows[:260]):
        rows.append(record(buf, b"s%d" % i, sbuf[r[2]:r[3]]))
    for i in range(8):
        idle += [len(rows), len(rows) + 1]
        rows.append(record(buf, b"e%d" % i, b""))
        rows.append(record(buf, b"f%d" % i, b"ACGT" + b"G" * (12 + i))[:4] + [-1, -1])
    lbuf, lrows = long_table()
    rng = np.random.default_rng(19)
    seqs = [lbuf[r[2]:r[3]] for r in lrows if r[3] - r[2] >= LONG]
    seqs += [body_of(rng, 90) + b"G" * (LONG - 88), body_of(rng, LONG + 3)]
    long = []
    for i, s in enumerate(seqs):
        if len(s) > LONG:
            long.append(len(rows))
        rows.append(record(buf, b"l%d" % i, s))
    idle.append(len(rows))
    rows.append([0, 1, len(buf) - 12, len(buf) + 1, 2, 15])        # past the buffer
    return bytes(buf), tuple(tuple(r) for r in rows), tuple(idle), tuple(long)


# ---- files: reads that end in adapter + G tail, bad ends, tails of other bases ---------------------------------------------------
def one_read(rng, n, adapter):
    """(sequence, quality) of n bases; kinds: plain, a bad 3' end, the adapter at the end, the adapter followed by a G tail
    (the instrument ran past the fragment), a G tail alone, a tail of another base"""
    seq = bytearray(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes())
    v = rng.integers(30, 41, n)
    kind = int(rng.integers(0, 10))
    if kind == 1:
        t = int(rng.integers(5, 30))
        v[n - t:] = rng.integers(2, 9, t)
    elif kind == 2:
        p = int(rng.integers(n // 2, n - 2))
        ins = adapter[:n - p]
        seq[p:p + len(ins)] = ins
    elif kind in (3, 4):                            # fragment, whole adapter, G to the end
        p = int(rng.integers(20, n - len(adapter) - 12))
        seq[p:] = adapter + b"G" * (n - p - len(adapter))
        if kind == 4:
            seq[int(rng.integers(p + len(adapter) + 10, n + 1)) - 1] = ord("A")
    elif kind == 5:
        t = int(rng.integers(8, 60))
        seq[n - t:] = b"G" * t
    elif kind == 6:
        t = int(rng.integers(8, 60))
        seq[n - t:] = bytes([LETTERS[int(rng.integers(0, 4))]]) * t
        seq[n - 1 - int(rng.integers(0, t))] = ord("N")
    return bytes(seq), bytes((v + 33).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def single_records(n=1500, seed=31):
    rng = np.random.default_rng(seed)
    return tuple((b"POLY:%d:%d" % (seed, i),) + one_read(rng, int(rng.integers(60, 151)), P.ADAPTER1) for i in range(n))


def trims(s, q, quality_cutoff, adapter, poly_g, poly_x, counts):
    """one read through the four trims in the chain's order; counts: [g reads, g bases, x reads, x bases], added to"""
    if quality_cutoff is not None and 10 not in q:
        a, z = P.quality_span(q, quality_cutoff[0], quality_cutoff[1])
        s, q = s[a:z], q[a:z]
    if 10 in s:                                     # (a wrapped record: none of the sequence rules applies)
        return s, q
    if poly_g is not None:
        c = loop_cut(s, 2, poly_g)
        counts[0] += c != len(s)
        counts[1] += len(s) - c
        s, q = s[:c], q[:c]
    if adapter is not None:
        c = P.adapter_cut(s, adapter, 100, 3)
        s, q = s[:c], q[:c]
    if poly_x is not None:
        c = loop_cut(s, None, poly_x)
        counts[2] += c != len(s)
        counts[3] += len(s) - c
        s, q = s[:c], q[:c]
    return s, q


class ExpectedSingle:
    """what filter_fastq(quality_cutoff, adapter, min_len, poly_g, poly_x) leaves behind"""

    def __init__(self, recs, quality_cutoff=None, adapter=None, min_len=None, poly_g=None, poly_x=None):
        self.poly = [0, 0, 0, 0]
        self.removed = self.n_out = 0
        out = []
        self.kept = []
        for h, s, q in recs:
            s2, q2 = trims(s, q, quality_cutoff, adapter, poly_g, poly_x, self.poly)
            self.removed += len(s) - len(s2)
            if min_len is not None and len(s2) < min_len:
                self.kept.append(None)
                continue
            self.n_out += 1
            self.kept.append(s2)
            out.append(b"@" + h + b"\n" + s2 + b"\n+\n" + q2 + b"\n")
        self.text = b"".join(out)
        self.n_in = len(recs)

    def result(self):
        return (self.n_in, self.n_out, self.removed, len(self.text))


def check_poly_report(rep, counts):
    assert [rep.poly_g_reads, rep.poly_g_bases, rep.poly_x_reads, rep.poly_x_bases] == list(counts)


@functools.lru_cache(maxsize=None)
def pair_records(n_pairs=800, seed=13):
    """the mates of tests/merge_expect.py's kind -- fragments shorter than, as long as and longer than the reads, a few wrapped
    records -- where the bytes behind a short fragment's adapter are G to the read's end in every second such pair"""
    r1, r2 = M.records(n_pairs, seed)
    rng = np.random.default_rng(seed)
    out = ([], [])
    for k, (recs, ad) in enumerate(((r1, P.ADAPTER1), (r2, P.ADAPTER2))):
        for h, s, q in recs:
            p = s.find(ad)
            if p >= 0 and 10 not in s and rng.integers(0, 2) and len(s) - p - len(ad) >= 10:
                s = s[:p + len(ad)] + b"G" * (len(s) - p - len(ad))
            out[k].append((h, s, q))
    return tuple(out[0]), tuple(out[1])


class ExpectedPaired:
    """what filter_fastq_paired(quality_cutoff, adapter, adapter2, min_len, overlap, merged_out, poly_g, poly_x) leaves behind:
    the per-mate trims in the chain's order, the overlap with its cut, the length filter (pair_filter "any"), the merge"""

    def __init__(self, recs1, recs2, quality_cutoff=None, adapters=(None, None), min_len=None, rules=X.DEFAULT, poly_g=None, poly_x=None):
        self.poly = [0, 0, 0, 0]
        self.removed = 0
        trimmed = ([], [])
        for k, recs in enumerate((recs1, recs2)):
            for h, s, q in recs:
                s2, q2 = trims(s, q, quality_cutoff, adapters[k], poly_g, poly_x, self.poly)
                self.removed += len(s) - len(s2)
                trimmed[k].append((h, s2, q2))
        w = M.Expected(tuple(trimmed[0]), tuple(trimmed[1]), rules, (min_len, min_len))
        self.removed += w.removed
        self.merged = w
        self.text = w.text

    def result(self):
        w = self.merged
        return (w.pairs_in, w.pairs_out, self.removed, len(self.text[0]), len(self.text[1]), w.dropped)

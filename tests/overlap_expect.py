"""What the overlap tests share (tests/test_overlap.py, test_overlap_iter.py, test_overlap_host.py): the rule of
ffq_table_pair_overlap (include/ffq.h) as plain loops over bytes -- never the package's own pair_overlap --, the expectation of
a call on two hand-made tables, generated paired-end files whose mates read one fragment from both ends, and the expectation
of filter_fastq_paired(overlap=...) on them.  Computed once per set of parameters and left unchanged."""
import functools

import numpy as np

import pairs_expect as P

MAX_LEN = 512
HIST_WORDS = 2 * MAX_LEN + 1
DEFAULT = (30, 5, 200)                # min_overlap, max_diff, diff_permille: fastp's
ADAPTER1, ADAPTER2 = P.ADAPTER1 + b"ACGTTGCA" * 70, P.ADAPTER2 + b"TTGACCAG" * 70       # what follows the fragment on either side


# ---- the rule --------------------------------------------------------------------------------------------------------
def cls(b):
    if b in b"Aa":
        return 0
    if b in b"Cc":
        return 1
    if b in b"Gg":
        return 2
    if b in b"Tt":
        return 3
    return 4


def loop_overlap(a, b, min_overlap, max_diff, diff_permille):
    """o* of the first accepted candidate, or None"""
    n1, n2 = len(a), len(b)
    if n1 < min_overlap or n2 < min_overlap:
        return None
    ca = [cls(x) for x in a]
    rb = []
    for j in range(n2):
        c = cls(b[n2 - 1 - j])
        rb.append(3 - c if c < 4 else 4)
    for o in list(range(0, n1 - min_overlap + 1)) + [-k for k in range(1, n2 - min_overlap + 1)]:
        lo, hi = max(0, o), min(n1, n2 + o)
        ov = hi - lo
        assert ov >= min_overlap
        limit = min(max_diff, (ov * diff_permille) // 1000)
        mm = 0
        for i in range(lo, hi):
            if not (ca[i] < 4 and ca[i] == rb[i - o]):
                mm += 1
                if mm > limit:                  # (only mm <= limit is asked for)
                    break
        if mm <= limit:
            return o
    return None


def row_ok(seen, row, sentinel):
    """a row's eligibility (ffq_table_trim_adapter's); seen: the buffer as the scanner saw it (with its sentinel), row:
    coordinates of it"""
    p2, p3, p4, p5 = row[2:]
    ok = min(p2, p3, p4, p5) >= 0 and p2 <= p3 <= len(seen) and p4 <= p5 <= len(seen) and p3 - p2 == p5 - p4
    if ok and sentinel and p3 > p2 and p2 < 1:
        ok = False
    return ok and 10 not in seen[p2:p3]


def expect_table(seen1, rows1, sent1, seen2, rows2, sent2, rules, trim):
    """per pair: (insert, c1, c2) -- insert as d_insert has it, c1 / c2 the lengths left (None: the row stays as it is)"""
    out = []
    for r1, r2 in zip(rows1, rows2):
        if not (row_ok(seen1, r1, sent1) and row_ok(seen2, r2, sent2)) or r1[3] - r1[2] > MAX_LEN or r2[3] - r2[2] > MAX_LEN:
            out.append((-2, None, None))
            continue
        a, b = seen1[r1[2]:r1[3]], seen2[r2[2]:r2[3]]
        o = loop_overlap(a, b, *rules)
        if o is None:
            out.append((-1, None, None))
            continue
        insert = len(b) + o
        if trim and o < 0:
            out.append((insert, min(len(a), insert), min(len(b), insert)))
        else:
            out.append((insert, None, None))
    return out


def summarize(per_pair, rows1, rows2):
    """(rows 1 out, rows 2 out, inserts, hist, counts) of a call over these pairs; rows*: int64[n][6] as the table holds them"""
    o1, o2 = np.array(rows1, dtype=np.int64).reshape(-1, 6).copy(), np.array(rows2, dtype=np.int64).reshape(-1, 6).copy()
    hist = np.zeros(HIST_WORDS, dtype=np.uint64)
    counts = [0] * 6
    ins = []
    for i, (insert, c1, c2) in enumerate(per_pair):
        ins.append(insert)
        counts[5 if insert == -2 else 0] += 1
        if insert >= 0:
            counts[1] += 1
            hist[insert] += 1
        changed = False
        for k, (o, c) in enumerate(((o1, c1), (o2, c2))):
            n = int(o[i, 3] - o[i, 2])
            if c is not None and c != n:
                o[i, 3], o[i, 5] = o[i, 2] + c, o[i, 4] + c
                counts[3 + k] += n - c
                changed = True
        counts[2] += changed
    return o1, o2, np.array(ins, dtype=np.int32), hist, counts


# ---- mates that read one fragment from both ends ---------------------------------------------------------------------------
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s):
    return s.translate(COMP)[::-1]


def mates_of(rng, frag_len, n1, n2, err=0.0):
    """(sequence 1, sequence 2) of a fragment of frag_len random bases read n1 bases from one end and n2 from the other, the
    adapters' bytes behind a fragment shorter than a read, every base changed with probability err"""
    frag = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, frag_len)].tobytes()
    s1 = (frag + ADAPTER1)[:n1]
    s2 = (revcomp(frag) + ADAPTER2)[:n2]
    out = []
    for s in (s1, s2):
        s = bytearray(s)
        for i in np.flatnonzero(rng.random(len(s)) < err):
            s[i] = b"ACGT"[(b"ACGT".index(bytes([s[i]]).upper()) + int(rng.integers(1, 4))) % 4]
        out.append(bytes(s))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def records(n_pairs=1200, seed=5):
    """(records of mate 1, records of mate 2): lists of (header, sequence, quality).  Fragments of 20..400 bases, reads of
    100..150 (so: fragments shorter than min_overlap, shorter than the reads, between, longer than both), one pair in five
    unrelated, mismatches at 2 %, a few Ns and lower-case stretches, bad 3' ends for the quality trim; mate 2's headers are
    longer, so fills of one size hold different numbers of records"""
    rng = np.random.default_rng(seed)
    m1, m2 = [], []
    for i in range(n_pairs):
        name = b"OVL:%d:%d" % (seed, i)
        h1, h2 = name + b"/1", name + b" 2:N:0:" + b"ACGTACGT" * int(rng.integers(1, 6))
        n1, n2 = int(rng.integers(100, 151)), int(rng.integers(100, 151))
        kind = int(rng.integers(0, 10))
        frag = int(rng.integers(20, 401))
        if kind < 2:
            s1, _ = mates_of(rng, 400, n1, n2)
            _, s2 = mates_of(rng, 400, n1, n2)
        else:
            s1, s2 = mates_of(rng, frag, n1, n2, 0.02)
        s1, s2 = bytearray(s1), bytearray(s2)
        if kind == 2:
            s1[int(rng.integers(0, n1))] = ord("N")
            s2[int(rng.integers(0, n2))] = ord("N")
        if kind == 3:
            s1[10:40] = bytes(s1[10:40]).lower()
        q = []
        for n in (n1, n2):
            v = rng.integers(30, 41, n)
            if rng.integers(0, 4) == 0:
                t = int(rng.integers(3, 30))
                v[n - t:] = rng.integers(2, 9, t)
            q.append(bytes((v + 33).astype(np.uint8)))
        m1.append((h1, bytes(s1), q[0]))
        m2.append((h2, bytes(s2), q[1]))
    return tuple(m1), tuple(m2)


class Expected:
    """what filter_fastq_paired(overlap=rules, ...) leaves behind: the order is quality, adapter, overlap, filter (length
    alone; pair_filter "any")"""

    def __init__(self, recs1, recs2, rules=DEFAULT, quality_cutoff=None, adapters=(None, None), min_len=(None, None), use_overlap=True):
        self.text = [[], []]
        self.removed = 0
        self.dropped = {"mate1_only": 0, "mate2_only": 0, "both": 0}
        self.analysed = self.overlapped = self.trimmed = 0
        self.bases = [0, 0]
        self.hist = np.zeros(HIST_WORDS, dtype=np.uint64)
        self.pairs_in = len(recs1)
        self.pairs_out = 0
        self.kinds = set()
        for (h1, s1, q1), (h2, s2, q2) in zip(recs1, recs2):
            cut = []
            for (s, q), ad in (((s1, q1), adapters[0]), ((s2, q2), adapters[1])):
                n = len(s)
                if quality_cutoff is not None:
                    a, z = P.quality_span(q, quality_cutoff[0], quality_cutoff[1])
                    s, q = s[a:z], q[a:z]
                if ad is not None:
                    c = P.adapter_cut(s, ad, 100, 3)
                    s, q = s[:c], q[:c]
                self.removed += n - len(s)
                cut.append((s, q))
            (s1, q1), (s2, q2) = cut
            if use_overlap:
                self.analysed += 1
                o = loop_overlap(s1, s2, *rules)
                self.kinds.add("none" if o is None else "cut" if o < 0 else "kept")
                if o is not None:
                    self.overlapped += 1
                    insert = len(s2) + o
                    self.hist[insert] += 1
                    if o < 0:
                        c1, c2 = min(len(s1), insert), min(len(s2), insert)
                        self.bases[0] += len(s1) - c1
                        self.bases[1] += len(s2) - c2
                        self.removed += len(s1) - c1 + len(s2) - c2
                        self.trimmed += (c1 != len(s1)) or (c2 != len(s2))
                        s1, q1, s2, q2 = s1[:c1], q1[:c1], s2[:c2], q2[:c2]
            v1 = min_len[0] is not None and len(s1) < min_len[0]
            v2 = min_len[1] is not None and len(s2) < min_len[1]
            if v1 or v2:
                self.dropped["both" if v1 and v2 else "mate1_only" if v1 else "mate2_only"] += 1
                continue
            self.pairs_out += 1
            self.text[0].append(b"@" + h1 + b"\n" + s1 + b"\n+\n" + q1 + b"\n")
            self.text[1].append(b"@" + h2 + b"\n" + s2 + b"\n+\n" + q2 + b"\n")
        self.text = [b"".join(self.text[0]), b"".join(self.text[1])]

    def result(self):
        return (self.pairs_in, self.pairs_out, self.removed, len(self.text[0]), len(self.text[1]), self.dropped)

    def check_report(self, rep):
        assert (rep.pairs_analysed, rep.pairs_overlapped, rep.pairs_trimmed, list(rep.bases_removed)) == \
            (self.analysed, self.overlapped, self.trimmed, self.bases)
        assert rep.insert_hist.dtype == np.uint64 and (rep.insert_hist == self.hist).all()
        assert rep.insert_peak == (int(np.argmax(self.hist)) if self.hist.any() else None)


def run(F, data1, data2, entrypos, fbufsize, rules=DEFAULT, opener1=None, opener2=None, **kw):
    """filter_fastq_paired(overlap=OverlapRules(*rules)) over two byte strings -> (result, out1, out2, overlap report)"""
    import io
    o1, o2 = io.BytesIO(), io.BytesIO()
    fh1 = opener1(data1) if opener1 else io.BytesIO(data1)
    fh2 = opener2(data2) if opener2 else io.BytesIO(data2)
    rep = F.OverlapReport() if rules is not None else None
    try:
        res = F.filter_fastq_paired(fh1, fh2, o1, o2, fbufsize=fbufsize, entrypos=entrypos,
                                    overlap=None if rules is None else F.OverlapRules(*rules), overlap_report=rep, **kw)
    finally:
        fh1.close()
        fh2.close()
    return res, o1.getvalue(), o2.getvalue(), rep

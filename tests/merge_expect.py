"""What the merge tests share (tests/test_merge.py, test_merge_iter.py, test_merge_host.py): the rule of ffq_table_pair_merge
(include/ffq.h) as a plain loop over bytes -- never the package's own merge_mates --, the expectation of a call on two hand-made
tables, generated paired-end files, and the expectation of filter_fastq_paired(merged_out=...) on them.  Computed once per set
of parameters and left unchanged."""
import functools
import io

import numpy as np

import overlap_expect as X

MAX_LEN = 512
COMP = {65: 84, 84: 65, 67: 71, 71: 67, 97: 116, 116: 97, 99: 103, 103: 99}


# ---- the rule --------------------------------------------------------------------------------------------------------
def loop_merge(a, qa, b, qb, ins):
    """(base, qual, positions inside the overlap, of those taken from mate 2), or None: the lines as they stand, ins as d_insert
    has it.  The caller has checked the rows; the lengths and ins are checked here."""
    n1, n2 = len(a), len(b)
    assert len(qa) == n1 and len(qb) == n2
    if n1 > MAX_LEN or n2 > MAX_LEN or ins < 0:
        return None
    o = ins - n2
    if not (-n2 < o and o < n1):
        return None
    L = n2 + o if o < 0 else max(n1, n2 + o)
    base, qual = bytearray(), bytearray()
    ov = taken = 0
    for p in range(L):
        in_a = p < n1
        j2 = p - o
        in_b = 0 <= j2 < n2
        bi = n2 - 1 - j2
        assert in_a or in_b
        if in_a and in_b:
            take_b = qb[bi] > qa[p]
            ov += 1
            taken += take_b
        else:
            take_b = not in_a
        if take_b:
            base.append(COMP.get(b[bi], b[bi]))
            qual.append(qb[bi])
        else:
            base.append(a[p])
            qual.append(qa[p])
    return bytes(base), bytes(qual), ov, taken


def row_ok(seen, row, sentinel):
    """a row's eligibility (ffq_table_stats'); seen: the buffer as the scanner saw it (with its sentinel), row: coordinates"""
    p2, p3, p4, p5 = row[2:]
    ok = min(p2, p3, p4, p5) >= 0 and p2 <= p3 <= len(seen) and p4 <= p5 <= len(seen) and p3 - p2 == p5 - p4
    if ok and sentinel and p3 > p2 and (p2 < 1 or p4 < 1):
        ok = False
    return ok


def header_ok(seen, row):
    return row[0] >= 0 and row[0] + 1 <= row[1] <= len(seen)


def merged_text(seen1, r1, sent1, seen2, r2, sent2, ins):
    """(text, bases, overlap, taken) of a pair, or None: it is not merged"""
    if not (row_ok(seen1, r1, sent1) and row_ok(seen2, r2, sent2) and header_ok(seen1, r1)):
        return None
    if r1[3] - r1[2] > MAX_LEN or r2[3] - r2[2] > MAX_LEN:
        return None
    m = loop_merge(seen1[r1[2]:r1[3]], seen1[r1[4]:r1[5]], seen2[r2[2]:r2[3]], seen2[r2[4]:r2[5]], ins)
    if m is None:
        return None
    base, qual, ov, taken = m
    return b"@" + seen1[r1[0] + 1:r1[1]] + b"\n" + base + b"\n+\n" + qual + b"\n", len(base), ov, taken


def summarize(per_pair, rows1, rows2, ords):
    """(text, off, rest 1, rest 2, rest ordinals, counts) of a call over these pairs; per_pair: merged_text's answers; rows*:
    int64[n][6] as the tables hold them; ords: j per pair"""
    text, off, keep = bytearray(), [0], []
    counts = [0] * 6
    for k, m in enumerate(per_pair):
        if m is None:
            keep.append(k)
            counts[1] += 1
        else:
            text += m[0]
            counts[0] += 1
            counts[3] += m[1]
            counts[4] += m[2]
            counts[5] += m[3]
        off.append(len(text))
    counts[2] = len(text)
    rows1, rows2 = np.asarray(rows1, dtype=np.int64).reshape(-1, 6), np.asarray(rows2, dtype=np.int64).reshape(-1, 6)
    return (bytes(text), np.array(off, dtype=np.int64), rows1[keep], rows2[keep], np.asarray(ords, dtype=np.int64)[keep], counts)


# ---- generated paired-end files --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def records(n_pairs=2000, seed=11):
    """(records of mate 1, records of mate 2): lists of (header, sequence, quality), the sequence possibly wrapped (a b"\\n"
    inside both lines).  Fragments of 20..400 bases read 100..150 from either end (short: adapters behind the fragment;
    middling: the mates overlap; long: they do not), mismatches at 2 % with a LOW quality on one side, Ns, a few wrapped
    records; mate 2's headers are longer, so fills of one size hold different numbers of records."""
    rng = np.random.default_rng(seed)
    m1, m2 = [], []
    for i in range(n_pairs):
        name = b"MRG:%d:%d" % (seed, i)
        h1, h2 = name + b"/1", name + b" 2:N:0:" + b"ACGTACGT" * int(rng.integers(1, 6))
        n1, n2 = int(rng.integers(100, 151)), int(rng.integers(100, 151))
        kind = int(rng.integers(0, 12))
        frag = int(rng.integers(20, 401))
        if kind < 2:
            s1, _ = X.mates_of(rng, 400, n1, n2)
            _, s2 = X.mates_of(rng, 400, n1, n2)
        else:
            s1, s2 = X.mates_of(rng, frag, n1, n2, 0.02)
        s1, s2 = bytearray(s1), bytearray(s2)
        if kind == 2:
            s1[int(rng.integers(0, n1))] = ord("N")
            s2[int(rng.integers(0, n2))] = ord("N")
        if kind == 3:
            s1[10:40] = bytes(s1[10:40]).lower()
        q = [bytes((rng.integers(20, 41, n) + 33).astype(np.uint8)) for n in (n1, n2)]
        s1, s2 = bytes(s1), bytes(s2)
        if kind == 4 and i % 3 == 0:                 # wrapped: both lines of a mate broken at the same place
            w = int(rng.integers(20, 80))
            q = [x.replace(b"@", b"A") for x in q]      # (no continuation line that looks like a header)
            if i % 2:
                s1, q[0] = s1[:w] + b"\n" + s1[w:], q[0][:w] + b"\n" + q[0][w:]
            else:
                s2, q[1] = s2[:w] + b"\n" + s2[w:], q[1][:w] + b"\n" + q[1][w:]
        m1.append((h1, s1, q[0]))
        m2.append((h2, s2, q[1]))
    return tuple(m1), tuple(m2)


def file_of(recs):
    return b"".join(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n" for h, s, q in recs)


class Expected:
    """what filter_fastq_paired(overlap=rules, merged_out=..., min_len=...) leaves behind: overlap (with its cut), the length
    filter (pair_filter "any"), merge"""

    def __init__(self, recs1, recs2, rules=X.DEFAULT, min_len=(None, None), merge=True):
        out = [[], [], []]
        self.removed = 0
        self.dropped = {"mate1_only": 0, "mate2_only": 0, "both": 0}
        self.pairs_in = len(recs1)
        self.pairs_out = self.pairs_merged = self.bases_merged = self.overlap_positions = self.taken = 0
        self.written = [0, 0]
        self.kinds = set()
        for (h1, s1, q1), (h2, s2, q2) in zip(recs1, recs2):
            ins = -2
            if 10 not in s1 and 10 not in s2:
                o = X.loop_overlap(s1, s2, *rules)
                ins = -1 if o is None else len(s2) + o
                if o is not None and o < 0:
                    c1, c2 = min(len(s1), ins), min(len(s2), ins)
                    self.removed += len(s1) - c1 + len(s2) - c2
                    s1, q1, s2, q2 = s1[:c1], q1[:c1], s2[:c2], q2[:c2]
            # (the length of a wrapped record's sequence slice includes its newline)
            v1 = min_len[0] is not None and len(s1) < min_len[0]
            v2 = min_len[1] is not None and len(s2) < min_len[1]
            if v1 or v2:
                self.dropped["both" if v1 and v2 else "mate1_only" if v1 else "mate2_only"] += 1
                continue
            self.pairs_out += 1
            m = loop_merge(s1, q1, s2, q2, ins) if merge and ins >= 0 else None
            self.kinds.add("wrapped" if ins == -2 else "none" if ins == -1 else "merged" if m else "unmergeable")
            if m is not None:
                out[2].append(b"@" + h1 + b"\n" + m[0] + b"\n+\n" + m[1] + b"\n")
                self.pairs_merged += 1
                self.bases_merged += len(m[0])
                self.overlap_positions += m[2]
                self.taken += m[3]
                continue
            out[0].append(b"@" + h1 + b"\n" + s1 + b"\n+\n" + q1 + b"\n")
            out[1].append(b"@" + h2 + b"\n" + s2 + b"\n+\n" + q2 + b"\n")
            self.written[0] += 1
            self.written[1] += 1
        self.text = [b"".join(x) for x in out]

    def result(self):
        return (self.pairs_in, self.pairs_out, self.removed, len(self.text[0]), len(self.text[1]), self.dropped)

    def check_report(self, rep):
        assert (rep.pairs_merged, rep.bases_merged, rep.bytes_merged, rep.overlap_positions, rep.taken_from_mate2) == \
            (self.pairs_merged, self.bases_merged, len(self.text[2]), self.overlap_positions, self.taken)


def run(F, data1, data2, entrypos, fbufsize, rules=X.DEFAULT, merge=True, **kw):
    """filter_fastq_paired over two byte strings -> (result, out1, out2, merged, merge report, FilterReports)"""
    o1, o2, om = io.BytesIO(), io.BytesIO(), io.BytesIO()
    rep = F.MergeReport() if merge else None
    reps = (F.FilterReport(), F.FilterReport())
    res = F.filter_fastq_paired(io.BytesIO(data1), io.BytesIO(data2), o1, o2, fbufsize=fbufsize, entrypos=entrypos,
                                overlap=F.OverlapRules(*rules), merged_out=om if merge else None, merge_report=rep,
                                report=reps[0], report2=reps[1], **kw)
    return res, o1.getvalue(), o2.getvalue(), om.getvalue(), rep, reps

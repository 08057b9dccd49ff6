"""What the correction tests share (tests/test_correct.py, test_correct_iter.py, test_correct_host.py): the rule of
ffq_table_pair_correct (include/ffq.h) as a plain loop over bytes -- never the package's own correct_mates --, the expectation of
a call on two hand-made tables, generated paired-end files, and the expectation of filter_fastq_paired(correction=...) on them.
Computed once per set of parameters and left unchanged."""
import functools
import io

import numpy as np

import merge_expect as M
import overlap_expect as X
import pairs_expect as P

MAX_LEN = 512
GOOD, BAD, QUAL_BASE = 30, 14, 33          # fastp's values
COMP = {65: 84, 84: 65, 67: 71, 71: 67, 97: 116, 116: 97, 99: 103, 103: 99}
CLS = {65: 0, 97: 0, 67: 1, 99: 1, 71: 2, 103: 2, 84: 3, 116: 3}


# ---- the rule --------------------------------------------------------------------------------------------------------
def loop_correct(a, qa, b, qb, ins, good=GOOD, bad=BAD, qual_base=QUAL_BASE):
    """None: the pair is not looked at.  Else (a, qa, b, qb, corrected in mate 1, in mate 2, mismatch positions, matrix[20]): the
    four lines as the pass leaves them.  The caller has checked the rows; the lengths and ins are checked here."""
    n1, n2 = len(a), len(b)
    assert len(qa) == n1 and len(qb) == n2
    if n1 > MAX_LEN or n2 > MAX_LEN or ins < 0:
        return None
    o = ins - n2
    if not (-n2 < o and o < n1):
        return None
    G, B = qual_base + good, qual_base + bad
    assert 0 <= B < G <= 255
    a, qa, b, qb = bytearray(a), bytearray(qa), bytearray(b), bytearray(qb)
    fix1 = fix2 = mism = 0
    matrix = [0] * 20
    for p in range(max(0, o), min(n1, n2 + o)):
        bi = n2 - 1 - (p - o)
        ca, cb = CLS.get(a[p], 4), CLS.get(b[bi], 4)
        if ca < 4 and cb < 4 and ca == 3 - cb:
            continue
        mism += 1
        if qa[p] >= G and qb[bi] <= B and ca < 4:
            b[bi], qb[bi] = COMP[a[p]], qa[p]
            matrix[4 * cb + CLS[b[bi]]] += 1
            fix2 += 1
        elif qb[bi] >= G and qa[p] <= B and cb < 4:
            a[p], qa[p] = COMP[b[bi]], qb[bi]
            matrix[4 * ca + CLS[a[p]]] += 1
            fix1 += 1
    return bytes(a), bytes(qa), bytes(b), bytes(qb), fix1, fix2, mism, matrix


def pair_correct(seen1, r1, sent1, seen2, r2, sent2, ins, **rules):
    """loop_correct for a pair of rows (coordinates of the buffers as seen), or None: it is not looked at.  No word about the
    header: the rule does not ask."""
    if not (M.row_ok(seen1, r1, sent1) and M.row_ok(seen2, r2, sent2)):
        return None
    if r1[3] - r1[2] > MAX_LEN or r2[3] - r2[2] > MAX_LEN:
        return None
    return loop_correct(seen1[r1[2]:r1[3]], seen1[r1[4]:r1[5]], seen2[r2[2]:r2[3]], seen2[r2[4]:r2[5]], ins, **rules)


def counts_of(per_pair):
    """the six counts and the matrix of a call over these pairs; per_pair: pair_correct's answers"""
    counts, matrix = [0] * 6, [0] * 20
    for c in per_pair:
        if c is None:
            counts[5] += 1
            continue
        counts[0] += 1
        counts[1] += 1 if c[4] + c[5] else 0
        counts[2] += c[4]
        counts[3] += c[5]
        counts[4] += c[6]
        matrix = [x + y for x, y in zip(matrix, c[7])]
    return counts, matrix


def apply(seen1, rows1, seen2, rows2, per_pair):
    """both buffers (as seen) behind a call; the rows of different pairs share no bytes"""
    s1, s2 = bytearray(seen1), bytearray(seen2)
    for r1, r2, c in zip(rows1, rows2, per_pair):
        if c is not None:
            s1[r1[2]:r1[3]], s1[r1[4]:r1[5]], s2[r2[2]:r2[3]], s2[r2[4]:r2[5]] = c[0], c[1], c[2], c[3]
    return bytes(s1), bytes(s2)


# ---- generated paired-end files --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def records(n_pairs=1500, seed=17, wrapped=True):
    """merge_expect.records' pairs with the qualities a correction needs: most calls sure (Q30..40), one in eight poor (Q2..14),
    one in eight between the thresholds (Q15..29) -- so that a mismatch meets sure against poor (corrected, on either side), sure
    against sure and middling against anything (left as they are) --, and a bad 3' end on a quarter of the reads for the quality
    trim.  Mismatches at 2 %, Ns, lower case, a few wrapped records (wrapped=False: those pairs are left out)."""
    r1, r2 = M.records(n_pairs, seed)
    if not wrapped:
        keep = [i for i in range(len(r1)) if 10 not in r1[i][1] and 10 not in r2[i][1]]
        r1, r2 = tuple(r1[i] for i in keep), tuple(r2[i] for i in keep)
    rng = np.random.default_rng([seed, 99])

    def quals(q):
        n = len(q)
        kind = rng.integers(0, 8, n)
        v = np.where(kind == 0, rng.integers(2, 15, n), np.where(kind == 1, rng.integers(15, 30, n), rng.integers(30, 41, n))) + 33
        if rng.integers(0, 4) == 0:
            t = int(rng.integers(3, 30))
            v[n - t:] = rng.integers(2, 9, t) + 33
        out = v.astype(np.uint8)
        nl = np.frombuffer(q, dtype=np.uint8) == 10             # (a wrapped record keeps its newline)
        out[nl] = 10
        return bytes(np.where(out == 64, 65, out).astype(np.uint8))     # (no '@' in a quality line)
    return tuple((h, s, quals(q)) for h, s, q in r1), tuple((h, s, quals(q)) for h, s, q in r2)


file_of = M.file_of


@functools.lru_cache(maxsize=None)
def overlap_of(s1, s2, rules):
    """overlap_expect.loop_overlap, once per pair of sequences (the expectations of several tests meet the same pairs)"""
    return X.loop_overlap(s1, s2, *rules)


class Expected:
    """what filter_fastq_paired(overlap=rules, correction=..., [quality_cutoff], [merged_out], [dedup], min_len=...) leaves behind:
    quality trim, overlap (with its cut), correction, the length filter (pair_filter "any"), dedup by the sequences as read, merge"""

    def __init__(self, recs1, recs2, rules=X.DEFAULT, min_len=(None, None), merge=False, correct=True, quality_cutoff=None, dedup=False):
        out = [[], [], []]
        self.removed = 0
        self.dropped = {"mate1_only": 0, "mate2_only": 0, "both": 0}
        self.pairs_in = len(recs1)
        self.pairs_out = self.pairs_merged = self.duplicates = 0
        self.counts, self.matrix = [0] * 5, [0] * 20
        self.uncorrected = 0
        seen = set()
        for (h1, s1, q1), (h2, s2, q2) in zip(recs1, recs2):
            key = (s1, s2)
            wrapped = 10 in s1 or 10 in s2
            if quality_cutoff is not None:
                assert not wrapped
                (a1, e1), (a2, e2) = P.quality_span(q1, 0, quality_cutoff), P.quality_span(q2, 0, quality_cutoff)
                self.removed += len(s1) - (e1 - a1) + len(s2) - (e2 - a2)
                s1, q1, s2, q2 = s1[a1:e1], q1[a1:e1], s2[a2:e2], q2[a2:e2]
            ins = -2
            if not wrapped:
                o = overlap_of(s1, s2, tuple(rules))
                ins = -1 if o is None else len(s2) + o
                if o is not None and o < 0:
                    c1, c2 = min(len(s1), ins), min(len(s2), ins)
                    self.removed += len(s1) - c1 + len(s2) - c2
                    s1, q1, s2, q2 = s1[:c1], q1[:c1], s2[:c2], q2[:c2]
            c = loop_correct(s1, q1, s2, q2, ins) if correct and ins >= 0 else None
            if c is not None:
                s1, q1, s2, q2 = c[:4]
                self.counts = [x + y for x, y in zip(self.counts, (1, 1 if c[4] + c[5] else 0, c[4], c[5], c[6]))]
                self.matrix = [x + y for x, y in zip(self.matrix, c[7])]
                self.uncorrected += c[6] - c[4] - c[5]
            v1 = min_len[0] is not None and len(s1) < min_len[0]
            v2 = min_len[1] is not None and len(s2) < min_len[1]
            if v1 or v2:
                self.dropped["both" if v1 and v2 else "mate1_only" if v1 else "mate2_only"] += 1
                continue
            if dedup:
                if key in seen:
                    self.duplicates += 1
                    continue
                seen.add(key)
            self.pairs_out += 1
            m = M.loop_merge(s1, q1, s2, q2, ins) if merge and ins >= 0 else None
            if m is not None:
                out[2].append(b"@" + h1 + b"\n" + m[0] + b"\n+\n" + m[1] + b"\n")
                self.pairs_merged += 1
                continue
            out[0].append(b"@" + h1 + b"\n" + s1 + b"\n+\n" + q1 + b"\n")
            out[1].append(b"@" + h2 + b"\n" + s2 + b"\n+\n" + q2 + b"\n")
        self.text = [b"".join(x) for x in out]

    def result(self):
        return (self.pairs_in, self.pairs_out, self.removed, len(self.text[0]), len(self.text[1]), self.dropped)

    def check_report(self, rep):
        assert (rep.pairs_checked, rep.pairs_corrected, rep.bases_corrected[0], rep.bases_corrected[1], rep.mismatches) == tuple(self.counts)
        assert np.asarray(rep.matrix).reshape(-1).tolist() == self.matrix

    def shows_something(self):
        """corrections in mate 1 AND in mate 2, and mismatches that stay (qualities between the thresholds)"""
        return self.counts[2] > 0 and self.counts[3] > 0 and self.uncorrected > 0 and self.counts[0] > self.counts[1] > 0


def run(F, data1, data2, entrypos, fbufsize, rules=X.DEFAULT, merge=False, correct=True, **kw):
    """filter_fastq_paired over two byte strings -> (result, out1, out2, merged, CorrectionReport, OverlapReport, FilterReports)"""
    o1, o2, om = io.BytesIO(), io.BytesIO(), io.BytesIO()
    crep = F.CorrectionReport() if correct else None
    orep = F.OverlapReport()
    reps = (F.FilterReport(), F.FilterReport())
    res = F.filter_fastq_paired(io.BytesIO(data1), io.BytesIO(data2), o1, o2, fbufsize=fbufsize, entrypos=entrypos,
                                overlap=F.OverlapRules(*rules), overlap_report=orep, merged_out=om if merge else None,
                                correction=F.CorrectionRules(GOOD, BAD) if correct else None, correction_report=crep,
                                report=reps[0], report2=reps[1], **kw)
    return res, o1.getvalue(), o2.getvalue(), om.getvalue(), crep, orep, reps

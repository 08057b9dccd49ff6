"""What the dedup tests share (tests/test_dedup.py, test_dedup_iter.py, test_dedup_host.py): the rule of include/ffq.h
(ffq_table_seq_keys, ffq_dedup_select) as plain loops over bytes and a Python dict -- never the package's own seq_key --, inputs
drawn from a small pool of reads, and the expectation of filter_fastq(dedup=...) / filter_fastq_paired(dedup=...) on them.  The
trims, the content rules, the overlap and the merge are the loops of pairs_expect / overlap_expect / merge_expect.  Computed once
per set of parameters and left unchanged."""
import functools
import io

import numpy as np

import merge_expect as M
import overlap_expect as O
import pairs_expect as P

M64 = (1 << 64) - 1
KEY_NONE = 0
MIN_SLOTS = 1024


# ---- the rule --------------------------------------------------------------------------------------------------------
def sm(z):
    z ^= z >> 30
    z = (z * 0xbf58476d1ce4e5b9) & M64
    z ^= z >> 27
    z = (z * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


@functools.lru_cache(maxsize=8192)
def loop_key(seq):
    """(remembered per byte string: the tests ask for the same read's key at many addresses)"""
    n = len(seq)
    total = 0
    for k in range((n + 3) // 4):
        w = 0
        for j in range(4):
            i = 4 * k + j
            b = seq[i] if i < n else 0
            w |= b << (8 * j)
        total = (total + sm(((k + 1) << 32) | w)) & M64
    key = sm((total + n * 0x9e3779b97f4a7c15) & M64)
    return key if key else 1


def loop_pair_key(k1, k2):
    if k1 == KEY_NONE or k2 == KEY_NONE:
        return KEY_NONE
    k = sm((sm(k1) + k2) & M64)
    return k if k else 1


def row_keyed(seen, row, sentinel):
    """is the row keyed?  seen: the buffer as the scanner saw it (with its sentinel byte, if any); row: six coordinates of it"""
    p2, p3, p4, p5 = row[2:]
    if min(p2, p3, p4, p5) < 0 or not (p2 <= p3 <= len(seen)) or not (p4 <= p5 <= len(seen)) or p3 - p2 != p5 - p4:
        return False
    if sentinel and p3 > p2 and p2 < 1:
        return False
    for i in range(p2, p3):
        if seen[i] == 10:
            return False
    return True


def row_key(seen, row, sentinel):
    return loop_key(seen[row[2]:row[3]]) if row_keyed(seen, row, sentinel) else KEY_NONE


def slots_for(slots, distinct, n):
    """the growth rule"""
    need = 2 * (distinct + n)
    if slots >= MIN_SLOTS and need <= slots:
        return slots
    s = max(slots, MIN_SLOTS)
    while s < need:
        s *= 2
    return s


class LoopSet:
    """the set as a dict: key -> global ordinal of its first copy"""

    def __init__(self, expected=0):
        self.first = {}
        self.submitted = 0
        self.slots = slots_for(0, expected, 0)
        self.rehashes = 0

    def select(self, keys, drop=True):
        """keys of the rows of one call, in order -> (positions in the call of the kept rows, the six counts)"""
        n = len(keys)
        want = slots_for(self.slots, len(self.first), n)
        if want != self.slots and n:
            self.slots = want
            self.rehashes += 1
        kept, dups, nokey = [], 0, 0
        for i, k in enumerate(keys):
            g = self.submitted + i
            if k == KEY_NONE:
                nokey += 1
                kept.append(i)
            elif k in self.first:
                dups += 1
            else:
                self.first[k] = g
                kept.append(i)
        self.submitted += n
        counts = [len(kept), dups, nokey, len(self.first), self.slots, self.rehashes]
        return (kept if drop else list(range(n))), counts


# ---- a file of reads drawn from a pool ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def records(n=3000, pool=900, seed=5, empties=False):
    """(header, sequence, quality) x n: the sequence is one of `pool` distinct reads of 40..150 bases -- a tenth of them with
    an adapter inside, a few with Ns --, header and quality are the copy's own: a third of the copies have a bad 3' end of their
    own length, so that a quality trim cuts the copies of one read differently.  Some records are wrapped (a newline in both
    lines: no key); empties: some reads have no bases (the Python scanner reads those record for record, the device scanners do
    not: include/ffq.h at ffq_table_render_fastq)."""
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(pool):
        m = int(rng.integers(40, 151))
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, m)].copy()
        kind = int(rng.integers(0, 20))
        if kind < 2:
            p = int(rng.integers(m // 2, m - 2))
            ins = np.frombuffer(P.ADAPTER1, dtype=np.uint8)[:m - p]
            s[p:p + len(ins)] = ins
        elif kind < 4:
            s[rng.integers(0, m, 3)] = ord("N")
        reads.append(s.tobytes())
    assert len(set(reads)) == pool
    out = []
    for i in range(n):
        s = reads[int(rng.integers(0, pool))]
        m = len(s)
        v = rng.integers(25, 41, m)
        kind = int(rng.integers(0, 30))
        if kind < 10:
            t = int(rng.integers(3, 35))
            v[m - t:] = rng.integers(2, 9, t)
        elif kind < 12:
            v[:] = rng.integers(8, 14, m)              # a low mean: the content rules drop this copy
        q = bytes((v + 33).astype(np.uint8))
        if kind == 13:                                  # wrapped: both lines broken at the same place
            w = int(rng.integers(10, m - 10))
            q = q.replace(b"@", b"A")
            s, q = s[:w] + b"\n" + s[w:], q[:w] + b"\n" + q[w:]
        if empties and kind == 14:
            s = q = b""
        out.append((b"DUP:%d:%d len=%d" % (seed, i, m), s, q))
    return tuple(out)


TRIM = dict(quality_cutoff=(5, 15), adapter=P.ADAPTER1, err_permille=100, min_overlap=3, min_len=30)
CONTENT = dict(max_n=2, min_mean_quality=15, qualified_quality=15, max_unqualified_percent=None, max_expected_errors=None, min_complexity=None)


def key_of_record(s):
    """a record as the scanner cuts it: the sequence slice of a wrapped record holds its newline -- no key"""
    return KEY_NONE if 10 in s else loop_key(s)


def keys_tell_sequences_apart(recs):
    """in this input, equal key <=> equal sequence (among the keyed records)"""
    by_key = {}
    for _h, s, _q in recs:
        if 10 not in s:
            by_key.setdefault(loop_key(s), set()).add(s)
    return all(len(v) == 1 for v in by_key.values())


class Expected:
    """what filter_fastq(dedup=DedupRules(count_only=...)) leaves behind, with (TRIM, CONTENT) or without any rule"""

    def __init__(self, recs, rules=False, drop=True):
        self.records_in = len(recs)
        self.removed = 0
        out = []
        seen = {}
        self.keyed = self.unkeyed = self.duplicates = 0
        self.first_copy_filtered = 0          # reads whose first copy the filters dropped and whose later copy was written
        lost = set()
        for h, s, q in recs:
            key = key_of_record(s)
            s2, q2 = s, q
            v = 0
            if rules:
                if 10 not in s:
                    a, z = P.quality_span(q, *TRIM["quality_cutoff"])
                    s2, q2 = s[a:z], q[a:z]
                    cut = P.adapter_cut(s2, TRIM["adapter"], TRIM["err_permille"], TRIM["min_overlap"])
                    s2, q2 = s2[:cut], q2[:cut]
                    self.removed += len(s) - len(s2)
                v = 1 if len(s2) < TRIM["min_len"] else (P.content_verdict(s2, q2, CONTENT) if 10 not in s else 0)
            if v:
                if key != KEY_NONE and key not in seen:
                    lost.add(key)
                continue
            if key == KEY_NONE:
                self.unkeyed += 1
            else:
                self.keyed += 1
                if key in seen:
                    self.duplicates += 1
                    if drop:
                        continue
                else:
                    seen[key] = True
                    if key in lost:
                        self.first_copy_filtered += 1
            out.append(b"@" + h + b"\n" + s2 + b"\n+\n" + q2 + b"\n")
        self.distinct = len(seen)
        self.records_out = len(out)
        self.text = b"".join(out)

    def result(self):
        return (self.records_in, self.records_out, self.removed, len(self.text))

    def check_report(self, rep):
        assert (rep.keyed, rep.unkeyed, rep.distinct, rep.duplicates) == (self.keyed, self.unkeyed, self.distinct, self.duplicates)
        assert rep.duplication_rate == (self.duplicates / self.keyed if self.keyed else 0.0)


def run(F, data, entrypos, fbufsize, rules=False, dedup=True, count_only=False, opened=None):
    """filter_fastq over a byte string -> (result, output, DedupReport or None)"""
    out = io.BytesIO()
    rep = F.DedupReport() if dedup else None
    kw = dict(TRIM, content=F.ContentRules(**CONTENT)) if rules else {}
    fh = opened if opened is not None else io.BytesIO(data)
    res = F.filter_fastq(fh, out, fbufsize, entrypos=entrypos, dedup=F.DedupRules(count_only=count_only) if dedup else None,
                         dedup_report=rep, **kw)
    return res, out.getvalue(), rep


# ---- pairs -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_records(n=1500, pool=500, seed=7):
    """pairs drawn from the first `pool` pairs of merge_expect.records (fragments short, middling and long, a few wrapped): the
    sequences are the pool pair's, headers and mate 1's quality the copy's own; a fifth of the copies have a mate 1 whose
    quality is low throughout, which the content rule of the pair runs drops -- sometimes the FIRST copy of its pair"""
    rng = np.random.default_rng(seed)
    p1, p2 = M.records(pool, 11)
    m1, m2 = [], []
    for i in range(n):
        j = int(rng.integers(0, pool))
        (_h1, s1, q1), (_h2, s2, q2) = p1[j], p2[j]
        if 10 not in s1:
            v = rng.integers(25, 41, len(s1))
            if int(rng.integers(0, 5)) == 0:
                v[:] = rng.integers(3, 9, len(s1))
            q1 = bytes((v + 33).astype(np.uint8))
        name = b"PDUP:%d:%d" % (seed, i)
        m1.append((name + b"/1", s1, q1))
        m2.append((name + b" 2:N:0:" + b"ACGT" * int(rng.integers(1, 9)), s2, q2))
    return tuple(m1), tuple(m2)


PAIR_CONTENT = dict(max_n=None, min_mean_quality=12, qualified_quality=15, max_unqualified_percent=None, max_expected_errors=None,
                    min_complexity=None)
PAIR_MIN_LEN = 40


class ExpectedPairs:
    """what filter_fastq_paired(overlap=DEFAULT, merged_out=..., min_len=PAIR_MIN_LEN, content=PAIR_CONTENT, dedup=...) leaves
    behind: keys as scanned, overlap (with its cut), the filter (pair_filter "any"), dedup, merge"""

    def __init__(self, recs1, recs2, drop=True, dedup=True):
        out = [[], [], []]
        self.pairs_in = len(recs1)
        self.removed = self.pairs_out = self.pairs_merged = 0
        self.dropped = {"mate1_only": 0, "mate2_only": 0, "both": 0}
        self.keyed = self.unkeyed = self.duplicates = 0
        self.first_copy_filtered = 0
        seen, lost = {}, set()
        for (h1, s1, q1), (h2, s2, q2) in zip(recs1, recs2):
            key = loop_pair_key(key_of_record(s1), key_of_record(s2))
            ins = -2
            if 10 not in s1 and 10 not in s2:
                o = O.loop_overlap(s1, s2, *O.DEFAULT)
                ins = -1 if o is None else len(s2) + o
                if o is not None and o < 0:
                    c1, c2 = min(len(s1), ins), min(len(s2), ins)
                    self.removed += len(s1) - c1 + len(s2) - c2
                    s1, q1, s2, q2 = s1[:c1], q1[:c1], s2[:c2], q2[:c2]
            v = []
            for s, q in ((s1, q1), (s2, q2)):
                v.append(1 if len(s) < PAIR_MIN_LEN else (P.content_verdict(s, q, PAIR_CONTENT) if 10 not in s else 0))
            if v[0] or v[1]:
                self.dropped["both" if v[0] and v[1] else "mate1_only" if v[0] else "mate2_only"] += 1
                if key != KEY_NONE and key not in seen:
                    lost.add(key)
                continue
            if dedup:
                if key == KEY_NONE:
                    self.unkeyed += 1
                else:
                    self.keyed += 1
                    if key in seen:
                        self.duplicates += 1
                        if drop:
                            continue
                    else:
                        seen[key] = True
                        if key in lost:
                            self.first_copy_filtered += 1
            self.pairs_out += 1
            m = M.loop_merge(s1, q1, s2, q2, ins) if ins >= 0 else None
            if m is not None:
                out[2].append(b"@" + h1 + b"\n" + m[0] + b"\n+\n" + m[1] + b"\n")
                self.pairs_merged += 1
                continue
            out[0].append(b"@" + h1 + b"\n" + s1 + b"\n+\n" + q1 + b"\n")
            out[1].append(b"@" + h2 + b"\n" + s2 + b"\n+\n" + q2 + b"\n")
        self.distinct = len(seen)
        self.text = [b"".join(x) for x in out]

    def result(self):
        return (self.pairs_in, self.pairs_out, self.removed, len(self.text[0]), len(self.text[1]), self.dropped)

    check_report = Expected.check_report


def run_pairs(F, data1, data2, entrypos, fbufsize, dedup=True, count_only=False):
    """filter_fastq_paired over two byte strings -> (result, out1, out2, merged, DedupReport or None)"""
    o1, o2, om = io.BytesIO(), io.BytesIO(), io.BytesIO()
    rep = F.DedupReport() if dedup else None
    res = F.filter_fastq_paired(io.BytesIO(data1), io.BytesIO(data2), o1, o2, fbufsize=fbufsize, entrypos=entrypos,
                                overlap=F.OverlapRules(*O.DEFAULT), merged_out=om, min_len=PAIR_MIN_LEN,
                                content=F.ContentRules(**PAIR_CONTENT), dedup=F.DedupRules(count_only=count_only) if dedup else None,
                                dedup_report=rep)
    return res, o1.getvalue(), o2.getvalue(), om.getvalue(), rep

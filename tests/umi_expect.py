"""What the UMI tests share (tests/test_umi.py, test_umi_host.py, test_umi_iter.py): the rule of ffq_table_take_umi and
ffq_table_render_fastq_umi (include/ffq.h) as plain loops over bytes -- never the package's own umi_take / umi_name --, the hand
cases of the issue, a seeded table, and the expectation of filter_fastq / filter_fastq_paired with `umi=`.  No package code in
here.  Coordinates: a row minus `add` indexes the buffer the scanner saw; with a sentinel that buffer is b'\\n' + bytes, and its
byte 0 is never read.  Computed once per set of parameters and left unchanged."""
import collections
import functools

import numpy as np

READ1, READ2, PER_READ = 1, 2, 3
LOCS = {"read1": READ1, "read2": READ2, "per_read": PER_READ}
TAKE_LONG = 4096              # bases above which the take gives a row a wave of its own (csrc/ffq_umi.h)
RENDER_LONG = 4096            # output bytes above which the render does (csrc/ffq_render.h)

Rules = collections.namedtuple("Rules", "loc length skip prefix delim", defaults=("read1", 8, 0, b"", b":"))


# ---- the rule: one read ------------------------------------------------------------------------------------------------
def loop_take(seq, qual, length, skip):
    """(tag or None, sequence, quality) of an ELIGIBLE read"""
    n = len(seq)
    if n < length:
        return None, seq, qual
    cut = min(length + skip, n)
    return seq[:length], seq[cut:], qual[cut:]


def loop_name(header, tags, rules):
    """the header with the insert in front of its first blank; tags: the one tag, or the two of per_read"""
    k = len(header)
    for i, b in enumerate(header):
        if b in b" \t":
            k = i
            break
    ins = rules.delim + (rules.prefix + b"_" if rules.prefix else b"") + b"_".join(tags)
    return header[:k] + ins + header[k:]


# ---- the rule: rows ----------------------------------------------------------------------------------------------------
def eligible(seen, row, add=0, sentinel=False):
    p1, p2, p3, p4, p5 = (int(x) - add for x in row[1:])
    ok = min(p2, p3, p4, p5) >= 0 and p2 <= p3 <= len(seen) and p4 <= p5 <= len(seen) and p3 - p2 == p5 - p4
    if ok and sentinel and p3 > p2 and (p2 == 0 or p4 == 0):
        ok = False                           # (a line with the virtual newline in it is not inside the buffer)
    return bool(ok and 10 not in seen[p2:p3] and 10 not in seen[p4:p5] and p2 == p1 + 1)


def loop_take_rows(seen, rows, length, skip, add=0, sentinel=False):
    """(new rows, [changed, bases removed, skipped]) for rows (- add) over `seen`"""
    out, stats = [], [0, 0, 0]
    for row in rows:
        row = [int(x) for x in row]
        if not eligible(seen, row, add, sentinel):
            stats[2] += 1
            out.append(row)
            continue
        n = row[3] - row[2]
        cut = min(length + skip, n) if n >= length else 0
        if cut:
            stats[0] += 1
            stats[1] += cut
        out.append([row[0], row[1], row[2] + cut, row[3], row[4] + cut, row[5]])
    return np.array(out, dtype=np.int64).reshape(-1, 6), stats


def carried(seen, row, length, add=0):
    """the tag a source row carries, or None"""
    p1, p2 = int(row[1]) - add, int(row[2]) - add
    if p1 < 0 or p2 < 0 or p1 + 1 + length > p2 or p1 + 1 + length > len(seen):
        return None
    tag = seen[p1 + 1:p1 + 1 + length]
    return None if 10 in tag else tag


def slices(seen, row, add=0, sentinel=False):
    """(header, sequence, quality) of a renderable row, or None (ffq_table_render_fastq's rule)"""
    p0, p1, p2, p3, p4, p5 = (int(x) - add for x in row)
    ok = min(p0, p1, p2, p3, p4, p5) >= 0 and p0 + 1 <= p1 and p2 <= p3 and p4 <= p5 and max(p1, p3, p5) <= len(seen)
    if ok and sentinel and ((p2 == 0 and p3 > 0) or (p4 == 0 and p5 > 0)):
        ok = False
    return (seen[p0 + 1:p1], seen[p2:p3], seen[p4:p5]) if ok else None


Side = collections.namedtuple("Side", "seen rows add sentinel", defaults=(0, False))


def loop_render(side, rules, src1=None, src2=None):
    """(text, offsets [n + 1], [bytes, rows rendered, rows skipped, rows tagged]) of side.rows rendered with the tags their
    source rows carry; rules None: the plain render"""
    out, off, stats = [], [0], [0, 0, 0, 0]
    loc = LOCS[rules.loc] if rules is not None else 0
    for i, row in enumerate(side.rows):
        cut = slices(side.seen, row, side.add, side.sentinel)
        if cut is None:
            out.append(b"")
            stats[2] += 1
        else:
            h, s, q = cut
            tags = []
            if loc in (READ1, PER_READ):
                tags.append(carried(src1.seen, src1.rows[i], rules.length, src1.add))
            if loc in (READ2, PER_READ):
                tags.append(carried(src2.seen, src2.rows[i], rules.length, src2.add))
            if tags and None not in tags:
                h = loop_name(h, tags, rules)
                stats[3] += 1
            out.append(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n")
            stats[1] += 1
        off.append(off[-1] + len(out[-1]))
    stats[0] = off[-1]
    return b"".join(out), off, stats


# ---- the issue's hand cases ------------------------------------------------------------------------------------------------
# (sequence, len, skip) -> (tag, what is left); the quality is cut alike
HAND_TAKE = [
    (b"ACGTACG", 8, 3, None, b"ACGTACG"),                     # len - 1: shorter than the tag, unchanged
    (b"ACGTACGT", 8, 3, b"ACGTACGT", b""),                    # len: the tag is all there is
    (b"ACGTACGTTT", 8, 3, b"ACGTACGT", b""),                  # len + skip - 1: the skip is cut short
    (b"ACGTACGTTTT", 8, 3, b"ACGTACGT", b""),                 # len + skip
    (b"ACGTACGTTTTC", 8, 3, b"ACGTACGT", b"C"),
    (b"", 8, 3, None, b""),                                   # 0
    (b"ACGTACGTTTTC", 8, 0, b"ACGTACGT", b"TTTC"),
    (b"N", 1, 0, b"N", b""),
    (b"A" * 64 + b"C" * 64 + b"G", 64, 64, b"A" * 64, b"G"),
]

P16 = b"Abcdefgh01234567"
# (header, tags, prefix, delim) -> name
HAND_NAME = [
    (b"read1", (b"ACGT",), b"", b":", b"read1:ACGT"),                              # no blank
    (b"r\t1 x", (b"ACGT",), b"", b":", b"r:ACGT\t1 x"),                            # a tab in front of a space
    (b" lead", (b"ACGT",), b"", b":", b":ACGT lead"),                              # the blank first: k = 0
    (b"r", (b"A",), b"", b":", b"r:A"),                                            # one byte
    (b" ", (b"A",), b"", b"_", b"_A "),
    (b"r 1:N:0", (b"ACGTACGT",), b"UMI", b":", b"r:UMI_ACGTACGT 1:N:0"),
    (b"r 1:N:0", (b"ACGT",), P16, b"#", b"r#" + P16 + b"_ACGT 1:N:0"),             # a prefix of 16
    (b"r/1", (b"AAAA", b"CCCC"), b"", b":", b"r/1:AAAA_CCCC"),                     # per_read
    (b"r/1 z", (b"AAAA", b"CCCC"), b"U", b":", b"r/1:U_AAAA_CCCC z"),
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
    """One buffer with a record per hand case of the take, then the rows that are not eligible.  Returns (bytes, rows, number
    of ineligible rows): rows index the bytes (no sentinel, add 0)."""
    buf, rows = bytearray(b"##"), []
    for i, (seq, *_rest) in enumerate(HAND_TAKE):
        rows.append(record(buf, b"h%d x" % i, seq, bytes(33 + (j % 40) for j in range(len(seq)))))
    first_bad = len(rows)
    p0 = len(buf)
    buf += b"@w\nACGTACGTACGT\nACGTAC\n+\n"
    p4 = len(buf)
    buf += b"IIIIIIIIIIII\nIIIIII\n"
    rows.append([p0, p0 + 2, p0 + 3, p0 + 22, p4, p4 + 19])                # a wrapped record
    r = record(buf, b"fa", b"ACGTACGTACGTACGT")
    rows.append(r[:4] + [-1, -1])                                          # a FASTA row
    r = record(buf, b"q", b"ACGTACGTACGTACGT", b"IIIIIIII\nIIIIIII")
    rows.append(r)                                                         # a newline in the quality only
    r = record(buf, b"moved", b"ACGTACGTACGTACGT")
    rows.append([r[0], r[1], r[2] + 2, r[3], r[4] + 2, r[5]])              # pos2 != pos1 + 1: an earlier pass cut the front
    rows.append([r[0], r[1], r[2], r[3], r[4], r[5] - 1])                  # unequal lengths
    rows.append([r[0], r[1], r[2], r[3], len(buf) - 3, len(buf) + 13])     # past the buffer
    return bytes(buf), rows, len(rows) - first_bad


def body_of(rng, n):
    return np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, n)].tobytes()


@functools.lru_cache(maxsize=None)
def seeded_table(n_rows=4000, seed=11):
    """(bytes, rows): read lengths 0..220 with the short ones (0..70) as likely as the rest, one row in fifty not eligible (a wrapped
    record, a FASTA row, a newline in the quality, a front that is cut already), headers with and without blanks"""
    rng = np.random.default_rng(seed)
    buf, rows = bytearray(b"#"), []
    for i in range(n_rows):
        n = int(rng.integers(0, 71)) if rng.integers(0, 2) else int(rng.integers(0, 221))
        seq = body_of(rng, n)
        qual = (rng.integers(33, 74, n, dtype=np.uint8)).tobytes()
        h = (b"S%d" % i) + (b"", b" 1:N:0", b"\tx y")[i % 3]
        if i % 50 == 7 and n >= 4:
            kind = (i // 50) % 4
            if kind == 0:
                p0 = len(buf)
                buf += b"@" + h + b"\n" + seq[:n // 2] + b"\n" + seq[n // 2:] + b"\n+\n"
                p4 = len(buf)
                buf += qual[:n // 2] + b"\n" + qual[n // 2:] + b"\n"
                rows.append([p0, p0 + 1 + len(h), p0 + 2 + len(h), p0 + 3 + len(h) + n, p4, p4 + n + 1])
            elif kind == 1:
                rows.append(record(buf, h, seq, qual)[:4] + [-1, -1])
            elif kind == 2:
                rows.append(record(buf, h, seq, qual[:1] + b"\n" + qual[2:]))
            else:
                r = record(buf, h, seq, qual)
                rows.append([r[0], r[1], r[2] + 1, r[3], r[4] + 1, r[5]])
        else:
            rows.append(record(buf, h, seq, qual))
    return bytes(buf), tuple(tuple(r) for r in rows)


@functools.lru_cache(maxsize=None)
def seeded_want(length, skip):
    buf, rows = seeded_table()
    return loop_take_rows(buf, rows, length, skip)


# ---- files ---------------------------------------------------------------------------------------------------------------
def fastq_text(recs):
    return b"".join(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n" for h, s, q in recs)


@functools.lru_cache(maxsize=None)
def single_records(n=400, seed=5, wrapped=True):
    """mixed reads: lengths 0..150 -- some shorter than a UMI of 8 --, headers with a space, a tab or no blank, a few wrapped
    records (never touched by the take)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        m = int(rng.integers(1, 12)) if rng.integers(0, 6) == 0 else int(rng.integers(12, 151))
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, m)].tobytes()
        q = (rng.integers(35, 74, m, dtype=np.uint8)).tobytes()
        h = (b"U%d:%d" % (seed, i)) + (b" 1:N:0:ACGT", b"", b"\tleft right")[i % 3]
        if wrapped and i % 41 == 5 and m >= 30:
            s, q = s[:20] + b"\n" + s[20:], q[:20] + b"\n" + q[20:]
        out.append((h, s, q))
    return tuple(out)


def take_record(s, q, rules):
    """(tag or None, s, q, took): one record of a file through the take (a wrapped record is not eligible)"""
    if 10 in s or 10 in q or len(s) != len(q):
        return None, s, q
    return loop_take(s, q, rules.length, rules.skip)


class ExpectedSingle:
    """what filter_fastq(umi=rules, ends=EndRules(trim_front=front), quality_cutoff, adapter, min_len, dedup) leaves behind: the
    take in front of every trim, the chain's order behind it, the names of the records that are written"""

    def __init__(self, recs, rules, front=0, quality_cutoff=None, adapter=None, min_len=None, dedup=False):
        import pairs_expect as P
        self.taken = self.removed = self.skipped = self.tagged = self.n_out = self.umi_bases = 0
        out, seen = [], set()
        for h, s, q in recs:
            n0 = len(s)
            wrapped = 10 in s or 10 in q
            tag = None
            if wrapped:
                self.skipped += 1
            else:
                tag, s2, q2 = loop_take(s, q, rules.length, rules.skip)
                self.taken += tag is not None
                self.umi_bases += len(s) - len(s2)
                s2, q2 = s2[front:], q2[front:]
                if quality_cutoff is not None:
                    a, z = P.quality_span(q2, quality_cutoff[0], quality_cutoff[1])
                    s2, q2 = s2[a:z], q2[a:z]
                if adapter is not None:
                    c = P.adapter_cut(s2, adapter, 100, 3)
                    s2, q2 = s2[:c], q2[:c]
            if wrapped:
                s2, q2 = s, q
                n0 = len(s2)
            self.removed += n0 - len(s2)
            if min_len is not None and len(s2) < min_len:
                continue
            if dedup and not wrapped:
                if s in seen:
                    continue
                seen.add(s)
            self.n_out += 1
            self.tagged += tag is not None
            out.append(b"@" + (loop_name(h, (tag,), rules) if tag is not None else h) + b"\n" + s2 + b"\n+\n" + q2 + b"\n")
        self.text = b"".join(out)
        self.n_in = len(recs)

    def result(self):
        return (self.n_in, self.n_out, self.removed, len(self.text))


@functools.lru_cache(maxsize=None)
def pair_records(n=300, seed=8):
    """mates with the same names: (records of file 1, of file 2); either mate is now and then shorter than a UMI of 8"""
    r1, r2 = single_records(n, seed, wrapped=False), single_records(n, seed + 100, wrapped=False)
    return r1, tuple((h1, s, q) for (h1, _s, _q), (_h, s, q) in zip(r1, r2))


class ExpectedPaired:
    """what filter_fastq_paired(umi=rules, min_len) leaves behind (pair_filter "any"): the take on the mates the location names,
    the SAME insert in both names"""

    def __init__(self, recs1, recs2, rules, min_len=None):
        loc = LOCS[rules.loc]
        self.removed = self.pairs_out = self.tagged = 0
        out = ([], [])
        for a, b in zip(recs1, recs2):
            cut, tags = [], []
            for k, (h, s, q) in enumerate((a, b)):
                tag = None
                if loc == PER_READ or loc == k + 1:
                    tag, s, q = take_record(s, q, rules)
                    tags.append(tag)
                cut.append((h, s, q))
            self.removed += len(a[1]) - len(cut[0][1]) + len(b[1]) - len(cut[1][1])
            if min_len is not None and min(len(cut[0][1]), len(cut[1][1])) < min_len:
                continue
            self.pairs_out += 1
            for k, (h, s, q) in enumerate(cut):
                if None not in tags:
                    h = loop_name(h, tuple(tags), rules)
                    self.tagged += 1
                out[k].append(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n")
        self.text = (b"".join(out[0]), b"".join(out[1]))
        self.pairs_in = len(recs1)

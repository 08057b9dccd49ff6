"""What the ends tests share (tests/test_ends.py, test_ends_plan.py, test_ends_device.py, test_ends_stream.py): the rule of
ffq_table_trim_ends (include/ffq.h) as a plain loop over bytes -- never the package's own ends_cut --, the hand values of the
issue, a seeded table of six read profiles, tables whose decisive window lies on the chunk edges, long rows, the pool of the
grid tests, generated files, and the expectation of filter_fastq / filter_fastq_paired on them: the loop first, then what
tests/poly_expect.py expects of the trims behind it.  Computed once per set of parameters and left unchanged.  No package code
in here."""
import collections
import functools

import numpy as np

import pairs_expect as P
import poly_expect as PE

LONG = 4096                                     # quality bytes above which the library gives a row a wave of its own (csrc/ffq_ends.h)

# the rules: counts (keep_len 0: no limit) and three windows, each None or (window, quality)
Rules = collections.namedtuple("Rules", "trim_front trim_tail keep_len front right tail", defaults=(0, 0, 0, None, None, None))


# ---- the rule --------------------------------------------------------------------------------------------------------
def window_sums(v, a, b, W):
    """S(i, W) for i = a .. b - W, by a running sum"""
    if b - a < W:
        return []
    s = sum(v[a:a + W])
    out = [s]
    for i in range(a + 1, b - W + 1):
        s += v[i + W - 1] - v[i - 1]
        out.append(s)
    return out


def loop_cut(q, r, qual_base=33):
    """(a, b) of the quality line q (bytes) under the rules r"""
    n = len(q)
    v = [x - qual_base for x in q]
    a = min(r.trim_front, n)
    b = n - min(r.trim_tail, n - a)
    if r.keep_len > 0 and b - a > r.keep_len:
        b = a + r.keep_len
    if r.front is not None and b > a:
        W = min(r.front[0], b - a)
        T = r.front[1] * W
        s = None
        for i, S in enumerate(window_sums(v, a, b, W)):
            if S >= T:
                s = a + i
                break
        if s is None:
            return (0, 0)
        a = s
        while v[a] < r.front[1]:
            a += 1
    if r.right is not None and b > a:
        W = min(r.right[0], b - a)
        T = r.right[1] * W
        s = None
        for i, S in enumerate(window_sums(v, a, b, W)):
            if S < T:
                s = a + i
                break
        if s is not None:
            b2 = s
            while b2 < s + W and v[b2] >= r.right[1]:
                b2 += 1
            b = b2
    if r.tail is not None and b > a:
        W = min(r.tail[0], b - a)
        T = r.tail[1] * W
        e = None
        for i, S in enumerate(window_sums(v, a, b, W)):
            if S >= T:
                e = a + i + W                           # (the last one that passes stays)
        if e is None:
            return (0, 0)
        b = e
        while v[b - 1] < r.tail[1]:
            b -= 1
    if a >= b:
        a = b = 0
    return (a, b)


def loop_rows(seen, rows, r, qual_base=33, add=0):
    """(new rows, [changed, bases removed, skipped], (n, a, b) of the eligible rows) for rows (+ add) over `seen` (bytes: the
    buffer as the scanner saw it, with its sentinel if it has one)"""
    out, stats, spans = [], [0, 0, 0], []
    for row in rows:
        row = [int(x) for x in row]
        p2, p3, p4, p5 = (x - add for x in row[2:])
        ok = min(p2, p3, p4, p5) >= 0 and p2 <= p3 <= len(seen) and p4 <= p5 <= len(seen) and p3 - p2 == p5 - p4
        if ok and 10 in seen[p4:p5]:
            ok = False
        if not ok:
            stats[2] += 1
            out.append(row)
            continue
        n = p5 - p4
        a, b = loop_cut(seen[p4:p5], r, qual_base)
        spans.append((n, a, b))
        if b - a != n:
            stats[0] += 1
            stats[1] += n - (b - a)
        out.append(row[:2] + [row[2] + a, row[2] + b, row[4] + a, row[4] + b])
    return np.array(out, dtype=np.int64).reshape(-1, 6), stats, spans


# ---- the issue's hand values ---------------------------------------------------------------------------------------------
# The issue writes a quality line with one character per base, `u` for Q30 and `2` for Q2 -- a notation, not the Phred+33
# characters, which are '?' and '#'.
def hand_line(text):
    return text.replace("u", "?").replace("2", "#").encode()


WQ = (4, 20)
FRONT, RIGHT, TAIL = Rules(front=WQ), Rules(right=WQ), Rules(tail=WQ)
ALL3 = Rules(front=WQ, right=WQ, tail=WQ)
HAND = [
    ("uuuuuuuu", ALL3, (0, 8)),
    ("22uuuuuu", FRONT, (2, 8)),
    ("2u2uuuuu", FRONT, (1, 8)),
    ("uuuuu2u222", RIGHT, (0, 5)),
    ("uuuuu2u222", TAIL, (0, 7)),
    ("uuuu2222uuuu", RIGHT, (0, 4)),
    ("uuuu2222uuuu", TAIL, (0, 12)),
    ("uuuuuu222", RIGHT, (0, 6)),
    ("2222", FRONT, (0, 0)),
    ("2222", RIGHT, (0, 0)),
    ("u2", FRONT, (0, 0)),
    ("u2", RIGHT, (0, 1)),
    ("u2", TAIL, (0, 0)),
    ("u22", TAIL, (0, 0)),
    ("uuuuuuuuuu", Rules(3, 2, 4), (3, 7)),
    ("uuu", Rules(5, 2), (0, 0)),
    ("2uuu2uuuu", Rules(trim_front=1, front=(1, 20), right=(1, 20)), (1, 4)),
    ("", Rules(trim_front=1, front=WQ), (0, 0)),
]

# the settings every table goes through: each window alone, all three, the widest window, the narrowest, fixed trims only
SETTINGS = collections.OrderedDict([
    ("front", FRONT), ("right", RIGHT), ("tail", TAIL), ("all three", ALL3),
    ("window 64", Rules(front=(64, 25), right=(64, 25), tail=(64, 25))),
    ("window 1", Rules(front=(1, 20), right=(1, 20), tail=(1, 20))),
    ("fixed", Rules(5, 3, 100)),
])


def pkg_rules(F, r):
    """r as the package's EndRules (F: its fastqandfurious module)"""
    return None if r is None else F.EndRules(r.trim_front, r.trim_tail, r.keep_len or None, r.front, r.right, r.tail)


def record(buf, header, qual, seq=None):
    """a four-line record appended to buf (a bytearray); its row"""
    p0 = len(buf)
    buf += b"@" + header + b"\n"
    p2 = len(buf)
    buf += (b"A" * len(qual) if seq is None else seq) + b"\n+\n"
    p4 = len(buf)
    buf += qual + b"\n"
    return [p0, p2 - 1, p2, p2 + len(qual), p4, p4 + len(qual)]


def ineligible(buf, rows, names):
    """the rows no rule applies to, appended"""
    p0 = len(buf)
    buf += b"@w\nACGT\nAC\n+\n"
    p4 = len(buf)
    buf += b"####\n##\n"
    rows.append([p0, p0 + 2, p0 + 3, p0 + 10, p4, p4 + 7]); names.append("a wrapped record, the lengths agree")
    p0 = len(buf)
    buf += b"@x\n" + b"A" * 23 + b"\n+\n"
    p4 = len(buf)
    buf += b"?" * 10 + b"\n" + b"#" * 12 + b"\n"
    rows.append([p0, p0 + 2, p0 + 3, p0 + 26, p4, p4 + 23]); names.append("a newline in the quality only")
    p0 = len(buf)
    buf += b"@u\n" + b"A" * 13 + b"\n+\n" + b"#" * 12 + b"\n"
    rows.append([p0, p0 + 2, p0 + 3, p0 + 16, p0 + 19, p0 + 31]); names.append("unequal lengths")
    rows.append([p0, p0 + 2, p0 + 3, p0 + 16, -1, -1]); names.append("a FASTA row")
    rows.append([p0, p0 + 2, p0 + 3, p0 + 16, 1 << 40, (1 << 40) + 13]); names.append("far outside the buffer")
    rows.append([p0, p0 + 2, p0 + 3, p0 + 16, len(buf) - 12, len(buf) + 1]); names.append("past the buffer")


def hand_table():
    """One buffer with a four-line record per hand line, then the ineligible rows.  Returns (bytes, rows, names of the
    ineligible rows): rows index the bytes (no sentinel, add 0)."""
    buf, rows, names = bytearray(b"##"), [], []
    for i, (text, _r, _want) in enumerate(HAND):
        rows.append(record(buf, b"h%d" % i, hand_line(text)))
    ineligible(buf, rows, names)
    return bytes(buf), rows, names


# ---- a seeded table of six read profiles -------------------------------------------------------------------------------------
PROFILES = ("flat", "decayed tail", "bad head", "all bad", "dips", "tiny")
WEIGHTS = (0.30, 0.17, 0.17, 0.15, 0.13, 0.08)


def profile_quality(rng, kind, n):
    """n quality values (Phred) of the profile"""
    v = rng.integers(30, 41, n)
    if kind == "decayed tail" and n > 0:
        k = int(rng.integers(1, n + 1))
        v[n - k:] = np.clip(np.linspace(36, 2, k) + rng.integers(-6, 7, k), 0, 41).astype(np.int64)
    elif kind == "bad head" and n > 0:
        k = min(n, int(rng.integers(1, 41)))
        v[:k] = rng.integers(2, 11, k)
    elif kind == "all bad":
        v = rng.integers(0, 16, n)
    elif kind == "dips":
        for _ in range(3):
            if n > 0:
                at, k = int(rng.integers(0, n)), int(rng.integers(1, 7))
                v[at:at + k] = 2
    return (v + 33).astype(np.uint8).tobytes()


def profile_line(rng):
    kind = PROFILES[int(rng.choice(len(PROFILES), p=WEIGHTS))]
    n = int(rng.integers(0, 4)) if kind == "tiny" else int(rng.integers(0, 221))
    return profile_quality(rng, kind, n)


@functools.lru_cache(maxsize=None)
def seeded_table(n_rows=4000, seed=11):
    """(bytes, rows): lengths 0..220 from the six profiles; runs of ineligible rows -- wrapped, FASTA -1, outside the buffer --
    at three places, 54 rows in all"""
    rng = np.random.default_rng(seed)
    buf, rows = bytearray(b"#"), []
    i = 0
    while len(rows) < n_rows:
        if len(rows) in (500, 1500, 2500):
            for _ in range(3):
                ineligible(buf, rows, [])
        rows.append(record(buf, b"r%d" % i, profile_line(rng)))
        i += 1
    return bytes(buf), tuple(tuple(r) for r in rows[:n_rows])


@functools.lru_cache(maxsize=None)
def seeded_want(setting):
    buf, rows = seeded_table()
    return loop_rows(buf, rows, SETTINGS[setting])


# ---- the decisive window on the chunk edges ----------------------------------------------------------------------------------
EDGE_OFFSETS = tuple(range(50, 81)) + tuple(range(118, 139))
EDGE_WINDOWS = (1, 4, 8, 9, 63, 64)
EDGE_LEN = 200


def edge_line(stage, pattern, o, W):
    """200 quality bytes of Q2 and Q40 whose cut by the stage alone lies at o: a step at o, or an island of W bytes next to
    it in a line that is otherwise all bad (front, tail) or all good (right)"""
    good, bad = 40 + 33, 2 + 33
    q = bytearray(EDGE_LEN)
    for i in range(EDGE_LEN):
        if stage == "front":
            ok = i >= o if pattern == "step" else o <= i < o + W
        elif stage == "right":
            ok = i < o if pattern == "step" else not o <= i < o + W
        else:
            ok = i < o if pattern == "step" else o - W <= i < o
        q[i] = good if ok else bad
    return bytes(q)


def edge_rules(stage, W):
    return Rules(**{stage: (W, 20)})


@functools.lru_cache(maxsize=None)
def edge_table(stage):
    """(bytes, rows, (o, W, pattern) per row) for one stage: every offset x every window x both patterns"""
    buf, rows, what = bytearray(b"#"), [], []
    for W in EDGE_WINDOWS:
        for pattern in ("step", "island"):
            for o in EDGE_OFFSETS:
                rows.append(record(buf, b"e", edge_line(stage, pattern, o, W)))
                what.append((o, W, pattern))
    return bytes(buf), tuple(tuple(r) for r in rows), tuple(what)


# ---- long rows -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_table(seed=5):
    """(bytes, rows, names): quality lines of 4096, 4097, 5000 and 20000 bytes among short ones; the decisive window of each
    stage straddles 1023 / 1024 and 2047 / 2048; one line all bad, one all good, one with a newline at byte 9000"""
    rng = np.random.default_rng(seed)
    buf, rows, names = bytearray(b"#"), [], []
    sbuf, srows = seeded_table()

    def some_short(k):
        for r in srows[k:k + 12]:
            rows.append(record(buf, b"s", sbuf[r[4]:r[5]]))
            names.append("short")

    def line(n, lo, hi, good=True):
        """n bytes, good (bad) but for [lo, hi)"""
        v = rng.integers(30, 41, n) if good else rng.integers(2, 9, n)
        v[lo:hi] = rng.integers(2, 9, hi - lo) if good else rng.integers(30, 41, hi - lo)
        return (v + 33).astype(np.uint8).tobytes()

    some_short(0)
    for n in (LONG, LONG + 1, 5000, 20000):
        for edge in (1024, 2048):
            rows.append(record(buf, b"l", line(n, 0, edge - 2)))            # front: the first good window straddles the edge
            names.append("front %d %d" % (n, edge))
            rows.append(record(buf, b"l", line(n, edge - 1, n)))            # right: the first bad window
            names.append("right %d %d" % (n, edge))
            rows.append(record(buf, b"l", line(n, n - edge - 2, n)))        # tail, counted from the back
            names.append("tail %d %d" % (n, edge))
            rows.append(record(buf, b"l", line(n, edge - 2, edge + 1, good=False)))     # three good bytes on the edge, all else bad
            names.append("island %d %d" % (n, edge))
        some_short(100 + n % 1000)
    rows.append(record(buf, b"bad", line(20000, 0, 0, good=False))); names.append("all bad")
    rows.append(record(buf, b"good", line(20000, 0, 0))); names.append("all good")
    nl = bytearray(line(20000, 10, 30))
    nl[9000] = 10
    rows.append(record(buf, b"nl", bytes(nl))); names.append("newline")
    some_short(2000)
    return bytes(buf), tuple(tuple(r) for r in rows), tuple(names)


# ---- the pool of the tables above one pass of the grid (tests/grid_expect.py) -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_pool():
    """(bytes, rows, idle, long): every row of the hand table but the last, 260 of the seeded table's eligible rows, empty and
    ineligible rows, a few long rows.  idle: the pool rows with nothing to do under any setting (empty or ineligible); long: those
    above LONG.  No sentinel, add 0."""
    hbuf, hrows, names = hand_table()
    assert names[-1] == "past the buffer"
    buf, rows = bytearray(hbuf), [list(r) for r in hrows[:-1]]
    idle = [i for i, (text, _r, _w) in enumerate(HAND) if text == ""] + list(range(len(HAND), len(rows)))
    sbuf, srows = seeded_table()
    for i, r in enumerate(srows[:260]):
        rows.append(record(buf, b"s%d" % i, sbuf[r[4]:r[5]]))
    for i in range(8):
        idle += [len(rows), len(rows) + 1]
        rows.append(record(buf, b"e%d" % i, b""))
        rows.append(record(buf, b"f%d" % i, b"#" * (12 + i))[:4] + [-1, -1])
    lbuf, lrows, lnames = long_table()
    long = []
    for r, name in zip(lrows, lnames):
        n = r[5] - r[4]
        if LONG <= n <= 5000 and name.split()[0] in ("front", "right", "island"):
            if n > LONG:
                long.append(len(rows))
            rows.append(record(buf, b"l", lbuf[r[4]:r[5]]))
    for i, q in enumerate((b"D" * 4200, b"D" * 4500, b"#" * 4300)):   # long rows that stay as they are, one that goes away
        long.append(len(rows))
        rows.append(record(buf, b"g%d" % i, q))
    idle.append(len(rows))
    rows.append([0, 1, 2, 15, len(buf) - 12, len(buf) + 1])        # past the buffer
    return bytes(buf), tuple(tuple(r) for r in rows), tuple(idle), tuple(long)


# ---- files ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def single_records(n=1500, seed=37):
    """(header, sequence, quality): the reads of tests/poly_expect.py -- adapters, G tails, bad 3' ends --, every second one with
    the quality of one of the six profiles; a few reads of two bases"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s, q = PE.one_read(rng, int(rng.integers(60, 151)), P.ADAPTER1)
        if rng.integers(0, 2):
            kind = PROFILES[int(rng.choice(len(PROFILES) - 1, p=np.array(WEIGHTS[:-1]) / sum(WEIGHTS[:-1])))]
            q = profile_quality(rng, kind, len(s))
        if i % 211 == 7:
            s, q = s[:2], q[:2]
        out.append((b"ENDS:%d:%d" % (seed, i), s, q))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pair_records(seed=17):
    """the mates of tests/poly_expect.py (fragments shorter than, as long as and longer than the reads, adapters, G tails, a few
    wrapped records), every third record that is not wrapped with the quality of one of the profiles"""
    rng = np.random.default_rng(seed)
    out = ([], [])
    for k, recs in enumerate(PE.pair_records()):
        for h, s, q in recs:
            if 10 not in q and rng.integers(0, 3) == 0:
                kind = PROFILES[int(rng.choice(len(PROFILES) - 1, p=np.array(WEIGHTS[:-1]) / sum(WEIGHTS[:-1])))]
                q = profile_quality(rng, kind, len(s))
            out[k].append((h, s, q))
    return tuple(out[0]), tuple(out[1])


def fastq(recs):
    return b"".join(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n" for h, s, q in recs)


def cut_records(recs, r, qual_base=33):
    """(the records as the ends step leaves them, reads cut, bases cut)"""
    out, reads, bases = [], 0, 0
    for h, s, q in recs:
        if r is not None and 10 not in q and len(s) == len(q):
            a, b = loop_cut(q, r, qual_base)
            reads += b - a != len(q)
            bases += len(q) - (b - a)
            s, q = s[a:b], q[a:b]
        out.append((h, s, q))
    return tuple(out), reads, bases


class ExpectedSingle:
    """what filter_fastq(ends, quality_cutoff, adapter, min_len, poly_g, poly_x) leaves behind: the loop, then
    poly_expect.ExpectedSingle on what it left"""

    def __init__(self, recs, r, quality_cutoff=None, adapter=None, min_len=None, poly_g=None, poly_x=None):
        cut, self.reads_cut, self.bases_cut = cut_records(recs, r)
        self.rest = PE.ExpectedSingle(cut, quality_cutoff, adapter, min_len, poly_g, poly_x)
        self.text = self.rest.text

    def result(self):
        n_in, n_out, removed, n_bytes = self.rest.result()
        return (n_in, n_out, removed + self.bases_cut, n_bytes)


class ExpectedPaired:
    """what filter_fastq_paired(ends=(r1, r2), ...) leaves behind: the loop per mate, then poly_expect.ExpectedPaired"""

    def __init__(self, recs1, recs2, rs, quality_cutoff=None, adapters=(None, None), min_len=None, rules=None, poly_g=None, poly_x=None):
        c1, n1, b1 = cut_records(recs1, rs[0])
        c2, n2, b2 = cut_records(recs2, rs[1])
        self.reads_cut, self.bases_cut = n1 + n2, b1 + b2
        kw = {} if rules is None else dict(rules=rules)
        self.rest = PE.ExpectedPaired(c1, c2, quality_cutoff, adapters, min_len, poly_g=poly_g, poly_x=poly_x, **kw)
        self.text = self.rest.text
        self.merged = self.rest.merged

    def result(self):
        r = self.rest.result()
        return r[:2] + (r[2] + self.bases_cut,) + r[3:]

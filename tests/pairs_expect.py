"""What tests/test_pairs_iter.py and tests/test_pairs_host.py share: two generated paired-end files and the expectation of
filter_fastq_paired on them as plain loops over the records' bytes -- the quality trim, the adapter cut, the content rules,
the pair rule and the id rule written out here, never the package's own Python statement of them.  Computed once per set of
parameters and left unchanged."""
import functools

import numpy as np

ADAPTER1, ADAPTER2 = b"AGATCGGAAGAGC", b"CTGTCTCTTATAC"
EE = [int(np.floor(1e6 * 10.0 ** (-v / 10.0) + 0.5)) for v in range(96)]
REASONS = ("length", "n", "mean_quality", "unqualified", "expected_errors", "complexity")
# the arguments of every run: cutadapt -q 5,10 -a ... -A ... -m 75:35 --max-n 1 (and fastp's -e, -u, -y; an expected-errors bound)
ARGS = dict(quality_cutoff=(5, 10), min_len=(75, 35), max_len=None, adapter=ADAPTER1, adapter2=ADAPTER2, err_permille=100, min_overlap=3)
CONTENT = dict(max_n=1, min_mean_quality=20, qualified_quality=15, max_unqualified_percent=30, max_expected_errors=0.8, min_complexity=30)


# ---- two files -------------------------------------------------------------------------------------------------------
def one_read(rng, n, adapter):
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
    v = rng.integers(30, 41, n)
    kind = rng.integers(0, 100)
    if kind < 4:                                   # Ns
        seq[rng.integers(0, n, rng.integers(2, 6))] = ord("N")
    elif kind < 8:                                 # low complexity
        seq[:] = ord("A")
        seq[rng.integers(0, n, 3)] = ord("C")
    elif kind < 12:                                # a low mean
        v = rng.integers(12, 19, n)
    elif kind < 16:                                # many unqualified bases, a good mean
        v[rng.random(n) < 0.4] = 12
    elif kind < 22:                                # expected errors around the bound
        v = rng.integers(20, 23, n)
    elif kind < 34:                                # a bad 3' end, sometimes a bad 5' end too
        t = int(rng.integers(5, min(41, n)))
        v[n - t:] = rng.integers(2, 9, t)
        if kind < 26:
            v[:3] = 2
    if rng.integers(0, 10) == 0 and n > 20:        # an adapter inside the read, or cut short by its end
        p = int(rng.integers(n // 2, n - 2))
        ins = np.frombuffer(adapter, dtype=np.uint8)[:n - p]
        seq[p:p + len(ins)] = ins
    return seq.tobytes(), bytes((v + 33).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def records(n_pairs=3000, seed=20, long_at=-1):
    """(records of mate 1, records of mate 2): lists of (header, sequence, quality); mate 1 has 80..150 bases, mate 2 30..150;
    long_at >= 0: that pair's mate 1 has 5000 bases"""
    rng = np.random.default_rng(seed)
    m1, m2 = [], []
    for i in range(n_pairs):
        name = b"SIM:%d:%d" % (seed, i)
        style = i % 4
        h1 = name + (b"/1", b" 1:N:0:ACGT", b"", b"\tfirst")[style]
        h2 = name + (b"/2", b" 2:N:0:ACGT", b"", b"/2 second")[style]
        n1 = 5000 if i == long_at else int(rng.integers(80, 151))
        m1.append((h1,) + one_read(rng, n1, ADAPTER1))
        m2.append((h2,) + one_read(rng, int(rng.integers(30, 151)), ADAPTER2))
    return tuple(m1), tuple(m2)


def fastq(recs):
    return b"".join(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n" for h, s, q in recs)


# ---- the rules as loops ----------------------------------------------------------------------------------------------
def trim_end(d):
    """bases the running-sum rule takes off the end `d` is walked from"""
    s = best = cut = 0
    for k, x in enumerate(d):
        s += x
        if s < 0:
            break
        if s > best:
            best, cut = s, k + 1
    return cut


def quality_span(q, front, back, base=33):
    n = len(q)
    start = trim_end([front - (b - base) for b in q])
    stop = n - trim_end([back - (b - base) for b in reversed(q)])
    return (start, stop) if start < stop else (0, 0)


def adapter_cut(seq, ad, err_permille, min_overlap):
    n, m = len(seq), len(ad)
    for p in range(0, n - min_overlap + 1):
        ov = min(m, n - p)
        allowed, mm = ov * err_permille // 1000, 0
        for j in range(ov):
            if ad[j] != 78 and seq[p + j] != ad[j]:
                mm += 1
                if mm > allowed:
                    break
        if mm <= allowed:
            return p
    return n


def content_verdict(seq, q, R, base=33):
    n = len(seq)
    if n == 0:
        return 0
    v = [min(max(b - base, 0), 95) for b in q]
    if R["max_n"] is not None and sum(1 for b in seq if b in b"Nn") > R["max_n"]:
        return 2
    if R["min_mean_quality"] is not None and sum(v) < R["min_mean_quality"] * n:
        return 3
    if R["max_unqualified_percent"] is not None and 100 * sum(1 for x in v if x < R["qualified_quality"]) > R["max_unqualified_percent"] * n:
        return 4
    if R["max_expected_errors"] is not None and sum(EE[x] for x in v) > int(round(R["max_expected_errors"] * 1e6)):
        return 5
    if R["min_complexity"] is not None and n >= 2 and 100 * sum(1 for i in range(n - 1) if seq[i] != seq[i + 1]) < R["min_complexity"] * (n - 1):
        return 6
    return 0


def id_of(h):
    for i in range(len(h)):
        if h[i] == 0x20 or h[i] == 0x09:
            h = h[:i]
            break
    if len(h) >= 2 and h[-2:] in (b"/1", b"/2"):
        h = h[:-2]
    return h


@functools.lru_cache(maxsize=None)
def judged(recs, mate, with_content=True):
    """every record of one mate on its own: [(verdict, bases removed, rendered text, trimmed length, sum of v of the trimmed read)]"""
    front, back = ARGS["quality_cutoff"]
    ad = ARGS["adapter"] if mate == 0 else ARGS["adapter2"]
    lo = ARGS["min_len"][mate]
    out = []
    for h, s, q in recs:
        a, z = quality_span(q, front, back)
        s2, q2 = s[a:z], q[a:z]
        cut = adapter_cut(s2, ad, ARGS["err_permille"], ARGS["min_overlap"])
        s2, q2 = s2[:cut], q2[:cut]
        v = 1 if len(s2) < lo else (content_verdict(s2, q2, CONTENT) if with_content else 0)
        out.append((v, len(s) - len(s2), b"@" + h + b"\n" + s2 + b"\n+\n" + q2 + b"\n", len(s2), sum(b - 33 for b in q2)))
    return tuple(out)


class Expected:
    """what filter_fastq_paired leaves behind for the first n_pairs pairs of (recs1, recs2)"""

    def __init__(self, recs1, recs2, pair_filter="any", n_pairs=None, with_content=True):
        j1, j2 = judged(recs1, 0, with_content), judged(recs2, 1, with_content)
        n = min(len(j1), len(j2)) if n_pairs is None else n_pairs
        self.pairs_in = n
        self.out = [[], []]
        self.hist = [dict.fromkeys(REASONS, 0), dict.fromkeys(REASONS, 0)]
        self.dropped = {"mate1_only": 0, "mate2_only": 0, "both": 0}
        self.removed = 0
        self.after = [[0, 0, 0], [0, 0, 0]]                  # per mate: records, bases, sum of v of what is written
        self.kept_at = []
        for i in range(n):
            a, b = j1[i], j2[i]
            v1, v2 = a[0], (0 if pair_filter == "first" else b[0])
            self.removed += a[1] + b[1]
            if v1:
                self.hist[0][REASONS[v1 - 1]] += 1
            if v2:
                self.hist[1][REASONS[v2 - 1]] += 1
            drop = (v1 or v2) if pair_filter == "any" else (v1 and v2) if pair_filter == "both" else v1
            if drop:
                self.dropped["both" if v1 and v2 else "mate1_only" if v1 else "mate2_only"] += 1
                continue
            self.kept_at.append(i)
            for k, r in enumerate((a, b)):
                self.out[k].append(r[2])
                self.after[k][0] += 1
                self.after[k][1] += r[3]
                self.after[k][2] += r[4]
        self.pairs_out = len(self.kept_at)
        self.text = [b"".join(self.out[0]), b"".join(self.out[1])]

    def result(self):
        return (self.pairs_in, self.pairs_out, self.removed, len(self.text[0]), len(self.text[1]), self.dropped)

    def prefix(self, k):
        """the text of either mate for the kept pairs among the first k pairs"""
        m = sum(1 for i in self.kept_at if i < k)
        return b"".join(self.out[0][:m]), b"".join(self.out[1][:m])


def content_rules(F):
    return F.ContentRules(**CONTENT)


def run(F, data1, data2, entrypos, fbufsize, pair_filter="any", check_names=True, reports=False, opener1=None, opener2=None, content=True):
    """filter_fastq_paired over two byte strings (io.BytesIO unless an opener makes the file object) ->
    (result or None, error or None, out1, out2, report, report2)"""
    import io
    o1, o2 = io.BytesIO(), io.BytesIO()
    rep = (F.FilterReport(200), F.FilterReport(200)) if reports else (None, None)
    res = err = None
    fh1 = opener1(data1) if opener1 else io.BytesIO(data1)
    fh2 = opener2(data2) if opener2 else io.BytesIO(data2)
    try:
        res = F.filter_fastq_paired(fh1, fh2, o1, o2, fbufsize=fbufsize, content=content_rules(F) if content else None, pair_filter=pair_filter,
                                    check_names=check_names, report=rep[0], report2=rep[1], entrypos=entrypos, **ARGS)
    except ValueError as e:
        err = str(e)
    finally:
        fh1.close()
        fh2.close()
    return res, err, o1.getvalue(), o2.getvalue(), rep[0], rep[1]


def check_reports(rep, rep2, recs1, recs2, want):
    """the reports' counts against the loop: dropped per mate, records / bases / quality sum before and after"""
    for k, (r, recs) in enumerate(((rep, recs1), (rep2, recs2))):
        assert r.dropped == want.hist[k], (k, r.dropped, want.hist[k])
        n = want.pairs_in
        assert int(r.before.head[0]) == n and int(r.before.head[1]) == 0
        assert int(r.before.head[2]) == sum(len(s) for _, s, _ in recs[:n])
        assert int(r.before.head[4]) == sum(b - 33 for _, _, q in recs[:n] for b in q)
        assert [int(r.after.head[0]), int(r.after.head[2]), int(r.after.head[4])] == want.after[k], k

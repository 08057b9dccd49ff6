"""Rows kept or dropped for what is in the read: ffq_table_select_reads on the device.

The expectation of every test is the plain loop below -- the rule of include/ffq.h written out here, byte by byte -- never
fastqandfurious.ContentRules.  The bulk case uses a numpy form of that loop, which is checked against the plain loop on the
hand vectors.  Every comparison is exact: the kept rows, d_idx, all eight counts.  Coordinates: a row minus `add` indexes the
buffer the scanner saw; with a sentinel that buffer is b'\\n' + bytes.

A miscounted quantity shows only where a verdict hangs on it, so the reads of the length and boundary tests are MADE to sit
on a rule's edge: one variant that the rule just keeps and one that it just drops.
"""
import functools

import numpy as np
import pytest

import grid_expect as GE

GROUP_BYTES = 32        # bytes of a row that its 8 lanes take per round (csrc/ffq_filter.h: FILTER_G * 4)
TILE = 160              # bases above which a row gets a wave of its own (FILTER_TILE)
WAVE_BYTES = 256        # bytes of a row that the 64 lanes of the long rows' kernel take per step

EE = [int(np.floor(1e6 * 10.0 ** (-v / 10.0) + 0.5)) for v in range(96)]      # (tests/test_filter_host.py checks it exactly)
OFF = dict(qual_base=33, max_n=-1, min_mean_qual=0, qualified_qual=15, max_unqualified_pct=-1, min_complexity_pct=0, max_ee_micro=-1)
NJ = 7


def rules(**kw):
    r = dict(OFF)
    r.update(kw)
    return r


# ---- the rule ------------------------------------------------------------------------------------------------------
def quantities(seq, q, R):
    n = len(seq)
    nN = sv = u = ee = d = 0
    for i in range(n):
        v = min(max(q[i] - R["qual_base"], 0), 95)
        if seq[i] in b"Nn":
            nN += 1
        sv += v
        if v < R["qualified_qual"]:
            u += 1
        ee += EE[v]
        if i < n - 1 and seq[i] != seq[i + 1]:
            d += 1
    return nN, sv, u, ee, d


def content_verdict(seq, q, R):
    """rules 2 to 6 on an eligible row, by a plain loop over its bytes"""
    n = len(seq)
    nN, sv, u, ee, d = quantities(seq, q, R)
    if R["max_n"] >= 0 and nN > R["max_n"]:
        return 2
    if R["min_mean_qual"] > 0 and sv < R["min_mean_qual"] * n:
        return 3
    if R["max_unqualified_pct"] >= 0 and 100 * u > R["max_unqualified_pct"] * n:
        return 4
    if R["max_ee_micro"] >= 0 and ee > R["max_ee_micro"]:
        return 5
    if R["min_complexity_pct"] > 0 and n >= 2 and 100 * d < R["min_complexity_pct"] * (n - 1):
        return 6
    return 0


def is_on(R):
    return R is not None and (R["max_n"] >= 0 or R["min_mean_qual"] > 0 or R["max_unqualified_pct"] >= 0 or R["max_ee_micro"] >= 0
                              or R["min_complexity_pct"] > 0)


def positions_ok(buf, p2, p3, p4, p5, sentinel):
    """the part of the eligibility that needs no byte of the row; buf: the buffer with its sentinel, if it has one"""
    ok = min(p2, p3, p4, p5) >= 0 and p2 <= p3 <= len(buf) and p4 <= p5 <= len(buf) and p3 - p2 == p5 - p4
    if ok and sentinel and p3 > p2 and (p2 < 1 or p4 < 1):
        ok = False                                           # a line with bytes in it that begins at the virtual newline
    return ok


def loop_select(buf, rows, R, lo, hi, add=0, sentinel=False, verdict=content_verdict):
    """(ordinals of the kept rows, the eight counts, the verdicts); buf: as the scanner saw it (b'\\n' + bytes with a sentinel)"""
    kept, counts, verdicts = [], [0] * 8, []
    on = is_on(R)
    for i, row in enumerate(np.asarray(rows, dtype=np.int64).reshape(-1, 6).tolist()):
        p2, p3, p4, p5 = (x - add for x in row[2:])
        v, judged = 0, True
        if not lo <= row[3] - row[2] <= hi:
            v = 1
            judged = positions_ok(buf, p2, p3, p4, p5, sentinel)          # (no byte of the row is read)
        elif on:
            judged = positions_ok(buf, p2, p3, p4, p5, sentinel) and 10 not in buf[p2:p3] and 10 not in buf[p4:p5]
            if judged:
                v = verdict(buf[p2:p3], buf[p4:p5], R)
        counts[v] += 1
        if on and not judged:
            counts[NJ] += 1
        if v == 0:
            kept.append(i)
        verdicts.append(v)
    return kept, counts, verdicts


_IS_N = np.zeros(256, dtype=np.int64)
_IS_N[[78, 110]] = 1
_EE_NP = np.array(EE, dtype=np.int64)


def np_verdict(seq, q, R):
    """content_verdict, a row at a time in numpy"""
    n = len(seq)
    if n == 0:
        return 0
    s = np.frombuffer(seq, dtype=np.uint8)
    v = np.clip(np.frombuffer(q, dtype=np.uint8).astype(np.int64) - R["qual_base"], 0, 95)
    if R["max_n"] >= 0 and int(_IS_N[s].sum()) > R["max_n"]:
        return 2
    if R["min_mean_qual"] > 0 and int(v.sum()) < R["min_mean_qual"] * n:
        return 3
    if R["max_unqualified_pct"] >= 0 and 100 * int((v < R["qualified_qual"]).sum()) > R["max_unqualified_pct"] * n:
        return 4
    if R["max_ee_micro"] >= 0 and int(_EE_NP[v].sum()) > R["max_ee_micro"]:
        return 5
    if R["min_complexity_pct"] > 0 and n >= 2 and 100 * int((s[1:] != s[:-1]).sum()) < R["min_complexity_pct"] * (n - 1):
        return 6
    return 0


# ---- tables by hand ------------------------------------------------------------------------------------------------
def record(buf, rows, seq, qual=None, seq_mod4=None, qual_mod4=None):
    """append a four-line record to `buf` (bytearray) and its row to `rows`; the sequence / the quality begin at an address
    = seq_mod4 / qual_mod4 modulo 4 (junk in front of the record, a longer '+' line)"""
    qual = b"I" * len(seq) if qual is None else qual
    if seq_mod4 is not None:
        buf += b"#" * ((seq_mod4 - (len(buf) + 3)) % 4)
    p0 = len(buf)
    buf += b"@h\n"
    p2 = len(buf)
    buf += seq + b"\n+"
    if qual_mod4 is not None:
        buf += b"x" * ((qual_mod4 - (len(buf) + 1)) % 4)
    buf += b"\n"
    p4 = len(buf)
    buf += qual + b"\n"
    rows.append([p0, p2 - 1, p2, p2 + len(seq), p4, p4 + len(qual)])


def table_of(reads, aligned=False):
    """aligned: record i's sequence starts at address i mod 4, its quality at another residue"""
    buf, rows = bytearray(b"#"), []
    for i, (s, q) in enumerate(reads):
        if aligned:
            record(buf, rows, s, q, i % 4, (i % 4 + 1 + (i // 4) % 3) % 4)
        else:
            record(buf, rows, s, q)
    return bytes(buf), np.array(rows, dtype=np.int64).reshape(-1, 6)


def one_read(rng, n, alphabet=b"ACGTNacgtn.", qlo=33, qhi=75):
    alpha = np.frombuffer(alphabet, dtype=np.uint8)
    return alpha[rng.integers(0, len(alpha), n)].tobytes(), rng.integers(qlo, qhi, n, dtype=np.uint8).tobytes()


def band(x):
    return list(range(x - 3, x + 4))


LENGTHS = sorted(set(list(range(0, 41)) + band(GROUP_BYTES) + band(TILE) + band(2 * TILE) + band(WAVE_BYTES)))


# ---- the device ------------------------------------------------------------------------------------------------------------
class Dev:
    """a buffer at the END of a device allocation of whole pages (a read past it leaves the allocation) and calls on it"""

    def __init__(self, ctx, data):
        self.ctx, self.n = ctx, len(data)
        self.size = (len(data) + 4095) // 4096 * 4096 + 4096
        self.base = ctx.dev_alloc(self.size)
        self.ptr = self.base + self.size - len(data)
        if len(data):
            ctx.h2d(self.ptr, np.frombuffer(data, dtype=np.uint8).copy())
        ctx.sync()

    def close(self):
        self.ctx.dev_free(self.base)

    def select(self, rows, R, lo=None, hi=None, sentinel=False, add=0, idx=True, ptr=None):
        """ffq_table_select_reads -> (kept rows int64[k][6], d_idx int64[k] or None, counts)"""
        import torch
        from fastqandfurious_amd import hip
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 6)
        n = rows.shape[0]
        t = torch.from_numpy(rows.copy()).cuda() if n else torch.zeros((1, 6), dtype=torch.int64, device="cuda")
        out = torch.full((n + 1, 6), -7, dtype=torch.int64, device="cuda")
        di = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        r = None if R is None else hip.ContentRulesStruct(*(R[name] for name, _ in hip.ContentRulesStruct._fields_))
        k, counts = self.ctx.table_select_reads(self.ptr if ptr is None else ptr, self.n, t.data_ptr(), n, out.data_ptr(), r, lo, hi,
                                                di.data_ptr() if idx else None, sentinel=sentinel, add=add)
        o, d = out.cpu().numpy(), di.cpu().numpy()
        assert (o[k:] == -7).all(), "rows behind the kept ones were written"
        assert (d[k if idx else 0:] == -7).all()
        return o[:k], (d[:k] if idx else None), counts


def check(dev, buf, rows, R, lo=None, hi=None, combos=((0, 0),), idx=True, want=None, verdict=content_verdict):
    """the device against the loop: kept rows, d_idx, the eight counts, for (sentinel, add) combinations; buf: the bytes"""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
    l, h = -(1 << 62) if lo is None else lo, (1 << 62) if hi is None else hi
    for sentinel, add in combos:
        if want is None or combos != ((0, 0),):
            kept, counts, verdicts = loop_select((b"\n" if sentinel else b"") + buf, rows + sentinel, R, l, h, 0, bool(sentinel), verdict)
        else:
            kept, counts, verdicts = want
        moved = rows + sentinel + add
        got, gi, gc = dev.select(moved, R, lo, hi, bool(sentinel), add, idx)
        assert gc == counts, (sentinel, add, gc, counts)
        assert sum(gc[:7]) == rows.shape[0] and gc[0] == len(kept)
        if idx:
            assert gi.tolist() == kept, (sentinel, add)
        assert (got == moved[kept]).all(), (sentinel, add)
    return kept, counts, verdicts


@pytest.fixture(scope="module")
def hand(gpu_ctx):
    """the hand table of the edge tests on the device, once"""
    buf, rows = table_of(EDGE_READS)
    dev = Dev(gpu_ctx, buf)
    yield dev, buf, rows
    dev.close()


def q(*vs):
    return bytes(33 + v for v in vs)


# every rule at its edge (others off): (what, rules, read kept, read dropped)
EDGES = [
    ("n == max_n", rules(max_n=2), (b"ANNA", b"IIII"), (b"ANnN", b"IIII")),
    ("n counts", rules(max_n=0), (b"AC.-XRYM", b"IIIIIIII"), (b"ACGn", b"IIII")),
    ("mean", rules(min_mean_qual=20), (b"ACGT", q(20, 19, 21, 20)), (b"ACGT", q(20, 19, 20, 20))),
    ("mean, clamp below", rules(min_mean_qual=1), (b"AC", bytes([0, 35])), (b"AC", bytes([0, 34]))),
    ("mean, clamp above", rules(min_mean_qual=95), (b"AC", bytes([255, 128])), (b"AC", bytes([255, 127]))),
    ("unqualified", rules(qualified_qual=15, max_unqualified_pct=25), (b"ACGTACGT", q(14, 0, 15, 15, 40, 40, 40, 40)),
     (b"ACGTACGT", q(14, 0, 14, 15, 40, 40, 40, 40))),
    ("unqualified 0", rules(qualified_qual=1, max_unqualified_pct=0), (b"ACG", q(1, 1, 1)), (b"ACG", q(1, 0, 1))),
    ("unqualified, clamp", rules(qualified_qual=95, max_unqualified_pct=50), (b"AC", bytes([255, 127])), (b"AC", bytes([126, 127]))),
    ("ee", rules(max_ee_micro=EE[10] + EE[20] + EE[3]), (b"ACG", q(10, 20, 3)), (b"ACG", q(10, 20, 2))),
    ("ee one over", rules(max_ee_micro=EE[0] * 2 + EE[60] - 1), (b"ACG", q(0, 0, 64)), (b"ACG", q(0, 0, 60))),
    ("ee 0", rules(max_ee_micro=0), (b"ACG", q(64, 95, 80)), (b"ACG", q(64, 63, 80))),
    ("complexity", rules(min_complexity_pct=50), (b"AACCG", b"IIIII"), (b"AACCC", b"IIIII")),
    ("complexity n = 2", rules(min_complexity_pct=100), (b"AC", b"II"), (b"AA", b"II")),
    ("complexity n = 1, 0", rules(min_complexity_pct=100), (b"A", b"I"), (b"AAA", b"III")),
    ("complexity case", rules(min_complexity_pct=100), (b"Aa", b"II"), (b"aa", b"II")),
]
EDGE_READS = [(b"", b"")] + [rd for e in EDGES for rd in e[2:]]


def test_the_loop_gives_the_hand_values():
    R = rules(qual_base=33)
    assert quantities(b"ANnCC", q(0, 10, 14, 15, 95), R) == (2, 134, 3, EE[0] + EE[10] + EE[14] + EE[15], 3)
    assert quantities(b"AC", bytes([0, 255]), R) == (0, 95, 1, 1000000, 1)
    assert EE[:4] == [1000000, 794328, 630957, 501187] and EE[63] == 1 and EE[64] == 0 and len(EE) == 96
    for what, R, keep, drop in EDGES:
        assert content_verdict(*keep, R) == 0, what
        assert content_verdict(*drop, R) != 0, what
        assert np_verdict(*keep, R) == 0 and np_verdict(*drop, R) == content_verdict(*drop, R), what
    # the first rule that fails is the verdict
    R = rules(max_n=0, min_mean_qual=30, max_unqualified_pct=0, max_ee_micro=0, min_complexity_pct=100)
    assert content_verdict(b"NN", q(0, 0), R) == 2 and content_verdict(b"AA", q(0, 0), R) == 3
    assert content_verdict(b"AA", q(14, 46), R) == 4 and content_verdict(b"AA", q(30, 30), R) == 5
    assert content_verdict(b"AA", q(70, 70), R) == 6 and content_verdict(b"AC", q(70, 70), R) == 0
    assert content_verdict(b"", b"", R) == 0
    buf, rows = table_of([(b"ACGT", b"IIII"), (b"AC\nGT", b"II\nII"), (b"NNNNNN", b"IIIIII")])
    rows = np.concatenate([rows, [[0, 1, 2, 6, -1, -1]]])
    assert loop_select(buf, rows, rules(max_n=0), 4, 5) == ([0, 1, 3], [3, 1, 0, 0, 0, 0, 0, 2], [0, 0, 1, 0])
    assert loop_select(buf, rows, rules(max_n=0), 4, 6) == ([0, 1, 3], [3, 0, 1, 0, 0, 0, 0, 2], [0, 0, 2, 0])
    assert loop_select(buf, rows, None, 4, 5) == ([0, 1, 3], [3, 1, 0, 0, 0, 0, 0, 0], [0, 0, 1, 0])


def test_the_numpy_form_is_the_loop():
    rng = np.random.default_rng(11)
    reads = [one_read(rng, int(rng.integers(0, 400)), qhi=110) for _ in range(80)] + EDGE_READS
    for R in (ALL_ON, rules(qual_base=64, max_n=3, max_ee_micro=10 ** 7), rules(qual_base=0, min_mean_qual=60, min_complexity_pct=70)):
        assert [np_verdict(s, qq, R) for s, qq in reads] == [content_verdict(s, qq, R) for s, qq in reads]


ALL_ON = rules(max_n=20, min_mean_qual=18, qualified_qual=12, max_unqualified_pct=35, max_ee_micro=45 * 10 ** 6, min_complexity_pct=60)


@pytest.mark.gpu
def test_every_rule_at_its_edge(hand):
    dev, buf, rows = hand
    for k, (what, R, keep, drop) in enumerate(EDGES):
        kept, counts, verdicts = check(dev, buf, rows, R, combos=((0, 0), (1, 0), (0, 5), (1, -1)))
        assert verdicts[1 + 2 * k] == 0 and verdicts[2 + 2 * k] != 0, what
        assert verdicts[0] == 0 and counts[NJ] == 0
        # ... and the two reads alone
        check(dev, buf, rows[1 + 2 * k:3 + 2 * k], R)
    # in combination: every rule on at once, with each read's own rule among them
    for what, R, keep, drop in EDGES:
        both = dict(ALL_ON)
        both.update({k: v for k, v in R.items() if v != OFF[k]})
        check(dev, buf, rows, both)
    # a row that fails two rules is counted under the first
    R = rules(max_n=0, min_mean_qual=30, max_unqualified_pct=0, max_ee_micro=0, min_complexity_pct=100)
    b2, r2 = table_of([(b"NN", q(0, 0)), (b"AA", q(0, 0)), (b"AA", q(14, 46)), (b"AA", q(30, 30)), (b"AA", q(70, 70)), (b"AC", q(70, 70)),
                       (b"NNN", q(0, 0, 0))])
    d2 = Dev(dev.ctx, b2)
    try:
        _, counts, verdicts = check(d2, b2, r2, R, lo=1, hi=2)
        assert verdicts == [2, 3, 4, 5, 6, 0, 1] and counts == [1, 1, 1, 1, 1, 1, 1, 0]
    finally:
        d2.close()


def with_changes(n, at, rng=None):
    """a sequence of n bases that changes behind exactly the positions `at` (seq[i] != seq[i + 1] for i in at)"""
    s, c = bytearray(n), 0
    for i in range(n):
        s[i] = b"ACGT"[c % 4]
        if i in at:
            c += 1 if rng is None else int(rng.integers(1, 4))
    return bytes(s)


def edge_reads(rng, n):
    """reads of n bases on the edge of each rule of EDGE_RULES: (rules, kept variant, dropped variant or None)"""
    out = []
    s, qq = one_read(rng, n, qhi=110)
    nN, sv, u, ee, d = quantities(s, qq, OFF)
    out.append((rules(max_n=nN), (s, qq)))
    out.append((rules(max_ee_micro=ee), (s, qq)))
    if nN:
        out.append((rules(max_n=nN - 1), (s, qq)))
    if ee:
        out.append((rules(max_ee_micro=ee - 1), (s, qq)))
    if n:
        # sv == m * n exactly, and one less
        m = int(rng.integers(2, 90))
        v = np.full(n, m, dtype=np.int64)
        for _ in range(n):
            i, j = rng.integers(0, n, 2)
            k = int(min(v[i], 95 - v[j], rng.integers(0, 40)))
            if i != j:
                v[i] -= k
                v[j] += k
        assert v.sum() == m * n
        lower = v.copy()
        lower[int(np.flatnonzero(lower > 0)[0])] -= 1
        for vv in (v, lower):
            out.append((rules(min_mean_qual=m), (s, bytes((vv + 33).astype(np.uint8)))))
        # the most unqualified bases that 30 per cent allow, and one more
        for k in (30 * n // 100, 30 * n // 100 + 1):
            if k <= n:
                vv = rng.integers(20, 60, n)
                vv[rng.permutation(n)[:k]] = rng.integers(0, 20, k)
                out.append((rules(qualified_qual=20, max_unqualified_pct=30), (s, bytes((vv + 33).astype(np.uint8)))))
    if n >= 2:
        # every pair differs (the only d that 100 per cent keep), and all but one; the fewest changes 1 per cent keeps, and one less
        out.append((rules(min_complexity_pct=100), (with_changes(n, set(range(n - 1)), rng), qq)))
        out.append((rules(min_complexity_pct=100), (with_changes(n, set(range(n - 1)) - {int(rng.integers(0, n - 1))}, rng), qq)))
        dmin = -(-(n - 1) // 100)
        for k in (dmin, dmin - 1):
            out.append((rules(min_complexity_pct=1), (with_changes(n, set(rng.permutation(n - 1)[:k].tolist())), qq)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("part", range(4))
def test_read_lengths(gpu_ctx, part):
    """every length 0..40 and around a group's round, the short / long threshold, twice the threshold and a wave's step; the
    sequence at every address mod 4, the quality at another residue; each read on the edge of the one rule that is on"""
    rng = np.random.default_rng(500 + part)
    for n in LENGTHS[part::4]:
        cases = edge_reads(rng, n)
        reads = [rd for _R, rd in cases for _ in range(4)]
        buf, rows = table_of(reads, aligned=True)
        assert {int(r[2]) % 4 for r in rows[:4]} == {0, 1, 2, 3} and all(int(r[2]) % 4 != int(r[4]) % 4 for r in rows)
        dev = Dev(gpu_ctx, buf)
        try:
            seen = set()
            for k, (R, _rd) in enumerate(cases):
                _, counts, verdicts = check(dev, buf, rows, R)
                assert len(set(verdicts[4 * k:4 * k + 4])) == 1 and counts[NJ] == 0
                seen.add((tuple(sorted(R.items())), verdicts[4 * k]))
            # (each rule saw a read it keeps and, where the length allows one, a read it drops)
            if n >= 2:
                assert {v for _r, v in seen} >= {0, 3, 4, 6}, (n, seen)
        finally:
            dev.close()


def boundary_cases():
    """(n, positions of the changes): a run that changes exactly at a dword edge, a lane edge, a round's edge, the step of a
    wave, and nowhere else -- with as many changes inside dwords beside it as 1 per cent needs to keep the row, so that the
    change at the edge decides (and one fewer: counted twice, it would keep a row that is dropped)"""
    out = []
    for n, edge in ((8, 3), (12, 7), (40, 31), (70, 63), (TILE, 31), (TILE, 127), (300, 255), (300, 159), (600, 511), (600, 255),
                    (2 * TILE + 1, 2 * TILE - 1), (257, 255), (258, 256)):
        dmin = -(-(n - 1) // 100)
        inner = [i for i in range(1, n - 1, 4) if abs(i - edge) > 4]           # pairs inside a dword
        out.append((n, {edge} | set(inner[:dmin - 1])))                          # d == dmin: kept only if the edge counts once
        if dmin >= 2:
            out.append((n, {edge} | set(inner[:dmin - 2])))                      # d == dmin - 1: dropped unless it counts twice
        out.append((n, set(inner[:dmin])))                                       # d == dmin without the edge
    return out


@pytest.mark.gpu
def test_complexity_across_boundaries(gpu_ctx):
    reads = [(with_changes(n, at), b"I" * n) for n, at in boundary_cases()]
    for (n, at), (s, _q) in zip(boundary_cases(), reads):
        assert quantities(s, _q, OFF)[4] == len(at)
    # a homopolymer of every length of the bands: d == 0 (dropped by 1 per cent from n = 2 on); with one change, kept up to n = 101
    reads += [(b"G" * n, b"I" * n) for n in LENGTHS] + [(b"G" * (n - 1) + b"T", b"I" * n) for n in LENGTHS if n >= 2]
    reads = [rd for rd in reads for _ in range(4)]
    buf, rows = table_of(reads, aligned=True)
    dev = Dev(gpu_ctx, buf)
    try:
        _, counts, verdicts = check(dev, buf, rows, rules(min_complexity_pct=1))
        cases = boundary_cases()
        for k, (n, at) in enumerate(cases):                  # (kept exactly when 100 * d reaches n - 1)
            assert verdicts[4 * k:4 * k + 4] == [0 if 100 * len(at) >= n - 1 else 6] * 4, (n, sorted(at))
        assert counts[0] > len(cases) and counts[6] > len(LENGTHS) * 4 - 12
        check(dev, buf, rows, rules(min_complexity_pct=100))
        # alternating reads of every length: d == n - 1, the only value 100 per cent keep; and with one pair equal
        alt = [(with_changes(n, set(range(n - 1))), b"I" * n) for n in LENGTHS]
        alt += [(with_changes(n, set(range(n - 1)) - {e}), b"I" * n) for n in LENGTHS
                for e in (0, 3, 4, 31, 32, 127, 159, 160, 255, 256, n - 2) if 0 <= e < n - 1]
    finally:
        dev.close()
    alt = [rd for rd in alt for _ in range(4)]
    buf, rows = table_of(alt, aligned=True)
    dev = Dev(gpu_ctx, buf)
    try:
        _, counts, verdicts = check(dev, buf, rows, rules(min_complexity_pct=100))
        assert verdicts[:4 * len(LENGTHS)] == [0] * (4 * len(LENGTHS))
        assert set(verdicts[4 * len(LENGTHS):]) == {6}
    finally:
        dev.close()


def ineligible_rows(buf, rows):
    """appends rows the content rules do not apply to (Ns throughout: judged, every one would be dropped); returns how many"""
    n0 = len(rows)
    record(buf, rows, b"NNNNNN\nNNNNNN", b"IIIIII\nIIIIII")                     # a wrapped record
    record(buf, rows, b"NNNNNN\nNNNNNN", b"IIIIIIIIIIIII")                       # a newline in the sequence only
    record(buf, rows, b"NNNNNNNNNNNNN", b"IIIIII\nIIIIII")                       # ... in the quality only
    record(buf, rows, b"N" * 200 + b"\n" + b"N" * 99, b"I" * 300)                # ... in a long row's sequence
    record(buf, rows, b"N" * 300, b"I" * 299 + b"\n")                            # ... as a long row's last quality byte
    record(buf, rows, b"NNNNNNNN", b"IIII")                                      # unequal lengths
    p0 = rows[-1][0]
    rows.append(rows[-1][:4] + [-1, -1])                                         # a FASTA row
    rows.append([p0, p0 + 2, p0 + 3, p0 + 7, len(buf) - 3, len(buf) + 1])        # past the buffer
    rows.append([p0, p0 + 2, len(buf) - 3, len(buf) + 1, p0 + 3, p0 + 7])
    rows.append([p0, p0 + 2, len(buf) - 2, len(buf) + 300, p0 + 3, p0 + 305])    # ... a long row
    rows.append([p0, p0 + 2, -5, -1, p0 + 11, p0 + 15])                          # in front of the buffer
    rows.append([p0, p0 + 2, p0 + 7, p0 + 3, p0 + 15, p0 + 11])                  # ends in front of starts
    return len(rows) - n0


@pytest.mark.gpu
def test_rows_that_are_not_judged(gpu_ctx):
    """each goes by its length alone, counts in [7], and no byte outside the buffer is read (the buffer ends its allocation)"""
    buf, rows = bytearray(b"#"), []
    record(buf, rows, b"ACGTACGT", b"IIIIIIII")
    record(buf, rows, b"ACGNACGT", b"IIIIIIII")
    n_bad = ineligible_rows(buf, rows)
    buf, rows = bytes(buf), np.array(rows, dtype=np.int64)
    dev = Dev(gpu_ctx, buf)
    try:
        R = rules(max_n=0)
        _, counts, verdicts = check(dev, buf, rows, R, combos=((0, 0), (1, 0), (0, 9), (1, (1 << 33) + 5)))
        assert verdicts == [0, 2] + [0] * n_bad and counts == [1 + n_bad, 0, 1, 0, 0, 0, 0, n_bad]
        for i in range(2, len(rows)):
            _, counts, _v = check(dev, buf, rows[i:i + 1], R)
            assert counts == [1, 0, 0, 0, 0, 0, 0, 1], i
            ln = int(rows[i][3] - rows[i][2])
            # dropped by its length: no byte is read, so only a row whose POSITIONS make it ineligible counts in [7]
            _, counts, _v = check(dev, buf, rows[i:i + 1], R, lo=ln + 1)
            assert counts[1] == 1 and counts[NJ] == (0 if i < 7 else 1), (i, counts)
            _, counts, _v = check(dev, buf, rows[i:i + 1], R, hi=ln)
            assert counts[0] == 1 and counts[NJ] == 1
        # with the sentinel, a line beginning at coordinate 0 (the virtual newline): not judged; one of length 0 there is
        r = rows[1] + 1
        n = int(r[3] - r[2])
        sub = np.array([[0, 1, 0, n, r[4], r[5]], r.tolist(), [0, 1, 0, 0, 0, 0], [r[0], r[1], r[2], r[3], 0, n]], dtype=np.int64)
        want = loop_select(b"\n" + buf, sub, R, -(1 << 62), 1 << 62, 0, True)
        got, gi, gc = dev.select(sub, R, sentinel=True, add=0)
        assert gc == want[1] == [3, 0, 1, 0, 0, 0, 0, 2] and gi.tolist() == want[0] == [0, 2, 3]
        # the last record's quality ends exactly at n_bytes; a sequence that ends there
        last = np.array([[0, 1, 2, 10, len(buf) - 8, len(buf)], [0, 1, len(buf) - 8, len(buf), 2, 10],
                         [0, 1, 2, 2 + 300, len(buf) - 300, len(buf)], [0, 1, len(buf) - 300, len(buf), 2, 2 + 300]], dtype=np.int64)
        check(dev, buf, last, rules(min_mean_qual=10, min_complexity_pct=1), combos=((0, 0), (1, 0)))
    finally:
        dev.close()


@pytest.mark.gpu
def test_compaction(gpu_ctx):
    import torch
    rng = np.random.default_rng(21)
    pool = [one_read(rng, int(rng.integers(0, 60)), qhi=80) for _ in range(300)]
    buf, rows = table_of(pool)
    dev = Dev(gpu_ctx, buf)
    try:
        R = rules(max_n=4, min_mean_qual=19)
        for n_rows in (0, 1, 255, 256, 257, 3 * 256 + 1):
            table = rows[rng.integers(0, len(pool), n_rows)] if n_rows else rows[:0]        # repeated, out of order
            kept, counts, _v = check(dev, buf, table, R, lo=3, hi=50, combos=((0, 0), (1, 0), (0, -3), (1, (1 << 40) + 1)))
            if n_rows > 200:
                assert 0 < len(kept) < n_rows and counts[1] and counts[2] and counts[3]
            check(dev, buf, table, R, lo=3, hi=50, idx=False)
            # all kept, none kept (by content, by length)
            assert check(dev, buf, table, rules(max_n=1000))[1][0] == n_rows
            assert check(dev, buf, table, rules(min_mean_qual=95), lo=1)[1][0] == 0
            assert check(dev, buf, table, R, lo=1000)[1][1] == n_rows
            # rules NULL / every rule off: ffq_table_select_seqlen_idx on the same table, and no buffer is needed
            for none in (None, dict(OFF)):
                got, gi, gc = dev.select(table, none, 3, 50, ptr=0)
                t = torch.from_numpy(np.ascontiguousarray(table)).cuda() if n_rows else torch.zeros((1, 6), dtype=torch.int64, device="cuda")
                o = torch.zeros((n_rows + 1, 6), dtype=torch.int64, device="cuda")
                di = torch.zeros((n_rows + 1,), dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                k = gpu_ctx.table_select_seqlen_idx(t.data_ptr(), n_rows, 3, 50, o.data_ptr(), di.data_ptr())
                assert gc == [k, n_rows - k, 0, 0, 0, 0, 0, 0]
                assert (got == o.cpu().numpy()[:k]).all() and gi.tolist() == di.cpu().numpy()[:k].tolist()
                assert gc == loop_select(buf, table, None, 3, 50)[1]
    finally:
        dev.close()


BULK_RULES = rules(max_n=30, min_mean_qual=17, qualified_qual=15, max_unqualified_pct=40, max_ee_micro=12 * 10 ** 6, min_complexity_pct=30)


def bulk_pool(rng, n_reads=400):
    """(bytes, rows): reads of 0..600 bases of four kinds at every alignment, the ineligible rows after every fortieth"""
    buf, rows = bytearray(b"#"), []
    for k in range(n_reads):
        n = int(rng.integers(0, 601))
        kind = int(rng.integers(0, 4))
        s, qq = one_read(rng, n, alphabet=b"ACGTN" if kind == 0 else b"AAAAAAAC" if kind == 1 else b"ACGT",
                         qlo=33 + (0, 10, 20, 2)[kind], qhi=33 + (42, 42, 45, 30)[kind])
        record(buf, rows, s, qq, k % 4, (k // 4) % 4)
        if k % 40 == 7:
            ineligible_rows(buf, rows)
    return bytes(buf), np.array(rows, dtype=np.int64)


@pytest.mark.gpu
def test_bulk(gpu_ctx):
    """20 000 random rows, lengths 0..600, mixed eligibility, all six rules on: a long list of some thousands of rows"""
    rng = np.random.default_rng(77)
    buf, rows = bulk_pool(rng)
    table = rows[rng.integers(0, len(rows), 20000)]
    R = BULK_RULES
    assert loop_select(buf, rows[::9], R, 20, 580, verdict=np_verdict) == loop_select(buf, rows[::9], R, 20, 580)
    memo = {}

    def once(s, qq, R):                                      # (the table repeats some nine hundred rows)
        if (s, qq) not in memo:
            memo[(s, qq)] = np_verdict(s, qq, R)
        return memo[(s, qq)]
    want = loop_select(buf, table, R, 20, 580, verdict=once)
    assert all(want[1][k] > 50 for k in range(8)), want[1]
    assert int((table[:, 3] - table[:, 2] > TILE).sum()) > 5000
    dev = Dev(gpu_ctx, buf)
    try:
        check(dev, buf, table, R, lo=20, hi=580, want=want)
        check(dev, buf, table[::-1], R, lo=20, hi=580, verdict=once)
    finally:
        dev.close()


# ---- more rows than one pass of the grid (tests/grid_expect.py) -------------------------------------------------------------
GRID_BOUNDS = (20, 580)


@functools.lru_cache(maxsize=None)
def grid_pool():
    """the bulk pool's kind; empty reads and reads at and one above the long rows' threshold; the ineligible rows once more at
    the very end, where "past the buffer" is past the buffer"""
    rng = np.random.default_rng(78)
    buf, rows = bulk_pool(rng, 300)
    buf, rows = bytearray(buf), rows.tolist()
    for n in (0, 0, 1, TILE, TILE, TILE + 1, TILE + 1):
        record(buf, rows, *one_read(rng, n, alphabet=b"ACGT", qlo=50, qhi=75))
    ineligible_rows(buf, rows)
    return bytes(buf), np.array(rows, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def grid_parts(sentinel):
    """the loop's answer for every pool row ALONE: (verdict, 1 if a content rule is on and the row is not judged)"""
    buf, rows = grid_pool()
    seen = (b"\n" if sentinel else b"") + buf
    per = [loop_select(seen, r + sentinel, BULK_RULES, *GRID_BOUNDS, 0, bool(sentinel)) for r in rows]
    return np.array([v[0] for _k, _c, v in per]), np.array([c[NJ] for _k, c, _v in per])


def grid_idle(sentinel=0):
    """pool rows with nothing to do: not judged, or dropped by their length (no byte of them is read)"""
    verdict, nj = grid_parts(sentinel)
    return np.flatnonzero((verdict == 1) | (nj == 1))


def grid_want(idx, sentinel):
    """(kept ordinals, the eight counts) of a call over pool[idx]"""
    verdict, nj = grid_parts(sentinel)
    v = verdict[idx]
    return np.flatnonzero(v == 0), np.bincount(v, minlength=7).tolist()[:7] + [int(nj[idx].sum())]


@pytest.mark.parametrize("arrangement", GE.ARRANGEMENTS)
def test_the_table_above_one_pass_is_what_the_loop_says(arrangement):
    buf, rows = grid_pool()
    n, P = GE.n_above(GE.P_SHORT), GE.P_SHORT
    assert n > 2 * 2048 * 32 and len(rows) < 500 and len(buf) < 1 << 20
    lengths = rows[:, 3] - rows[:, 2]
    for sentinel in (0, 1):
        idx = GE.table_idx(arrangement, n, P, len(rows), grid_idle(), seed=9)
        kept, counts = grid_want(idx, sentinel)
        at = GE.sample_rows(n, P)
        seen = (b"\n" if sentinel else b"") + buf
        assert len(at) >= 2000 and tuple(loop_select(seen, rows[idx[at]] + sentinel, BULK_RULES, *GRID_BOUNDS, 0, bool(sentinel))[:2]) == \
            (grid_want(idx[at], sentinel)[0].tolist(), grid_want(idx[at], sentinel)[1])
        assert sum(counts[:7]) == n and counts[0] == len(kept)
        for k, s in enumerate(GE.passes(n, P)):
            c = grid_want(idx[s], sentinel)[1]
            if (arrangement, k > 0) in (("late work", False), ("early work", True)):
                assert c[2:7] == [0] * 5 and c[1] > 0 and c[NJ] > 0, (k, c)
            else:
                # every verdict, rows that are not judged, empty reads, reads on both sides of the long rows' threshold
                assert all(x > 0 for x in c), (k, c)
                here = lengths[idx[s]]
                assert (here == 0).any() and ((here > 0) & (here <= TILE)).any() and (here > TILE).any()


@pytest.mark.gpu
def test_more_rows_than_one_pass_of_the_grid(gpu_ctx):
    """three steps of every workgroup of k_filter_rows, the last for 1001 of the 2048 with five rows for the last of those (and a
    long list of some hundred thousand rows): the kept rows, d_idx and the eight counts, in the three arrangements; "late
    work" with a sentinel and add = 500"""
    buf, rows = grid_pool()
    n, P = GE.n_above(GE.P_SHORT), GE.P_SHORT
    assert n > 2 * 2048 * 32
    dev = Dev(gpu_ctx, buf)
    try:
        for arrangement in GE.ARRANGEMENTS:
            sentinel, add = (1, 500) if arrangement == "late work" else (0, 0)
            idx = GE.table_idx(arrangement, n, P, len(rows), grid_idle(), seed=9)
            kept, counts = grid_want(idx, sentinel)
            moved = rows[idx] + sentinel + add
            got, gi, gc = dev.select(moved, BULK_RULES, *GRID_BOUNDS, bool(sentinel), add)
            GE.same_kept(gi, kept, P, arrangement)
            assert gc == counts, (arrangement, gc, counts)
            GE.same_rows(got, moved[kept], P, "%s: the kept rows (row: among the kept)" % arrangement)
    finally:
        dev.close()


@pytest.mark.gpu
def test_the_calls_around_it(gpu_ctx):
    """ffq_table_select_seqlen right after a content call on the same context (shared scratch); the argument errors"""
    import torch
    from fastqandfurious_amd import hip
    rng = np.random.default_rng(5)
    buf, rows = table_of([one_read(rng, int(rng.integers(0, 80))) for _ in range(700)])
    dev = Dev(gpu_ctx, buf)
    try:
        check(dev, buf, rows, ALL_ON, lo=10, hi=70)
        t = torch.from_numpy(rows.copy()).cuda()
        o = torch.zeros_like(t)
        torch.cuda.synchronize()
        k = gpu_ctx.table_select_seqlen(t.data_ptr(), len(rows), 30, 60, o.data_ptr())
        keep = [i for i, r in enumerate(rows.tolist()) if 30 <= r[3] - r[2] <= 60]
        assert k == len(keep) and (o.cpu().numpy()[:k] == rows[keep]).all()
        check(dev, buf, rows, ALL_ON, lo=10, hi=70)

        def refused(R=None, **kw):
            with pytest.raises(hip.FFQError) as ei:
                dev.select(rows[:4], R, **kw)
            assert ei.value.code == hip.E_ARG

        for bad in (dict(qual_base=-1), dict(qual_base=256), dict(max_n=-2), dict(min_mean_qual=-1), dict(min_mean_qual=96),
                    dict(qualified_qual=-1), dict(qualified_qual=96), dict(max_unqualified_pct=-2), dict(max_unqualified_pct=101),
                    dict(min_complexity_pct=-1), dict(min_complexity_pct=101), dict(max_ee_micro=-2)):
            refused(rules(max_n=0, **bad) if "max_n" not in bad else rules(**bad))
        refused(rules(max_n=0), ptr=0)                       # no buffer while a content rule is on
        with pytest.raises(hip.FFQError) as ei:              # d_out must not be d_table
            gpu_ctx.table_select_reads(dev.ptr, dev.n, t.data_ptr(), 4, t.data_ptr(), hip.ContentRulesStruct(33, 0, 0, 15, -1, 0, -1))
        assert ei.value.code == hip.E_ARG
        with pytest.raises(hip.FFQError) as ei:              # tables are 16-byte aligned
            gpu_ctx.table_select_reads(dev.ptr, dev.n, t.data_ptr() + 8, 4, o.data_ptr(), hip.ContentRulesStruct(33, 0, 0, 15, -1, 0, -1))
        assert ei.value.code == hip.E_ARG
        # a scan pending on the context
        data = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, qq) for i, (s, qq) in enumerate([(b"ACGT" * 9, b"I" * 36)] * 50))
        d2 = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
        d_tab = torch.empty((64, 6), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        gpu_ctx.scan_submit(d2.data_ptr(), len(data), d_tab.data_ptr(), 64)
        try:
            refused(rules(max_n=0))
        finally:
            gpu_ctx.scan_wait()
        # the table the library exports
        p = hip.lib().ffq_ee_micro_table()
        assert [int(p[i]) for i in range(96)] == EE
        check(dev, buf, rows, ALL_ON, lo=10, hi=70)
    finally:
        dev.close()

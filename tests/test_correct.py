"""Mismatched bases inside the mates' overlap corrected on the device: ffq_table_pair_correct on hand-made tables.

The expectation of every test is the plain loop of tests/correct_expect.py -- the rule of include/ffq.h written out byte by byte
-- never the package's own correct_mates.  Every comparison is exact: BOTH WHOLE ALLOCATIONS behind the call (the buffers and the
pages in front of them: a stray write anywhere shows), both tables (unchanged), the six counts, the matrix.  The two mates live
in different buffers with different `add`, mate 1 with a sentinel and mate 2 without; mate 2's first quality line lies at the
first byte of its buffer, the last pair's lines at the last bytes of theirs (test_overlap.Dev puts a buffer at the END of its
allocation).  The pass edits bytes, so every run uploads the buffers afresh.
"""
import functools

import numpy as np
import pytest

import correct_expect as K
import grid_expect as GE
from test_merge import ADD1, ADD2, alignments, build, seq_of
from test_overlap import Dev

SIZES = (0, 1, 2, 31, 32, 33, 257)    # group and workgroup edges: 8 lanes per pair, 32 pairs per step
LENS = (1, 15, 16, 17, 31, 32, 33, 150, 511, 512)
# (good, bad, qual_base): fastp's thresholds as the bytes '?' and '/', and thresholds above 0x80 (G = 150, B = 134)
RULES = ((30, 14, 33), (30, 14, 120))
EDGES = np.array([63, 62, 47, 48, 150, 149, 134, 135, 33, 255, 70, 40, 200, 128, 127, 100], dtype=np.uint8)


# ---- the hand table ----------------------------------------------------------------------------------------------------------
def qual_of(rng, n, mode):
    if mode == "edges":               # exactly at G, G - 1, B, B + 1 of both rule sets, and a few bytes around them
        return bytes(EDGES[rng.integers(0, len(EDGES), n)])
    if mode == "sure":
        return bytes(rng.integers(150, 256, n).astype(np.uint8))
    if mode == "poor":
        return bytes(rng.integers(11, 48, n).astype(np.uint8))
    v = rng.integers(0, 255, n)       # "wide": any byte but "\n"
    return bytes(np.where(v >= 10, v + 1, v).astype(np.uint8))


def facing(rng, a, n2, o, err, alphabet):
    """mate 2 whose reverse complement agrees with `a` placed at offset o, but for a share `err` of its bytes"""
    b = bytearray(seq_of(rng, n2, alphabet))
    for j in range(n2):
        p = (n2 - 1 - j) + o
        if 0 <= p < len(a) and rng.random() >= err:
            b[j] = K.COMP.get(a[p], a[p])
    return bytes(b)


def pair(rng, n1, n2, o=None, ins=None, flavour="", h=None, qm=("edges", "edges"), alphabet=b"ACGT", err=0.15):
    """a pair as test_merge.build takes it; ins: what d_insert holds for it (default: n2 + o)"""
    a = seq_of(rng, n1, alphabet)
    return dict(h=(b"r%d" % rng.integers(0, 10 ** 6)) if h is None else h, a=a, qa=qual_of(rng, n1, qm[0]),
                b=facing(rng, a, n2, 0 if o is None else o, err, alphabet), qb=qual_of(rng, n2, qm[1]),
                ins=(n2 + o) if ins is None else ins, flavour=flavour)


QMS = (("edges", "edges"), ("sure", "poor"), ("poor", "sure"), ("wide", "wide"), ("edges", "wide"), ("sure", "sure"))
ALPHABETS = (b"ACGT", b"ACGTacgt", b"ACGTN.", b"acgtn")
EMPTY = dict(h=b"e", a=b"", qa=b"", b=b"", qb=b"", ins=-1, flavour="")
NOT_LOOKED_AT = ("fasta1", "fasta2", "outside1", "outside2", "negative1", "negative2", "unequal1", "unequal2", "coord0")
HEADERS = ("header_neg", "header_empty", "header_out")          # looked at all the same: the rule does not ask about the header


def hand_pairs():
    rng = np.random.default_rng(31)
    pairs = [pair(rng, 150, 150, -30)]            # (pair 0: mate 2's quality line at the first byte of its buffer)
    k = 0
    for n1 in LENS:
        for n2 in LENS:
            for o in alignments(n1, n2):
                pairs.append(pair(rng, n1, n2, o, h=b"h" * (1 + k % 17), qm=QMS[k % 6], alphabet=ALPHABETS[k % 4], err=(0.15, 0.02, 0.5)[(k // 6) % 3]))
                k += 1
    # pairs that must not be looked at
    pairs += [pair(rng, 150, 150, ins=-1), pair(rng, 150, 150, ins=-2), pair(rng, 150, 150, ins=0), pair(rng, 150, 140, ins=290),
              pair(rng, 150, 140, ins=291), pair(rng, 150, 150, ins=-(1 << 31)), pair(rng, 150, 150, ins=(1 << 31) - 1),
              pair(rng, 513, 150, -10, flavour="long"), pair(rng, 150, 513, 10, flavour="long")]
    pairs += [pair(rng, 150, 150, -20, flavour=f) for f in NOT_LOOKED_AT + HEADERS]
    # one pair with work among seven empty ones in its wave's step, and the reverse
    while len(pairs) % 8:
        pairs.append(dict(EMPTY))
    pairs += [pair(rng, 512, 512, -1, err=0.3)] + [dict(EMPTY)] * 7
    pairs += [dict(EMPTY)] * 3 + [pair(rng, 511, 512, 3, err=0.3)] + [dict(EMPTY)] * 4
    pairs.append(pair(rng, 150, 150, -30))        # (the last pair: its lines at the last bytes of both buffers)
    return pairs


def rules_kw(rules):
    return dict(good=rules[0], bad=rules[1], qual_base=rules[2])


class HostTable:
    """both mates' bytes and rows, the insert sizes, and the loop's verdict per pair and rule set (computed once)"""

    def __init__(self, pairs):
        self.pairs, self.n = pairs, len(pairs)
        b1, r1, b2, r2 = build(pairs)
        self.bytes = (b1, b2)
        self.seen = (b"\n" + b1, b2)
        self.coord = (r1, r2)
        self.m = (np.array(r1, dtype=np.int64) + ADD1, np.array(r2, dtype=np.int64) + ADD2)
        self.ins = np.array([p["ins"] for p in pairs], dtype=np.int32)

    @functools.lru_cache(maxsize=None)
    def per_pair(self, rules):
        return [K.pair_correct(self.seen[0], a, True, self.seen[1], b, False, int(i), **rules_kw(rules))
                for a, b, i in zip(self.coord[0], self.coord[1], self.ins)]

    @functools.lru_cache(maxsize=None)
    def expect(self, n, rules):
        """(bytes 1, bytes 2, counts, matrix) behind a call over the first n pairs"""
        per = self.per_pair(rules)[:n]
        s1, s2 = K.apply(self.seen[0], self.coord[0][:n], self.seen[1], self.coord[1][:n], per)
        return (s1[1:], s2) + K.counts_of(per)


def whole(ctx, d):
    out = np.empty(d.size, dtype=np.uint8)
    ctx.d2h(out, d.base)
    return out


def run(ctx, bytes2, m, ins, n, rules, matrix=True):
    """The call over the first n pairs of freshly uploaded buffers, twice.  -> (both whole allocations in front of the first call,
    per call (counts, matrix, both whole allocations behind it)).  The tables and the insert sizes must stand."""
    import torch
    from fastqandfurious_amd import hip
    d = [Dev(ctx, b) for b in bytes2]
    try:
        t = [torch.from_numpy(x.copy()).cuda() for x in m]
        dins = torch.from_numpy(ins.copy()).cuda()
        torch.cuda.synchronize()
        v = (hip.table_view(d[0].ptr, d[0].n, t[0].data_ptr(), True, ADD1), hip.table_view(d[1].ptr, d[1].n, t[1].data_ptr(), False, ADD2))
        before = [whole(ctx, x) for x in d]
        for x, b in zip(before, bytes2):
            assert bytes(x[len(x) - len(b):]) == b
        out = []
        for _ in range(2):
            counts, mat = ctx.table_pair_correct(v[0], v[1], n, dins.data_ptr(), hip.CorrectRulesStruct(*rules), matrix=matrix)
            after = [whole(ctx, x) for x in d]
            out.append((counts, None if mat is None else mat.reshape(-1).tolist(), after))
        for x, want in zip(t, m):
            assert (x.cpu().numpy() == want).all(), "a table was written"
        assert (dins.cpu().numpy() == ins).all()
        return before, out
    finally:
        for x in d:
            x.close()


def same(before, got, want, bytes2, matrix=True):
    """the first call against the loop, the second one idempotent"""
    w1, w2, wcounts, wmatrix = want
    (counts, mat, after), (counts2, mat2, after2) = got
    assert counts == wcounts and counts[0] + counts[5] == wcounts[0] + wcounts[5]
    assert mat == (wmatrix if matrix else None)
    for k, (b, a, a2, w, raw) in enumerate(zip(before, after, after2, (w1, w2), bytes2)):
        pad = len(b) - len(raw)
        assert (a[:pad] == b[:pad]).all(), "mate %d: bytes in front of the buffer were written" % (k + 1)
        bad = np.flatnonzero(a[pad:] != np.frombuffer(w, dtype=np.uint8))
        assert bad.size == 0, "mate %d: %d bytes differ, the first at %d" % (k + 1, bad.size, bad[0])
        assert (a2 == a).all(), "mate %d: the second call changed bytes" % (k + 1)
    assert counts2 == [wcounts[0], 0, 0, 0, wcounts[4] - wcounts[2] - wcounts[3], wcounts[5]]
    assert mat2 == ([0] * 20 if matrix else None)


@pytest.fixture(scope="module")
def hand():
    pairs = hand_pairs()
    assert len(pairs) >= max(SIZES)
    T = HostTable(pairs)
    assert T.coord[1][0][4] == 0 and T.coord[0][0][0] == 1                 # mate 2's first quality line at byte 0
    assert T.coord[0][-1][5] == len(T.seen[0]) and T.coord[1][-1][5] == len(T.seen[1])
    return T


@pytest.mark.parametrize("rules", RULES)
def test_the_hand_table_holds_every_kind(hand, rules):
    """what the tests below rely on, said by the loop itself"""
    per = hand.per_pair(rules)
    G, B = rules[2] + rules[0], rules[2] + rules[1]
    kinds, at = set(), set()
    for p, c in zip(hand.pairs, per):
        n1, n2, o = len(p["a"]), len(p["b"]), p["ins"] - len(p["b"])
        should = p["flavour"] in ("",) + HEADERS and p["ins"] >= 0 and -n2 < o < n1
        assert (c is not None) == should, (p["flavour"], n1, n2, p["ins"])
        if c is None:
            continue
        kinds.add("one_right" if o == n1 - 1 else "one_left" if o == -(n2 - 1) else "zero" if o == 0 else "other")
        kinds |= {"mate1"} if c[4] else set()
        kinds |= {"mate2"} if c[5] else set()
        kinds |= {"stay"} if c[6] > c[4] + c[5] else set()
        kinds |= {"clean"} if c[6] == 0 and min(n1, n2 + o) - max(0, o) >= 16 else set()
        if p["flavour"] in HEADERS:
            kinds.add(p["flavour"])
        # a correction whose two qualities sit exactly at the thresholds, on either side, and a refusal one off
        for pos in range(max(0, o), min(n1, n2 + o)):
            qa, qb = p["qa"][pos], p["qb"][n2 - 1 - (pos - o)]
            for x, y, side in ((qa, qb, 2), (qb, qa, 1)):
                if c[0][pos] != p["a"][pos] or c[2][n2 - 1 - (pos - o)] != p["b"][n2 - 1 - (pos - o)]:
                    if x == G and y <= B:
                        at.add(("G", side))
                    if x >= G and y == B:
                        at.add(("B", side))
                elif K.CLS.get(p["a"][pos], 4) < 4 and K.CLS.get(p["b"][n2 - 1 - (pos - o)], 4) < 4 and \
                        K.CLS[p["a"][pos]] != 3 - K.CLS[p["b"][n2 - 1 - (pos - o)]]:
                    if x == G - 1 and y <= B:
                        at.add(("G-1", side))
                    if x >= G and y == B + 1:
                        at.add(("B+1", side))
    assert per[0] is not None and per[-1] is not None
    assert kinds == {"one_right", "one_left", "zero", "other", "mate1", "mate2", "stay", "clean"} | set(HEADERS)
    assert at == {(e, s) for e in ("G", "B", "G-1", "B+1") for s in (1, 2)}, at
    counts, matrix = K.counts_of(per)
    assert counts[0] > 400 and counts[5] > 20 and counts[1] > 100 and counts[2] > 200 and counts[3] > 200
    m = np.array(matrix).reshape(5, 4)
    assert m[4].sum() > 0 and (m[:4].sum(axis=1) > 0).all() and (m.sum(axis=0) > 0).all(), "N and '.' replaced, every base both ways"
    assert all(m[i][i] == 0 for i in range(4)), "a base is never corrected to its own class: that would have been a match"
    assert any(x >= 0x80 for p in hand.pairs for x in p["qa"] + p["qb"])
    assert {len(p["a"]) for p, c in zip(hand.pairs, per) if c} >= set(LENS) <= {len(p["b"]) for p, c in zip(hand.pairs, per) if c}


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_pair_counts(gpu_ctx, hand, n):
    rules = RULES[n % 2]
    before, got = run(gpu_ctx, hand.bytes, hand.m, hand.ins, n, rules)
    same(before, got, hand.expect(n, rules), hand.bytes)


@pytest.mark.gpu
@pytest.mark.parametrize("rules", RULES)
def test_whole_table(gpu_ctx, hand, rules):
    want = hand.expect(hand.n, rules)
    before, got = run(gpu_ctx, hand.bytes, hand.m, hand.ins, hand.n, rules)
    same(before, got, want, hand.bytes)
    assert want[2][2] > 0 and want[2][3] > 0 and want[0] != hand.bytes[0] and want[1] != hand.bytes[1]


@pytest.mark.gpu
def test_without_the_matrix(gpu_ctx, hand):
    before, got = run(gpu_ctx, hand.bytes, hand.m, hand.ins, hand.n, RULES[0], matrix=False)
    same(before, got, hand.expect(hand.n, RULES[0]), hand.bytes, matrix=False)


@pytest.mark.gpu
def test_argument_errors(gpu_ctx, hand):
    import ctypes
    import torch
    from fastqandfurious_amd import hip
    n = 4
    d = [Dev(gpu_ctx, x) for x in hand.bytes]
    try:
        t = [torch.from_numpy(x.copy()).cuda() for x in hand.m]
        dins = torch.from_numpy(hand.ins.copy()).cuda()
        torch.cuda.synchronize()
        v1 = hip.table_view(d[0].ptr, d[0].n, t[0].data_ptr(), True, ADD1)
        v2 = hip.table_view(d[1].ptr, d[1].n, t[1].data_ptr(), False, ADD2)

        def call(a=v1, b=v2, ins=dins.data_ptr(), rules=(30, 14, 33), pairs=n):
            counts = (ctypes.c_int64 * 6)()
            r = hip.CorrectRulesStruct(*rules) if rules is not None else None
            rc = hip.lib().ffq_table_pair_correct(gpu_ctx.handle, ctypes.byref(a), ctypes.byref(b), pairs, ctypes.c_void_p(ins),
                                                  None if r is None else ctypes.byref(r), counts, None)
            return rc, list(counts)
        rc, counts = call()
        assert rc == 0 and counts[0] + counts[5] == n
        assert call(pairs=0, ins=None) == (0, [0] * 6)
        bad = [dict(ins=None), dict(ins=dins.data_ptr() + 2), dict(rules=None), dict(rules=(14, 14, 33)), dict(rules=(30, -1, 33)),
               dict(rules=(30, 14, 226)), dict(rules=(30, 14, -1)), dict(pairs=-1),
               dict(a=hip.table_view(0, d[0].n, t[0].data_ptr(), True, ADD1)), dict(b=hip.table_view(0, d[1].n, t[1].data_ptr(), False, ADD2)),
               dict(a=hip.table_view(d[0].ptr, d[0].n, t[0].data_ptr() + 8, True, ADD1)),
               dict(b=hip.table_view(d[1].ptr, d[1].n, t[1].data_ptr() + 8, False, ADD2))]
        for kw in bad:
            assert call(**kw)[0] == hip.E_ARG, kw
        assert call(rules=(30, 14, 225))[0] == 0
        # a scan pending on the context
        data = b"@r\nACGT\n+\nIIII\n" * 50
        dd = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
        tt = torch.empty((64, 6), dtype=torch.int64, device="cuda")
        gpu_ctx.scan_submit(dd.data_ptr(), len(data), tt.data_ptr(), 64)
        try:
            assert call()[0] == hip.E_ARG
        finally:
            gpu_ctx.scan_wait()
        assert call()[0] == 0
    finally:
        for x in d:
            x.close()


# ---- more pairs than one pass of the grid (tests/grid_expect.py) -------------------------------------------------------------
# The pass edits bytes, so a table expanded from a pool must not repeat ROWS: the buffers are the concatenation of the pool
# pairs' own texts, pool_text[idx], the rows are offset accordingly, and the expected buffers are pool_after[idx].
SHORT_LENS = (1, 15, 16, 17, 31, 32, 33, 40)
GRID_RULES = RULES[0]


class Pool:
    """pairs of about 40 bases, each built on its own: its two texts, its rows relative to them, what the loop makes of it"""

    def __init__(self):
        rng = np.random.default_rng(37)
        pairs = []
        k = 0
        for n1 in SHORT_LENS:
            for n2 in SHORT_LENS:
                for o in alignments(n1, n2):
                    pairs.append(pair(rng, n1, n2, o, h=b"h" * (1 + k % 9), qm=QMS[k % 6], alphabet=ALPHABETS[k % 4], err=(0.15, 0.02, 0.5)[(k // 6) % 3]))
                    k += 1
        pairs += [pair(rng, 40, 40, -5, flavour=f) for f in ("outside1", "outside2", "negative1", "negative2", "unequal1", "unequal2")]
        pairs += [pair(rng, 33, 33, ins=-1), pair(rng, 33, 33, ins=-2), pair(rng, 33, 31, ins=64), pair(rng, 33, 33, ins=(1 << 31) - 1)]
        pairs += [dict(EMPTY)] * 2
        self.pairs, self.n = pairs, len(pairs)
        self.text, self.after, self.rel, nums = ([], []), ([], []), ([], []), []
        for p in pairs:
            b1, r1, b2, r2 = build([p])
            c = K.pair_correct(b"\n" + b1, r1[0], True, b2, r2[0], False, p["ins"], **rules_kw(GRID_RULES))
            a1, a2 = K.apply(b"\n" + b1, r1, b2, r2, [c])
            self.text[0].append(b1)
            self.text[1].append(b2)
            self.after[0].append(a1[1:])
            self.after[1].append(a2)
            self.rel[0].append(r1[0])                 # (mate 1: coordinates behind the sentinel, 1 = the text's first byte)
            self.rel[1].append(r2[0])
            nums.append([0, 0, 0, 0, 0, 1] + [0] * 20 if c is None else [1, 1 if c[4] + c[5] else 0, c[4], c[5], c[6], 0] + c[7])
        self.nums = np.array(nums, dtype=np.int64)
        self.ins = np.array([p["ins"] for p in pairs], dtype=np.int32)
        self.idle = [i for i, p in enumerate(pairs) if p["ins"] == -1]
        self.len = tuple(np.array([len(x) for x in t], dtype=np.int64) for t in self.text)
        self.rel = tuple(np.array(r, dtype=np.int64) for r in self.rel)

    def table(self, idx):
        """(bytes 1, bytes 2), (rows 1, rows 2) as the tables hold them, insert sizes, (expected bytes), counts, matrix"""
        raw = tuple(b"".join([t[i] for i in idx.tolist()]) for t in self.text)
        want = tuple(b"".join([t[i] for i in idx.tolist()]) for t in self.after)
        off = tuple(np.concatenate([[0], np.cumsum(ln[idx])[:-1]]) for ln in self.len)
        m = (self.rel[0][idx] + off[0][:, None] + ADD1, self.rel[1][idx] + off[1][:, None] + ADD2)
        s = self.nums[idx].sum(axis=0).tolist()
        return raw, m, self.ins[idx], want, s[:6], s[6:]


@functools.lru_cache(maxsize=None)
def pool():
    return Pool()


def grid_idx(arrangement):
    P = pool()
    return GE.table_idx(arrangement, GE.n_above(GE.P_SHORT), GE.P_SHORT, P.n, P.idle, seed=89)


@pytest.mark.parametrize("arrangement", GE.ARRANGEMENTS)
def test_the_pairs_above_one_pass_are_what_the_loop_says(arrangement):
    """the expanded table's expectation is the pool's: checked by the loop itself on sampled pairs of the big buffers"""
    P = pool()
    n = GE.n_above(GE.P_SHORT)
    assert n > 2 * 2048 * 32 and P.n < 400 and len(P.idle) >= 1
    idx = grid_idx(arrangement)
    raw, m, ins, want, counts, matrix = P.table(idx)
    assert len(raw[0]) < 64 << 20 and len(raw[1]) < 64 << 20 and counts[0] + counts[5] == n
    seen = (b"\n" + raw[0], raw[1])
    got = [bytearray(seen[0]), bytearray(seen[1])]
    for k in GE.sample_rows(n, GE.P_SHORT).tolist():
        r1, r2 = (m[0][k] - ADD1).tolist(), (m[1][k] - ADD2).tolist()
        c = K.pair_correct(seen[0], r1, True, seen[1], r2, False, int(ins[k]), **rules_kw(GRID_RULES))
        assert (c is None) == (P.nums[idx[k]][5] == 1)
        if c is not None:
            assert [1, 1 if c[4] + c[5] else 0, c[4], c[5], c[6], 0] + c[7] == P.nums[idx[k]].tolist()
            for s, r, lines in ((0, r1, c[:2]), (1, r2, c[2:4])):
                assert bytes(np.frombuffer(want[s], dtype=np.uint8)[r[2] - (1 - s):r[3] - (1 - s)]) == lines[0]
                assert bytes(np.frombuffer(want[s], dtype=np.uint8)[r[4] - (1 - s):r[5] - (1 - s)]) == lines[1]
    for k, s in enumerate(GE.passes(n, GE.P_SHORT)):
        c = P.nums[idx[s]].sum(axis=0)
        if (arrangement, k > 0) in (("late work", False), ("early work", True)):
            assert c[:5].sum() == 0 and c[5] == s.stop - s.start
        else:
            assert all(x > 0 for x in c[:6]), (k, c)


@pytest.mark.gpu
def test_more_pairs_than_one_pass_of_the_grid(gpu_ctx):
    """three steps of every workgroup of k_pair_correct, the last one for 1001 of the 2048 with five pairs for the last of those:
    every byte of both buffers, the six counts, the matrix; idempotent"""
    P = pool()
    for arrangement in GE.ARRANGEMENTS:
        idx = grid_idx(arrangement)
        n = len(idx)
        assert n > 2 * GE.P_SHORT
        raw, m, ins, want, counts, matrix = P.table(idx)
        before, got = run(gpu_ctx, raw, m, ins, n, GRID_RULES)
        for k in range(2):
            a = got[0][2][k]
            bad = np.flatnonzero(a[len(a) - len(raw[k]):] != np.frombuffer(want[k], dtype=np.uint8))
            if bad.size:
                off = np.concatenate([[0], np.cumsum(P.len[k][idx])])
                r = int(np.searchsorted(off, bad[0], side="right") - 1)
                raise AssertionError("%s: mate %d: %d bytes differ, the first in pair %d, pass %d" % (arrangement, k + 1, bad.size, r, r // GE.P_SHORT))
        same(before, got, want + (counts, matrix), raw)

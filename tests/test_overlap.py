"""The overlap of the mates of a pair on the device: ffq_table_pair_overlap on hand-made tables.

The expectation of every test is the plain loop of tests/overlap_expect.py -- the rule of include/ffq.h written out byte by
byte -- never the package's own pair_overlap.  Every comparison is exact: both output tables, d_insert, d_hist, the six
counts.  The two mates always live in different buffers with different `add`, mate 1 with a sentinel and mate 2 without.
"""
import ctypes
import functools

import numpy as np
import pytest

import grid_expect as GE
import overlap_expect as X


ADD1, ADD2 = 1000, -5                 # mate 1: sentinel, add 1000; mate 2: no sentinel, add -5
SIZES = (0, 1, 2, 31, 32, 33, 257)    # group and workgroup edges for 8 lanes per pair, 32 pairs per workgroup
RULESETS = {"default": X.DEFAULT, "short": (20, 5, 200), "strict": (12, 0, 0), "loose": (30, 40, 100)}


# ---- the hand table ----------------------------------------------------------------------------------------------------------
def flip(s, at):
    s = bytearray(s)
    for i in at:
        s[i] = b"ACGT"[(b"ACGT".index(bytes([s[i]]).upper()) + 1) % 4]
    return bytes(s)


def hand_pairs():
    """[(sequence 1, sequence 2, flavour)]; flavour: "" or what makes the pair not analysed"""
    rng = np.random.default_rng(3)
    pairs = [(b"", b"", ""), (b"", X.mates_of(rng, 100, 150, 150)[1], ""), (X.mates_of(rng, 100, 150, 150)[0], b"", "")]
    # lengths around min_overlap (30, and 20 / 12 of the other rule sets), word edges of the packing, 150, 511 / 512; fragments
    # shorter than the reads (cut), equal, between (an overlap, not cut), longer than both (none), shorter than min_overlap
    for n in (11, 12, 13, 19, 20, 21, 29, 30, 31, 15, 16, 17, 32, 33, 47, 48, 49, 150, 511, 512):
        for frag in (n - 7, n - 1, n, n + 1, n + 9, 2 * n - 16, 2 * n + 5, 14):
            if frag >= 1:
                pairs.append(X.mates_of(rng, frag, n, n) + ("",))
    for n1, n2 in ((150, 100), (100, 150), (40, 31), (31, 40), (512, 30), (30, 512), (33, 16), (17, 150)):
        for frag in (25, 35, 90, 120, 200, 600):
            pairs.append(X.mates_of(rng, frag, n1, n2) + ("",))
    # above FFQ_OVERLAP_MAX_LEN: not analysed, either mate
    pairs += [X.mates_of(rng, 100, 513, 150) + ("long",), X.mates_of(rng, 100, 150, 513) + ("long",), X.mates_of(rng, 600, 513, 513) + ("long",)]
    # mismatches at and one above max_diff (overlap 100: the permille bound is 20), at and one above the permille bound where it is
    # the smaller (overlap 20 under "short": 4; overlap 30 under "default": 6 > max_diff, so 5 / 6)
    for frag, bads in ((100, (5, 6)), (20, (3, 4, 5)), (30, (5, 6)), (12, (0, 1))):
        s1, s2 = X.mates_of(rng, frag, 150, 150)
        for bad in bads:
            pairs.append((flip(s1, [1 + 2 * i for i in range(bad)]), s2, ""))
            pairs.append((s1, flip(s2, [1 + 2 * i for i in range(bad)]), ""))
    # an N in one mate, an N in both at the same place (still a mismatch), lower case (matches)
    s1, s2 = X.mates_of(rng, 60, 100, 100)
    for k in range(1, 8):
        a, b = bytearray(s1), bytearray(s2)
        for i in range(k):
            a[5 + 7 * i] = ord("N")
            b[59 - (5 + 7 * i)] = ord("n" if i & 1 else "N")
        pairs += [(bytes(a), bytes(b), ""), (bytes(a), s2, ""), (s1, bytes(b), "")]
    pairs += [(s1.lower(), s2, ""), (s1, s2.lower(), ""), (s1.lower(), s2.lower(), ""), (s1.replace(b"A", b"."), s2, "")]
    # order: every candidate qualifies -> o* = 0, nothing is cut; a tandem repeat where positive and negative candidates qualify
    pairs += [(b"A" * 150, b"T" * 150, ""), (b"a" * 150, b"T" * 97, ""), (b"ACGTACGTAC" * 6, X.revcomp(b"ACGTACGTAC" * 5), ""),
              (b"AC" * 40, X.revcomp(b"AC" * 30), ""), (b"AC" * 30, X.revcomp(b"AC" * 40), "")]
    # not analysed: a wrapped sequence in either mate, a FASTA row, rows pointing outside, lines of two lengths
    w1, w2 = X.mates_of(rng, 100, 150, 150)
    wrapped1, wrapped2 = w1[:70] + b"\n" + w1[70:], w2[:149] + b"\n" + w2[149:]
    pairs += [(wrapped1, w2, "wrapped"), (w1, wrapped2, "wrapped"), (w1, w2, "fasta1"), (w1, w2, "fasta2"), (w1, w2, "outside1"),
              (w1, w2, "outside2"), (w1, w2, "negative1"), (w1, w2, "unequal1"), (w1, w2, "unequal2")]
    # 64 such pairs in front of a real one (whole waves without work, then one group with work), and -- at a multiple of eight -- a
    # 512-base pair without an overlap beside seven empty ones in its wave
    while len(pairs) % 8:
        pairs.append((b"", b"", ""))
    pairs += [(w1, w2, ("fasta1", "outside2", "wrapped0", "unequal2")[i % 4]) for i in range(64)] + [(w1, w2, "")]
    while len(pairs) % 8:
        pairs.append((b"", b"", ""))
    pairs += [(X.mates_of(rng, 1200, 512, 512) + ("",))] + [(b"", b"", "")] * 7
    pairs += [(b"", b"", "")] * 3 + [X.mates_of(rng, 1300, 512, 511) + ("",)] + [(b"", b"", "")] * 4
    return pairs


def build_mate(pairs, k, first, last):
    """(bytes, rows in positions of the bytes) of mate k: first's sequence at the buffer's first byte, last's at its last"""
    buf, rows = bytearray(), []

    def put(i, seq, flavour, newline=True):
        seq = seq if not flavour.startswith("wrapped0") else seq[:50] + b"\n" + seq[51:]
        p2 = len(buf)
        buf.extend(seq + (b"\n" if newline else b""))
        n = len(seq)
        # the quality line is never read: it lies anywhere inside the buffer, here over the sequence itself
        row = [7 * i, 7 * i + 3, p2, p2 + n, p2, p2 + n]
        if flavour == "fasta%d" % (k + 1):
            row[4] = row[5] = None
        elif flavour == "outside%d" % (k + 1):
            row[3] = row[5] = p2 + (1 << 40)
        elif flavour == "negative%d" % (k + 1):
            row[2], row[4] = -(1 << 30), -(1 << 30)
        elif flavour == "unequal%d" % (k + 1) and n:
            row[5] -= 1
        return row
    rows = [None] * len(pairs)
    rows[first] = put(first, pairs[first][k], pairs[first][2])
    for i, p in enumerate(pairs):
        if i not in (first, last):
            if i % 5 == 0:
                buf.extend(b"@junk %d\n" % i)
            rows[i] = put(i, p[k], p[2])
    rows[last] = put(last, pairs[last][k], pairs[last][2], newline=False)
    return bytes(buf), rows


class HostTable:
    """both mates' bytes and rows, and the loop's verdict per pair and rule set (computed when first asked for)"""

    def __init__(self, pairs, first, last):
        self.pairs = pairs
        b1, r1 = build_mate(pairs, 0, first[0], last[0])
        b2, r2 = build_mate(pairs, 1, first[1], last[1])
        self.bytes = (b1, b2)
        # coordinates of the buffer as the scanner saw it: mate 1 has its sentinel in front
        self.seen = (b"\n" + b1, b2)
        c1 = [[None if x is None else x + 1 for x in r] for r in r1]
        self.coord = ([[-1 - ADD1 if x is None else x for x in r] for r in c1], [[-100 - ADD2 if x is None else x for x in r] for r in r2])
        self.m = (np.array(self.coord[0], dtype=np.int64) + ADD1, np.array(self.coord[1], dtype=np.int64) + ADD2)
        self.n = len(pairs)

    @functools.lru_cache(maxsize=None)
    def per_pair(self, rules, trim):
        return X.expect_table(self.seen[0], self.coord[0], True, self.seen[1], self.coord[1], False, rules, trim)

    def expect(self, n, rules, trim):
        return X.summarize(self.per_pair(rules, trim)[:n], self.m[0][:n], self.m[1][:n])


class Table(HostTable):
    """... and both mates on the device"""

    def __init__(self, ctx, pairs, first, last):
        import torch
        from fastqandfurious_amd import hip
        HostTable.__init__(self, pairs, first, last)
        b1, b2 = self.bytes
        self.d = (Dev(ctx, b1), Dev(ctx, b2))
        self.t = tuple(torch.from_numpy(m.copy()).cuda() for m in self.m)
        torch.cuda.synchronize()
        self.v = (hip.table_view(self.d[0].ptr, self.d[0].n, self.t[0].data_ptr(), True, ADD1),
                  hip.table_view(self.d[1].ptr, self.d[1].n, self.t[1].data_ptr(), False, ADD2))

    def close(self):
        for d in self.d:
            d.close()


class Dev:
    """bytes at the END of a device allocation of whole pages: a read past them leaves the allocation"""

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


def rules_struct(rules, trim):
    from fastqandfurious_amd import hip
    return hip.OverlapRulesStruct(rules[0], rules[1], rules[2], 1 if trim else 0)


def run(ctx, T, n, rules, trim, in_place=False, insert=True, hist=True, accumulate=False, prefill=None):
    """-> (rows 1, rows 2, inserts, hist, counts) as they stand behind the call"""
    import torch
    if in_place:
        o1, o2 = T.t[0].clone(), T.t[1].clone()
        v = tuple(type(x)(x.d_buf, x.n_bytes, x.sentinel, x.add, o.data_ptr()) for x, o in zip(T.v, (o1, o2)))
    else:
        o1 = torch.full((n + 1, 6), -7, dtype=torch.int64, device="cuda")
        o2 = torch.full((n + 1, 6), -7, dtype=torch.int64, device="cuda")
        v = T.v
    di = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    dh = torch.from_numpy((np.full(X.HIST_WORDS + 1, 99, dtype=np.int64) if prefill is None else np.append(prefill.astype(np.int64), 99))).cuda()
    torch.cuda.synchronize()
    counts = ctx.table_pair_overlap(v[0], v[1], n, rules_struct(rules, trim), o1.data_ptr(), o2.data_ptr(), di.data_ptr() if insert else None,
                                    dh.data_ptr() if hist else None, accumulate)
    r1, r2, gi, gh = o1.cpu().numpy(), o2.cpu().numpy(), di.cpu().numpy(), dh.cpu().numpy()
    if in_place:
        assert (r1[n:] == T.m[0][n:]).all() and (r2[n:] == T.m[1][n:]).all(), "rows behind the call's were written"
    else:
        assert (r1[n:] == -7).all() and (r2[n:] == -7).all(), "rows behind the call's were written"
    assert (gi[n if insert else 0:] == -7).all() and gh[-1] == 99
    assert counts[0] + counts[5] == n
    return r1[:n], r2[:n], gi[:n], gh[:-1].astype(np.uint64), counts


def same(got, want, insert=True, hist=True):
    r1, r2, gi, gh, counts = got
    w1, w2, wi, wh, wcounts = want
    assert counts == wcounts
    assert (r1 == w1).all() and (r2 == w2).all()
    if insert:
        assert (gi == wi).all(), np.flatnonzero(gi != wi)[:8]
    if hist:
        assert (gh == wh).all()


def hand_layout(pairs):
    """(first, last) of the hand table: a 150-base pair at the buffer's first byte of either mate, one at its last"""
    plain = [i for i, p in enumerate(pairs) if p[2] == "" and len(p[0]) == len(p[1]) == 150]
    return (plain[0], plain[1]), (plain[2], plain[3])


@pytest.fixture(scope="module")
def hand(gpu_ctx):
    pairs = hand_pairs()
    assert len(pairs) >= max(SIZES)
    by = {p[2] for p in pairs}
    assert {"", "long", "wrapped", "wrapped0", "fasta1", "fasta2", "outside1", "outside2", "negative1", "unequal1", "unequal2"} <= by
    plain = [i for i, p in enumerate(pairs) if p[2] == "" and len(p[0]) == len(p[1]) == 150]
    T = Table(gpu_ctx, pairs, *hand_layout(pairs))
    assert T.coord[0][plain[0]][2] == 1 and T.coord[1][plain[1]][2] == 0
    assert T.coord[0][plain[2]][3] == len(T.seen[0]) and T.coord[1][plain[3]][3] == len(T.seen[1])
    yield T
    T.close()


@pytest.mark.gpu
def test_the_hand_table_holds_every_kind(hand):
    """what the tests below rely on"""
    per = hand.per_pair(X.DEFAULT, True)
    kinds = {"not analysed" if i == -2 else "none" if i == -1 else "cut" if c1 is not None else "kept" for i, c1, _ in per}
    assert kinds == {"not analysed", "none", "cut", "kept"}
    for i, p in enumerate(hand.pairs):
        assert (per[i][0] == -2) == (p[2] != ""), (i, p[2])
    # a cut that shortens mate 1 only by less than mate 2, and both directions of n1 != n2 among the cut pairs
    cuts = [(len(p[0]), len(p[1]), per[i]) for i, p in enumerate(hand.pairs) if per[i][1] is not None]
    assert any(n1 > n2 for n1, n2, _ in cuts) and any(n1 < n2 for n1, n2, _ in cuts)
    # the bounds: exactly at and one above, under the rule set where each bound is the smaller
    assert len({x[0] for x in per}) > 20
    # order: all A against all T is o* = 0
    i = hand.pairs.index((b"A" * 150, b"T" * 150, ""))
    assert per[i] == (150, None, None)
    # the tandem repeats: an overlap is found at o* >= 0 although a negative candidate qualifies as well
    i = hand.pairs.index((b"AC" * 40, X.revcomp(b"AC" * 30), ""))
    assert per[i] == (60, None, None)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_pair_counts(gpu_ctx, hand, n):
    same(run(gpu_ctx, hand, n, X.DEFAULT, True), hand.expect(n, X.DEFAULT, True))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RULESETS))
def test_whole_table_under_every_rule_set(gpu_ctx, hand, name):
    rules = RULESETS[name]
    want = hand.expect(hand.n, rules, True)
    assert want[4][1] > 0 and want[4][2] > 0 and want[4][5] > 64
    got = run(gpu_ctx, hand, hand.n, rules, True)
    same(got, want)
    # in place gives the same rows
    same(run(gpu_ctx, hand, hand.n, rules, True, in_place=True), want)


@pytest.mark.gpu
def test_bounds_exactly_at_and_one_above(hand):
    """the loop itself says that the hand table's mismatch pairs sit on either side of both bounds"""
    base = [i for i, p in enumerate(hand.pairs) if p[2] == "" and len(p[0]) == len(p[1]) == 150]
    per_d, per_s, per_t = (hand.per_pair(RULESETS[k], True) for k in ("default", "short", "strict"))
    # "default": a 100-base overlap takes 5 changed bases (in either mate) and not 6 -- max_diff; the third is the pair behind the 64
    assert sum(per_d[i][0] == 100 for i in base) == 3
    # "short": a 20-base overlap takes 3 and 4 (20 * 200 / 1000, the smaller bound there) and not 5
    assert sum(per_s[i][0] == 20 for i in base) == 4
    # "strict": a 12-base overlap takes none (the pair is there twice unchanged, twice with one changed base)
    assert sum(per_t[i][0] == 12 for i in base) == 2


@pytest.mark.gpu
def test_analyse_only_leaves_every_row(gpu_ctx, hand):
    """trim = 0: rows copied unchanged (out of place) or untouched (in place), d_insert and d_hist filled all the same"""
    want = hand.expect(hand.n, X.DEFAULT, False)
    assert want[4][2:5] == [0, 0, 0] and (want[0] == hand.m[0]).all() and (want[1] == hand.m[1]).all()
    cut = hand.expect(hand.n, X.DEFAULT, True)
    assert (want[2] == cut[2]).all() and (want[3] == cut[3]).all()
    same(run(gpu_ctx, hand, hand.n, X.DEFAULT, False), want)
    same(run(gpu_ctx, hand, hand.n, X.DEFAULT, False, in_place=True), want)


@pytest.mark.gpu
def test_optional_outputs_and_accumulate(gpu_ctx, hand):
    n = 200
    want = hand.expect(n, X.DEFAULT, True)
    same(run(gpu_ctx, hand, n, X.DEFAULT, True, insert=False), want, insert=False)
    got = run(gpu_ctx, hand, n, X.DEFAULT, True, hist=False)
    same(got, want, hist=False)
    assert (got[3] == 99).all()                       # no histogram asked for: none written
    # accumulate = 0 overwrites whatever was there (run() prefills with 99); accumulate = 1 adds
    pre = (np.arange(X.HIST_WORDS, dtype=np.uint64) * 3) % 11
    got = run(gpu_ctx, hand, n, X.DEFAULT, True, accumulate=True, prefill=pre)
    assert (got[3] == pre + want[3]).all()
    got = run(gpu_ctx, hand, n, X.DEFAULT, True, accumulate=True, prefill=got[3])
    assert (got[3] == pre + 2 * want[3]).all()
    # no pair: the histogram is zeroed or left
    got = run(gpu_ctx, hand, 0, X.DEFAULT, True)
    assert not got[3].any() and got[4] == [0] * 6
    got = run(gpu_ctx, hand, 0, X.DEFAULT, True, accumulate=True, prefill=pre)
    assert (got[3] == pre).all()


# ---- a seeded mixed table ----------------------------------------------------------------------------------------------------
def mixed_pairs(n=513, seed=17):
    rng = np.random.default_rng(seed)
    pairs = []
    for i in range(n):
        kind = int(rng.integers(0, 12))
        n1, n2 = int(rng.integers(30, 301)), int(rng.integers(30, 301))
        if kind < 7:
            s1, s2 = X.mates_of(rng, int(rng.integers(10, 500)), n1, n2, 0.03)
            if kind == 0:
                s1 = s1.lower()
            if kind == 1:
                s1, s2 = bytearray(s1), bytearray(s2)
                s1[int(rng.integers(0, n1))] = ord("N")
                s2[int(rng.integers(0, n2))] = ord("N")
                s1, s2 = bytes(s1), bytes(s2)
            pairs.append((s1, s2, ""))
        elif kind < 9:
            pairs.append((X.mates_of(rng, 700, n1, n2)[0], X.mates_of(rng, 700, n1, n2)[1], ""))
        elif kind == 9:
            pairs.append((b"", b"", "") if rng.integers(0, 2) else X.mates_of(rng, 20, n1, n2) + ("",))
        else:
            s1, s2 = X.mates_of(rng, 100, n1, n2)
            pairs.append((s1, s2, ("wrapped0", "fasta1", "fasta2", "outside1", "unequal2", "negative1")[int(rng.integers(0, 6))]))
    return pairs


@pytest.mark.gpu
def test_seeded_mixed_table(gpu_ctx):
    pairs = mixed_pairs()
    assert len(pairs) == 513
    T = Table(gpu_ctx, pairs, (0, 1), (2, 3))
    try:
        for name in ("default", "short"):
            rules = RULESETS[name]
            per = T.per_pair(rules, True)
            # the table holds at least one pair of each kind -- or the comparison below would say little
            kinds = {"not analysed" if i == -2 else "none" if i == -1 else "cut" if c1 is not None else "kept" for i, c1, _ in per}
            assert kinds == {"not analysed", "none", "cut", "kept"}
            want = T.expect(T.n, rules, True)
            assert all(c > 0 for c in want[4])
            same(run(gpu_ctx, T, T.n, rules, True), want)
            same(run(gpu_ctx, T, T.n, rules, True, in_place=True), want)
    finally:
        T.close()


# ---- more pairs than one pass of the grid (tests/grid_expect.py) -----------------------------------------------------------------
# A group of eight lanes takes pair i, then pair i + P_GRID, in the same four LDS planes: only the planes' guard words are cleared,
# once, so every pair behind a group's first finds its predecessor's words behind its own.  The pool is the hand table.
P_GRID = GE.P_SHORT


@functools.lru_cache(maxsize=None)
def pool():
    pairs = hand_pairs()
    return HostTable(pairs, *hand_layout(pairs))


def idle_pairs(H):
    """pool pairs with nothing to do: not analysed, or without a base"""
    return [i for i, p in enumerate(H.pairs) if p[2] != "" or not (p[0] or p[1])]


@functools.lru_cache(maxsize=None)
def pool_parts(H, rules, trim):
    """the loop's answer for every pool pair ALONE: (rows of mate 1 out, of mate 2, insert, the six counts, kind)"""
    per = H.per_pair(rules, trim)
    o1, o2, ins, _hist, _counts = X.summarize(per, H.m[0], H.m[1])
    counts = np.array([X.summarize(per[i:i + 1], H.m[0][i:i + 1], H.m[1][i:i + 1])[4] for i in range(H.n)], dtype=np.int64)
    kinds = np.array(["not analysed" if i == -2 else "none" if i == -1 else "cut" if c1 is not None else "kept" for i, c1, _ in per])
    return o1, o2, ins, counts, kinds


def expand(parts, idx):
    """what a call over pool[idx] gives, as X.summarize states it"""
    o1, o2, ins, counts, _kinds = parts
    gi = ins[idx]
    hist = np.bincount(gi[gi >= 0], minlength=X.HIST_WORDS).astype(np.uint64)
    return o1[idx], o2[idx], gi, hist, counts[idx].sum(axis=0).tolist()


def used_plane_pairs(H, parts, idx):
    """per pass behind the first: the pairs that are cut and shorter, in both mates, than the pair that had their group's planes
    before them -- what is left in the planes reaches beyond their own words"""
    n1, n2 = (np.array([len(p[k]) if p[2] == "" else 0 for p in H.pairs]) for k in (0, 1))
    cut = parts[3][:, 2] > 0
    i = np.arange(P_GRID, len(idx))
    ok = cut[idx[i]] & (n1[idx[i]] < n1[idx[i - P_GRID]]) & (n2[idx[i]] < n2[idx[i - P_GRID]])
    return [int(ok[i // P_GRID == k].sum()) for k in range(1, (len(idx) + P_GRID - 1) // P_GRID)]


class Expanded:
    """pool[idx] as run() takes it: the pool's buffers on the device, a table of its own"""

    def __init__(self, T, idx):
        import torch
        self.m = (T.m[0][idx], T.m[1][idx])
        self.t = tuple(torch.from_numpy(m.copy()).cuda() for m in self.m)
        torch.cuda.synchronize()
        self.v = tuple(type(x)(x.d_buf, x.n_bytes, x.sentinel, x.add, t.data_ptr()) for x, t in zip(T.v, self.t))
        self.n = len(idx)


def same_above(got, want):
    for g, w, what in zip(got[:3], want[:3], ("mate 1's rows", "mate 2's rows", "insert sizes")):
        GE.same_rows(g, w, P_GRID, what)
    assert (got[3] == want[3]).all(), ("histogram", np.flatnonzero(got[3] != want[3])[:8])
    assert got[4] == want[4]


@pytest.mark.parametrize("arrangement", GE.ARRANGEMENTS)
def test_the_table_above_one_pass_is_what_the_loop_says(arrangement):
    """the expansion through idx against the plain loop on 2000 of the table's pairs; what every pass holds"""
    H, rules = pool(), X.DEFAULT
    n = GE.n_above(P_GRID)
    assert n > 2 * 2048 * 32 and H.n <= 512
    parts = pool_parts(H, rules, True)
    idle = idle_pairs(H)
    assert (parts[3][idle][:, 1:5] == 0).all() and {"cut", "kept", "none"} <= set(parts[4][[i for i in range(H.n) if i not in idle]])
    idx = GE.table_idx(arrangement, n, P_GRID, H.n, idle, seed=23)
    rows = GE.sample_rows(n, P_GRID)
    assert len(rows) >= 2000 and {0, P_GRID - 1, P_GRID, 2 * P_GRID - 1, 2 * P_GRID, n - 1} <= set(rows.tolist())
    j = idx[rows]
    per = X.expect_table(H.seen[0], [H.coord[0][k] for k in j], True, H.seen[1], [H.coord[1][k] for k in j], False, rules, True)
    same_above(X.summarize(per, H.m[0][j], H.m[1][j]), expand(parts, j))
    for k, s in enumerate(GE.passes(n, P_GRID)):
        counts, kinds = parts[3][idx[s]].sum(axis=0), set(parts[4][idx[s]])
        if (arrangement, k > 0) in (("late work", False), ("early work", True)):
            assert not counts[1:5].any() and kinds <= {"not analysed", "none"} and counts[0] > 0 and counts[5] > 0
        else:
            assert (counts > 0).all() and kinds == {"not analysed", "none", "cut", "kept"}, (k, counts)
            # mates of very different lengths, and overlaps that end at the last base of mate 1
            here = sorted(set(idx[s].tolist()))
            assert {(512, 30), (30, 512)} <= {(len(H.pairs[i][0]), len(H.pairs[i][1])) for i in here}
            assert any(parts[4][i] == "kept" and parts[2][i] >= len(H.pairs[i][0]) > 0 for i in here)
    if arrangement == "random":
        assert all(c > 100 for c in used_plane_pairs(H, parts, idx)), used_plane_pairs(H, parts, idx)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RULESETS))
def test_more_pairs_than_one_pass_of_the_grid(gpu_ctx, hand, name):
    """three steps of every workgroup, the last for 1001 of the 2048 and five pairs for the last of those: every pair's rows and
    insert size, the histogram and the six counts, out of place and in place, in the three arrangements"""
    rules = RULESETS[name]
    n = GE.n_above(P_GRID)
    assert n > 2 * 2048 * 32
    parts = pool_parts(hand, rules, True)
    for arrangement in GE.ARRANGEMENTS:
        idx = GE.table_idx(arrangement, n, P_GRID, hand.n, idle_pairs(hand), seed=23)
        if arrangement == "random":
            # passes 2 and 3 each hold pairs that are cut on planes a longer pair has used
            used = used_plane_pairs(hand, parts, idx)
            assert len(used) == 2 and all(c > 0 for c in used), used
        want = expand(parts, idx)
        T = Expanded(hand, idx)
        same_above(run(gpu_ctx, T, n, rules, True), want)
        same_above(run(gpu_ctx, T, n, rules, True, in_place=True), want)


# ---- arguments -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors(gpu_ctx, hand):
    import torch
    from fastqandfurious_amd import hip
    n = 4
    out1 = torch.zeros((n + 1, 6), dtype=torch.int64, device="cuda")
    out2 = torch.zeros((n + 1, 6), dtype=torch.int64, device="cuda")
    dh = torch.zeros(X.HIST_WORDS + 1, dtype=torch.int64, device="cuda")
    di = torch.zeros(n + 2, dtype=torch.int32, device="cuda")
    v1, v2, t1, t2, d1, d2 = hand.v[0], hand.v[1], hand.t[0], hand.t[1], hand.d[0], hand.d[1]
    ok = hip.OverlapRulesStruct(30, 5, 200, 1)

    def call(a=v1, b=v2, r=ok, o1=out1.data_ptr(), o2=out2.data_ptr(), h=dh.data_ptr(), ins=di.data_ptr()):
        counts = (ctypes.c_int64 * 6)()
        rc = hip.lib().ffq_table_pair_overlap(gpu_ctx.handle, ctypes.byref(a), ctypes.byref(b), n, None if r is None else ctypes.byref(r),
                                              ctypes.c_void_p(o1), ctypes.c_void_p(o2), ctypes.c_void_p(ins), ctypes.c_void_p(h), 0, counts)
        return rc, list(counts)
    rc, counts = call()
    assert rc == 0 and counts[0] + counts[5] == n
    S = hip.OverlapRulesStruct
    bad = [dict(r=None), dict(r=S(0, 5, 200, 1)), dict(r=S(513, 5, 200, 1)), dict(r=S(30, -1, 200, 1)), dict(r=S(30, 513, 200, 1)),
           dict(r=S(30, 5, -1, 1)), dict(r=S(30, 5, 1001, 1)), dict(r=S(30, 5, 200, 2)), dict(r=S(30, 5, 200, -1)),
           dict(a=hip.table_view(0, d1.n, t1.data_ptr(), True, ADD1)), dict(b=hip.table_view(0, d2.n, t2.data_ptr(), False, ADD2)),   # NULL buffers
           dict(a=hip.table_view(d1.ptr, d1.n, t1.data_ptr() + 8, True, ADD1)), dict(b=hip.table_view(d2.ptr, d2.n, t2.data_ptr() + 8, False, ADD2)),
           dict(o1=out1.data_ptr() + 8), dict(o2=out2.data_ptr() + 8), dict(h=dh.data_ptr() + 4), dict(ins=di.data_ptr() + 2)]
    for kw in bad:
        rc, _ = call(**kw)
        assert rc == hip.E_ARG, kw
    # the extremes of every range are taken
    for r in (S(1, 0, 0, 0), S(512, 512, 1000, 1)):
        assert call(r=r)[0] == 0
    # the Python layer raises
    with pytest.raises(hip.FFQError) as ei:
        gpu_ctx.table_pair_overlap(v1, v2, n, S(0, 5, 200, 1), out1.data_ptr(), out2.data_ptr())
    assert ei.value.code == hip.E_ARG
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

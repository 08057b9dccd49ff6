"""The two mates of a pair merged into one read on the device: ffq_table_pair_merge on hand-made tables.

The expectation of every test is the plain loop of tests/merge_expect.py -- the rule of include/ffq.h written out byte by
byte -- never the package's own merge_mates.  Every comparison is exact: d_text (and the pre-filled bytes behind the total),
d_off, both rest tables, d_rest_ord, n_rest, the six counts.  The two mates live in different buffers with different `add`,
mate 1 with a sentinel and mate 2 without; mate 2's first quality line lies at the first byte of its buffer, the last pair's
lines at the last bytes of theirs (test_overlap.Dev puts a buffer at the END of its allocation).
"""
import functools

import numpy as np
import pytest

import grid_expect as GE
import merge_expect as M
import overlap_expect as X
from test_overlap import Dev


ADD1, ADD2 = 1000, -5                 # mate 1: sentinel, add 1000; mate 2: no sentinel, add -5
SIZES = (0, 1, 2, 31, 32, 33, 257)    # group and workgroup edges: 8 lanes per pair, 32 pairs per step, 256 per workgroup
LENS = (1, 2, 15, 16, 17, 31, 32, 33, 150, 511, 512)
FILL = 0xEE


# ---- the hand table ----------------------------------------------------------------------------------------------------------
def seq_of(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def qual_of(rng, n, mode):
    if mode == "tie":
        return b"I" * n
    if mode == "low":
        return bytes((rng.integers(35, 40, n)).astype(np.uint8))
    if mode == "high":
        return bytes((rng.integers(60, 65, n)).astype(np.uint8))
    if mode == "wide":                # any byte but "\n", 0x80 and above among them
        v = rng.integers(0, 255, n)
        return bytes(np.where(v >= 10, v + 1, v).astype(np.uint8))
    return bytes((rng.integers(60, 64, n)).astype(np.uint8))          # "band": ties are frequent


def pair(rng, n1, n2, o=None, ins=None, flavour="", h=None, qm=("band", "band"), alphabet=b"ACGT"):
    """a pair as a dict; ins: what d_insert holds for it (default: n2 + o)"""
    return dict(h=(b"r%d" % rng.integers(0, 10 ** 6)) if h is None else h, a=seq_of(rng, n1, alphabet), qa=qual_of(rng, n1, qm[0]),
                b=seq_of(rng, n2, alphabet), qb=qual_of(rng, n2, qm[1]), ins=(n2 + o) if ins is None else ins, flavour=flavour)


def alignments(n1, n2):
    """the o that every length pair is tried with: overlaps of one position at either end, 0, mate 2 sticking out in front with
    n1 < L, mate 2 inside mate 1 (n2 + o < n1), one in the middle"""
    out = {n1 - 1, -(n2 - 1), 0}
    if n2 >= 3:
        out.add(-1 if n2 - 1 > n1 else -(n2 - 1) // 2)
    if n1 - n2 >= 2:
        out.add(1)
    out.add((n1 - n2) // 2)
    return sorted(x for x in out if -n2 < x < n1)


def hand_pairs():
    rng = np.random.default_rng(23)
    empty = dict(h=b"e", a=b"", qa=b"", b=b"", qb=b"", ins=-1, flavour="")
    pairs = [pair(rng, 150, 150, -30)]            # (pair 0: mate 2's quality line at the first byte of its buffer)
    # every length with every length, every alignment of alignments(); headers of 1..17 bytes in turn
    k = 0
    for n1 in LENS:
        for n2 in LENS:
            for o in alignments(n1, n2):
                qm = (("band", "band"), ("tie", "tie"), ("low", "high"), ("high", "low"), ("wide", "wide"), ("band", "wide"))[k % 6]
                al = (b"ACGT", b"ACGTacgt", b"ACGTN.", b"acgtn")[k % 4]
                pairs.append(pair(rng, n1, n2, o, h=b"h" * (1 + k % 17), qm=qm, alphabet=al))
                k += 1
    pairs.append(pair(rng, 150, 140, 20, h=bytes(rng.integers(33, 127, 5000).astype(np.uint8))))
    # pairs that must not merge
    pairs += [pair(rng, 150, 150, ins=-1), pair(rng, 150, 150, ins=-2), pair(rng, 150, 150, ins=0), pair(rng, 150, 140, ins=290),
              pair(rng, 150, 140, ins=291), pair(rng, 150, 150, ins=-(1 << 31)), pair(rng, 150, 150, ins=(1 << 31) - 1),
              pair(rng, 513, 150, -10, flavour="long"), pair(rng, 150, 513, 10, flavour="long")]
    pairs += [pair(rng, 150, 150, -20, flavour=f) for f in ("fasta1", "fasta2", "outside1", "outside2", "negative1", "negative2", "unequal1",
                                                              "unequal2", "coord0", "header_neg", "header_empty", "header_out")]
    # 64 unmerged pairs in front of one merged pair, and the reverse
    while len(pairs) % 64:
        pairs.append(dict(empty))
    pairs += [pair(rng, 100, 100, ins=-1) for _ in range(64)] + [pair(rng, 100, 100, -10)]
    while len(pairs) % 64:
        pairs.append(pair(rng, 40, 50, 5, h=b"x" * (1 + len(pairs) % 16)))
    pairs += [pair(rng, 90, 100, -10, h=b"y" * (1 + i % 16)) for i in range(64)] + [pair(rng, 100, 100, ins=-1)]
    # one merged pair among seven empty ones in its wave's step
    while len(pairs) % 8:
        pairs.append(dict(empty))
    pairs += [pair(rng, 512, 512, -1)] + [dict(empty)] * 7
    pairs += [dict(empty)] * 3 + [pair(rng, 511, 512, 3)] + [dict(empty)] * 4
    pairs.append(pair(rng, 150, 150, -30))        # (the last pair: its lines at the last bytes of both buffers)
    return pairs


def build(pairs):
    """(bytes 1, rows 1, bytes 2, rows 2): rows in coordinates of the buffers AS SEEN (mate 1 behind its sentinel)"""
    b1, b2, r1, r2 = bytearray(), bytearray(), [], []
    last = len(pairs) - 1
    for i, p in enumerate(pairs):
        f, n1, n2 = p["flavour"], len(p["a"]), len(p["b"])
        nl = b"" if i == last else b"\n"
        p0 = len(b1) + 1
        b1 += b"@" + p["h"] + b"\n" + p["a"] + b"\n+\n" + p["qa"] + nl
        p1 = p0 + 1 + len(p["h"])
        row = [p0, p1, p1 + 1, p1 + 1 + n1, p1 + 4 + n1, p1 + 4 + 2 * n1]
        if f == "fasta1":
            row[4] = row[5] = -1 - ADD1
        elif f == "outside1":
            row[3] = row[5] = row[2] + (1 << 40)
        elif f == "negative1":
            row[2] = row[4] = -(1 << 30)
        elif f == "unequal1":
            row[5] -= 1
        elif f == "coord0":
            row[2], row[3] = 0, n1
        elif f == "header_neg":
            row[0] = -3
        elif f == "header_empty":
            row[1] = row[0]
        elif f == "header_out":
            row[1] = 1 << 41
        r1.append(row)
        if i == 0:
            q4 = len(b2)
            b2 += p["qb"] + b"\n"
            p0 = len(b2)
            b2 += b"@m2\n" + p["b"] + b"\n"
            row = [p0, p0 + 3, p0 + 4, p0 + 4 + n2, q4, q4 + n2]
        else:
            p0 = len(b2)
            hd = b"@m2 %d" % i
            b2 += hd + b"\n" + p["b"] + b"\n+\n" + p["qb"] + nl
            p1 = p0 + len(hd)
            row = [p0, p1, p1 + 1, p1 + 1 + n2, p1 + 4 + n2, p1 + 4 + 2 * n2]
        if f == "fasta2":
            row[4] = row[5] = -1 - ADD2
        elif f == "outside2":
            row[3] = row[5] = row[2] + (1 << 40)
        elif f == "negative2":
            row[2] = row[4] = -(1 << 30)
        elif f == "unequal2":
            row[5] -= 1
        r2.append(row)
    return bytes(b1), r1, bytes(b2), r2


class HostTable:
    """both mates' bytes and rows, the insert sizes, and the loop's verdict per pair (computed once)"""

    def __init__(self, pairs):
        self.pairs, self.n = pairs, len(pairs)
        b1, r1, b2, r2 = build(pairs)
        self.bytes = (b1, b2)
        self.seen = (b"\n" + b1, b2)
        self.coord = (r1, r2)
        self.m = (np.array(r1, dtype=np.int64) + ADD1, np.array(r2, dtype=np.int64) + ADD2)
        self.ins = np.array([p["ins"] for p in pairs], dtype=np.int32)

    @functools.lru_cache(maxsize=None)
    def per_pair(self):
        return [M.merged_text(self.seen[0], a, True, self.seen[1], b, False, int(i)) for a, b, i in zip(self.coord[0], self.coord[1], self.ins)]

    def expect(self, n, ords=None):
        return M.summarize(self.per_pair()[:n], self.m[0][:n], self.m[1][:n], np.arange(n) if ords is None else ords)


class Table(HostTable):
    """... and both mates on the device"""

    def __init__(self, ctx, pairs):
        import torch
        from fastqandfurious_amd import hip
        HostTable.__init__(self, pairs)
        self.d = (Dev(ctx, self.bytes[0]), Dev(ctx, self.bytes[1]))
        self.t = tuple(torch.from_numpy(m.copy()).cuda() for m in self.m)
        self.dins = torch.from_numpy(self.ins.copy()).cuda()
        torch.cuda.synchronize()
        self.v = (hip.table_view(self.d[0].ptr, self.d[0].n, self.t[0].data_ptr(), True, ADD1),
                  hip.table_view(self.d[1].ptr, self.d[1].n, self.t[1].data_ptr(), False, ADD2))

    def close(self):
        for d in self.d:
            d.close()


def run(ctx, T, n, dins=None, dord=None, cap=None, slack=100, off=True, rest_ord=True, v=None):
    """-> (rc, text buffer with its slack, off, rest 1, rest 2, rest ordinals, n_rest, counts) as they stand behind the call"""
    import torch
    need = T.expect(n)[5][2]
    cap = need + slack if cap is None else cap
    text = torch.full((need + slack + 16,), FILL, dtype=torch.uint8, device="cuda")
    doff = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda")
    o1 = torch.full((n + 1, 6), -7, dtype=torch.int64, device="cuda")
    o2 = torch.full((n + 1, 6), -7, dtype=torch.int64, device="cuda")
    ro = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    v = T.v if v is None else v
    rc, n_rest, counts = ctx.table_pair_merge(v[0], v[1], n, (T.dins if dins is None else dins).data_ptr(), text.data_ptr() + 3, cap,
                                              o1.data_ptr(), o2.data_ptr(), d_ord=None if dord is None else dord.data_ptr(),
                                              d_off=doff.data_ptr() if off else None, d_rest_ord=ro.data_ptr() if rest_ord else None)
    return rc, text.cpu().numpy(), doff.cpu().numpy(), o1.cpu().numpy(), o2.cpu().numpy(), ro.cpu().numpy(), n_rest, counts


def same(got, want, n, off=True, rest_ord=True, written=True):
    rc, text, doff, o1, o2, ro, n_rest, counts = got
    wtext, woff, w1, w2, word, wcounts = want
    assert counts == wcounts and counts[0] + counts[1] == n and n_rest == wcounts[1]
    if written:
        assert rc == 0
        assert bytes(text[3:3 + len(wtext)]) == wtext
        assert (text[:3] == FILL).all() and (text[3 + len(wtext):] == FILL).all(), "bytes outside the text were written"
    else:
        assert (text == FILL).all(), "the text was touched"
    if off:
        assert (doff[:n + 1] == woff).all() and doff[n + 1] == -7
    else:
        assert (doff == -7).all()
    k = wcounts[1]
    assert (o1[:k] == w1).all() and (o2[:k] == w2).all() and (o1[k:] == -7).all() and (o2[k:] == -7).all()
    if rest_ord:
        assert (ro[:k] == word).all() and (ro[k:] == -7).all()
    else:
        assert (ro == -7).all()


@pytest.fixture(scope="module")
def hand(gpu_ctx):
    pairs = hand_pairs()
    assert len(pairs) >= max(SIZES)
    T = Table(gpu_ctx, pairs)
    assert T.coord[1][0][4] == 0 and T.coord[0][0][0] == 1                 # mate 2's first quality line at byte 0
    assert T.coord[0][-1][5] == len(T.seen[0]) and T.coord[1][-1][5] == len(T.seen[1])
    yield T
    T.close()


@pytest.mark.gpu
def test_the_hand_table_holds_every_kind(hand):
    """what the tests below rely on, said by the loop itself"""
    per = hand.per_pair()
    for p, m in zip(hand.pairs, per):
        n1, n2, o = len(p["a"]), len(p["b"]), p["ins"] - len(p["b"])
        should = p["flavour"] == "" and p["ins"] >= 0 and -n2 < o < n1
        assert (m is not None) == should, (p["flavour"], n1, n2, p["ins"])
    assert per[0] is not None and per[-1] is not None
    want = hand.expect(hand.n)
    off, counts = want[1], want[5]
    merged = [k for k, m in enumerate(per) if m is not None]
    assert {int(off[k]) % 16 for k in merged} == set(range(16)), "merged records begin at every shift"
    assert counts[0] > 500 and counts[1] > 100 and 0 < counts[5] < counts[4]
    kinds = set()
    for k in merged:
        p = hand.pairs[k]
        n1, n2 = len(p["a"]), len(p["b"])
        o = p["ins"] - n2
        L = len(per[k][0]) - 6 - len(p["h"])
        assert L % 2 == 0
        L //= 2
        kinds.add("one_right" if o == n1 - 1 else "one_left" if o == -(n2 - 1) else "zero" if o == 0 else "other")
        if o < 0 and n1 < L:
            kinds.add("neg_longer")
        if o >= 0 and n2 + o < n1:
            kinds.add("inside")
        if n1 != n2:
            kinds.add("unequal_lengths")
        if len(p["h"]) == 5000:
            kinds.add("long_header")
        if any(x >= 0x80 for x in p["qa"] + p["qb"]):
            kinds.add("high_bytes")
    assert kinds == {"one_right", "one_left", "zero", "other", "neg_longer", "inside", "unequal_lengths", "long_header", "high_bytes"}
    assert {len(hand.pairs[k]["h"]) for k in merged} >= {1, 14, 15, 16, 17, 5000}
    assert {len(hand.pairs[k]["a"]) for k in merged} >= set(LENS) <= {len(hand.pairs[k]["b"]) for k in merged}


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_pair_counts(gpu_ctx, hand, n):
    same(run(gpu_ctx, hand, n), hand.expect(n), n)


@pytest.mark.gpu
def test_whole_table(gpu_ctx, hand):
    want = hand.expect(hand.n)
    same(run(gpu_ctx, hand, hand.n), want, hand.n)
    # without the optional outputs
    same(run(gpu_ctx, hand, hand.n, off=False, rest_ord=False), want, hand.n, off=False, rest_ord=False)
    # a capacity that is exactly the need
    same(run(gpu_ctx, hand, hand.n, cap=want[5][2], slack=0), want, hand.n)


@pytest.mark.gpu
def test_text_one_byte_short(gpu_ctx, hand):
    """FFQ_E_TABLE_FULL: counts[2] is the need, the offsets and the rest tables are written, the text is not touched"""
    from fastqandfurious_amd import hip
    for n in (33, hand.n):
        want = hand.expect(n)
        got = run(gpu_ctx, hand, n, cap=want[5][2] - 1)
        assert got[0] == hip.E_TABLE_FULL
        same(got, want, n, written=False)


# ---- more pairs than one pass of the grid (tests/grid_expect.py) -------------------------------------------------------------
SHORT_LENS = (1, 2, 15, 16, 17, 31, 32, 33)


@functools.lru_cache(maxsize=None)
def grid_pairs():
    """a pool of short pairs, so that 601 095 of them merge into less than 64 MiB: every length of SHORT_LENS with every other in
    every alignment, a few pairs of 150 bases, pairs that must not merge of every flavour, empty pairs"""
    rng = np.random.default_rng(29)
    pairs = [pair(rng, 33, 33, -7)]
    k = 0
    for n1 in SHORT_LENS:
        for n2 in SHORT_LENS:
            for o in alignments(n1, n2):
                qm = (("band", "band"), ("tie", "tie"), ("low", "high"), ("high", "low"), ("wide", "wide"), ("band", "wide"))[k % 6]
                pairs.append(pair(rng, n1, n2, o, h=b"h" * (1 + k % 17), qm=qm, alphabet=(b"ACGT", b"ACGTacgt", b"ACGTN.", b"acgtn")[k % 4]))
                k += 1
    pairs += [pair(rng, 150, 150 - i, 3 * i - 20) for i in range(10)]
    pairs += [pair(rng, 33, 33, ins=-1), pair(rng, 33, 33, ins=-2), pair(rng, 33, 33, ins=0), pair(rng, 33, 31, ins=64), pair(rng, 33, 31, ins=65),
              pair(rng, 33, 33, ins=-(1 << 31)), pair(rng, 33, 33, ins=(1 << 31) - 1), pair(rng, 513, 33, -10, flavour="long")]
    pairs += [pair(rng, 40, 40, -5, flavour=f) for f in ("fasta1", "fasta2", "outside1", "outside2", "negative1", "negative2", "unequal1",
                                                          "unequal2", "coord0", "header_neg", "header_empty", "header_out")]
    pairs += [dict(h=b"e", a=b"", qa=b"", b=b"", qb=b"", ins=-1, flavour="")] * 4
    pairs.append(pair(rng, 33, 33, -7))
    return pairs


@functools.lru_cache(maxsize=None)
def grid_host():
    return HostTable(grid_pairs())


def grid_idx(H, arrangement):
    idle = [i for i, m in enumerate(H.per_pair()) if m is None]
    return GE.table_idx(arrangement, GE.n_above(GE.P_WIDE), GE.P_WIDE, H.n, idle, seed=83)


def grid_want(H, idx):
    """M.summarize's answer for pool[idx] with the identity for d_ord"""
    per = H.per_pair()
    texts = [m[0] if m is not None else b"" for m in per]
    nums = np.array([[1, 0, len(m[0]), m[1], m[2], m[3]] if m is not None else [0, 1, 0, 0, 0, 0] for m in per], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(nums[idx, 2])])
    keep = np.flatnonzero(nums[idx, 1] == 1)
    return b"".join([texts[i] for i in idx.tolist()]), off, H.m[0][idx][keep], H.m[1][idx][keep], keep, nums[idx].sum(axis=0).tolist()


class Expanded:
    """pool[idx] as run() takes it: the pool's buffers on the device, tables and insert sizes of its own"""

    def __init__(self, T, idx, want):
        import torch
        self.t = (torch.from_numpy(T.m[0][idx]).cuda(), torch.from_numpy(T.m[1][idx]).cuda())
        self.dins = torch.from_numpy(T.ins[idx]).cuda()
        torch.cuda.synchronize()
        self.v = tuple(type(x)(x.d_buf, x.n_bytes, x.sentinel, x.add, t.data_ptr()) for x, t in zip(T.v, self.t))
        self.want = want

    def expect(self, n):
        return self.want


def same_above(got, want, n, P, what, written=True):
    rc, text, doff, o1, o2, ro, n_rest, counts = got
    wtext, woff, w1, w2, word, wcounts = want
    GE.same_rows(doff[:n + 1], woff, P, what + ": offsets")
    k = wcounts[1]
    GE.same_kept(ro[:n_rest], word, P, what + ": the pairs that are not merged")
    GE.same_rows(o1[:k], w1, P, what + ": mate 1's rest (row: among the rest)")
    GE.same_rows(o2[:k], w2, P, what + ": mate 2's rest (row: among the rest)")
    if written:
        bad = np.flatnonzero(text[3:3 + len(wtext)] != np.frombuffer(wtext, dtype=np.uint8))
        if bad.size:
            r = int(np.searchsorted(woff, bad[0], side="right") - 1)
            raise AssertionError("%s: first difference at text byte %d: pair %d, pass %d" % (what, bad[0], r, r // P))
    same(got, want, n, written=written)


@pytest.mark.parametrize("arrangement", GE.ARRANGEMENTS)
def test_the_pairs_above_one_pass_are_what_the_loop_says(arrangement):
    H = grid_host()
    n, P = GE.n_above(GE.P_WIDE), GE.P_WIDE
    assert n > 2048 * 256 and H.n < 400
    idx = grid_idx(H, arrangement)
    want = grid_want(H, idx)
    assert len(want[0]) == want[5][2] < 64 << 20 and want[5][0] + want[5][1] == n
    at = GE.sample_rows(n, P)
    j = idx[at]
    per = [M.merged_text(H.seen[0], H.coord[0][k], True, H.seen[1], H.coord[1][k], False, int(H.ins[k])) for k in j.tolist()]
    loop, mine = M.summarize(per, H.m[0][j], H.m[1][j], np.arange(len(j))), grid_want(H, j)
    assert len(at) >= 2000 and loop[0] == mine[0] and loop[5] == mine[5] and all((a == b).all() for a, b in zip(loop[1:5], mine[1:5]))
    flavours = {p["flavour"] for p in H.pairs}
    for k, s in enumerate(GE.passes(n, P)):
        c = grid_want(H, idx[s])[5]
        here = {H.pairs[i]["flavour"] for i in set(idx[s].tolist())}
        if (arrangement, k > 0) in (("late work", False), ("early work", True)):
            assert c[0] == 0 and c[2:] == [0] * 4 and c[1] == s.stop - s.start
        else:
            assert all(x > 0 for x in c) and here == flavours and len(flavours) == 14, (k, c)
            lens = {(len(H.pairs[i]["a"]), len(H.pairs[i]["b"])) for i in set(idx[s].tolist())}
            assert {(0, 0), (1, 1), (33, 1), (1, 33), (150, 150)} <= lens


@pytest.mark.gpu
def test_more_pairs_than_one_pass_of_the_grid(gpu_ctx):
    """two steps of every workgroup of k_merge_sum and the kernels behind it, the second for 301 of the 2048 with seven pairs for
    the last of those: every byte of the text, every offset, both rest tables, the rest ordinals and the six counts; and a text
    one byte short: the need reported, nothing written, the offsets and the rest all the same"""
    from fastqandfurious_amd import hip
    H = grid_host()
    T = Table(gpu_ctx, H.pairs)
    try:
        for arrangement in GE.ARRANGEMENTS:
            idx = grid_idx(H, arrangement)
            n = len(idx)
            assert n > 2048 * 256
            want = grid_want(H, idx)
            E = Expanded(T, idx, want)
            same_above(run(gpu_ctx, E, n), want, n, GE.P_WIDE, arrangement)
            if arrangement == "random":
                got = run(gpu_ctx, E, n, cap=want[5][2] - 1)
                assert got[0] == hip.E_TABLE_FULL
                same_above(got, want, n, GE.P_WIDE, arrangement + ", one byte short", written=False)
    finally:
        T.close()


@pytest.mark.gpu
def test_ordinals_into_a_larger_insert_array(gpu_ctx, hand):
    """d_ord: a non-monotone map; pair k's insert size is d_insert[d_ord[k]], and d_rest_ord holds d_ord[k]"""
    import torch
    n = hand.n
    rng = np.random.default_rng(5)
    ords = rng.permutation(2 * n + 7)[:n].astype(np.int64)
    assert (np.diff(ords) < 0).any() and (np.diff(ords) > 0).any()
    big = np.full(2 * n + 7, 77, dtype=np.int32)
    big[ords] = hand.ins
    dins, dord = torch.from_numpy(big).cuda(), torch.from_numpy(ords).cuda()
    torch.cuda.synchronize()
    same(run(gpu_ctx, hand, n, dins=dins, dord=dord), hand.expect(n, ords), n)
    same(run(gpu_ctx, hand, 33, dins=dins, dord=dord), hand.expect(33, ords[:33]), 33)


@pytest.mark.gpu
def test_trim_or_not_the_text_is_the_same(gpu_ctx):
    """ffq_table_pair_overlap with trim 1 and with trim 0, each followed by the merge with the insert sizes it wrote: o is
    taken against the current length of mate 2, so the cut changes nothing"""
    import torch
    from fastqandfurious_amd import hip
    rng = np.random.default_rng(41)
    pairs = []
    for i in range(300):
        n1, n2 = int(rng.integers(40, 200)), int(rng.integers(40, 200))
        s1, s2 = X.mates_of(rng, int(rng.integers(20, 420)), n1, n2, 0.02)
        p = pair(rng, n1, n2, 0, h=b"t%d" % i, qm=("band", "wide") if i % 2 else ("band", "band"))
        p["a"], p["b"], p["ins"] = s1, s2, -7
        pairs.append(p)
    T = Table(gpu_ctx, pairs)
    try:
        texts = []
        for trim in (1, 0):
            o1, o2 = torch.empty_like(T.t[0]), torch.empty_like(T.t[1])
            dins = torch.full((T.n,), -9, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            oc = gpu_ctx.table_pair_overlap(T.v[0], T.v[1], T.n, hip.OverlapRulesStruct(30, 5, 200, trim), o1.data_ptr(), o2.data_ptr(),
                                            d_insert=dins.data_ptr())
            assert oc[1] > 100 and (oc[2] > 50) == bool(trim)
            v = tuple(type(x)(x.d_buf, x.n_bytes, x.sentinel, x.add, o.data_ptr()) for x, o in zip(T.v, (o1, o2)))
            ins = dins.cpu().numpy()
            rows = (o1.cpu().numpy() - ADD1, o2.cpu().numpy() - ADD2)
            per = [M.merged_text(T.seen[0], list(a), True, T.seen[1], list(b), False, int(i)) for a, b, i in zip(rows[0], rows[1], ins)]
            want = M.summarize(per, rows[0] + ADD1, rows[1] + ADD2, np.arange(T.n))
            assert want[5][0] == oc[1] and want[5][5] > 0
            text = torch.full((want[5][2] + 64,), FILL, dtype=torch.uint8, device="cuda")
            r1, r2 = torch.empty_like(o1), torch.empty_like(o2)
            torch.cuda.synchronize()
            rc, n_rest, counts = gpu_ctx.table_pair_merge(v[0], v[1], T.n, dins.data_ptr(), text.data_ptr(), want[5][2], r1.data_ptr(),
                                                          r2.data_ptr())
            assert rc == 0 and counts == want[5] and n_rest == want[5][1]
            got = text.cpu().numpy()
            assert bytes(got[:want[5][2]]) == want[0] and (got[want[5][2]:] == FILL).all()
            texts.append(want[0])
        assert texts[0] == texts[1] and len(texts[0]) > 10000
    finally:
        T.close()


@pytest.mark.gpu
def test_argument_errors(gpu_ctx, hand):
    import ctypes
    import torch
    from fastqandfurious_amd import hip
    n = 4
    text = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    o1 = torch.zeros((n + 1, 6), dtype=torch.int64, device="cuda")
    o2 = torch.zeros((n + 1, 6), dtype=torch.int64, device="cuda")
    aux = torch.zeros(n + 2, dtype=torch.int64, device="cuda")
    v1, v2, t1, t2, d1, d2 = hand.v[0], hand.v[1], hand.t[0], hand.t[1], hand.d[0], hand.d[1]

    def call(a=v1, b=v2, ins=hand.dins.data_ptr(), ordp=None, off=None, r1=o1.data_ptr(), r2=o2.data_ptr(), ro=None):
        counts = (ctypes.c_int64 * 6)()
        n_rest = ctypes.c_int64()
        rc = hip.lib().ffq_table_pair_merge(gpu_ctx.handle, ctypes.byref(a), ctypes.byref(b), n, ctypes.c_void_p(ins), ctypes.c_void_p(ordp),
                                            ctypes.c_void_p(text.data_ptr()), 4096, ctypes.c_void_p(off), ctypes.c_void_p(r1), ctypes.c_void_p(r2),
                                            ctypes.c_void_p(ro), ctypes.byref(n_rest), counts)
        return rc, list(counts)
    rc, counts = call()
    assert rc == 0 and counts[0] + counts[1] == n
    bad = [dict(ins=None), dict(ins=hand.dins.data_ptr() + 2), dict(ordp=aux.data_ptr() + 4), dict(off=aux.data_ptr() + 4), dict(ro=aux.data_ptr() + 4),
           dict(a=hip.table_view(0, d1.n, t1.data_ptr(), True, ADD1)), dict(b=hip.table_view(0, d2.n, t2.data_ptr(), False, ADD2)),
           dict(a=hip.table_view(d1.ptr, d1.n, t1.data_ptr() + 8, True, ADD1)), dict(b=hip.table_view(d2.ptr, d2.n, t2.data_ptr() + 8, False, ADD2)),
           dict(r1=o1.data_ptr() + 8), dict(r2=o2.data_ptr() + 8), dict(r1=t1.data_ptr()), dict(r2=t2.data_ptr()), dict(r2=o1.data_ptr())]
    for kw in bad:
        assert call(**kw)[0] == hip.E_ARG, kw
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

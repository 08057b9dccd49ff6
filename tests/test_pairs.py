"""Two tables whose rows are mates: ffq_table_select_pairs and ffq_table_pair_names on the device, on hand-made tables.

The expectation of every test is a plain loop in this file -- the rules of include/ffq.h written out, byte by byte -- never
the package's own Python statement of them.  Every comparison is exact: the kept rows of both tables, d_idx, both
histograms, the five pair counts; the four numbers of the names check.  The two mates always live in different buffers with
different `add`, mate 1 with a sentinel and mate 2 without.
"""
import ctypes
import functools

import numpy as np
import pytest

import grid_expect as GE


EE = [int(np.floor(1e6 * 10.0 ** (-v / 10.0) + 0.5)) for v in range(96)]
RULES = dict(qual_base=33, max_n=1, min_mean_qual=20, qualified_qual=15, max_unqualified_pct=30, min_complexity_pct=30,
             max_ee_micro=1000000)
OFF = dict(qual_base=33, max_n=-1, min_mean_qual=0, qualified_qual=15, max_unqualified_pct=-1, min_complexity_pct=0, max_ee_micro=-1)
SIZES = (0, 1, 2, 255, 256, 257, 513)
MODES = ("any", "both", "first")
ADD1, ADD2 = 1000, -5                 # mate 1: sentinel, add 1000; mate 2: no sentinel, add -5


# ---- the rules, as plain loops -------------------------------------------------------------------------------------------
def content_verdict(seq, q, R):
    n = len(seq)
    nN = sv = u = ee = d = 0
    for i in range(n):
        v = min(max(q[i] - R["qual_base"], 0), 95)
        nN += seq[i] in b"Nn"
        sv += v
        u += v < R["qualified_qual"]
        ee += EE[v]
        d += i < n - 1 and seq[i] != seq[i + 1]
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


def mate_verdicts(seen, rows, R, lo, hi, sentinel):
    """[(verdict, judged)] of every row, each judged alone; seen: the buffer as the scanner saw it (with its sentinel), rows:
    coordinates of it"""
    out = []
    for row in rows:
        p2, p3, p4, p5 = row[2:]
        ok = min(p2, p3, p4, p5) >= 0 and p2 <= p3 <= len(seen) and p4 <= p5 <= len(seen) and p3 - p2 == p5 - p4
        if ok and sentinel and p3 > p2 and (p2 < 1 or p4 < 1):
            ok = False
        if not lo <= row[3] - row[2] <= hi:
            out.append((1, ok))                         # (no byte of the row is read)
            continue
        v, judged = 0, True
        if is_on(R):
            judged = ok and 10 not in seen[p2:p3] and 10 not in seen[p4:p5]
            if judged:
                v = content_verdict(seen[p2:p3], seen[p4:p5], R)
        out.append((v, judged))
    return out


def hist_of(verdicts, on):
    h = [0] * 8
    for v, judged in verdicts:
        h[v] += 1
        h[7] += on and not judged
    return h


def loop_pairs(ver1, ver2, mode, on1, on2):
    """(kept ordinals, hist1, hist2, pairs)"""
    kept, pairs = [], [0] * 5
    for i, ((v1, _), (v2, _)) in enumerate(zip(ver1, ver2)):
        if mode == "first":
            v2 = 0
        drop = (v1 or v2) if mode == "any" else (v1 and v2) if mode == "both" else v1
        pairs[1 if drop else 0] += 1
        if v1 and v2:
            pairs[4] += 1
        elif v1:
            pairs[2] += 1
        elif v2:
            pairs[3] += 1
        if not drop:
            kept.append(i)
    return kept, hist_of(ver1, on1), ([0] * 8 if mode == "first" else hist_of(ver2, on2)), pairs


def loop_id(h):
    for i in range(len(h)):
        if h[i] == 0x20 or h[i] == 0x09:
            h = h[:i]
            break
    if len(h) >= 2 and h[-2:] in (b"/1", b"/2"):
        h = h[:-2]
    return h


def loop_names(seen1, rows1, seen2, rows2):
    """(equal, different, not compared, first different or -1); seen: with the sentinel, rows: coordinates of it"""
    eq = df = nc = 0
    first = -1
    for i, (a, b) in enumerate(zip(rows1, rows2)):
        if not all(r[0] >= 0 and r[0] + 1 <= r[1] <= len(s) for r, s in ((a, seen1), (b, seen2))):
            nc += 1
        elif loop_id(seen1[a[0] + 1:a[1]]) == loop_id(seen2[b[0] + 1:b[1]]):
            eq += 1
        else:
            df += 1
            first = i if first < 0 else first
    return eq, df, nc, first


# ---- the device --------------------------------------------------------------------------------------------------------------
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


def dev_rows(rows):
    import torch
    rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 6)
    t = torch.from_numpy(rows.copy()).cuda() if rows.shape[0] else torch.zeros((1, 6), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return t


def rules_struct(R):
    from fastqandfurious_amd import hip
    return None if R is None else hip.ContentRulesStruct(*(R[name] for name, _ in hip.ContentRulesStruct._fields_))


def select_pairs(ctx, view1, view2, t1, t2, n, R1, R2, lo, hi, mode, idx=True):
    """-> (out1[k], out2[k], idx[k], hist1, hist2, pairs)"""
    import torch
    out1 = torch.full((n + 1, 6), -7, dtype=torch.int64, device="cuda")
    out2 = torch.full((n + 1, 6), -7, dtype=torch.int64, device="cuda")
    di = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    k, h1, h2, pairs = ctx.table_select_pairs(view1, view2, n, out1.data_ptr(), out2.data_ptr(), rules_struct(R1), rules_struct(R2),
                                              lo, hi, mode, di.data_ptr() if idx else None)
    o1, o2, d = out1.cpu().numpy(), out2.cpu().numpy(), di.cpu().numpy()
    assert (o1[k:] == -7).all() and (o2[k:] == -7).all() and (d[k if idx else 0:] == -7).all(), "rows behind the kept ones were written"
    assert pairs[0] == k and pairs[0] + pairs[1] == n
    return o1[:k], o2[:k], d[:k], h1, h2, pairs


# ---- the hand table of ffq_table_select_pairs ----------------------------------------------------------------------------
def acgt(n):
    return (b"ACGT" * (n // 4 + 1))[:n]


def kinds():
    """name -> (sequence, quality, wrapped, fasta); with RULES and the bounds of the test, judged alone:
    mate 1 (1..200): v = 0 but for "empty" (1); mate 2 (0..170): v = 0 but for "l180" (1); and the rules' own reads"""
    def qv(*vs):
        return bytes(33 + v for v in vs)
    k = {}
    k["ok"] = (acgt(40), b"I" * 40)
    k["empty"] = (b"", b"")
    k["one"] = (b"A", b"I")
    k["n"] = (b"ACNNGT" + acgt(34), b"I" * 40)                                       # rule 2
    k["meanq"] = (acgt(40), qv(*([10] * 40)))                                        # rule 3
    k["unq"] = (acgt(40), qv(*([5] * 16 + [40] * 24)))                               # rule 4 (mean 26)
    k["ee"] = (acgt(150), qv(*([20] * 150)))                                         # rule 5 (mean 20, none unqualified, 1.5 errors)
    k["cplx"] = (b"A" * 40, b"I" * 40)                                               # rule 6
    k["l160"] = (acgt(160), b"I" * 160)                                              # the short rows' last length
    k["l161"] = (acgt(161), b"I" * 161)                                              # a wave of its own
    k["l160n"] = (b"NN" + acgt(158), b"I" * 160)                                     # rule 2, short row
    k["l161c"] = (b"C" * 161, b"I" * 161)                                            # rule 6, long row
    k["l180"] = (acgt(180), b"I" * 180)                                              # mate 2: too long
    k["wrapped"] = (acgt(20) + b"\n" + acgt(20), b"I" * 20 + b"\n" + b"I" * 20)      # not judged, kept by its length
    k["fasta"] = (acgt(30), None)                                                    # pos4 = pos5 = -1
    return k


def pair_plan():
    """(kind of mate 1, kind of mate 2) of 513 pairs: every combination, and every class on both sides of the block edge
    at 256 (and of the one at 512)"""
    names = list(kinds())
    plan = [(names[i % len(names)], names[(i // len(names) + i) % len(names)]) for i in range(513)]
    fail = {1: ("empty", "l180"), 2: ("n", "n"), 3: ("meanq", "meanq"), 4: ("unq", "unq"), 5: ("ee", "ee"), 6: ("cplx", "l161c")}
    for r in range(1, 7):
        f1, f2 = fail[r]
        for at, pr in ((255 - 2 * (r - 1), (f1, "ok")), (254 - 2 * (r - 1), ("ok", f2)), (256 + 2 * (r - 1), (f1, "ok")),
                       (257 + 2 * (r - 1), ("l161", f2))):
            plan[at] = pr
    plan[243], plan[268], plan[242], plan[269] = ("n", "cplx"), ("l160n", "ee"), ("ok", "ok"), ("one", "empty")
    plan[510], plan[511], plan[512] = ("cplx", "ok"), ("ok", "meanq"), ("ee", "unq")
    return plan


def build_mate(plan_kinds, junk):
    """(bytes, rows in coordinates of the bytes) of one mate's file"""
    K = kinds()
    buf, rows = bytearray(junk), []
    for i, name in enumerate(plan_kinds):
        seq, qual = K[name]
        p0 = len(buf)
        buf += b"@r%d\n" % i
        p1 = len(buf) - 1
        p2 = len(buf)
        buf += seq + b"\n"
        if qual is None:
            rows.append([p0, p1, p2, p2 + len(seq), -1, -1])
            continue
        buf += b"+\n"
        p4 = len(buf)
        buf += qual + b"\n"
        rows.append([p0, p1, p2, p2 + len(seq), p4, p4 + len(qual)])
    return bytes(buf), np.array(rows, dtype=np.int64).reshape(-1, 6)


BOUNDS = ((1, 0), (200, 170))         # (min of mate 1, of mate 2), (max of mate 1, of mate 2)


@functools.lru_cache(maxsize=None)
def hand_host():
    """both mates' files, their rows as the tables hold them, and every row's verdict by the loop, once"""
    plan = pair_plan()
    b1, r1 = build_mate([p[0] for p in plan], b"")
    b2, r2 = build_mate([p[1] for p in plan], b"##junk##\n")
    # mate 1 has a sentinel: coordinate = position + 1; FASTA rows keep their -1
    c1 = np.where(r1 < 0, r1, r1 + 1)
    m1 = np.where(r1 < 0, r1, c1 + ADD1)
    m2 = np.where(r2 < 0, r2, r2 + ADD2)
    # (a -1 minus add is not a coordinate of the buffer either way: ADD1 > 0 keeps it negative, ADD2 < 0 makes it 4 -- so the
    # FASTA rows of mate 2 are given positions that stay outside)
    m2 = np.where(r2 < 0, -100, m2)
    c2 = np.where(r2 < 0, -100 - ADD2, r2)
    seen1 = b"\n" + b1
    ver = {}
    for name, R in (("rules", RULES), ("off", None)):
        ver[name] = (mate_verdicts(seen1, c1.tolist(), R, BOUNDS[0][0], BOUNDS[1][0], True),
                     mate_verdicts(b2, c2.tolist(), R, BOUNDS[0][1], BOUNDS[1][1], False))
    return dict(b1=b1, b2=b2, c1=c1, c2=c2, m1=m1, m2=m2, ver=ver, plan=plan)


@pytest.fixture(scope="module")
def hand(gpu_ctx):
    """... and both files on the device"""
    from fastqandfurious_amd import hip
    H = dict(hand_host())
    d1, d2 = Dev(gpu_ctx, H["b1"]), Dev(gpu_ctx, H["b2"])
    t1, t2 = dev_rows(H["m1"]), dev_rows(H["m2"])
    v1 = hip.table_view(d1.ptr, d1.n, t1.data_ptr(), True, ADD1)
    v2 = hip.table_view(d2.ptr, d2.n, t2.data_ptr(), False, ADD2)
    H.update(v1=v1, v2=v2, t1=t1, t2=t2, d1=d1, d2=d2)
    yield H
    d1.close()
    d2.close()


@pytest.mark.gpu
def test_the_hand_table_holds_every_class(hand):
    """what the tests below rely on: every rule fires on either side, on both sides of the block edge, and not judged rows exist"""
    ver1, ver2 = hand["ver"]["rules"]
    for ver in (ver1, ver2):
        for lo, hi in ((236, 256), (256, 276)):
            assert {v for v, _ in ver[lo:hi]} >= {0, 1, 2, 3, 4, 5, 6}, (lo, hi)
        assert any(not judged for _, judged in ver)
    classes = {(bool(a[0]), bool(b[0])) for a, b in zip(ver1, ver2)}
    assert len(classes) == 4
    assert {(bool(a[0]), bool(b[0])) for a, b in zip(ver1[240:256], ver2[240:256])} >= {(True, False), (False, True), (True, True), (False, False)}
    assert {(bool(a[0]), bool(b[0])) for a, b in zip(ver1[256:272], ver2[256:272])} >= {(True, False), (False, True), (True, True), (False, False)}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", SIZES)
def test_select_pairs_with_every_rule(gpu_ctx, hand, n, mode):
    ver1, ver2 = hand["ver"]["rules"]
    kept, h1, h2, pairs = loop_pairs(ver1[:n], ver2[:n], mode, True, True)
    o1, o2, idx, g1, g2, gp = select_pairs(gpu_ctx, hand["v1"], hand["v2"], hand["t1"], hand["t2"], n, RULES, RULES, BOUNDS[0], BOUNDS[1], mode)
    assert gp == pairs and g1 == h1 and g2 == h2
    assert idx.tolist() == kept
    assert (o1 == hand["m1"][kept]).all() and (o2 == hand["m2"][kept]).all()
    assert sum(g1[:7]) == n and (mode == "first" or sum(g2[:7]) == n)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_one_mate_with_rules_the_other_by_length(gpu_ctx, hand, mode):
    """rules on mate 2 only (the positions-only kernel judges mate 1), and the other way round; no d_idx"""
    n = 513
    for R1, R2, k1, k2 in ((None, RULES, "off", "rules"), (RULES, OFF, "rules", "off")):
        ver1, ver2 = hand["ver"][k1][0], hand["ver"][k2][1]
        kept, h1, h2, pairs = loop_pairs(ver1, ver2, mode, is_on(R1), is_on(R2))
        o1, o2, _idx, g1, g2, gp = select_pairs(gpu_ctx, hand["v1"], hand["v2"], hand["t1"], hand["t2"], n, R1, R2, BOUNDS[0], BOUNDS[1], mode,
                                                idx=False)
        assert (gp, g1, g2) == (pairs, h1, h2)
        assert (o1 == hand["m1"][kept]).all() and (o2 == hand["m2"][kept]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_length_only_reads_no_buffer(gpu_ctx, hand, mode):
    """no content rule on either side: both d_buf NULL"""
    from fastqandfurious_amd import hip
    n = 513
    v1 = hip.table_view(0, hand["d1"].n, hand["t1"].data_ptr(), True, ADD1)
    v2 = hip.table_view(0, hand["d2"].n, hand["t2"].data_ptr(), False, ADD2)
    ver1, ver2 = hand["ver"]["off"]
    kept, h1, h2, pairs = loop_pairs(ver1, ver2, mode, False, False)
    o1, o2, idx, g1, g2, gp = select_pairs(gpu_ctx, v1, v2, hand["t1"], hand["t2"], n, None, None, BOUNDS[0], BOUNDS[1], mode)
    assert (gp, g1, g2, idx.tolist()) == (pairs, h1, h2, kept)
    assert (o1 == hand["m1"][kept]).all() and (o2 == hand["m2"][kept]).all()
    assert g1[2:] == [0] * 6 and g2[2:] == [0] * 6


@pytest.mark.gpu
def test_more_blocks_than_the_count_kernel_has_workgroups(gpu_ctx):
    """k_pair_len strides over the pairs with at most 2048 workgroups of 256, k_pair_count over the blocks of 256 pairs with at
    most 1024: 2048 * 256 + 300 pairs, judged by their length alone (positions made up, no buffer), so that a workgroup of
    either takes a second block and the last block is a part of one"""
    import torch
    from fastqandfurious_amd import hip
    n = 2048 * 256 + 300
    assert n > GE.P_WIDE
    rng = np.random.default_rng(7)
    len1, len2 = rng.integers(0, 100, n), rng.integers(0, 100, n)
    rows1, rows2 = np.zeros((n, 6), dtype=np.int64), np.zeros((n, 6), dtype=np.int64)
    for rows, ln in ((rows1, len1), (rows2, len2)):
        rows[:, 0] = np.arange(n) * 7
        rows[:, 2] = 1000
        rows[:, 3] = 1000 + ln
    t1, t2 = dev_rows(rows1), dev_rows(rows2)
    v1, v2 = hip.table_view(0, 1 << 20, t1.data_ptr(), True, 0), hip.table_view(0, 1 << 20, t2.data_ptr(), False, 0)
    for mode in MODES:
        f1 = ~((len1 >= 20) & (len1 <= 90))
        f2 = ~((len2 >= 10) & (len2 <= 80)) if mode != "first" else np.zeros(n, dtype=bool)
        drop = (f1 | f2) if mode == "any" else (f1 & f2) if mode == "both" else f1
        kept = np.flatnonzero(~drop)
        pairs = [int((~drop).sum()), int(drop.sum()), int((f1 & ~f2).sum()), int((f2 & ~f1).sum()), int((f1 & f2).sum())]
        o1, o2, idx, g1, g2, gp = select_pairs(gpu_ctx, v1, v2, t1, t2, n, None, None, (20, 10), (90, 80), mode)
        assert gp == pairs
        assert g1[:2] == [int(((len1 >= 20) & (len1 <= 90)).sum()), int(((len1 < 20) | (len1 > 90)).sum())]
        GE.same_kept(idx, kept, GE.P_WIDE, mode)
        assert (idx == np.array(kept)).all() and (o1 == rows1[kept]).all() and (o2 == rows2[kept]).all()


# ---- more pairs than one pass of the grid (tests/grid_expect.py): the pool is the hand table, either mate with an idx of its own
def grid_pairs(H, arrangement):
    """(idx of mate 1, idx of mate 2): both mates idle in the same part of the table"""
    n, P = GE.n_above(GE.P_SHORT), GE.P_SHORT
    out = []
    for k, ver in enumerate(H["ver"]["rules"]):
        idle = [i for i, (v, judged) in enumerate(ver) if v == 1 or not judged]
        out.append(GE.table_idx(arrangement, n, P, len(ver), idle, seed=50 + k))
    return out


def grid_pairs_want(H, idx1, idx2, mode):
    ver1, ver2 = H["ver"]["rules"]
    return loop_pairs([ver1[i] for i in idx1.tolist()], [ver2[i] for i in idx2.tolist()], mode, True, True)


@pytest.mark.parametrize("arrangement", GE.ARRANGEMENTS)
def test_the_pairs_above_one_pass_are_what_the_loop_says(arrangement):
    H = hand_host()
    n, P = GE.n_above(GE.P_SHORT), GE.P_SHORT
    assert n > 2 * 2048 * 32
    idx1, idx2 = grid_pairs(H, arrangement)
    assert len(idx1) == len(idx2) == n and (idx1 != idx2).sum() > n // 2
    at = GE.sample_rows(n, P)
    assert len(at) >= 2000
    # the verdicts of the table's own rows by the loop, against the pool's through idx
    ver1, ver2 = H["ver"]["rules"]
    assert mate_verdicts(b"\n" + H["b1"], H["c1"][idx1[at]].tolist(), RULES, BOUNDS[0][0], BOUNDS[1][0], True) == [ver1[i] for i in idx1[at]]
    assert mate_verdicts(H["b2"], H["c2"][idx2[at]].tolist(), RULES, BOUNDS[0][1], BOUNDS[1][1], False) == [ver2[i] for i in idx2[at]]
    for k, s in enumerate(GE.passes(n, P)):
        kept, h1, h2, pairs = grid_pairs_want(H, idx1[s], idx2[s], "any")
        if (arrangement, k > 0) in (("late work", False), ("early work", True)):
            assert h1[2:7] == [0] * 5 and h2[2:7] == [0] * 5 and h1[7] > 0 and h2[7] > 0 and h1[1] > 0 and h2[1] > 0
        else:
            assert all(x > 0 for x in h1 + h2 + pairs), (k, h1, h2, pairs)
            names = {H["plan"][i][0] for i in idx1[s]} | {H["plan"][i][1] for i in idx2[s]}
            assert names == set(kinds())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_more_pairs_than_one_pass_of_the_grid(gpu_ctx, hand, mode):
    """content rules on both mates: k_filter_rows takes three steps over either table, the last for 1001 of its 2048 workgroups
    with five rows for the last of those; the kept rows of both, d_idx, both histograms, the five pair counts"""
    from fastqandfurious_amd import hip
    P = GE.P_SHORT
    for arrangement in GE.ARRANGEMENTS:
        idx1, idx2 = grid_pairs(hand, arrangement)
        n = len(idx1)
        assert n > 2 * 2048 * 32
        kept, h1, h2, pairs = grid_pairs_want(hand, idx1, idx2, mode)
        m1, m2 = hand["m1"][idx1], hand["m2"][idx2]
        t1, t2 = dev_rows(m1), dev_rows(m2)
        v1 = hip.table_view(hand["d1"].ptr, hand["d1"].n, t1.data_ptr(), True, ADD1)
        v2 = hip.table_view(hand["d2"].ptr, hand["d2"].n, t2.data_ptr(), False, ADD2)
        o1, o2, idx, g1, g2, gp = select_pairs(gpu_ctx, v1, v2, t1, t2, n, RULES, RULES, BOUNDS[0], BOUNDS[1], mode)
        GE.same_kept(idx, kept, P, arrangement)
        assert gp == pairs and g1 == h1 and g2 == h2, (arrangement, gp, pairs, g1, h1, g2, h2)
        GE.same_rows(o1, m1[kept], P, "%s: mate 1's kept rows (row: among the kept)" % arrangement)
        GE.same_rows(o2, m2[kept], P, "%s: mate 2's kept rows (row: among the kept)" % arrangement)


@pytest.mark.gpu
def test_first_reads_nothing_of_mate_2(gpu_ctx, hand):
    """FFQ_PAIR_FIRST with rules on both sides, mate 2's d_buf NULL and a poisoned hist2: it comes back all zero"""
    import torch
    from fastqandfurious_amd import hip
    n = 513
    v2 = hip.table_view(0, hand["d2"].n, hand["t2"].data_ptr(), False, ADD2)
    out1 = torch.full((n, 6), -7, dtype=torch.int64, device="cuda")
    out2 = torch.full((n, 6), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    r = rules_struct(RULES)
    bounds = (ctypes.c_int64 * 4)(BOUNDS[0][0], BOUNDS[1][0], BOUNDS[0][1], BOUNDS[1][1])
    k = ctypes.c_int64(-1)
    h1, h2, pairs = (ctypes.c_int64 * 8)(*[99] * 8), (ctypes.c_int64 * 8)(*[99] * 8), (ctypes.c_int64 * 5)(*[99] * 5)
    rc = hip.lib().ffq_table_select_pairs(gpu_ctx.handle, ctypes.byref(hand["v1"]), ctypes.byref(v2), n, bounds, ctypes.byref(r),
                                          ctypes.byref(r), 2, ctypes.c_void_p(out1.data_ptr()), ctypes.c_void_p(out2.data_ptr()), None,
                                          ctypes.byref(k), h1, h2, pairs)
    assert rc == 0
    ver1, ver2 = hand["ver"]["rules"]
    kept, w1, _w2, wp = loop_pairs(ver1, ver2, "first", True, True)
    assert list(h2) == [0] * 8
    assert list(h1) == w1 and list(pairs) == wp and k.value == len(kept)
    assert wp[3] == wp[4] == 0 and wp[2] == sum(1 for v, _ in ver1 if v)
    assert (out1.cpu().numpy()[:k.value] == hand["m1"][kept]).all() and (out2.cpu().numpy()[:k.value] == hand["m2"][kept]).all()


@pytest.mark.gpu
def test_a_table_paired_with_itself_is_select_reads(gpu_ctx, hand):
    """select_pairs(T, T, ANY) gives the rows and counts ffq_table_select_reads(T) gives"""
    import torch
    n = 513
    out = torch.full((n, 6), -7, dtype=torch.int64, device="cuda")
    di = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    d1 = hand["d1"]
    k, counts = gpu_ctx.table_select_reads(d1.ptr, d1.n, hand["t1"].data_ptr(), n, out.data_ptr(), rules_struct(RULES), 1, 200,
                                           di.data_ptr(), sentinel=True, add=ADD1)
    o1, o2, idx, g1, g2, gp = select_pairs(gpu_ctx, hand["v1"], hand["v1"], hand["t1"], hand["t1"], n, RULES, RULES, (1, 1), (200, 200), "any")
    assert g1 == counts and g2 == counts
    assert gp == [k, n - k, 0, 0, n - k]
    assert idx.tolist() == di.cpu().numpy()[:k].tolist()
    assert (o1 == out.cpu().numpy()[:k]).all() and (o2 == o1).all()


@pytest.mark.gpu
def test_select_pairs_argument_errors(gpu_ctx, hand):
    import torch
    from fastqandfurious_amd import hip
    n = 4
    out1 = torch.zeros((n + 1, 6), dtype=torch.int64, device="cuda")
    out2 = torch.zeros((n + 1, 6), dtype=torch.int64, device="cuda")
    v1, v2, t1, t2 = hand["v1"], hand["v2"], hand["t1"], hand["t2"]

    def call(a=v1, b=v2, R1=RULES, R2=RULES, mode="any", o1=out1.data_ptr(), o2=out2.data_ptr()):
        return gpu_ctx.table_select_pairs(a, b, n, o1, o2, rules_struct(R1), rules_struct(R2), None, None, mode)
    assert call()[3][0] + call()[3][1] == n
    for bad in (dict(mode=3), dict(mode=-1), dict(R2=dict(RULES, min_mean_qual=96)), dict(R1=dict(RULES, max_n=-2)),
                dict(b=hip.table_view(0, hand["d2"].n, t2.data_ptr(), False, ADD2)),                  # NULL buffer under a rule
                dict(a=hip.table_view(0, hand["d1"].n, t1.data_ptr(), True, ADD1), mode="first"),
                dict(o1=t1.data_ptr()), dict(o2=t2.data_ptr()),                                       # d_out is d_table
                dict(o1=out1.data_ptr() + 8),                                                         # alignment
                dict(a=hip.table_view(hand["d1"].ptr, hand["d1"].n, t1.data_ptr() + 8, True, ADD1))):
        with pytest.raises(hip.FFQError) as ei:
            call(**bad)
        assert ei.value.code == hip.E_ARG, bad
    # FIRST does not judge mate 2: its NULL buffer and its rules are nobody's business
    call(b=hip.table_view(0, hand["d2"].n, t2.data_ptr(), False, ADD2), mode="first")


# ---- ffq_table_pair_names ------------------------------------------------------------------------------------------------
ID_LENGTHS = (1, 3, 4, 5, 31, 32, 33, 64, 65, 300)


def make_id(n, salt=0):
    return bytes(65 + (i * 7 + salt) % 26 for i in range(n))


def name_cases():
    """[(header of mate 1, header of mate 2)]"""
    cases = []
    for n in ID_LENGTHS:
        i = make_id(n)
        cases += [(i, i), (i + b"/1", i + b"/2"), (i + b" 1:N:0:ACGT", i + b"\t2:N:0:TTTT"), (i + b"/1 x", i + b"/2")]
        cases += [(i, bytes([i[0] ^ 1]) + i[1:]), (i, i[:-1] + bytes([i[-1] ^ 1])), (i, i + b"x"), (i + b"x y", i + b" y")]
        cases += [(i + b"/1", i + b"/3"), (i + b" same", i + b"/2 other")]
    cases += [(b"/1", b"/2"), (b"/1", b""), (b"/1", b"/"), (b"", b""), (b" a", b"\tb"), (b"a/1/1", b"a/1/2"), (b"a/1/1", b"a/2"), (b"1", b"2"),
              (b"ab", b"ab\x00"), (b"x\x00y z", b"x\x00y")]
    return cases


def build_headers(headers, junk):
    buf, rows = bytearray(junk), []
    for h in headers:
        p0 = len(buf)
        buf += b"@" + h + b"\n"
        rows.append([p0, len(buf) - 1, 0, 0, 0, 0])
    return buf, rows


def names_on_device(ctx, b1, rows1, b2, rows2):
    """rows: positions in the bytes; mate 1 gets its sentinel and ADD1, mate 2 ADD2 -> the four numbers, and the loop's"""
    from fastqandfurious_amd import hip
    c1 = [[r[0] + 1, r[1] + 1] + r[2:] for r in rows1]
    d1, d2 = Dev(ctx, bytes(b1)), Dev(ctx, bytes(b2))
    try:
        t1 = dev_rows(np.array(c1, dtype=np.int64).reshape(-1, 6) + np.array([ADD1, ADD1, 0, 0, 0, 0]))
        t2 = dev_rows(np.array(rows2, dtype=np.int64).reshape(-1, 6) + np.array([ADD2, ADD2, 0, 0, 0, 0]))
        got = ctx.table_pair_names(hip.table_view(d1.ptr, d1.n, t1.data_ptr(), True, ADD1),
                                   hip.table_view(d2.ptr, d2.n, t2.data_ptr(), False, ADD2), len(rows1))
    finally:
        d1.close()
        d2.close()
    return got, loop_names(b"\n" + bytes(b1), c1, bytes(b2), rows2)


@pytest.mark.gpu
def test_the_id_loop_gives_the_hand_values():
    assert loop_id(b"r1/1 comment") == b"r1" and loop_id(b"r1\t/2") == b"r1" and loop_id(b"/1") == b"" and loop_id(b"/") == b"/"
    assert loop_id(b"a/3") == b"a/3" and loop_id(b"") == b"" and loop_id(b" x") == b"" and loop_id(b"a/1/2") == b"a/1"


@pytest.mark.gpu
def test_pair_names_on_every_case(gpu_ctx):
    cases = name_cases()
    b1, rows1 = build_headers([c[0] for c in cases], b"")
    b2, rows2 = build_headers([c[1] for c in cases], b"#\n")
    # a header without a delimiter that ends with the buffer's last byte, on either side
    tail = make_id(33, 5)
    for buf, rows in ((b1, rows1), (b2, rows2)):
        p0 = len(buf)
        buf += b"@" + tail
        rows.append([p0, len(buf), 0, 0, 0, 0])
    got, want = names_on_device(gpu_ctx, b1, rows1, b2, rows2)
    assert got == want
    equal = [loop_id(a) == loop_id(b) for a, b in cases]
    assert want[0] == sum(equal) + 1 and want[1] == len(cases) - sum(equal) and want[2] == 0 and want[3] == equal.index(False)
    # some of them one pair at a time: which pair is wrong shows
    got_each = []
    for a, b in cases[:12] + cases[-10:]:
        h1, r1 = build_headers([a], b"")
        h2, r2 = build_headers([b], b"")
        g, w = names_on_device(gpu_ctx, h1, r1, h2, r2)
        got_each.append((g, w))
    assert all(g == w for g, w in got_each), [i for i, (g, w) in enumerate(got_each) if g != w]


@pytest.mark.gpu
def test_pair_names_one_long_id_in_a_wave_of_short_ones(gpu_ctx):
    """a wave of eight groups: one with a 300-byte id, four with 1-byte ids, three without a row -- the shape a round loop that
    is not uniform over the wave hangs on; and the same with the long id last, and differing in its last byte"""
    long_id = make_id(300, 3)
    for heads1, heads2 in (([long_id, b"a", b"b", b"c", b"d"], [long_id, b"a", b"b", b"c", b"d"]),
                           ([b"a", b"b", b"c", b"d", long_id + b"/1"], [b"a", b"b", b"x", b"d", long_id[:-1] + b"#/2"]),
                           ([long_id], [long_id + b" c"])):
        b1, rows1 = build_headers(heads1, b"")
        b2, rows2 = build_headers(heads2, b"")
        got, want = names_on_device(gpu_ctx, b1, rows1, b2, rows2)
        assert got == want


@pytest.mark.gpu
def test_pair_names_rows_that_are_not_compared_and_the_first_different(gpu_ctx):
    """600 pairs (19 workgroups of 32): different pairs at 77, 300 and 599, and rows that point outside in between"""
    heads = [b"r%d" % i for i in range(600)]
    b1, rows1 = build_headers([h + b"/1" for h in heads], b"")
    b2, rows2 = build_headers([h + b"/2 c" for h in heads], b"")
    for i in (77, 300, 599):
        rows2[i] = list(rows2[(i + 1) % 600])
    n1, n2 = len(b1), len(b2)
    rows1[5][1] = n1 + 3                           # ends behind the buffer
    rows2[6][0] = -1                               # pos0 - add < 0
    rows1[40][1] = rows1[40][0]                    # pos0 + 1 > pos1
    rows2[41] = [-100, -100, 0, 0, 0, 0]
    rows1[500] = [n1 + 10, n1 + 20, 0, 0, 0, 0]
    rows1[300][1] = n1 + 1                         # a different pair that is not compared either
    got, want = names_on_device(gpu_ctx, b1, rows1, b2, rows2)
    assert got == want
    assert want == (600 - 2 - 6, 2, 6, 77)
    from fastqandfurious_amd import hip
    assert gpu_ctx.table_pair_names(hip.table_view(0, 0, 0), hip.table_view(0, 0, 0), 0) == (0, 0, 0, -1)


# ---- more pairs than one pass of the grid: the names --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def names_pool():
    """(bytes 1, rows 1, bytes 2, rows 2, class of every pool pair by the loop: 0 equal, 1 different, 2 not compared): the cases
    of name_cases(), a header that ends with the buffer on either side, and rows that point outside"""
    cases = name_cases()
    b1, rows1 = build_headers([c[0] for c in cases], b"")
    b2, rows2 = build_headers([c[1] for c in cases], b"#\n")
    n1, n2 = len(b1), len(b2)
    for k in range(6):
        rows1.append(list(rows1[3 * k]))
        rows2.append(list(rows2[3 * k]))
    rows1[-6][1] = n1 + 400                         # ends behind the buffer
    rows2[-5][0] = -1 - ADD2 - 7                    # begins in front of it
    rows1[-4][1] = rows1[-4][0]                     # pos0 + 1 > pos1
    rows2[-3] = [-100, -100, 0, 0, 0, 0]
    rows1[-2] = [n1 + 1000, n1 + 1020, 0, 0, 0, 0]
    rows2[-1][1] = n2 + 400
    tail = make_id(33, 5)
    for buf, rows in ((b1, rows1), (b2, rows2)):
        p0 = len(buf)
        buf += b"@" + tail
        rows.append([p0, len(buf), 0, 0, 0, 0])
    c1 = [[r[0] + 1, r[1] + 1] + r[2:] for r in rows1]
    cls = []
    for a, b in zip(c1, rows2):
        eq, df, nc, _first = loop_names(b"\n" + bytes(b1), [a], bytes(b2), [b])
        cls.append(0 if eq else 1 if df else 2)
    return bytes(b1), np.array(c1, dtype=np.int64), bytes(b2), np.array(rows2, dtype=np.int64), np.array(cls)


def names_want(cls, idx):
    """(equal, different, not compared, first different or -1) of pool[idx]"""
    c = cls[idx]
    df = np.flatnonzero(c == 1)
    return int((c == 0).sum()), int(df.size), int((c == 2).sum()), int(df[0]) if df.size else -1


NAMES_PLACES = ("none", "inside pass 1", "first of pass 2", "last row")


def names_tables():
    """[(what, idx)]: the three arrangements, and tables whose ONLY different pair stands at one of three places, or nowhere"""
    cls = names_pool()[4]
    n, P = GE.n_above(GE.P_SHORT), GE.P_SHORT
    out = [(a, GE.table_idx(a, n, P, len(cls), np.flatnonzero(cls == 2), seed=61)) for a in GE.ARRANGEMENTS]
    same = np.flatnonzero(cls != 1)
    base = same[np.random.default_rng(62).integers(0, len(same), n)]
    for what, at in zip(NAMES_PLACES, (None, 40001, P, n - 1)):
        idx = base.copy()
        if at is not None:
            idx[at] = int(np.flatnonzero(cls == 1)[at % int((cls == 1).sum())])
        out.append((what, idx))
    return out


def test_the_names_above_one_pass_are_what_the_loop_says():
    b1, c1, b2, r2, cls = names_pool()
    n, P = GE.n_above(GE.P_SHORT), GE.P_SHORT
    assert n > 2 * 2048 * 32 and len(cls) < 200 and set(cls.tolist()) == {0, 1, 2} and int((cls == 2).sum()) == 6
    tables = names_tables()
    at = GE.sample_rows(n, P)
    for what, idx in tables:
        assert len(idx) == n
        if what in ("random", "last row"):
            j = idx[at]
            eq, df, nc, first = loop_names(b"\n" + b1, c1[j].tolist(), b2, r2[j].tolist())
            assert len(at) >= 2000 and (eq, df, nc, first) == names_want(cls, j)
        want = names_want(cls, idx)
        if what in NAMES_PLACES:
            assert want[1] == (what != "none") and want[3] == {"none": -1, "inside pass 1": 40001, "first of pass 2": P, "last row": n - 1}[what]
            assert 0 < 40001 < P and want[2] > 0
        for k, s in enumerate(GE.passes(n, P)):
            w = names_want(cls, idx[s])
            if (what, k > 0) in (("late work", False), ("early work", True)):
                assert w[:2] == (0, 0) and w[2] == s.stop - s.start
            elif what in GE.ARRANGEMENTS:
                assert min(w[:3]) > 0


@pytest.mark.gpu
def test_pair_names_more_pairs_than_one_pass_of_the_grid(gpu_ctx):
    """three steps of every workgroup of k_pair_names; the four numbers in the three arrangements, and `first` with the only
    different pair inside pass 1, as the first pair of pass 2, as the table's last row, and nowhere (-1)"""
    from fastqandfurious_amd import hip
    b1, c1, b2, r2, cls = names_pool()
    d1, d2 = Dev(gpu_ctx, b1), Dev(gpu_ctx, b2)
    try:
        for what, idx in names_tables():
            t1 = dev_rows(c1[idx] + np.array([ADD1, ADD1, 0, 0, 0, 0]))
            t2 = dev_rows(r2[idx] + np.array([ADD2, ADD2, 0, 0, 0, 0]))
            got = gpu_ctx.table_pair_names(hip.table_view(d1.ptr, d1.n, t1.data_ptr(), True, ADD1),
                                           hip.table_view(d2.ptr, d2.n, t2.data_ptr(), False, ADD2), len(idx))
            want = names_want(cls, idx)
            assert tuple(got) == want, "%s: got %s, expected %s (first different: pass %s)" % (what, tuple(got), want, want[3] // GE.P_SHORT)
    finally:
        d1.close()
        d2.close()

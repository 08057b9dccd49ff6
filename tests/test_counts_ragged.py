"""How the table and pair passes' counts leave a workgroup whose waves are not all at work (csrc/ffq_rows.h: wg_counts_flush,
lds_hist_flush): tables of 1, 9, 33, 65 and 257 rows of 20 to 60 bases.

    1          one group of lanes has a row: three of the workgroup's four waves reach the flush with nothing
    9          the second wave has one row (eight lanes per row)
    33         a second workgroup has one row, in the kernels with eight lanes per row
    65, 257    the same two cases in the kernels with a lane per row

Every table is the first n rows of one corpus whose first nine rows count in every counter of every call and hold one
ineligible row (test_the_corpora_count_in_every_counter says so by the loops); the table of one row is a row that counts.
Every expectation is a plain loop another test module already has -- the *_expect.py files and the loops of test_trim.py,
test_filter.py, test_stats.py, test_render.py, test_pairs.py -- and every count, histogram and matrix word is compared exactly.
"""
import numpy as np
import pytest

import dedup_expect as DX
import overlap_expect as OX
import test_correct as TC
import test_dedup as TD
import test_filter as TF
import test_merge as TM
import test_overlap as TO
import test_pairs as TP
import test_render as TR
import test_stats as TS
import test_trim as TT

SIZES = (1, 9, 33, 65, 257)
N = max(SIZES)
COVERED = tuple(n for n in SIZES if n >= 9)
RULES = dict(qual_base=33, max_n=1, min_mean_qual=20, qualified_qual=15, max_unqualified_pct=30, min_complexity_pct=30, max_ee_micro=300000)
LO, HI = 20, 55                       # the length bounds of the selecting calls: a read of 58 bases fails them
CYCLES = 40                           # statistics: reads above 40 bases count in head word 3
OVERLAP_RULES = TO.RULESETS["short"]
CORRECT_RULES = TC.RULES[0]


# ---- the corpora ---------------------------------------------------------------------------------------------------------
def q(vals):
    return bytes(v + 33 for v in vals)


def single_reads():
    """257 (sequence, quality) of 20 to 60 bases; the first nine by hand: one per verdict of RULES"""
    rng = np.random.default_rng(2501)
    good = TM.seq_of(rng, 40)
    reads = [(good, q([16] * 5 + [38] * 30 + [16] * 5)),                # 0 kept; its ends are trimmed at a cutoff of 20
             (TM.seq_of(rng, 30), q([38] * 30)),                        # 1 (its row is made ineligible)
             (TM.seq_of(rng, 58), q([38] * 58)),                        # 2 too long
             (b"ACGTNNNACGT" + TM.seq_of(rng, 19), q([38] * 30)),       # 3 too many N
             (TM.seq_of(rng, 36), q([10] * 36)),                        # 4 low mean quality
             (TM.seq_of(rng, 40), q([5] * 16 + [40] * 24)),             # 5 too many unqualified bases
             (TM.seq_of(rng, 40), q([15] * 12 + [40] * 28)),            # 6 expected errors: 12 x 31 623 millionths, none unqualified
             (b"A" * 40, q([38] * 40)),                                 # 7 low complexity
             (good, q([38] * 40))]                                      # 8 kept: the sequence of read 0 again, a duplicate
    while len(reads) < N:
        n = int(rng.integers(20, 61))
        reads.append(TF.one_read(rng, n) if len(reads) % 3 else (TM.seq_of(rng, n), q(rng.integers(2, 41, n).tolist())))
    for i in range(40, N, 37):
        reads[i] = reads[i - 13]                                        # more duplicates
    return reads


def single_table():
    """(bytes -- a multiple of 16 --, rows): four-line records of single_reads(); row 1 reaches past the buffer"""
    buf, rows = bytearray(b"#"), []
    for i, (s, qual) in enumerate(single_reads()):
        TS.record(buf, rows, s, qual, header=b"@r%d" % i)
    rows[1] = rows[1][:4] + [len(buf) - 3, len(buf) + 1]
    return TD.finish(buf, rows)


def mate2_reads():
    """mate 2 of every read of single_reads(), judged by its length alone: 20..55 bases, 58 for pairs 3 and 8"""
    rng = np.random.default_rng(2502)
    return [TF.one_read(rng, 58 if i in (3, 8) or i % 11 == 10 else int(rng.integers(20, 56))) for i in range(N)]


def pair_tables():
    """(bytes 1, coordinates 1, bytes 2, coordinates 2): mate 1 behind a sentinel, as test_pairs.py has its mates"""
    b1, r1 = single_table()
    b2, r2 = bytearray(b"##"), []
    for i, (s, qual) in enumerate(mate2_reads()):
        TS.record(b2, r2, s, qual, header=b"@m%d" % i)
    return b1, (r1 + 1).tolist(), bytes(b2), r2


def name_tables(n):
    """headers of n pairs: ids of 20 to 60 bytes with /1 and /2, pair 1 (n > 2) not compared, the LAST pair different"""
    rng = np.random.default_rng(2503)
    ids = [TP.make_id(int(rng.integers(20, 61)), salt=i) for i in range(n)]
    b1, rows1 = TP.build_headers([x + b"/1" for x in ids], b"")
    b2, rows2 = TP.build_headers([x + b"/2 2:N:0" for x in ids[:-1]] + [ids[-1][:-1] + b"#/2"], b"#\n")
    if n > 2:
        rows1[1] = [-10, -5, 0, 0, 0, 0]
    return b1, rows1, b2, rows2


def overlap_pairs():
    """(sequence 1, sequence 2, flavour): fragments shorter than the reads (cut), between (an overlap), longer (none)"""
    rng = np.random.default_rng(2504)
    pairs = [OX.mates_of(rng, 25, 40, 45) + ("",), OX.mates_of(rng, 30, 40, 40) + ("fasta1",), OX.mates_of(rng, 60, 40, 50) + ("",),
             OX.mates_of(rng, 200, 50, 50) + ("",)]
    while len(pairs) < N:
        n1, n2 = (int(x) for x in rng.integers(20, 61, 2))
        flavour = ("wrapped0", "unequal2", "outside2")[len(pairs) % 3] if len(pairs) % 29 == 7 else ""
        pairs.append(OX.mates_of(rng, int(rng.integers(20, 130)), n1, n2, err=0.02) + (flavour,))
    return pairs


def insert_pairs(module, qms):
    """pairs as test_merge.build takes them, made by test_merge.pair or test_correct.pair: overlaps of every kind, pair 1 a FASTA
    row, pair 2 without an insert size"""
    rng = np.random.default_rng(2505)
    pairs = []
    while len(pairs) < N:
        k = len(pairs)
        n1, n2 = (int(x) for x in rng.integers(20, 61, 2))
        o = int(rng.integers(-(n2 - 1), n1))
        pairs.append(module.pair(rng, n1, n2, o, h=b"p%d" % k, qm=qms[k % len(qms)], flavour="fasta1" if k % 31 == 1 else "",
                                 **(dict(ins=-1) if k % 31 == 2 else {})))
    return pairs


def merge_pairs():
    return insert_pairs(TM, (("band", "band"), ("low", "high"), ("high", "low"), ("tie", "tie")))


def correct_pairs():
    return insert_pairs(TC, (("sure", "poor"), ("poor", "sure"), ("edges", "edges"), ("sure", "sure")))


# ---- what the loops say of them ------------------------------------------------------------------------------------------------
def single_keys(buf, rows):
    return [DX.row_key(buf, r, False) for r in np.asarray(rows).tolist()]


def pairs_want(n):
    b1, c1, b2, c2 = pair_tables()
    ver1 = TP.mate_verdicts(b"\n" + b1, c1[:n], RULES, LO, HI, True)
    ver2 = TP.mate_verdicts(b2, c2[:n], None, LO, HI, False)
    return TP.loop_pairs(ver1, ver2, "any", True, False)


def test_the_corpora_count_in_every_counter():
    buf, rows = single_table()
    assert len(buf) % 16 == 0 and len(rows) == N
    assert all(20 <= r[3] - r[2] <= 60 for r in rows.tolist())
    for n in COVERED:
        _want, stats = TT.loop_rows(buf, rows[:n], 20, 20)
        assert min(stats) > 0, ("trim", n, stats)
        _kept, counts, _v = TF.loop_select(buf, rows[:n], RULES, LO, HI)
        assert min(counts) > 0, ("select_reads", n, counts)
        head = TS.loop_words(TS.records_of(buf, rows[:n]), CYCLES)[:7]
        assert head.min() > 0, ("stats", n, head)
        assert min(TR.loop_render(buf, rows[:n])[2]) > 0, ("render", n)
        keys = single_keys(buf, rows[:n])
        kept, counts = DX.LoopSet(0).select(keys, True)
        assert DX.KEY_NONE in keys and min(counts[:3]) > 0 and counts[3] > 0, ("dedup", n, counts)
        _kept, h1, h2, pairs = pairs_want(n)
        assert min(pairs) > 0 and min(h1) > 0 and h2[0] > 0 and h2[1] > 0 and h2[2:] == [0] * 6, ("select_pairs", n, pairs, h1, h2)
        b1, rows1, b2, rows2 = name_tables(n)
        c1 = [[r[0] + 1, r[1] + 1] + r[2:] for r in rows1]
        assert TP.loop_names(b"\n" + bytes(b1), c1, bytes(b2), rows2) == (n - 2, 1, 1, n - 1)
    assert TP.loop_names(*[x for b, r in (name_tables(1)[:2], name_tables(1)[2:]) for x in (bytes(b), r)]) == (0, 1, 0, 0)
    T = TO.HostTable(overlap_pairs(), (0, 0), (N - 1, N - 1))
    M = TM.HostTable(merge_pairs())
    C = TC.HostTable(correct_pairs())
    for n in COVERED:
        *_rest, hist, counts = T.expect(n, OVERLAP_RULES, True)
        assert min(counts) > 0 and hist.sum() == counts[1], ("overlap", n, counts)
        assert min(M.expect(n)[5]) > 0, ("merge", n, M.expect(n)[5])
        _s1, _s2, counts, matrix = C.expect(n, CORRECT_RULES)
        assert min(counts) > 0 and sum(matrix) == counts[2] + counts[3], ("correct", n, counts)


# ---- the device ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def single(gpu_ctx):
    import torch
    buf, rows = single_table()
    dev16, devf = TD.Dev(gpu_ctx, buf), TF.Dev(gpu_ctx, buf)
    yield dict(buf=buf, rows=rows, dev16=dev16, devf=devf, dbuf=torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).cuda())
    dev16.close()
    devf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_trim_quality(gpu_ctx, single, n):
    TT.check_device(gpu_ctx, single["buf"], single["rows"][:n], 20, 20, combos=((0, 0, False), (0, 0, True)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_select_reads(single, n):
    TF.check(single["devf"], single["buf"], single["rows"][:n], RULES, LO, HI)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_stats(gpu_ctx, single, n):
    rows = single["rows"][:n]
    TS.check_device(gpu_ctx, single["buf"], rows, CYCLES, dbuf=single["dbuf"], want=TS.loop_words(TS.records_of(single["buf"], rows), CYCLES))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_render_fastq(gpu_ctx, single, n):
    TR.check(gpu_ctx, single["buf"], single["rows"][:n], dbuf=single["dbuf"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_seq_keys_and_the_set(gpu_ctx, single, n):
    from fastqandfurious_amd import hip
    keys = TD.check_keys(single["dev16"], single["buf"], single["rows"][:n])
    dd = hip.Dedup(gpu_ctx, 0, 0)
    try:
        model = DX.LoopSet(0)
        first = TD.check_call(dd, model, keys)
        again = TD.check_call(dd, model, keys)                         # every key is in the set: nothing is entered
        assert again[3] == first[3] and again[1] == sum(1 for k in keys if k != DX.KEY_NONE)
    finally:
        dd.close()


@pytest.fixture(scope="module")
def mates(gpu_ctx):
    from fastqandfurious_amd import hip
    b1, c1, b2, c2 = pair_tables()
    m1, m2 = np.array(c1, dtype=np.int64) + TP.ADD1, np.array(c2, dtype=np.int64) + TP.ADD2
    d1, d2 = TP.Dev(gpu_ctx, b1), TP.Dev(gpu_ctx, b2)
    t1, t2 = TP.dev_rows(m1), TP.dev_rows(m2)
    yield dict(m1=m1, m2=m2, t1=t1, t2=t2, v1=hip.table_view(d1.ptr, d1.n, t1.data_ptr(), True, TP.ADD1),
               v2=hip.table_view(d2.ptr, d2.n, t2.data_ptr(), False, TP.ADD2))
    d1.close()
    d2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_select_pairs(gpu_ctx, mates, n):
    """mate 1 by RULES (k_filter_rows), mate 2 by its length (k_pair_len), the pairs by k_pair_count"""
    kept, h1, h2, pairs = pairs_want(n)
    o1, o2, idx, g1, g2, gp = TP.select_pairs(gpu_ctx, mates["v1"], mates["v2"], mates["t1"], mates["t2"], n, RULES, None,
                                              (LO, LO), (HI, HI), "any")
    assert (gp, g1, g2, idx.tolist()) == (pairs, h1, h2, kept)
    assert (o1 == mates["m1"][kept]).all() and (o2 == mates["m2"][kept]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_pair_names(gpu_ctx, n):
    """the first different pair is the last one: the minimum has to come from the last group that has a pair"""
    got, want = TP.names_on_device(gpu_ctx, *name_tables(n))
    assert got == want and want[3] == n - 1


@pytest.fixture(scope="module")
def overlap_table(gpu_ctx):
    T = TO.Table(gpu_ctx, overlap_pairs(), (0, 0), (N - 1, N - 1))
    yield T
    T.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_pair_overlap(gpu_ctx, overlap_table, n):
    T = overlap_table
    TO.same(TO.run(gpu_ctx, T, n, OVERLAP_RULES, True), T.expect(n, OVERLAP_RULES, True))
    TO.same(TO.run(gpu_ctx, T, n, OVERLAP_RULES, False, hist=False), T.expect(n, OVERLAP_RULES, False), hist=False)


@pytest.fixture(scope="module")
def correct_table():
    return TC.HostTable(correct_pairs())


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_pair_correct(gpu_ctx, correct_table, n):
    T = correct_table
    before, got = TC.run(gpu_ctx, T.bytes, T.m, T.ins, n, CORRECT_RULES)
    TC.same(before, got, T.expect(n, CORRECT_RULES), T.bytes)


@pytest.fixture(scope="module")
def merge_table(gpu_ctx):
    T = TM.Table(gpu_ctx, merge_pairs())
    yield T
    T.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_pair_merge(gpu_ctx, merge_table, n):
    TM.same(TM.run(gpu_ctx, merge_table, n), merge_table.expect(n), n)

"""What filter_fastq and filter_fastq_paired make of the ROUNDS of the device route, without a GPU: the fakes of
tests/plan_fakes.py play a script of two END_REFILL rounds and one END_OK round whose count vectors hold a different small
prime in every slot -- a getter read at the wrong index, summed twice or not at all shows in a total.  The totals below are
literals, added up by hand from the script by what each slot MEANS (hip.py's docstrings); the texts are short and fixed.
Asserted: the result, every field of every report, both FilterReport.dropped, and the ordered log of the writes to the
outputs (merged first within a round; compressed: the EOF markers at the end)."""
import io
import itertools

import numpy as np
import pytest

from plan_fakes import FakeScanner, no_rounds  # noqa: F401

PRIMES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113,
          127, 131, 137, 139, 149, 151, 157, 163, 167, 173, 179, 181, 191, 193, 197, 199, 211, 223, 227, 229, 233, 239, 241, 251,
          257, 263, 269, 271, 277, 281, 283, 293, 307, 311, 313, 317, 331, 337, 347, 349, 353, 359, 367, 373, 379, 383, 389, 397,
          401, 409, 419, 421, 431, 433, 439, 443, 449, 457, 461, 463, 467, 479, 487, 491, 499, 503, 509, 521, 523, 541, 547, 557,
          563, 569, 571, 577, 587, 593, 599, 601, 607, 613, 617, 619, 631, 641, 643, 647, 653, 659, 661, 673, 677, 683, 691, 701,
          709, 719, 727, 733, 739, 743, 751, 757, 761, 769, 773, 787, 797, 809, 811, 821, 823, 827, 829, 839, 853, 857, 859, 863,
          877, 881, 883, 887, 907, 911, 919, 929, 937, 941, 947, 953, 967, 971, 977, 983, 991, 997, 1009, 1013, 1019, 1021, 1031,
          1033, 1039, 1049, 1051, 1061, 1063, 1069, 1087, 1091, 1093, 1097, 1103, 1109, 1117, 1123, 1129, 1151, 1153, 1163, 1171,
          1181, 1187, 1193, 1201, 1213, 1217, 1223, 1229, 1231, 1237, 1249, 1259, 1277, 1279, 1283, 1289, 1291, 1297, 1301, 1303,
          1307, 1319, 1321, 1327, 1361, 1367, 1373, 1381, 1399, 1409, 1423, 1427, 1429, 1433, 1439, 1447, 1451, 1453, 1459, 1471,
          1481, 1483, 1487, 1489, 1493, 1499, 1511, 1523, 1531, 1543, 1549, 1553, 1559, 1567, 1571, 1579, 1583, 1597, 1601, 1607,
          1609, 1613, 1619, 1621, 1627, 1637, 1657, 1663, 1667, 1669, 1693, 1697, 1699, 1709, 1721, 1723, 1733, 1741, 1747, 1753,
          1759, 1777, 1783, 1787, 1789, 1801, 1811, 1823, 1831, 1847, 1861, 1867, 1871, 1873, 1877, 1879, 1889, 1901, 1907, 1913)
END_OK, END_REFILL = 0, 1
ROUNDS = 3
EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
HIST = np.arange(1025, dtype=np.uint64) * 3 + 1
MATRIX = np.arange(20, dtype=np.int64).reshape(5, 4) + 7


@pytest.fixture(scope="module")
def F(pkg):
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


def arr(b):
    return np.frombuffer(b, dtype=np.uint8)


def mate_script(k, compress, primes):
    """the three fills (rounds) of stream k (0, 1); the primes are handed out in the order of this text.  One slot of each
    "is there anything to write" count is 0 once: mate 2 has no text (no members) in round 1"""
    script = []
    for r in range(ROUNDS):
        take = lambda n: [next(primes) for _ in range(n)]       # noqa: E731
        e = {"filter_counts": take(8), "ends_trimmed": tuple(take(3)), "trimmed": tuple(take(3)), "adapter_trimmed": tuple(take(3)),
             "poly_trimmed": (tuple(take(3)), tuple(take(3)))}
        rendered, deflated, n_scanned = take(3), take(4), take(1)[0]
        if k == 1 and r == 1:
            rendered[0] = deflated[1] = 0
        e["rendered"] = (None if compress else arr(b"@m%dr%d\n" % (k + 1, r)), tuple(rendered))
        e["compressed"] = (arr(b"Z%d%d" % (k + 1, r)), tuple(deflated))
        e["selected"] = (np.zeros(0, dtype=np.int64), n_scanned, None, None)
        e["next"] = (np.zeros((0, 6), dtype=np.int64), np.zeros(0, dtype=np.uint8), 0, END_REFILL if r < ROUNDS - 1 else END_OK, 0)
        script.append(e)
    script[-1]["dedup_counts"] = [next(primes) for _ in range(6)]
    return script


def pair_script(compress, primes, last_end=(END_OK, 0, 0)):
    """the three rounds of the pair; round 0 merges pairs into no text (no members)"""
    script = []
    for r in range(ROUNDS):
        take = lambda n: [next(primes) for _ in range(n)]       # noqa: E731
        n_in, n_out = take(2)
        merged, deflated = take(6), take(4)
        if r == 0:
            merged[2] = deflated[1] = 0
        script.append({"next": (n_in, n_out) + ((END_REFILL, 0, 0) if r < ROUNDS - 1 else last_end),
                       "merged": (arr(b"" if compress else b"@merged r%d\n" % r), merged),
                       "merged_bgzf": (arr(b"ZM%d" % r), tuple(deflated)),
                       "overlap": (take(6), HIST), "corrected": (take(6), MATRIX),
                       "selected": (np.zeros(0, dtype=np.int64), take(5))})
    script[-1]["dedup_counts"] = [next(primes) for _ in range(6)]
    script[-1]["mismatch"] = (b"read9/1 x", b"read8/2 y")
    return script


class Outputs:
    """three files that log their writes into one list"""

    def __init__(self):
        self.log = []
        self.out1, self.out2, self.merged = (self.File(self.log, name) for name in ("out1", "out2", "merged"))

    class File:
        def __init__(self, log, name):
            self.log, self.name = log, name

        def write(self, data):
            self.log.append((self.name, bytes(data)))


def run_paired(F, no_rounds, pair_filter, merge, compress, last_end=(END_OK, 0, 0)):
    primes = iter(PRIMES)
    sc = FakeScanner(scripts=(mate_script(0, compress, primes), mate_script(1, compress, primes)))
    no_rounds.script = pair_script(compress, primes, last_end)
    outs = Outputs()
    reps = dict(report=F.FilterReport(8), report2=F.FilterReport(8), overlap_report=F.OverlapReport(),
                correction_report=F.CorrectionReport(), dedup_report=F.DedupReport(), poly_report=F.PolyReport(),
                ends_report=F.EndsReport())
    if merge:
        reps["merge_report"] = F.MergeReport()
    if compress:
        reps["compress_report"] = F.CompressReport()
    for rep in reps.values():                               # (a report is reset, not added to)
        for name, v in list(vars(rep).items()):
            if isinstance(v, int) and name != "max_cycles":
                setattr(rep, name, 99)

    def call():
        return F.filter_fastq_paired(io.BytesIO(b""), io.BytesIO(b""), outs.out1, outs.out2, 4096, entrypos=sc, pair_filter=pair_filter,
                                     quality_cutoff=(5, 20), adapter=b"ACGTACGT", adapter2=b"TTGCA", min_len=(30, 20),
                                     content=F.ContentRules(max_n=2), overlap=F.OverlapRules(), correction=F.CorrectionRules(),
                                     dedup=F.DedupRules(), poly_g=10, poly_x=12, ends=F.EndRules(trim_front=1),
                                     merged_out=outs.merged if merge else None, compress="bgzf" if compress else None, **reps)
    return call, sc, outs, reps


def check_paired_reports(F, reps, pair_filter, merge, compress, finished=True):
    # ---- per mate: filter_counts()[1:7] by reason; a mate that is not judged counts nothing
    reasons = F.ContentRules.REASONS
    assert len(reasons) == 6
    assert reps["report"].dropped == dict(zip(reasons, (3 + 137 + 311, 5 + 139 + 313, 7 + 149 + 317, 11 + 151 + 331, 13 + 157 + 337,
                                                        17 + 163 + 347)))
    want2 = (547 + 743 + 967, 557 + 751 + 971, 563 + 757 + 977, 569 + 761 + 983, 571 + 769 + 991, 577 + 773 + 997)
    assert reps["report2"].dropped == dict(zip(reasons, want2 if pair_filter != "first" else (0,) * 6))
    # ---- both mates together: ends_trimmed()[0:2]; poly_trimmed()[0][0:2] and [1][0:2]
    e = reps["ends_report"]
    assert (e.reads_cut, e.bases_cut) == (23 + 173 + 353 + 593 + 797 + 1013, 29 + 179 + 359 + 599 + 809 + 1019)
    p = reps["poly_report"]
    assert (p.poly_g_reads, p.poly_g_bases) == (61 + 227 + 409 + 643 + 857 + 1063, 67 + 229 + 419 + 647 + 859 + 1069)
    assert (p.poly_x_reads, p.poly_x_bases) == (73 + 239 + 431 + 659 + 877 + 1091, 79 + 241 + 433 + 661 + 881 + 1093)
    # ---- the pair: overlap()[0][0:5], corrected()[0][0:5], merged()[1][0, 2, 3, 4, 5]
    o = reps["overlap_report"]
    assert (o.pairs_analysed, o.pairs_overlapped, o.pairs_trimmed) == (1297 + 1511 + 1723, 1301 + 1523 + 1733, 1303 + 1531 + 1741)
    assert o.bases_removed == [1307 + 1543 + 1747, 1319 + 1549 + 1753]
    assert o.insert_hist.tolist() == (HIST if finished else HIST * 0).tolist()
    c = reps["correction_report"]
    assert (c.pairs_checked, c.pairs_corrected, c.mismatches) == (1327 + 1559 + 1777, 1361 + 1567 + 1783, 1381 + 1583 + 1801)
    assert c.bases_corrected == [1367 + 1571 + 1787, 1373 + 1579 + 1789]
    assert c.matrix.tolist() == (MATRIX if finished else MATRIX * 0).tolist()
    if merge:
        m = reps["merge_report"]
        assert (m.pairs_merged, m.bytes_merged, m.bases_merged) == (1229 + 1451 + 1637, 0 + 1459 + 1663, 1249 + 1471 + 1667)
        assert (m.overlap_positions, m.taken_from_mate2) == (1259 + 1481 + 1669, 1277 + 1483 + 1693)
    # ---- the pair's dedup_counts() at the end: keyed = kept + duplicates - unkeyed
    d = reps["dedup_report"]
    want = (1871 + 1873 - 1877, 1877, 1879, 1873) if finished else (0, 0, 0, 0)
    assert (d.keyed, d.unkeyed, d.distinct, d.duplicates) == want
    if compress:
        # both mates' compressed()[1] and, merging, the pair's merged_bgzf()[1]
        z = reps["compress_report"]
        ins = 103 + 271 + 461 + 701 + 919 + 1123 + ((1279 + 1487 + 1697) if merge else 0)
        outs = 107 + 277 + 463 + 709 + 0 + 1129 + ((0 + 1489 + 1699) if merge else 0)
        members = 109 + 281 + 467 + 719 + 937 + 1151 + ((1289 + 1493 + 1709) if merge else 0)
        stored = 113 + 283 + 479 + 727 + 941 + 1153 + ((1291 + 1499 + 1721) if merge else 0)
        assert (z.bytes_in, z.bytes_out, z.members, z.members_stored) == (ins, outs, members, stored)


def paired_writes(merge, compress, finished=True):
    log = []
    for r in range(ROUNDS):
        if merge and r != 0:
            log.append(("merged", b"ZM%d" % r if compress else b"@merged r%d\n" % r))
        log.append(("out1", b"Z1%d" % r if compress else b"@m1r%d\n" % r))
        if r != 1:
            log.append(("out2", b"Z2%d" % r if compress else b"@m2r%d\n" % r))
    if compress and finished:
        log += [("out1", EOF), ("out2", EOF)] + ([("merged", EOF)] if merge else [])
    return log


@pytest.mark.parametrize("pair_filter,merge,compress", list(itertools.product(("any", "both", "first"), (False, True), (False, True))))
def test_three_rounds_of_a_pair(F, no_rounds, pair_filter, merge, compress):
    call, sc, outs, reps = run_paired(F, no_rounds, pair_filter, merge, compress)
    res = call()
    # pairs_in: n_in; pairs_out: n_out (+ merged()[1][0]); bases_removed: [1] of the five trims of both mates + overlap()[0][3:5]
    removed = ((29 + 179 + 359) + (41 + 193 + 379) + (53 + 211 + 397) + (67 + 229 + 419) + (79 + 241 + 433)
               + (599 + 809 + 1019) + (613 + 823 + 1033) + (631 + 839 + 1051) + (647 + 859 + 1069) + (661 + 881 + 1093)
               + (1307 + 1543 + 1747) + (1319 + 1549 + 1753))
    # selected()[1][2:5]; under "both" a pair with one failed mate is kept and the one-mate counts are not taken
    dropped = {"mate1_only": 0 if pair_filter == "both" else 1427 + 1609 + 1847,
               "mate2_only": 0 if pair_filter == "both" else 1429 + 1613 + 1861, "both": 1433 + 1619 + 1867}
    assert res == F.PairedFilterResult(1217 + 1439 + 1621, 1223 + 1447 + 1627 + ((1229 + 1451 + 1637) if merge else 0), removed,
                                       89 + 257 + 443, 677 + 0 + 1103, dropped)
    check_paired_reports(F, reps, pair_filter, merge, compress)
    assert outs.log == paired_writes(merge, compress)
    assert [s.closed for s in sc.streams] == [1, 1] and [p.closed for p in no_rounds.made] == [1]
    assert reps["report"].dropped is not reps["report2"].dropped


@pytest.mark.parametrize("compress", (False, True))
def test_a_name_error_in_the_last_round_comes_behind_its_drains(F, hip_consts, no_rounds, compress):
    call, sc, outs, reps = run_paired(F, no_rounds, "any", True, compress, last_end=(hip_consts.END_ERR_PAIR_NAMES, 0, 4711))
    with pytest.raises(ValueError) as e:
        call()
    assert str(e.value) == "pair 4711: the two records are not mates: b'read9' and b'read8'"
    check_paired_reports(F, reps, "any", True, compress, finished=False)
    assert outs.log == paired_writes(True, compress, finished=False)
    assert [s.closed for s in sc.streams] == [1, 1] and [p.closed for p in no_rounds.made] == [1]


@pytest.fixture(scope="module")
def hip_consts(pkg):
    from fastqandfurious_amd import hip
    return hip


@pytest.mark.parametrize("compress", (False, True))
def test_three_fills_of_one_file(F, compress):
    sc = FakeScanner(scripts=(mate_script(0, compress, iter(PRIMES)),))
    outs = Outputs()
    reps = dict(report=F.FilterReport(8), dedup_report=F.DedupReport(), poly_report=F.PolyReport(), ends_report=F.EndsReport())
    if compress:
        reps["compress_report"] = F.CompressReport()
    res = F.filter_fastq(io.BytesIO(b""), outs.out1, 4096, entrypos=sc, quality_cutoff=(5, 20), adapter=b"ACGTACGT", min_len=30,
                         content=F.ContentRules(max_n=2), dedup=F.DedupRules(), poly_g=10, poly_x=12, ends=F.EndRules(trim_front=1),
                         compress="bgzf" if compress else None, **reps)
    # records_in: selected()[1] (the stream filters); records_out: rendered()[1][1]; bytes_out: rendered()[1][0]
    removed = (29 + 179 + 359) + (41 + 193 + 379) + (53 + 211 + 397) + (67 + 229 + 419) + (79 + 241 + 433)
    assert res == F.FilterResult(127 + 293 + 487, 97 + 263 + 449, removed, 89 + 257 + 443)
    assert reps["report"].dropped == dict(zip(F.ContentRules.REASONS, (3 + 137 + 311, 5 + 139 + 313, 7 + 149 + 317, 11 + 151 + 331,
                                                                       13 + 157 + 337, 17 + 163 + 347)))
    e, p, d = reps["ends_report"], reps["poly_report"], reps["dedup_report"]
    assert (e.reads_cut, e.bases_cut) == (23 + 173 + 353, 29 + 179 + 359)
    assert (p.poly_g_reads, p.poly_g_bases, p.poly_x_reads, p.poly_x_bases) == (61 + 227 + 409, 67 + 229 + 419, 73 + 239 + 431, 79 + 241 + 433)
    assert (d.keyed, d.unkeyed, d.distinct, d.duplicates) == (491 + 499 - 503, 503, 509, 499)
    if compress:
        z = reps["compress_report"]
        assert (z.bytes_in, z.bytes_out, z.members, z.members_stored) == (103 + 271 + 461, 107 + 277 + 463, 109 + 281 + 467, 113 + 283 + 479)
    assert outs.log == [("out1", b"Z1%d" % r if compress else b"@m1r%d\n" % r) for r in range(ROUNDS)] + ([("out1", EOF)] if compress else [])
    assert [s.closed for s in sc.streams] == [1]
    assert sc.streams[0].log[0] == ("set_dedup", True, 0, 0)

"""Merging the mates of a pair on the host: fastqandfurious.merge_mates / merge_mergeable against the plain loop of
tests/merge_expect.py, and filter_fastq_paired(merged_out=...) with the Python scanner on a pair written by hand.  No GPU."""
import io

import numpy as np
import pytest

import merge_expect as M
import overlap_expect as X

LENS = (1, 2, 15, 16, 17, 31, 32, 33, 150, 511, 512)


def F():
    import fastqandfurious_amd  # noqa: F401
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


def want_of(a, qa, b, qb, ins):
    m = M.loop_merge(a, qa, b, qb, ins)
    return None if m is None else m[:2]


def rnd(rng, n, lo, hi):
    return bytes(rng.integers(lo, hi, n).astype(np.uint8))


def test_merge_mates_is_the_loop_on_seeded_pairs():
    f = F()
    rng = np.random.default_rng(7)
    merged = 0
    for t in range(1500):
        n1, n2 = (int(rng.integers(0, 60)), int(rng.integers(0, 60))) if t % 3 else (int(rng.choice(LENS)), int(rng.choice(LENS)))
        a = np.frombuffer(b"ACGTacgtN.", dtype=np.uint8)[rng.integers(0, 10, n1)].tobytes()
        b = np.frombuffer(b"ACGTacgtN.", dtype=np.uint8)[rng.integers(0, 10, n2)].tobytes()
        qa, qb = (rnd(rng, n1, 60, 64), rnd(rng, n2, 60, 64)) if t % 2 else (rnd(rng, n1, 0, 256), rnd(rng, n2, 0, 256))
        ins = int(rng.integers(-3, n1 + n2 + 3))
        want = want_of(a, qa, b, qb, ins)
        assert f.merge_mates(a, qa, b, qb, ins) == want, (n1, n2, ins)
        merged += want is not None
    assert merged > 1000


@pytest.mark.parametrize("n1", LENS)
def test_merge_mates_edge_alignments(n1):
    """overlaps of one position at either end, o = 0, mate 2 sticking out in front, mate 2 inside mate 1, and the first insert
    sizes on either side that do not merge; ties, qb above and below qa, bytes >= 0x80, lower case, N and '.'"""
    f = F()
    rng = np.random.default_rng(n1)
    for n2 in LENS:
        a, b = rnd(rng, n1, 33, 127), np.frombuffer(b"ACGTacgtN.", dtype=np.uint8)[rng.integers(0, 10, n2)].tobytes()
        for qa, qb in ((b"I" * n1, b"I" * n2), (b"5" * n1, b"I" * n2), (b"I" * n1, b"5" * n2), (rnd(rng, n1, 120, 140), rnd(rng, n2, 120, 140))):
            for o in {n1 - 1, -(n2 - 1), 0, -(n2 // 2), (n1 - n2) // 2, 1, -1}:
                if -n2 < o < n1:
                    got = f.merge_mates(a, qa, b, qb, n2 + o)
                    assert got == want_of(a, qa, b, qb, n2 + o) and got is not None, (n1, n2, o)
                    assert len(got[0]) == len(got[1]) == (n2 + o if o < 0 else max(n1, n2 + o))
            for ins in (0, n1 + n2, -1, -2, None):
                assert f.merge_mates(a, qa, b, qb, ins) is None
    assert f.merge_mates(b"A" * 513, b"I" * 513, b"T" * 100, b"I" * 100, 300) is None
    assert f.merge_mates(b"A" * 100, b"I" * 99, b"T" * 100, b"I" * 100, 150) is None


def test_a_tie_goes_to_mate_1_and_the_surer_base_wins():
    f = F()
    #            a = ACGTAC, rb = revcomp(b); o = 2: positions 2..5 overlap
    a, qa = b"ACGTAC", b"IIII5I"
    b, qb = b"ttGNAC", b"5III5I"          # revcomp: GTNCaa; qualities reversed: I5III5
    assert M.loop_merge(a, qa, b, qb, 8)[:2] == (b"ACGTNCaa", b"IIIIIII5")
    assert f.merge_mates(a, qa, b, qb, 8) == (b"ACGTNCaa", b"IIIIIII5")


PAIR1 = (b"@p1/1\nACGTACGTAAGG\n+\nIIIIIIII5555\n"         # overlaps p1/2 by 8 positions (insert 16): merged
         b"@p2/1\nACGTACGTAAGG\n+\nIIIIIIIIIIII\n"          # no overlap with p2/2: both written
         b"@p3/1\nACGTACGTAAGG\n+\nIIIIIIIIIIII\n")         # overlaps, mate 2 too short for min_len: dropped
PAIR2 = (b"@p1/2\nAAAACCTTACGT\n+\n5555IIIIIIII\n"         # revcomp: ACGTAAGGTTTT
         b"@p2/2\nCCCCCCCCCCCC\n+\nIIIIIIIIIIII\n"
         b"@p3/2\nCCTTACGT\n+\nIIIIIIII\n")


def test_filter_fastq_paired_writes_a_hand_written_pair_merged():
    f = F()
    o1, o2, om = io.BytesIO(), io.BytesIO(), io.BytesIO()
    rep, r1, r2 = f.MergeReport(), f.FilterReport(), f.FilterReport()
    res = f.filter_fastq_paired(io.BytesIO(PAIR1), io.BytesIO(PAIR2), o1, o2, fbufsize=1 << 12, entrypos=f.entrypos, min_len=(None, 10),
                                overlap=f.OverlapRules(6, 0, 0), merged_out=om, merge_report=rep, report=r1, report2=r2)
    assert om.getvalue() == b"@p1/1\nACGTACGTAAGGTTTT\n+\nIIIIIIIIIIII5555\n"
    assert o1.getvalue() == b"@p2/1\nACGTACGTAAGG\n+\nIIIIIIIIIIII\n"
    assert o2.getvalue() == b"@p2/2\nCCCCCCCCCCCC\n+\nIIIIIIIIIIII\n"
    assert res == (3, 2, 0, len(o1.getvalue()), len(o2.getvalue()), {"mate1_only": 0, "mate2_only": 1, "both": 0})
    assert (rep.pairs_merged, rep.bases_merged, rep.bytes_merged, rep.overlap_positions, rep.taken_from_mate2) == (1, 16, len(om.getvalue()), 8, 4)
    # `after` counts what went to the two ordinary files
    assert int(r1.after.head[0]) == 1 == int(r2.after.head[0]) and int(r1.before.head[0]) == 3


def test_the_two_value_errors():
    f = F()
    with pytest.raises(ValueError, match="merged_out needs overlap"):
        f.filter_fastq_paired(io.BytesIO(PAIR1), io.BytesIO(PAIR2), io.BytesIO(), io.BytesIO(), entrypos=f.entrypos, merged_out=io.BytesIO())
    with pytest.raises(ValueError, match="merge_report needs merged_out"):
        f.filter_fastq_paired(io.BytesIO(PAIR1), io.BytesIO(PAIR2), io.BytesIO(), io.BytesIO(), entrypos=f.entrypos,
                              overlap=f.OverlapRules(6, 0, 0), merge_report=f.MergeReport())


def test_without_merged_out_nothing_changes():
    """the bytes and the result of the call as it was before merging existed: literals for the hand-written pair, and the
    overlap tests' own expectation for a generated file"""
    f = F()
    o1, o2 = io.BytesIO(), io.BytesIO()
    res = f.filter_fastq_paired(io.BytesIO(PAIR1), io.BytesIO(PAIR2), o1, o2, fbufsize=1 << 12, entrypos=f.entrypos, min_len=(None, 10),
                                overlap=f.OverlapRules(6, 0, 0))
    assert o1.getvalue() == b"@p1/1\nACGTACGTAAGG\n+\nIIIIIIII5555\n@p2/1\nACGTACGTAAGG\n+\nIIIIIIIIIIII\n"
    assert o2.getvalue() == b"@p1/2\nAAAACCTTACGT\n+\n5555IIIIIIII\n@p2/2\nCCCCCCCCCCCC\n+\nIIIIIIIIIIII\n"
    assert res == (3, 2, 0, len(o1.getvalue()), len(o2.getvalue()), {"mate1_only": 0, "mate2_only": 1, "both": 0})
    recs1, recs2 = X.records(300)
    want = X.Expected(recs1, recs2, min_len=(20, 20))
    d1, d2 = M.file_of(recs1), M.file_of(recs2)
    res, t1, t2, rep = X.run(f, d1, d2, f.entrypos, 1 << 14, min_len=20)
    assert (t1, t2) == tuple(want.text) and tuple(res) == want.result()
    want.check_report(rep)


def test_the_host_route_on_generated_files():
    """filter_fastq_paired(merged_out=...) with the Python scanner against the loop's expectation: three files, result, reports"""
    f = F()
    recs1, recs2 = M.records(400)
    want = M.Expected(recs1, recs2, min_len=(40, 40))
    assert want.kinds >= {"wrapped", "none", "merged"} and want.pairs_merged > 100 and want.written[0] > 50 and want.taken > 0
    assert sum(want.dropped.values()) > 0
    res, t1, t2, tm, rep, reps = M.run(f, M.file_of(recs1), M.file_of(recs2), f.entrypos, 1 << 14, min_len=40)
    assert (t1, t2, tm) == tuple(want.text)
    assert tuple(res) == want.result()
    want.check_report(rep)
    assert int(reps[0].after.head[0]) + int(reps[0].after.head[1]) == want.written[0]

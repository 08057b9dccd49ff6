"""Correcting bases inside the mates' overlap on the host: fastqandfurious.correct_mates / correct_correctable against the plain
loop of tests/correct_expect.py, and filter_fastq_paired(correction=...) with the Python scanner on pairs written by hand and on
generated files.  No GPU."""
import io

import numpy as np
import pytest

import correct_expect as K
import overlap_expect as X

LENS = (1, 2, 15, 16, 17, 31, 32, 33, 150, 511, 512)


def F():
    import fastqandfurious_amd  # noqa: F401
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


def rnd(rng, n, lo, hi):
    return bytes(rng.integers(lo, hi, n).astype(np.uint8))


def facing(rng, a, n2, o, err):
    """mate 2 (n2 bytes) whose reverse complement agrees with `a` placed at offset o, but for a share `err` of its bytes"""
    alphabet = np.frombuffer(b"ACGTacgtN.", dtype=np.uint8)
    b = bytearray(alphabet[rng.integers(0, 10, n2)].tobytes())
    for j in range(n2):
        p = (n2 - 1 - j) + o
        if 0 <= p < len(a) and rng.random() >= err:
            b[j] = K.COMP.get(a[p], a[p])
    return bytes(b)


def test_correct_mates_is_the_loop_on_seeded_pairs():
    f = F()
    rng = np.random.default_rng(7)
    looked = fixed1 = fixed2 = stay = 0
    for t in range(1500):
        n1, n2 = (int(rng.integers(0, 60)), int(rng.integers(0, 60))) if t % 3 else (int(rng.choice(LENS)), int(rng.choice(LENS)))
        good, bad, base = ((30, 14, 33), (30, 14, 64), (20, 19, 33), (100, 0, 120), (1, 0, 0))[t % 5]
        G, B = base + good, base + bad
        ins = int(rng.integers(-3, n1 + n2 + 3))
        a = np.frombuffer(b"ACGTacgtN.", dtype=np.uint8)[rng.integers(0, 10, n1)].tobytes()
        b = facing(rng, a, n2, ins - n2, 0.2)
        near = np.array([G, G - 1 if G else 0, B, B + 1, min(G + 5, 255), max(B - 5, 0)], dtype=np.uint8)
        qa, qb = (bytes(near[rng.integers(0, 6, n1)]), bytes(near[rng.integers(0, 6, n2)])) if t % 2 else (rnd(rng, n1, 0, 256), rnd(rng, n2, 0, 256))
        want = K.loop_correct(a, qa, b, qb, ins, good, bad, base)
        got = f.correct_mates(a, qa, b, qb, ins, f.CorrectionRules(good, bad), base)
        if want is None:
            assert got == (a, qa, b, qb, 0, 0), (n1, n2, ins)
            continue
        assert got == want[:6], (n1, n2, ins, good, bad, base)
        # idempotent
        assert f.correct_mates(*got[:4], ins, f.CorrectionRules(good, bad), base) == got[:4] + (0, 0)
        looked += 1
        fixed1 += want[4]
        fixed2 += want[5]
        stay += want[6] - want[4] - want[5]
    assert looked > 1000 and fixed1 > 300 and fixed2 > 300 and stay > 1000


def test_the_rule_on_a_pair_written_by_hand():
    """'?' is Q30 (G), '/' Q14 (B), '.' Q13, '0' Q15.  n1 = 8, n2 = 6, insert 8: o = 2, a[p] faces b[7 - p] for p = 2..7"""
    f = F()
    R = f.CorrectionRules()
    # p:             2 3 4 5 6 7
    # a[p]           G A A C G G        comp(b[7 - p]) = G T A C N C: mismatches at p = 3, 6, 7
    a, qa = b"ACGAACGG", b"III?II/0"     # qa[3] sure, qa[6] poor, qa[7] just above poor
    b, qb = b"GNGTAC", b"?.IIII"          # qb[0] (p = 7) sure, qb[1] (p = 6, the N) poor, qb[4] (p = 3) neither
    # p = 3: sure against a call that is not poor; p = 6: poor against poor; p = 7: sure against Q15: all three stay
    assert K.loop_correct(a, qa, b, qb, 8)[:7] == (a, qa, b, qb, 0, 0, 3)
    assert f.correct_mates(a, qa, b, qb, 8, R) == (a, qa, b, qb, 0, 0)
    # p = 3 with mate 2's call poor: b[4] becomes comp(a[3]) = T and takes mate 1's quality
    got = f.correct_mates(a, qa, b, b"?.II/I", 8, R)
    assert got == (a, qa, b"GNGTTC", b"?.II?I", 0, 1) == K.loop_correct(a, qa, b, b"?.II/I", 8)[:6]
    # p = 6 with mate 1 sure: the poor N is replaced by comp(G) = C
    got = f.correct_mates(a, b"III?II?0", b, qb, 8, R)
    assert got == (a, b"III?II?0", b"GCGTAC", b"??IIII", 0, 1) == K.loop_correct(a, b"III?II?0", b, qb, 8)[:6]
    # p = 6 the other way round, the N sure and mate 1 poor: an N is never written over a base
    got = f.correct_mates(a, qa, b, b"?IIIII", 8, R)
    assert got == (a, qa, b, b"?IIIII", 0, 0) == K.loop_correct(a, qa, b, b"?IIIII", 8)[:6]
    # p = 7 with mate 1 poor: a[7] becomes comp(b[0]) = C and takes mate 2's quality; p = 6 is still poor against poor
    got = f.correct_mates(a, b"III?II//", b, qb, 8, R)
    assert got == (b"ACGAACGC", b"III?II/?", b, qb, 1, 0) == K.loop_correct(a, b"III?II//", b, qb, 8)[:6]
    # exactly at the thresholds on both sides, and one off
    for q_sure, q_poor, fixed in ((b"?", b"/", 1), (b">", b"/", 0), (b"?", b"0", 0)):
        got = f.correct_mates(b"A", q_sure, b"A", q_poor, 1, R)
        assert got == ((b"A", q_sure, b"T", q_sure, 0, 1) if fixed else (b"A", q_sure, b"A", q_poor, 0, 0)) == K.loop_correct(b"A", q_sure, b"A", q_poor, 1)[:6]
        got = f.correct_mates(b"A", q_poor, b"A", q_sure, 1, R)
        assert got == ((b"T", q_sure, b"A", q_sure, 1, 0) if fixed else (b"A", q_poor, b"A", q_sure, 0, 0)) == K.loop_correct(b"A", q_poor, b"A", q_sure, 1)[:6]


def test_correctable_is_the_rule_s_eligibility():
    f = F()
    buf1, buf2 = b"@h\nACGTACGT\n+\nIIIIIIII\n", b"@h\nACGT\n+\nIIII\n"
    p1, p2 = (0, 2, 3, 11, 14, 22), (0, 2, 3, 7, 10, 14)
    for ins, want in ((None, False), (-1, False), (0, False), (1, True), (11, True), (12, False)):
        assert f.correct_correctable(buf1, p1, buf2, p2, ins) is want, ins
    assert f.correct_correctable(buf1, (-5, -5, 3, 11, 14, 22), buf2, p2, 5)            # the header is not asked about
    assert not f.correct_correctable(buf1, (0, 2, 3, 11, 14, 21), buf2, p2, 5)          # two lengths
    assert not f.correct_correctable(buf1, (0, 2, 3, 11, -1, -1), buf2, p2, 5)          # a FASTA row
    assert not f.correct_correctable(buf1, p1, buf2, (0, 2, 3, 7, 10, 99), 5)           # outside


def test_the_value_errors():
    f = F()
    d1, d2 = b"@p/1\nACGT\n+\nIIII\n", b"@p/2\nACGT\n+\nIIII\n"

    def call(**kw):
        return f.filter_fastq_paired(io.BytesIO(d1), io.BytesIO(d2), io.BytesIO(), io.BytesIO(), entrypos=f.entrypos, **kw)
    with pytest.raises(ValueError, match="correction needs overlap"):
        call(correction=f.CorrectionRules())
    with pytest.raises(ValueError, match="correction_report needs correction"):
        call(overlap=f.OverlapRules(), correction_report=f.CorrectionReport())
    with pytest.raises(TypeError):
        call(overlap=f.OverlapRules(), correction=(30, 14))
    with pytest.raises(ValueError, match="qual_base"):
        call(overlap=f.OverlapRules(), correction=f.CorrectionRules(200, 14), qual_base=64)
    for good, bad in ((14, 14), (10, 14), (30, -1), (256, 14)):
        with pytest.raises(ValueError):
            f.CorrectionRules(good, bad)
    r = f.CorrectionRules()
    assert (r.good_quality, r.bad_quality) == (30, 14)


@pytest.mark.parametrize("merge", (False, True))
def test_the_host_route_on_generated_files(merge):
    """filter_fastq_paired(correction=...) with the Python scanner against an expectation assembled from the loop: the files, the
    result, the CorrectionReport; with and without merged_out"""
    f = F()
    recs1, recs2 = K.records(500)
    want = K.Expected(recs1, recs2, min_len=(40, 40), merge=merge)
    assert want.shows_something(), (want.counts, want.uncorrected)
    assert sum(want.dropped.values()) > 0 and (want.pairs_merged > 100) == merge
    res, t1, t2, tm, crep, _orep, reps = K.run(f, K.file_of(recs1), K.file_of(recs2), f.entrypos, 1 << 14, merge=merge, min_len=40)
    assert (t1, t2, tm) == tuple(want.text)
    assert tuple(res) == want.result()
    want.check_report(crep)
    # the correction changed what is written: the same run without it writes other bytes
    plain = K.Expected(recs1, recs2, min_len=(40, 40), merge=merge, correct=False)
    # ... unless every pair with an overlap is merged: the merge takes the surer call at a mismatch itself, so a merged record
    # reads the same with or without the correction in front of it
    assert (plain.text != want.text) == (not merge) and [len(x) for x in plain.text] == [len(x) for x in want.text]
    # `before` is of the records as read, `after` of the records as written
    assert int(reps[0].before.head[0]) + int(reps[0].before.head[1]) == len(recs1)


def test_without_correction_nothing_changes():
    """the bytes and the result of the call as it was before the correction existed: the overlap tests' own expectation"""
    f = F()
    recs1, recs2 = X.records(300)
    want = X.Expected(recs1, recs2, min_len=(20, 20))
    res, t1, t2, rep = X.run(f, K.file_of(recs1), K.file_of(recs2), f.entrypos, 1 << 14, min_len=20)
    assert (t1, t2) == tuple(want.text) and tuple(res) == want.result()
    want.check_report(rep)
    recs1, recs2 = K.records(300)
    plain = K.Expected(recs1, recs2, min_len=(40, 40), correct=False)
    res, t1, t2, _tm, crep, _orep, _reps = K.run(f, K.file_of(recs1), K.file_of(recs2), f.entrypos, 1 << 14, correct=False, min_len=40)
    assert crep is None and (t1, t2) == (plain.text[0], plain.text[1]) and tuple(res) == plain.result()


def test_after_counts_the_corrected_bytes():
    """report.after is of the records as written: a corrected base is counted in its new class"""
    f = F()
    # mate 2's reverse complement is ACGTACGTACGTACGTACGTACGTACGTACGTACGT but for one base (a T where mate 1 has an A), poor
    s1 = b"ACGTACGTACGTACGTACGTACGTACGTACGTACGT"
    s2 = bytearray(X.revcomp(s1))
    assert s2[3] == ord("T") and s1[-4] == ord("A")
    s2[3] = ord("G")
    q1, q2 = b"I" * 36, bytearray(b"I" * 36)
    q2[3] = ord("#")
    d1, d2 = b"@p/1\n" + s1 + b"\n+\n" + q1 + b"\n", b"@p/2\n" + bytes(s2) + b"\n+\n" + bytes(q2) + b"\n"
    o1, o2 = io.BytesIO(), io.BytesIO()
    r1, r2, crep = f.FilterReport(), f.FilterReport(), f.CorrectionReport()
    f.filter_fastq_paired(io.BytesIO(d1), io.BytesIO(d2), o1, o2, entrypos=f.entrypos, overlap=f.OverlapRules(30, 5, 200),
                          correction=f.CorrectionRules(), correction_report=crep, report=r1, report2=r2)
    assert o1.getvalue() == d1 and o2.getvalue() == b"@p/2\n" + X.revcomp(s1) + b"\n+\n" + b"I" * 36 + b"\n"
    assert (crep.pairs_checked, crep.pairs_corrected, crep.bases_corrected, crep.mismatches) == (1, 1, [0, 1], 1)
    assert crep.matrix[2][3] == 1 and crep.matrix.sum() == 1              # a G became a T
    assert r2.before != r2.after and r1.before == r1.after

"""filter_fastq_paired(correction=...) on the device: two streams walked in lockstep (hip.PairStream, ffq_pair_set_correct) against
the host route and against the plain loops of tests/correct_expect.py -- three output files, result, CorrectionReport,
OverlapReport and FilterReports.  The fills are small and mate 2's headers are longer than mate 1's, so a run takes many rounds,
the two files' fills drift and the rounds cut them at different places: a mate's fill is corrected over several rounds."""
import gzip
import io

import pytest

import correct_expect as K

pytestmark = pytest.mark.gpu

N_PAIRS = 1500
MIN_LEN = 40


@pytest.fixture(scope="module")
def F(pkg):
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


@pytest.fixture(scope="module")
def C(gpu_ctx):
    from fastqandfurious_amd import _fastqandfurious
    return _fastqandfurious


def recs_of(case):
    if case == "dedup":                      # every fifth pair once more, far behind its first copy
        r1, r2 = K.records(N_PAIRS, wrapped=False)
        return r1 + r1[::5], r2 + r2[::5]
    return K.records(N_PAIRS, wrapped=case != "quality")


CASES = {"plain": {}, "merged": dict(merge=True), "quality": dict(quality_cutoff=20), "dedup": dict(dedup=True),
         "merged dedup quality": dict(merge=True, dedup=True, quality_cutoff=20)}


def kw_of(F, case):
    kw = dict(CASES[case], min_len=MIN_LEN)
    if kw.get("dedup"):
        kw["dedup"] = F.DedupRules()
    return kw


def same_reports(got, want):
    (gc, go, gr), (wc, wo, wr) = got, want
    assert {k: v for k, v in gc.__dict__.items() if k != "matrix"} == {k: v for k, v in wc.__dict__.items() if k != "matrix"}
    assert (gc.matrix == wc.matrix).all()
    assert {k: v for k, v in go.__dict__.items() if k != "insert_hist"} == {k: v for k, v in wo.__dict__.items() if k != "insert_hist"}
    assert (go.insert_hist == wo.insert_hist).all()
    for x, y in zip(gr, wr):
        assert x.before == y.before and x.after == y.after and x.dropped == y.dropped


@pytest.mark.parametrize("case", list(CASES))
def test_device_and_host_write_the_same_three_files(F, C, case):
    r1, r2 = recs_of("quality" if "quality" in case else case)
    if "dedup" in case and "quality" in case:
        r1, r2 = r1 + r1[::5], r2 + r2[::5]
    d1, d2 = K.file_of(r1), K.file_of(r2)
    c = CASES[case]
    want = K.Expected(r1, r2, min_len=(MIN_LEN, MIN_LEN), merge=c.get("merge", False), quality_cutoff=c.get("quality_cutoff"),
                      dedup=c.get("dedup", False))
    assert want.shows_something(), (want.counts, want.uncorrected)
    assert (want.pairs_merged > 300) == c.get("merge", False) and (want.duplicates > 100) == c.get("dedup", False)
    host = K.run(F, d1, d2, F.entrypos, 1 << 14, **kw_of(F, case))
    assert host[1:4] == tuple(want.text) and tuple(host[0]) == want.result()
    want.check_report(host[4])
    for fbufsize in (1 << 14, 3 << 13):
        res, o1, o2, om, crep, orep, reps = K.run(F, d1, d2, C.entrypos, fbufsize, **kw_of(F, case))
        assert (o1, o2, om) == tuple(want.text) == host[1:4]
        assert tuple(res) == want.result() == tuple(host[0])
        want.check_report(crep)
        same_reports((crep, orep, reps), host[4:])


def test_many_rounds_and_drifting_fills(F, C):
    """what the comparison above relies on: at this fill size a run takes many rounds, and the two mates' fills end at different
    records -- a fill of one mate is corrected in pieces, round after round"""
    from fastqandfurious_amd import hip
    r1, r2 = K.records(N_PAIRS)
    st1, st2 = C.entrypos.open_stream(io.BytesIO(K.file_of(r1)), 1 << 14), C.entrypos.open_stream(io.BytesIO(K.file_of(r2)), 1 << 14)
    ps = hip.PairStream(st1, st2, "any", True)
    try:
        with pytest.raises(hip.FFQError) as ei:                    # needs the overlap
            ps.set_correct(F.CorrectionRules())
        assert ei.value.code == hip.E_ARG
        with pytest.raises(hip.FFQError) as ei:                    # not switched on: nothing to report
            ps.corrected()
        assert ei.value.code == hip.E_ARG
        ps.set_overlap(F.OverlapRules())
        with pytest.raises(hip.FFQError) as ei:                    # rules out of range
            ps.set_correct(hip.CorrectRulesStruct(14, 14, 33))
        assert ei.value.code == hip.E_ARG
        ps.set_correct(F.CorrectionRules())
        rounds, total, sizes = 0, [0] * 6, set()
        for n_in, n_out, end_state, _mate, _err in ps:
            assert end_state in (hip.END_OK, hip.END_REFILL)
            counts, matrix = ps.corrected()
            assert counts[0] + counts[5] == n_in and n_out == n_in
            total = [a + b for a, b in zip(total, counts)]
            assert int(matrix.sum()) == total[2] + total[3]           # the matrix sums over the rounds
            sizes.add(n_in)
            rounds += 1
            if rounds == 1:
                with pytest.raises(hip.FFQError) as ei:            # the walk has begun
                    ps.set_correct(F.CorrectionRules())
                assert ei.value.code == hip.E_ARG
                with pytest.raises(hip.FFQError) as ei:
                    ps.set_correct(None)
                assert ei.value.code == hip.E_ARG
        want = K.Expected(r1, r2)
        assert rounds > 40 and len(sizes) > 5
        assert total[:5] == want.counts and total[0] + total[5] == len(r1)
    finally:
        ps.close()
        st1.close()
        st2.close()


def test_compressed_outputs_hold_the_corrected_text(F, C):
    """compress="bgzf": each of the three files inflates to the text the uncompressed run writes -- the deflate sees corrected bytes"""
    r1, r2 = K.records(N_PAIRS)
    d1, d2 = K.file_of(r1), K.file_of(r2)
    for merge in (False, True):
        want = K.Expected(r1, r2, min_len=(MIN_LEN, MIN_LEN), merge=merge)
        res, o1, o2, om, crep, _orep, _reps = K.run(F, d1, d2, C.entrypos, 1 << 14, merge=merge, min_len=MIN_LEN, compress="bgzf")
        assert tuple(gzip.decompress(x) for x in (o1, o2)) == tuple(want.text[:2])
        assert (gzip.decompress(om) if merge else om) == want.text[2]
        assert tuple(res) == want.result()
        want.check_report(crep)
        hres, h1, h2, hm, hrep, _ho, _hr = K.run(F, d1, d2, F.entrypos, 1 << 14, merge=merge, min_len=MIN_LEN, compress="bgzf")
        assert tuple(gzip.decompress(x) for x in (h1, h2)) == tuple(want.text[:2]) and tuple(hres) == tuple(res)
        assert hrep.__dict__.keys() == crep.__dict__.keys() and (hrep.matrix == crep.matrix).all()


def test_correction_needs_overlap(F, C):
    with pytest.raises(ValueError, match="correction needs overlap"):
        F.filter_fastq_paired(io.BytesIO(b""), io.BytesIO(b""), io.BytesIO(), io.BytesIO(), entrypos=C.entrypos, correction=F.CorrectionRules())
    with pytest.raises(ValueError, match="correction_report needs correction"):
        F.filter_fastq_paired(io.BytesIO(b""), io.BytesIO(b""), io.BytesIO(), io.BytesIO(), entrypos=C.entrypos, overlap=F.OverlapRules(),
                              correction_report=F.CorrectionReport())

"""filter_fastq_paired(overlap=...) on the device: two streams walked in lockstep (hip.PairStream, ffq_pair_set_overlap) against
the plain loops of tests/overlap_expect.py -- output bytes, result and OverlapReport.  The fills are a few KiB and mate 2's
headers are longer than mate 1's, so the two files' fills drift and the rounds cut them at different places."""
import io

import numpy as np
import pytest

import overlap_expect as X
import pairs_expect as P

pytestmark = pytest.mark.gpu

FBUF = 6000


@pytest.fixture(scope="module")
def F(pkg):
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


@pytest.fixture(scope="module")
def C(gpu_ctx):
    from fastqandfurious_amd import _fastqandfurious
    return _fastqandfurious


def file_opener(tmp_path, name):
    def opener(data):
        p = tmp_path / name
        p.write_bytes(data)
        return open(p, "rb")
    return opener


def test_overlap_alone_against_the_loop(F, C, tmp_path):
    r1, r2 = X.records(1200, 5)
    want = X.Expected(r1, r2, min_len=(40, 40))
    assert want.kinds == {"none", "cut", "kept"} and want.trimmed > 0 and all(want.bases) and want.dropped["both"] > 0
    res, o1, o2, rep = X.run(F, P.fastq(r1), P.fastq(r2), C.entrypos, FBUF, opener1=file_opener(tmp_path, "r1.fq"),
                             opener2=file_opener(tmp_path, "r2.fq"), min_len=40)
    assert o1 == want.text[0] and o2 == want.text[1]
    assert tuple(res) == want.result()
    want.check_report(rep)
    assert rep.insert_peak is not None


def test_the_rounds_cut_the_fills_at_different_places(F, C, gpu_ctx, tmp_path):
    """the walk under the overlap: many rounds, either mate ahead at some time, the counts of every round and the running
    histogram add up to the loop's"""
    from fastqandfurious_amd import hip
    r1, r2 = X.records(1200, 5)
    want = X.Expected(r1, r2)
    fh1, fh2 = file_opener(tmp_path, "a.fq")(P.fastq(r1)), file_opener(tmp_path, "b.fq")(P.fastq(r2))
    st1, st2 = C.entrypos.open_stream(fh1, FBUF), C.entrypos.open_stream(fh2, FBUF)
    ps = hip.PairStream(st1, st2, "any", True)
    try:
        with pytest.raises(hip.FFQError) as ei:                    # not switched on: nothing to report
            ps.overlap()
        assert ei.value.code == hip.E_ARG
        with pytest.raises(hip.FFQError) as ei:
            ps.set_overlap(hip.OverlapRulesStruct(0, 5, 200, 1))
        assert ei.value.code == hip.E_ARG
        ps.set_overlap(F.OverlapRules(*X.DEFAULT))
        total, sizes, seen_hist = [0] * 6, [], 0
        for n_in, n_out, end_state, err_mate, err_offset in ps:
            assert end_state in (hip.END_OK, hip.END_REFILL)
            counts, hist = ps.overlap()
            assert counts[0] + counts[5] == n_in and counts[5] == 0 and n_out == n_in
            total = [a + b for a, b in zip(total, counts)]
            assert int(hist.sum()) == total[1] >= seen_hist
            seen_hist = int(hist.sum())
            sizes.append(n_in)
        assert total == [want.analysed, want.overlapped, want.trimmed, want.bases[0], want.bases[1], 0]
        assert (hist == want.hist).all()
        assert len(sizes) > 40 and len(set(sizes)) > 3 and sum(sizes) == 1200
        with pytest.raises(hip.FFQError) as ei:                    # the walk has begun
            ps.set_overlap(F.OverlapRules())
        assert ei.value.code == hip.E_ARG
    finally:
        ps.close()
        st1.close()
        st2.close()
        fh1.close()
        fh2.close()


def test_order_of_the_stages(F, C, tmp_path):
    """quality, adapter, overlap, filter"""
    r1, r2 = X.records(800, 6)
    kw = dict(quality_cutoff=(5, 10), adapters=(P.ADAPTER1, P.ADAPTER2), min_len=(40, 35))
    want = X.Expected(r1, r2, **kw)
    assert want.trimmed > 0 and X.Expected(r1, r2, use_overlap=False, **kw).text != want.text
    res, o1, o2, rep = X.run(F, P.fastq(r1), P.fastq(r2), C.entrypos, FBUF, opener1=file_opener(tmp_path, "r1.fq"),
                             opener2=file_opener(tmp_path, "r2.fq"), quality_cutoff=(5, 10), adapter=P.ADAPTER1, adapter2=P.ADAPTER2,
                             min_len=(40, 35))
    assert (o1, o2) == (want.text[0], want.text[1]) and tuple(res) == want.result()
    want.check_report(rep)


def test_without_overlap_nothing_differs(F, C):
    r1, r2 = X.records(400, 7)
    d1, d2 = P.fastq(r1), P.fastq(r2)
    res, o1, o2, rep = X.run(F, d1, d2, C.entrypos, FBUF, rules=None, min_len=40)
    p1, p2 = io.BytesIO(), io.BytesIO()
    plain = F.filter_fastq_paired(io.BytesIO(d1), io.BytesIO(d2), p1, p2, fbufsize=FBUF, entrypos=C.entrypos, min_len=40)
    assert (o1, o2, tuple(res)) == (p1.getvalue(), p2.getvalue(), tuple(plain))
    want = X.Expected(r1, r2, min_len=(40, 40), use_overlap=False)
    assert (o1, o2) == (want.text[0], want.text[1]) and tuple(res) == want.result()


def test_smoke_case_of_the_issue(F, C, tmp_path):
    """two files, no adapter named: adapter-free mates and an insert peak"""
    rng = np.random.default_rng(9)
    recs1, recs2 = [], []
    for i in range(300):
        s1, s2 = X.mates_of(rng, int(rng.normal(110, 4)), 150, 150)
        recs1.append((b"p%d/1" % i, s1, b"I" * 150))
        recs2.append((b"p%d/2" % i, s2, b"I" * 150))
    o1, o2 = io.BytesIO(), io.BytesIO()
    rep = F.OverlapReport()
    res = F.filter_fastq_paired(io.BytesIO(P.fastq(recs1)), io.BytesIO(P.fastq(recs2)), o1, o2, fbufsize=FBUF, entrypos=C.entrypos,
                                overlap=F.OverlapRules(), overlap_report=rep)
    assert res.pairs_out == 300 and rep.pairs_trimmed == 300 and 100 <= rep.insert_peak <= 120
    assert P.ADAPTER1 not in o1.getvalue() and P.ADAPTER2 not in o2.getvalue()
    assert res.bases_removed == sum(rep.bases_removed) == sum(150 - len(s) for o in (o1, o2) for s in o.getvalue().split(b"\n")[1::4])

"""filter_fastq and filter_fastq_paired with `ends` on the device route (the stream front end, ffq_stream_set_ends) against the
host route, whose output tests/test_ends_plan.py holds against the rule's loop: output bytes, result tuples and EndsReport, over
files of several fills.  The stream's own setter and its rules."""
import gzip
import io

import pytest

import ends_expect as E
import pairs_expect as P
from test_ends_plan import MIN_LEN, PAIR_ENDS, PAIRED, SINGLE, run_paired, run_single, want_single

FBUF = 1 << 16


@pytest.fixture(scope="module")
def F(pkg):
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


@pytest.fixture(scope="module")
def C(gpu_ctx):
    from fastqandfurious_amd import _fastqandfurious
    return _fastqandfurious


@pytest.fixture(scope="module")
def single_data():
    data = E.fastq(E.single_records())
    assert len(data) > 4 * FBUF                      # several fills
    return data


@pytest.mark.gpu
@pytest.mark.parametrize("kw", SINGLE, ids=lambda kw: "-".join(sorted(kw)))
def test_filter_fastq_gpu_scanner(F, C, single_data, kw):
    want = want_single(kw)
    hres, htext, hrep = run_single(F, io.BytesIO(single_data), F.entrypos, 1 << 14, **kw)
    res, text, rep = run_single(F, io.BytesIO(single_data), C.entrypos, FBUF, **kw)
    assert text == htext and text == want.text
    assert res == hres and res == want.result()
    assert rep.__dict__ == hrep.__dict__ and (rep.reads_cut, rep.bases_cut) == (want.reads_cut, want.bases_cut)


@pytest.mark.gpu
def test_every_step_switched_on(F, C, single_data):
    """quality trim, adapter, poly-G, poly-X, content rules, a report and BGZF output beside the ends step: the same text, the
    same counts on both routes"""
    kw = dict(quality_cutoff=(5, 15), adapter=P.ADAPTER1, poly_g=10, poly_x=10, min_len=MIN_LEN, compress="bgzf")
    outs = []
    for entrypos, fbufsize in ((F.entrypos, 1 << 14), (C.entrypos, FBUF)):
        out, erep, prep, rep, crep = io.BytesIO(), F.EndsReport(), F.PolyReport(), F.FilterReport(), F.CompressReport()
        res = F.filter_fastq(io.BytesIO(single_data), out, fbufsize, entrypos=entrypos, ends=E.pkg_rules(F, E.ALL3), ends_report=erep,
                             poly_report=prep, report=rep, compress_report=crep,
                             content=F.ContentRules(max_n=0, min_mean_quality=35, min_complexity=72), **kw)
        outs.append((tuple(res), gzip.decompress(out.getvalue()), erep.__dict__, prep.__dict__, dict(rep.dropped), rep.before.words.tolist(),
                     rep.after.words.tolist(), crep.bytes_in))
    assert outs[0] == outs[1]
    res, text = outs[0][:2]
    assert 0 < res[1] < res[0] and len(text) == res[3] == outs[0][7] and outs[0][2]["reads_cut"] > 300
    assert sum(outs[0][4].values()) == res[0] - res[1] and sum(1 for k, v in outs[0][4].items() if v) >= 4
    # without the ends step other bytes come out: it is not a step the others make up for
    out = io.BytesIO()
    F.filter_fastq(io.BytesIO(single_data), out, FBUF, entrypos=C.entrypos, content=F.ContentRules(max_n=0, min_mean_quality=35, min_complexity=72), **kw)
    assert gzip.decompress(out.getvalue()) != text


@pytest.mark.gpu
def test_the_stream_and_its_setter(F, C, gpu_ctx, single_data):
    """the stream itself: the rows of every fill are the loop's, ends_trimmed adds up; the setter's rules"""
    from fastqandfurious_amd import hip
    recs = E.single_records()
    cut, reads_cut, bases_cut = E.cut_records(recs, E.ALL3)
    st = C.entrypos.open_stream(io.BytesIO(single_data), FBUF)
    try:
        with pytest.raises(hip.FFQError) as ei:                    # not switched on: nothing to report
            st.ends_trimmed()
        assert ei.value.code == hip.E_ARG
        S = hip.EndsRulesStruct
        good = dict(trim_front=0, trim_tail=0, keep_len=0, qual_base=33, front_window=4, front_quality=20, right_window=4, right_quality=20,
                    tail_window=4, tail_quality=20)
        for bad in (dict(front_window=65), dict(right_window=-1), dict(tail_quality=0), dict(tail_quality=94), dict(trim_front=-1),
                    dict(trim_tail=-1), dict(keep_len=-1), dict(qual_base=256), dict(front_window=0, right_window=0, tail_window=0)):
            with pytest.raises(hip.FFQError, match="ffq_stream_set_ends") as ei:
                st.set_ends(S(**dict(good, **bad)))
            assert ei.value.code == hip.E_ARG, bad
        with pytest.raises(hip.FFQError, match="ffq_stream_set_ends"):
            st.set_ends(None)
        st.set_ends(S(**good))
        seqs, quals, total, fills = [], [], [0, 0, 0], 0
        for rows, fill, off, end_state, _err in st:
            assert end_state in (hip.END_OK, hip.END_REFILL)
            fb = bytes(fill)
            seqs += [fb[r[2] - off:r[3] - off] for r in rows.tolist()]
            quals += [fb[r[4] - off:r[5] - off] for r in rows.tolist()]
            total = [a + b for a, b in zip(total, st.ends_trimmed())]
            fills += 1
        assert fills >= 4 and seqs == [s for _h, s, _q in cut] and quals == [q for _h, _s, q in cut]
        assert total == [reads_cut, bases_cut, 0]
        with pytest.raises(hip.FFQError) as ei:                    # the stream has handed out a fill
            st.set_ends(S(**good))
        assert ei.value.code == hip.E_ARG
    finally:
        st.close()
    st = C.entrypos.open_stream(io.BytesIO(single_data), FBUF, True)       # qualities decoded beside the scan: not with a trim
    try:
        with pytest.raises(hip.FFQError) as ei:
            st.set_ends(E.pkg_rules(F, E.ALL3))
        assert ei.value.code == hip.E_ARG
    finally:
        st.close()


# ---- pairs -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair_files():
    r1, r2 = E.pair_records()
    return E.fastq(r1), E.fastq(r2)


@pytest.mark.gpu
@pytest.mark.parametrize("merge", (True, False))
def test_filter_fastq_paired_gpu_scanner(F, C, pair_files, merge):
    """different EndRules per mate; with merged_out the overlap and the merge see the reads as the ends step left them"""
    fbufsize = 1 << 14
    assert len(pair_files[0]) > 10 * fbufsize
    hres, htexts, hrep = run_paired(F, pair_files[0], pair_files[1], F.entrypos, 1 << 14, PAIR_ENDS, merge=merge, **PAIRED)
    res, texts, rep = run_paired(F, pair_files[0], pair_files[1], C.entrypos, fbufsize, PAIR_ENDS, merge=merge, **PAIRED)
    assert texts == htexts
    assert res == hres
    assert rep.__dict__ == hrep.__dict__ and rep.reads_cut > 200
    assert (len(texts[2]) > 0) == merge
    if merge:
        r1, r2 = E.pair_records()
        want = E.ExpectedPaired(r1, r2, PAIR_ENDS, PAIRED["quality_cutoff"], (P.ADAPTER1, P.ADAPTER2), MIN_LEN, poly_g=10)
        assert list(texts) == want.text and res == want.result()
        # the ends step changes what the overlap finds
        plain = E.ExpectedPaired(r1, r2, (None, None), PAIRED["quality_cutoff"], (P.ADAPTER1, P.ADAPTER2), MIN_LEN, poly_g=10)
        assert plain.text[2] != want.text[2] and plain.merged.pairs_merged != want.merged.pairs_merged

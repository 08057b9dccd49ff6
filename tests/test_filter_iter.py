"""The content rules through the stream front end (ffq_stream_set_content / ffq_stream_filter_counts), filter_fastq(content=)
and entryfunc_contentfilter on the GPU scanner.  The expectation is what the Python-scanner route gives for the same input
(tests/test_filter_host.py checks that route against the plain loop); every comparison is exact."""
import gzip
import io
import os

import numpy as np
import pytest

from test_adapter import AD
from test_stats import mixed_corpus

FBUF = 1 << 13


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """a few hundred mixed reads (wrapped ones, Ns, adapters, bad tails) and one that passes max_n = 0 only because the quality
    trim removes its Ns; (data, path, gz path)"""
    d = tmp_path_factory.mktemp("filter")
    data = mixed_corpus(count=150, seed=41, adapter=AD)
    data += b"@tail_of_n\n" + b"ACGTTGCA" * 6 + b"NNNNN\n+\n" + b"I" * 48 + b"#####\n"
    data += mixed_corpus(count=150, seed=42)
    p, z = d / "reads.fq", d / "reads.fq.gz"
    p.write_bytes(data)
    with gzip.open(str(z), "wb", compresslevel=1) as fh:
        fh.write(data)
    return data, str(p), str(z)


def content(F):
    return F.ContentRules(max_n=0, min_mean_quality=12, qualified_quality=15, max_unqualified_percent=60, max_expected_errors=4.0,
                          min_complexity=20)


@pytest.mark.gpu
@pytest.mark.parametrize("source", ("file", "gz", "bytesio"))
def test_filter_fastq_is_the_python_route(gpu_ctx, reads, source):
    from fastqandfurious_amd import fastqandfurious as F
    data, path, gz = reads
    assert len(data) > 5 * FBUF

    def opened():
        return open(path, "rb") if source == "file" else F.automagic_open(gz) if source == "gz" else io.BytesIO(data)
    for kw in (dict(quality_cutoff=(20, 20), adapter=AD, min_len=30, content=content(F)),
               dict(quality_cutoff=20, min_len=1, max_len=250, content=F.ContentRules(max_n=0)),
               dict(content=F.ContentRules(max_expected_errors=1.0, max_n=2)),
               dict(quality_cutoff=(20, 20), min_len=30)):
        want_out, want_rep = io.BytesIO(), F.FilterReport(200)
        want = F.filter_fastq(io.BytesIO(data), want_out, FBUF, entrypos=F.entrypos, report=want_rep, **kw)
        out, rep = io.BytesIO(), F.FilterReport(200)
        with opened() as fh:
            res = F.filter_fastq(fh, out, FBUF, report=rep, **kw)
        assert res == want and out.getvalue() == want_out.getvalue()
        assert rep.dropped == want_rep.dropped and sum(rep.dropped.values()) == res.records_in - res.records_out
        assert rep.before == want_rep.before and rep.after == want_rep.after
        if "content" not in kw:
            assert set(k for k, v in rep.dropped.items() if v) == {"length"}
    # the first configuration drops for its length, its Ns and its expected errors ...
    rep = F.FilterReport()
    out = io.BytesIO()
    F.filter_fastq(io.BytesIO(data), out, FBUF, quality_cutoff=(20, 20), adapter=AD, min_len=30, content=content(F), report=rep)
    assert rep.dropped["length"] and rep.dropped["n"] and rep.dropped["expected_errors"], rep.dropped
    # ... and judges the TRIMMED read: the one whose Ns the trim removes is written; untrimmed, max_n = 0 drops it
    assert b"@tail_of_n\n" + b"ACGTTGCA" * 6 + b"\n+\n" in out.getvalue()
    assert F.ContentRules(max_n=0).verdict(b"ACGTTGCA" * 6 + b"NNNNN", b"I" * 48 + b"#####") == 2
    out = io.BytesIO()
    F.filter_fastq(io.BytesIO(data), out, FBUF, content=F.ContentRules(max_n=0))
    assert b"@tail_of_n\n" not in out.getvalue()


@pytest.mark.gpu
@pytest.mark.parametrize("column", ("sequence", "header", "quality", "entry"))
@pytest.mark.parametrize("yield_dropped", (True, False))
def test_entryfunc_contentfilter_is_pushed_down(gpu_ctx, reads, column, yield_dropped):
    from fastqandfurious_amd import fastqandfurious as F, _fastqandfurious as C
    data, path, gz = reads
    ef = F.entryfunc_contentfilter(content(F), 20, 300, column, yield_dropped)
    assert F._pushes_down_content(ef) and not F._pushes_down(ef)
    want = list(F.readfastq_iter(io.BytesIO(data), FBUF, ef, F.entrypos))
    assert (None in want) == yield_dropped and 50 < sum(w is not None for w in want) < 290
    with open(path, "rb") as fh:
        assert list(F.readfastq_iter(fh, FBUF, ef, C.entrypos)) == want
    if column == "sequence":
        assert list(F.readfastq_iter(io.BytesIO(data), FBUF, ef, C.entrypos)) == want
        with F.automagic_open(gz) as fh:
            assert list(F.readfastq_iter(fh, FBUF, ef, C.entrypos)) == want


@pytest.mark.gpu
def test_a_subclass_with_its_own_call_is_not_pushed_down(gpu_ctx, reads):
    from fastqandfurious_amd import fastqandfurious as F, _fastqandfurious as C
    data, path, _gz = reads

    class Mine(F.entryfunc_contentfilter):
        def __call__(self, buf, pos, globaloffset=None):
            return pos[3] - pos[2]

    class MyRules(F.ContentRules):
        def verdict(self, sequence, quality):
            return 2 if sequence.startswith(b"A") else 0

    ef = Mine(content(F), 20, 300)
    assert not F._pushes_down_content(ef)
    want = list(F.readfastq_iter(io.BytesIO(data), FBUF, ef, F.entrypos))
    assert all(isinstance(w, int) for w in want) and len(want) == 301
    with open(path, "rb") as fh:
        assert list(F.readfastq_iter(fh, FBUF, ef, C.entrypos)) == want
    ef = F.entryfunc_contentfilter(MyRules(), 20, 300)
    assert not F._pushes_down_content(ef)
    want = list(F.readfastq_iter(io.BytesIO(data), FBUF, ef, F.entrypos))
    with open(path, "rb") as fh:
        assert list(F.readfastq_iter(fh, FBUF, ef, C.entrypos)) == want
    # (a wrapped record is not judged: its sequence holds a newline)
    assert not any(w is not None and w.startswith(b"A") and b"\n" not in w for w in want) and any(w is not None for w in want)


def _run(st, hip):
    """(rows handed out, the counts summed over the fills, records scanned)"""
    rows, total, scanned = [], [0] * 8, 0
    for r, _fill, _off, end, _err in st:
        assert end in (hip.END_OK, hip.END_REFILL)
        rows.append(np.array(r, dtype=np.int64).reshape(-1, 6))
        counts = st.filter_counts()
        idx, n_scanned, _c, _o = st.selected()
        assert sum(counts[:7]) == n_scanned and counts[0] == r.shape[0] == len(idx)
        total = [a + b for a, b in zip(total, counts)]
        scanned += n_scanned
    return np.concatenate(rows), total, scanned


@pytest.mark.gpu
@pytest.mark.parametrize("source", ("file", "push"))
def test_set_content_and_set_filter_in_either_order(gpu_ctx, reads, source):
    from fastqandfurious_amd import fastqandfurious as F, hip
    data, path, _gz = reads
    cr = content(F)
    fd = os.open(path, os.O_RDONLY)

    def stream(decode=False):
        return hip.PushStream(gpu_ctx, io.BytesIO(data), FBUF, decode=decode) if source == "push" else hip.FileStream(gpu_ctx, fd, FBUF, decode=decode)
    try:
        got = []
        for order in ("content first", "filter first", "content only", "filter only"):
            os.lseek(fd, 0, os.SEEK_SET)
            st = stream()
            try:
                if order == "content first":
                    st.set_content(cr)
                    st.set_filter(25, 280)
                elif order == "filter first":
                    st.set_filter(25, 280)
                    st.set_content(cr)
                elif order == "content only":
                    st.set_content(cr)
                else:
                    st.set_filter(25, 280)
                assert st.filtered
                got.append(_run(st, hip))
            finally:
                st.close()
        # what the Python scanner's route keeps
        for (rows, total, scanned), lo, hi, rules in zip(got, (25, 25, None, 25), (280, 280, None, 280), (cr, cr, cr, None)):
            ef = F.entryfunc_contentfilter(rules, lo, hi, "header") if rules is not None else F.entryfunc_lengthfilter(None, lo, hi, "header")
            want = list(F.readfastq_iter(io.BytesIO(data), FBUF, ef, F.entrypos))
            assert scanned == len(want) == 301 and total[0] == rows.shape[0] == sum(w is not None for w in want)
            assert [data[r[0] + 1:r[1]] for r in rows.tolist()] == [w for w in want if w is not None]
        assert (got[0][0] == got[1][0]).all() and got[0][1] == got[1][1]
        assert all(got[0][1][k] > 0 for k in (0, 1, 2, 3, 5, 7)), got[0][1]
        assert got[2][1][1] == 0 and got[2][1][7] > 0
        assert got[3][1][2:] == [0] * 6 and got[3][1][1] > 0                 # without content rules only [0] and [1]
        # refused: on a stream that decodes, behind the first fill, a field outside its range, no filter at all
        os.lseek(fd, 0, os.SEEK_SET)
        st = stream(decode=True)
        try:
            with pytest.raises(hip.FFQError) as e:
                st.set_content(cr)
            assert e.value.code == hip.E_ARG and "FFQ_F_DECODE_QUAL" in str(e.value)
        finally:
            st.close()
        os.lseek(fd, 0, os.SEEK_SET)
        st = stream()
        try:
            with pytest.raises(hip.FFQError) as e:
                st.set_content(hip.ContentRulesStruct(33, 0, 96, 15, -1, 0, -1))
            assert e.value.code == hip.E_ARG
            with pytest.raises(hip.FFQError) as e:
                st.filter_counts()
            assert e.value.code == hip.E_ARG
            next(iter(st))
            with pytest.raises(hip.FFQError) as e:
                st.set_content(cr)
            assert e.value.code == hip.E_ARG and "already" in str(e.value)
        finally:
            st.close()
    finally:
        os.close(fd)

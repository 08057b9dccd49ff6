"""filter_fastq and filter_fastq_paired with poly_g / poly_x: the host route (the Python scanner) against the expectation that
tests/poly_expect.py assembles record by record from plain loops -- quality trim, poly-G, adapter, poly-X, then the overlap, the
length filter and the merge --, and the device route (the stream front end, ffq_stream_set_poly) against the host route: output
bytes, result tuples and PolyReport.  The fills are small: a dozen of them, and a carry inside a tail."""
import gzip
import io

import pytest

import overlap_expect as X
import pairs_expect as P
import poly_expect as E

MIN_LEN = 30
SINGLE = (
    dict(poly_g=10, poly_x=10),
    dict(poly_g=10),
    dict(poly_x=12),
    dict(poly_g=10, poly_x=10, quality_cutoff=(5, 15), adapter=P.ADAPTER1, min_len=MIN_LEN),
    dict(poly_g=8, adapter=P.ADAPTER1, min_len=MIN_LEN),
)


@pytest.fixture(scope="module")
def F(pkg):
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


def run_single(F, fh, entrypos, fbufsize, **kw):
    out, rep = io.BytesIO(), F.PolyReport()
    rep.poly_g_reads = 99                           # (a report is reset, not added to)
    res = F.filter_fastq(fh, out, fbufsize, entrypos=entrypos, poly_report=rep, **kw)
    return tuple(res), out.getvalue(), rep


def want_single(kw):
    kw = dict(kw)
    if "quality_cutoff" not in kw:
        kw["quality_cutoff"] = None
    return E.ExpectedSingle(E.single_records(), **kw)


@pytest.mark.parametrize("kw", SINGLE, ids=lambda kw: "-".join(sorted(kw)))
def test_filter_fastq_python_scanner(F, kw):
    recs = E.single_records()
    want = want_single(kw)
    res, text, rep = run_single(F, io.BytesIO(P.fastq(recs)), F.entrypos, 1 << 14, **kw)
    assert text == want.text
    assert res == want.result()
    E.check_poly_report(rep, want.poly)
    assert sum(want.poly[1::2]) > 2000 and want.removed >= sum(want.poly[1::2])


def test_the_adapter_is_found_because_poly_g_ran_first(F):
    """fragment + adapter + G to the end of the read: behind poly-G the adapter runs into the read's end and is cut; without it
    the G tail stays.  (Here a whole adapter matches either way; what differs is what is left BEHIND the trims: the G tail
    never comes back, and a read whose adapter is cut short by poly-G's walk is only found after it.)"""
    recs = E.single_records()
    base = dict(adapter=P.ADAPTER1, min_len=MIN_LEN)
    with_g = E.ExpectedSingle(recs, poly_g=10, **base)
    without = E.ExpectedSingle(recs, **base)
    differ = [i for i, (a, b) in enumerate(zip(with_g.kept, without.kept)) if a != b]
    assert len(differ) > 50
    res, text, _rep = run_single(F, io.BytesIO(P.fastq(recs)), F.entrypos, 1 << 14, poly_g=10, **base)
    res0, text0, rep0 = run_single(F, io.BytesIO(P.fastq(recs)), F.entrypos, 1 << 14, **base)
    assert text == with_g.text and text0 == without.text and text != text0
    assert res[2] > res0[2] and rep0.__dict__ == F.PolyReport().__dict__
    # hand-made: the adapter's 12th base was already read as G.  An exact match (err_permille 0) of the whole adapter fails on
    # that base; poly-G walks through the tail and -- within its five mismatches -- into the adapter, back to its deepest G,
    # and leaves the fragment + b"AGATC": a prefix of the adapter at the read's end, which the adapter trim then finds
    read = b"ACGTTGCAAGCTTGCATGCAAGTCCATGACGT" + P.ADAPTER1[:11] + b"GG" + b"G" * 40
    fq = b"@one\n" + read + b"\n+\n" + b"I" * len(read) + b"\n"
    _r, plain, _p = run_single(F, io.BytesIO(fq), F.entrypos, 1 << 14, adapter=P.ADAPTER1, err_permille=0, min_overlap=3)
    _r, first, _p = run_single(F, io.BytesIO(fq), F.entrypos, 1 << 14, adapter=P.ADAPTER1, err_permille=0, min_overlap=3, poly_g=10)
    assert plain == fq
    assert first == b"@one\n" + read[:32] + b"\n+\n" + b"I" * 32 + b"\n"


PAIRED = dict(quality_cutoff=(5, 15), adapter=P.ADAPTER1, adapter2=P.ADAPTER2, min_len=MIN_LEN, poly_g=10, poly_x=10)


def run_paired(F, data1, data2, entrypos, fbufsize, **kw):
    o1, o2, om = io.BytesIO(), io.BytesIO(), io.BytesIO()
    rep = F.PolyReport()
    res = F.filter_fastq_paired(io.BytesIO(data1), io.BytesIO(data2), o1, o2, fbufsize=fbufsize, entrypos=entrypos,
                                overlap=F.OverlapRules(*X.DEFAULT), merged_out=om, poly_report=rep, **kw)
    return tuple(res), (o1.getvalue(), o2.getvalue(), om.getvalue()), rep


@pytest.fixture(scope="module")
def pair_files():
    r1, r2 = E.pair_records()
    return P.fastq(r1), P.fastq(r2)


@pytest.fixture(scope="module")
def pair_host(F, pair_files):
    """the host route, once: it does not depend on the size of a fill"""
    return run_paired(F, pair_files[0], pair_files[1], F.entrypos, 1 << 14, **PAIRED)


def test_filter_fastq_paired_python_scanner(F, pair_host):
    r1, r2 = E.pair_records()
    want = E.ExpectedPaired(r1, r2, PAIRED["quality_cutoff"], (P.ADAPTER1, P.ADAPTER2), MIN_LEN, poly_g=10, poly_x=10)
    res, texts, rep = pair_host
    assert list(texts) == want.text
    assert res == want.result()
    E.check_poly_report(rep, want.poly)
    assert want.poly[0] > 50 and want.merged.pairs_merged > 100 and len(want.text[0]) > 0
    # (here the adapter trim and the overlap would have cut the same tails: what the poly steps add is their share of the count)
    assert want.removed > want.poly[1] + want.poly[3] > 1000


# ---- the device route ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def C(gpu_ctx):
    from fastqandfurious_amd import _fastqandfurious
    return _fastqandfurious


@pytest.fixture(scope="module")
def single_files(tmp_path_factory):
    data = P.fastq(E.single_records())
    d = tmp_path_factory.mktemp("poly")
    (d / "s.fq").write_bytes(data)
    with gzip.open(str(d / "s.fq.gz"), "wb", compresslevel=1) as fh:
        fh.write(data)
    return data, str(d / "s.fq"), str(d / "s.fq.gz")


@pytest.mark.gpu
@pytest.mark.parametrize("source", ("file", "gz"))
@pytest.mark.parametrize("kw", SINGLE[:1] + SINGLE[3:], ids=lambda kw: "-".join(sorted(kw)))
def test_filter_fastq_gpu_scanner(F, C, single_files, source, kw):
    data, path, gz = single_files
    fbufsize = 1 << 15
    assert len(data) > 10 * fbufsize
    want = want_single(kw)
    hres, htext, hrep = run_single(F, io.BytesIO(data), F.entrypos, 1 << 14, **kw)
    with (open(path, "rb") if source == "file" else F.automagic_open(gz)) as fh:
        res, text, rep = run_single(F, fh, C.entrypos, fbufsize, **kw)
    assert text == want.text and text == htext
    assert res == want.result() and res == hres
    assert rep.__dict__ == hrep.__dict__
    E.check_poly_report(rep, want.poly)


@pytest.mark.gpu
def test_the_adapter_behind_a_g_tail_gpu_scanner(F, C, single_files):
    data = single_files[0]
    base = dict(adapter=P.ADAPTER1, min_len=MIN_LEN)
    with_g = E.ExpectedSingle(E.single_records(), poly_g=10, **base)
    without = E.ExpectedSingle(E.single_records(), **base)
    res, text, _rep = run_single(F, io.BytesIO(data), C.entrypos, 1 << 15, poly_g=10, **base)
    res0, text0, rep0 = run_single(F, io.BytesIO(data), C.entrypos, 1 << 15, **base)
    assert text == with_g.text and text0 == without.text and text != text0
    assert res == with_g.result() and res0 == without.result() and rep0.__dict__ == F.PolyReport().__dict__
    read = b"ACGTTGCAAGCTTGCATGCAAGTCCATGACGT" + P.ADAPTER1[:11] + b"GG" + b"G" * 40
    fq = (b"@one\n" + read + b"\n+\n" + b"I" * len(read) + b"\n") * 3
    _r, plain, _p = run_single(F, io.BytesIO(fq), C.entrypos, 1 << 15, adapter=P.ADAPTER1, err_permille=0, min_overlap=3)
    _r, first, _p = run_single(F, io.BytesIO(fq), C.entrypos, 1 << 15, adapter=P.ADAPTER1, err_permille=0, min_overlap=3, poly_g=10)
    assert plain == fq and first == (b"@one\n" + read[:32] + b"\n+\n" + b"I" * 32 + b"\n") * 3


@pytest.mark.gpu
@pytest.mark.parametrize("fbufsize", (1 << 13, 1 << 14))
def test_filter_fastq_paired_gpu_scanner(F, C, pair_files, pair_host, fbufsize):
    assert len(pair_files[0]) > 10 * fbufsize
    res, texts, rep = run_paired(F, pair_files[0], pair_files[1], C.entrypos, fbufsize, **PAIRED)
    hres, htexts, hrep = pair_host
    assert texts == htexts
    assert res == hres
    assert rep.__dict__ == hrep.__dict__ and rep.poly_g_reads > 50

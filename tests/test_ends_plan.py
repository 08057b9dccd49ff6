"""filter_fastq and filter_fastq_paired with `ends` on the host route (the Python scanner, entrypos=F.entrypos) against the
expectation that tests/ends_expect.py assembles record by record: the rule's loop first, then what tests/poly_expect.py expects
of the steps behind it -- quality trim, poly-G, adapter, poly-X, the overlap, the length filter, the merge.  Output bytes,
result tuples, EndsReport, and that the counts add up.  The device route: tests/test_ends_stream.py."""
import io

import pytest

import ends_expect as E
import overlap_expect as X
import pairs_expect as P

MIN_LEN = 30
SINGLE = (
    dict(ends=E.ALL3),
    dict(ends=E.SETTINGS["fixed"]),
    dict(ends=E.SETTINGS["window 64"], min_len=1),
    dict(ends=E.ALL3, quality_cutoff=(5, 15), adapter=P.ADAPTER1, poly_g=10, min_len=MIN_LEN),
    dict(ends=E.Rules(trim_front=2, right=(8, 25)), adapter=P.ADAPTER1, poly_x=10, min_len=MIN_LEN),
)


@pytest.fixture(scope="module")
def F(pkg):
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


def run_single(F, fh, entrypos, fbufsize, ends=None, **kw):
    out, rep = io.BytesIO(), F.EndsReport()
    rep.reads_cut = 99                              # (a report is reset, not added to)
    res = F.filter_fastq(fh, out, fbufsize, entrypos=entrypos, ends=E.pkg_rules(F, ends), ends_report=rep, **kw)
    return tuple(res), out.getvalue(), rep


def want_single(kw):
    kw = dict(kw)
    return E.ExpectedSingle(E.single_records(), kw.pop("ends"), **kw)


@pytest.mark.parametrize("kw", SINGLE, ids=lambda kw: "-".join(sorted(kw)))
def test_filter_fastq_python_scanner(F, kw):
    recs = E.single_records()
    want = want_single(kw)
    res, text, rep = run_single(F, io.BytesIO(E.fastq(recs)), F.entrypos, 1 << 14, **kw)
    assert text == want.text
    assert res == want.result()
    assert (rep.reads_cut, rep.bases_cut) == (want.reads_cut, want.bases_cut)
    assert want.reads_cut > 300 and want.bases_cut > 5000 and 0 < res[1] <= res[0] == len(recs)
    # the counts add up: what the ends step cut and what the steps behind it cut from what it left
    assert res[2] == want.bases_cut + want.rest.removed
    if set(kw) == {"ends"}:
        assert want.rest.removed == 0 and sum(len(r[1]) for r in recs) - res[2] == sum(len(s) for s in want.rest.kept)


def test_with_a_report(F):
    recs = E.single_records()
    kw = SINGLE[3]
    out, rep, erep = io.BytesIO(), F.FilterReport(), F.EndsReport()
    res = F.filter_fastq(io.BytesIO(E.fastq(recs)), out, 1 << 14, entrypos=F.entrypos, report=rep, ends_report=erep,
                         **dict(kw, ends=E.pkg_rules(F, kw["ends"])))
    want = want_single(kw)
    assert out.getvalue() == want.text and tuple(res) == want.result()
    # `before` is of the records as read, `after` of those written
    assert rep.before.reads == len(recs) and rep.before.bases == sum(len(r[1]) for r in recs)
    assert rep.after.reads == res.records_out and rep.after.bases == sum(len(s) for s in want.rest.kept if s is not None)
    assert rep.dropped["length"] == len(recs) - res.records_out
    assert (erep.reads_cut, erep.bases_cut) == (want.reads_cut, want.bases_cut)


def test_the_ends_step_runs_first(F):
    """the quality trim sees the read as the ends step left it: the fixed trim takes the 5' bases whatever they are, and what the
    running sum then cuts from the 5' end is counted from there"""
    q = b"I" * 3 + b"#" * 4 + b"I" * 30
    fq = b"@one\n" + b"ACGT" * 9 + b"A\n+\n" + q + b"\n"
    out = io.BytesIO()
    res = F.filter_fastq(io.BytesIO(fq), out, entrypos=F.entrypos, ends=F.EndRules(trim_front=3), quality_cutoff=(20, 20))
    assert out.getvalue() == b"@one\n" + (b"ACGT" * 9 + b"A")[7:] + b"\n+\n" + b"I" * 30 + b"\n" and res.bases_removed == 7
    out = io.BytesIO()
    F.filter_fastq(io.BytesIO(fq), out, entrypos=F.entrypos, quality_cutoff=(20, 20))
    assert out.getvalue() == fq                        # (alone, the running sum stops at the good bases in front)


PAIR_ENDS = (E.Rules(trim_front=1, front=(4, 20), right=(4, 20)), E.Rules(trim_tail=2, keep_len=120, right=(8, 22), tail=(4, 15)))
PAIRED = dict(quality_cutoff=(5, 15), adapter=P.ADAPTER1, adapter2=P.ADAPTER2, min_len=MIN_LEN, poly_g=10)


def run_paired(F, data1, data2, entrypos, fbufsize, ends, merge=True, **kw):
    o1, o2, om = io.BytesIO(), io.BytesIO(), io.BytesIO()
    rep = F.EndsReport()
    ends = tuple(E.pkg_rules(F, r) for r in ends) if isinstance(ends, tuple) and not isinstance(ends, E.Rules) else E.pkg_rules(F, ends)
    res = F.filter_fastq_paired(io.BytesIO(data1), io.BytesIO(data2), o1, o2, fbufsize=fbufsize, entrypos=entrypos,
                                overlap=F.OverlapRules(*X.DEFAULT), merged_out=om if merge else None, ends=ends, ends_report=rep, **kw)
    return tuple(res), (o1.getvalue(), o2.getvalue(), om.getvalue()), rep


def test_filter_fastq_paired_python_scanner(F):
    r1, r2 = E.pair_records()
    res, texts, rep = run_paired(F, E.fastq(r1), E.fastq(r2), F.entrypos, 1 << 14, PAIR_ENDS, **PAIRED)
    want = E.ExpectedPaired(r1, r2, PAIR_ENDS, PAIRED["quality_cutoff"], (P.ADAPTER1, P.ADAPTER2), MIN_LEN, poly_g=10)
    assert list(texts) == want.text
    assert res == want.result()
    assert (rep.reads_cut, rep.bases_cut) == (want.reads_cut, want.bases_cut) and want.reads_cut > 200
    assert want.merged.pairs_merged > 50 and len(want.text[0]) > 0
    assert res[2] == want.bases_cut + want.rest.removed
    # one EndRules for both mates; a mate without
    for ends, both in ((PAIR_ENDS[0], (PAIR_ENDS[0], PAIR_ENDS[0])), ((None, PAIR_ENDS[1]), (None, PAIR_ENDS[1]))):
        res, texts, rep = run_paired(F, E.fastq(r1), E.fastq(r2), F.entrypos, 1 << 14, ends, **PAIRED)
        want = E.ExpectedPaired(r1, r2, both, PAIRED["quality_cutoff"], (P.ADAPTER1, P.ADAPTER2), MIN_LEN, poly_g=10)
        assert list(texts) == want.text and res == want.result()
        assert (rep.reads_cut, rep.bases_cut) == (want.reads_cut, want.bases_cut)

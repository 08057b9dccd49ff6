"""UMIs through the streams: filter_fastq and filter_fastq_paired with `umi=` on the GPU route (ffq_stream_set_umi,
ffq_pair_set_umi: the take in front of every trim, the tag in the rendered names) against the `entrypos=F.entrypos` route, which
carries the UMI with the record, and both against text assembled by the loops of tests/umi_expect.py."""
import gzip
import io

import pytest

import umi_expect as E
from test_umi_host import CASES, rules_of, run_single

FBUF = 1 << 15                # several fills and a carry per file


def dedup_records(recs, rules):
    """... with 60 reads again under another UMI (no duplicates) and 30 full copies (duplicates)"""
    return recs + tuple((h + b"d", s[:rules.length][::-1] + s[rules.length:], q) for h, s, q in recs[:60]) + recs[:30]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("rules", (E.Rules(), E.Rules("read1", 5, 3, b"UMI", b"#")))
def test_filter_fastq_gpu_route(gpu_ctx, rules, case):
    from fastqandfurious_amd import fastqandfurious as F
    recs = E.single_records(3000, 6)
    if CASES[case].get("dedup"):
        recs = dedup_records(recs, rules)
    assert len(E.fastq_text(recs)) > 8 * FBUF
    want = E.ExpectedSingle(recs, rules, **CASES[case])
    host = run_single(F, recs, rules, F.entrypos, FBUF, **CASES[case])
    frep = F.FilterReport()
    res, text, rep = run_single(F, recs, rules, None, FBUF, report=frep, **CASES[case])
    assert text == want.text == host[1] and tuple(res) == want.result() == tuple(host[0])
    for r in (rep, host[2]):
        assert (r.reads_tagged, r.bases_removed, r.reads_skipped) == (want.tagged, want.umi_bases, want.skipped)
    assert want.skipped > 20 and 1000 < want.tagged < want.n_out
    # `before` sees the reads as read, `after` without their UMIs
    assert frep.before.bases == sum(len(s) - s.count(b"\n") for _h, s, _q in recs if 10 not in s)
    if CASES[case].get("dedup"):
        h0, s0, _q0 = next(r for r in recs[:60] if len(r[1]) > 20 and 10 not in r[1] and r[1][:rules.length][::-1] != r[1][:rules.length])
        assert text.count(b"@" + E.loop_name(h0, (s0[:rules.length],), rules) + b"\n") == 1
        assert text.count(b"@" + E.loop_name(h0 + b"d", (s0[:rules.length][::-1],), rules) + b"\n") == 1


@pytest.mark.gpu
def test_filter_fastq_bgzf_behind_the_tagged_render(gpu_ctx):
    from fastqandfurious_amd import fastqandfurious as F
    recs, rules = E.single_records(3000, 6), E.Rules("read1", 8, 0, b"UMI")
    want = E.ExpectedSingle(recs, rules, min_len=1)
    out = io.BytesIO()
    res = F.filter_fastq(io.BytesIO(E.fastq_text(recs)), out, FBUF, umi=rules_of(F, rules), min_len=1, compress="bgzf")
    assert gzip.decompress(out.getvalue()) == want.text and tuple(res) == want.result()


def run_paired(F, r1, r2, rules, entrypos, fbufsize=FBUF, **kw):
    o1, o2, rep = io.BytesIO(), io.BytesIO(), F.UmiReport()
    res = F.filter_fastq_paired(io.BytesIO(E.fastq_text(r1)), io.BytesIO(E.fastq_text(r2)), o1, o2, fbufsize, entrypos=entrypos,
                                umi=rules_of(F, rules), umi_report=rep, **kw)
    return res, (o1.getvalue(), o2.getvalue()), rep


def names(text):
    return [ln[1:] for ln in text.split(b"\n")[0::4] if ln]


@pytest.mark.gpu
@pytest.mark.parametrize("loc", ("read1", "read2", "per_read"))
def test_filter_fastq_paired_gpu_route(gpu_ctx, loc):
    from fastqandfurious_amd import fastqandfurious as F
    r1, r2 = E.pair_records(2000, 9)
    for rules, min_len in ((E.Rules(loc), None), (E.Rules(loc, 6, 2, b"Ab1", b"+"), 25)):
        # (min_len: pairs are dropped, and the tags follow their rows through the pair select)
        want = E.ExpectedPaired(r1, r2, rules, min_len)
        host = run_paired(F, r1, r2, rules, F.entrypos, min_len=min_len)
        res, text, rep = run_paired(F, r1, r2, rules, None, min_len=min_len)
        assert text == want.text == host[1]
        assert (res.pairs_in, res.pairs_out, res.bases_removed) == (want.pairs_in, want.pairs_out, want.removed) == tuple(host[0])[:3]
        assert rep.reads_tagged == host[2].reads_tagged == want.tagged and rep.bases_removed == host[2].bases_removed == want.removed
        assert min_len is None or want.pairs_out < want.pairs_in - 100
        # both outputs in step, both names of a pair with the same insert
        n1, n2 = names(text[0]), names(text[1])
        assert len(n1) == len(n2) == want.pairs_out and n1 == n2


@pytest.mark.gpu
@pytest.mark.parametrize("loc", ("read1", "per_read"))
def test_filter_fastq_paired_with_the_overlap_on(gpu_ctx, loc):
    """the overlap sees the reads without their UMIs, on either route alike; the names are the loop's"""
    import merge_expect as M
    from fastqandfurious_amd import fastqandfurious as F
    m1, m2 = M.records(600, 5)
    # (without the wrapped records: names() below reads the output four lines at a time)
    m1, m2 = zip(*[(a, b) for a, b in zip(m1, m2) if 10 not in a[1] and 10 not in b[1]])
    rules = E.Rules(loc, 6, 1, b"U")
    kw = dict(overlap=F.OverlapRules(), min_len=20, quality_cutoff=(5, 15))
    host = run_paired(F, m1, m2, rules, F.entrypos, **kw)
    res, text, rep = run_paired(F, m1, m2, rules, None, **kw)
    assert text == host[1] and tuple(res)[:5] == tuple(host[0])[:5]
    assert (rep.reads_tagged, rep.bases_removed, rep.reads_skipped) == (host[2].reads_tagged, host[2].bases_removed, host[2].reads_skipped)
    # by position, against the loop: record i of either output is a pair of the input, in input order, the same pair in both files;
    # its name is that pair's header with that pair's tags, and its bases are bases of that read behind its UMI
    want_names, rest = [], []
    for a, b in zip(m1, m2):
        took = [E.take_record(s, q, rules) if loc == "per_read" or k == 0 else (None, s, q) for k, (h, s, q) in enumerate((a, b))]
        tags = [x[0] for k, x in enumerate(took) if loc == "per_read" or k == 0]
        want_names.append(tuple(E.loop_name(h, tuple(tags), rules) if None not in tags else h for h, _s, _q in (a, b)))
        rest.append((took[0][1], took[1][1]))
    at = {n: i for i, n in enumerate(want_names)}
    assert len(at) == len(want_names)
    recs = [list(zip(*[iter(x.split(b"\n")[:-1])] * 4)) for x in text]
    assert len(recs[0]) == len(recs[1]) == res.pairs_out > 100 and rep.reads_tagged > 200
    last = -1
    for (n1, s1, _p1, _q1), (n2, s2, _p2, _q2) in zip(*recs):
        i = at.get((n1[1:], n2[1:]))
        assert i is not None and i > last, (n1, n2)
        assert s1 in rest[i][0] and s2 in rest[i][1], (n1, n2)
        last = i


@pytest.mark.gpu
def test_a_fill_of_short_records_renders_longer_than_it_was(gpu_ctx):
    """len = 64, a prefix of 16, read1: mate 2 gives no bases and gains 82 bytes a record -- its text is several times its fill, and
    nothing is cut short"""
    import numpy as np
    from fastqandfurious_amd import fastqandfurious as F
    rng = np.random.default_rng(2)
    r1 = tuple((b"%d" % i, E.body_of(rng, 64 + i % 3), b"I" * (64 + i % 3)) for i in range(3000))
    r2 = tuple((h, b"ACG"[:1 + i % 3], b"III"[:1 + i % 3]) for i, (h, _s, _q) in enumerate(r1))
    rules = E.Rules("read1", 64, 0, E.P16)
    want = E.ExpectedPaired(r1, r2, rules)
    for fbufsize in (1 << 20, 1 << 13):
        res, text, rep = run_paired(F, r1, r2, rules, None, fbufsize)
        assert text == want.text and len(text[1]) > 5 * len(E.fastq_text(r2)) and rep.reads_tagged == 6000

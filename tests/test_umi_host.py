"""UMIs on the host: umi_take, umi_name, umi_takable and index.umi_rows against the loops of tests/umi_expect.py, the argument
errors of filter_fastq / filter_fastq_paired, and both filters with `entrypos=F.entrypos` (the route that carries the UMI with
the record) against text assembled by the loop."""
import io

import numpy as np
import pytest

import umi_expect as E


def rules_of(F, r):
    return F.UmiRules(r.loc, r.length, r.skip, r.prefix, r.delim)


def test_umi_take_and_umi_name_equal_the_loop(pkg):
    from fastqandfurious_amd import fastqandfurious as F
    for seq, length, skip, tag, rest in E.HAND_TAKE:
        qual = bytes(33 + (j % 40) for j in range(len(seq)))
        assert F.umi_take(seq, qual, F.UmiRules("read1", length, skip)) == (tag, rest, qual[len(seq) - len(rest):]) == E.loop_take(seq, qual, length, skip)
    for header, tags, prefix, delim, want in E.HAND_NAME:
        r = E.Rules("per_read" if len(tags) == 2 else "read1", len(tags[0]), 0, prefix, delim)
        assert F.umi_name(header, tags, rules_of(F, r)) == want == E.loop_name(header, tags, r), header
    rng = np.random.default_rng(4)
    for _ in range(300):
        h = bytes(rng.choice(np.frombuffer(b"ab \t:/1", dtype=np.uint8), int(rng.integers(0, 12))))
        r = E.Rules("read1", 4, 0, (b"", b"Zz9")[int(rng.integers(0, 2))], b"+")
        assert F.umi_name(h, (b"ACGT",), rules_of(F, r)) == E.loop_name(h, (b"ACGT",), r), h


def test_umi_rows_equal_the_loop(pkg):
    from fastqandfurious_amd import index as X, fastqandfurious as F
    buf, rows, n_bad = E.hand_table()
    sbuf, srows = E.seeded_table()
    for length, skip in ((1, 0), (8, 3), (64, 64)):
        r = F.UmiRules("read1", length, skip)
        want, stats = E.loop_take_rows(buf, rows, length, skip)
        got = X.umi_rows(buf, np.array(rows, dtype=np.int64), r)
        assert got.shape == want.shape and (got == want).all()
        rows2 = np.array(rows, dtype=np.int64) + 1000
        rows2[np.array(rows) < 0] = -1
        want2 = want + 1000
        want2[want < 0] = -1
        assert (X.umi_rows(buf, rows2, r, shift=1000) == want2).all()
        assert (X.umi_rows(sbuf, np.array(srows, dtype=np.int64), r) == E.seeded_want(length, skip)[0]).all()
        assert sum(1 for x in rows if not F.umi_takable(buf, x)) == stats[2] == n_bad
        assert sum(1 for x in srows if not F.umi_takable(sbuf, x)) == E.seeded_want(length, skip)[1][2]


def test_argument_errors(pkg):
    from fastqandfurious_amd import fastqandfurious as F
    for name, bad in (("loc", dict(loc="read3")), ("loc", dict(loc=1)), ("length", dict(length=0)), ("length", dict(length=65)),
                      ("length", dict(length=8.0)), ("skip", dict(skip=-1)), ("skip", dict(skip=65)), ("prefix", dict(prefix=b"A" * 17)),
                      ("prefix", dict(prefix=b"a-b")), ("prefix", dict(prefix="UMI")), ("delim", dict(delim=b" ")), ("delim", dict(delim=b"::")),
                      ("delim", dict(delim=b"")), ("delim", dict(delim=b"\x7f"))):
        with pytest.raises(ValueError, match=name):
            F.UmiRules(**bad)
        # a rule that went out of range after it was made: the filters name the setting before anything is opened or read
        r = F.UmiRules()
        for k, v in bad.items():
            setattr(r, k, v)
        fh = io.BytesIO(b"@a\nACGT\n+\nIIII\n")
        with pytest.raises(ValueError, match="umi.*" + name):
            F.filter_fastq(fh, io.BytesIO(), entrypos=F.entrypos, umi=r)
        assert fh.tell() == 0
    for loc in ("read2", "per_read"):
        fh = io.BytesIO(b"@a\nACGT\n+\nIIII\n")
        with pytest.raises(ValueError, match="umi"):
            F.filter_fastq(fh, io.BytesIO(), entrypos=F.entrypos, umi=F.UmiRules(loc))
        with pytest.raises(ValueError, match="umi"):
            F.filter_fastq(fh, io.BytesIO(), umi=F.UmiRules(loc))          # (the GPU route: refused before a stream is opened)
        assert fh.tell() == 0
    fh1, fh2 = io.BytesIO(b"@a\nACGT\n+\nIIII\n"), io.BytesIO(b"@a\nACGT\n+\nIIII\n")
    with pytest.raises(ValueError, match="umi"):
        F.filter_fastq_paired(fh1, fh2, io.BytesIO(), io.BytesIO(), entrypos=F.entrypos, umi=F.UmiRules(), overlap=F.OverlapRules(),
                              merged_out=io.BytesIO())
    with pytest.raises(ValueError, match="umi_report"):
        F.filter_fastq_paired(fh1, fh2, io.BytesIO(), io.BytesIO(), entrypos=F.entrypos, umi_report=F.UmiReport())
    with pytest.raises(TypeError):
        F.filter_fastq(fh1, io.BytesIO(), entrypos=F.entrypos, umi=E.Rules())
    with pytest.raises(TypeError):
        F.filter_fastq(fh1, io.BytesIO(), entrypos=F.entrypos, umi=F.UmiRules(), umi_report=object())
    assert fh1.tell() == 0 and fh2.tell() == 0


CASES = (dict(), dict(min_len=20), dict(front=2, quality_cutoff=(5, 20), adapter=b"AGATCGGAAGAGC", min_len=15), dict(dedup=True))


def run_single(F, recs, rules, entrypos, fbufsize=1 << 16, front=0, quality_cutoff=None, adapter=None, min_len=None, dedup=False, **kw):
    out, rep = io.BytesIO(), F.UmiReport()
    res = F.filter_fastq(io.BytesIO(E.fastq_text(recs)), out, fbufsize, entrypos=entrypos, umi=rules_of(F, rules), umi_report=rep,
                         ends=F.EndRules(trim_front=front) if front else None, quality_cutoff=quality_cutoff, adapter=adapter, min_len=min_len,
                         dedup=F.DedupRules() if dedup else None, **kw)
    return res, out.getvalue(), rep


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("rules", (E.Rules(), E.Rules("read1", 5, 3, b"UMI", b"#")))
def test_filter_fastq_host_route(pkg, rules, case):
    from fastqandfurious_amd import fastqandfurious as F
    recs = E.single_records()
    if CASES[case].get("dedup"):
        recs = recs + tuple((h + b"d", s[:rules.length][::-1] + s[rules.length:], q) for h, s, q in recs[:60]) + recs[:30]
    want = E.ExpectedSingle(recs, rules, **CASES[case])
    res, text, rep = run_single(F, recs, rules, F.entrypos, **CASES[case])
    assert text == want.text and tuple(res) == want.result()
    assert (rep.reads_tagged, rep.bases_removed, rep.reads_skipped) == (want.tagged, want.umi_bases, want.skipped)
    assert want.skipped > 3 and want.tagged < want.n_out and want.tagged > 100
    if CASES[case].get("dedup"):
        # two reads that differ only in their UMI both survive; a full copy does not
        h0, s0, _q0 = next(r for r in recs[:60] if len(r[1]) > 20 and 10 not in r[1] and r[1][:rules.length][::-1] != r[1][:rules.length])
        assert text.count(b"@" + E.loop_name(h0, (s0[:rules.length],), rules) + b"\n") == 1            # (its full copy is dropped)
        assert text.count(b"@" + E.loop_name(h0 + b"d", (s0[:rules.length][::-1],), rules) + b"\n") == 1
        assert len(E.single_records()) + 40 < want.n_out <= len(recs) - 25


@pytest.mark.parametrize("loc", ("read1", "read2", "per_read"))
def test_filter_fastq_paired_host_route(pkg, loc):
    from fastqandfurious_amd import fastqandfurious as F
    r1, r2 = E.pair_records()
    for rules, min_len in ((E.Rules(loc), None), (E.Rules(loc, 6, 2, b"Ab1", b"+"), 25)):
        want = E.ExpectedPaired(r1, r2, rules, min_len)
        o1, o2, rep = io.BytesIO(), io.BytesIO(), F.UmiReport()
        res = F.filter_fastq_paired(io.BytesIO(E.fastq_text(r1)), io.BytesIO(E.fastq_text(r2)), o1, o2, 1 << 16, entrypos=F.entrypos,
                                    umi=rules_of(F, rules), umi_report=rep, min_len=min_len)
        assert (o1.getvalue(), o2.getvalue()) == want.text
        assert (res.pairs_in, res.pairs_out, res.bases_removed) == (want.pairs_in, want.pairs_out, want.removed)
        assert rep.reads_tagged == want.tagged and rep.bases_removed == want.removed and 0 < want.tagged < 2 * want.pairs_out + int(min_len is not None)

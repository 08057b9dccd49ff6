"""The content rules on the host: EE_MICRO, ContentRules, entryfunc_contentfilter and filter_fastq(content=...) with the
Python scanner.  The expectation is the plain loop of tests/test_filter.py (content_verdict: the rule of include/ffq.h byte
by byte), never ContentRules itself."""
import io
from decimal import Decimal, getcontext

import numpy as np
import pytest

from test_filter import EDGES, EE, OFF, content_verdict, one_read, quantities, rules


@pytest.fixture(scope="module")
def F(pkg):
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


def as_rules(cr):
    """a ContentRules as the loop takes the rules"""
    return {k: getattr(cr, k) for k in OFF}


def test_ee_micro_is_the_formula(F):
    getcontext().prec = 50
    assert len(F.EE_MICRO) == 96 and list(F.EE_MICRO) == EE
    for v, x in enumerate(F.EE_MICRO):
        exact = Decimal(10 ** 6) * Decimal(10) ** (Decimal(-v) / Decimal(10))
        assert x == int((exact + Decimal("0.5")).to_integral_value(rounding="ROUND_FLOOR")), v
        frac = exact - int(exact)
        assert abs(frac - Decimal("0.5")) > Decimal("0.001"), v          # no entry near a rounding boundary
    assert F.EE_MICRO[0] == 10 ** 6 and F.EE_MICRO[10] == 10 ** 5 and F.EE_MICRO[63] == 1 and not any(F.EE_MICRO[64:])


def make(F, R):
    """the ContentRules that says what the loop's rules say"""
    cr = F.ContentRules(max_n=None if R["max_n"] < 0 else R["max_n"], min_mean_quality=R["min_mean_qual"] or None,
                        qualified_quality=R["qualified_qual"],
                        max_unqualified_percent=None if R["max_unqualified_pct"] < 0 else R["max_unqualified_pct"],
                        max_expected_errors=None if R["max_ee_micro"] < 0 else R["max_ee_micro"] / 1e6,
                        min_complexity=R["min_complexity_pct"] or None, qual_base=R["qual_base"])
    assert as_rules(cr) == R
    return cr


def test_verdict_at_every_edge(F):
    for what, R, keep, drop in EDGES:
        cr = make(F, R)
        assert cr.active
        assert cr.verdict(*keep) == 0 == content_verdict(*keep, R), what
        assert cr.verdict(*drop) == content_verdict(*drop, R) != 0, what
    R = rules(max_n=0, min_mean_qual=30, max_unqualified_pct=0, max_ee_micro=0, min_complexity_pct=100)
    cr = make(F, R)
    for i, rd in enumerate(((b"NN", b"!!"), (b"AA", b"!!"), (b"AA", b"/O"), (b"AA", b"??"), (b"AA", b"gg"))):
        assert cr.verdict(*rd) == content_verdict(*rd, R) == i + 2
        assert F.ContentRules.REASONS[cr.verdict(*rd) - 1] == ("n", "mean_quality", "unqualified", "expected_errors", "complexity")[i]
    assert cr.verdict(b"", b"") == 0 and cr.verdict(b"AC", b"gg") == 0
    assert F.ContentRules.REASONS == ("length", "n", "mean_quality", "unqualified", "expected_errors", "complexity")
    # random reads, several rule sets, every byte value in the quality
    rng = np.random.default_rng(3)
    reads = [one_read(rng, int(rng.integers(0, 300)), qhi=110) for _ in range(150)]
    reads.append((b"A" * 255, bytes(b for b in range(256) if b != 10)))
    for R in (rules(max_n=3), rules(qual_base=64, min_mean_qual=9), rules(qualified_qual=40, max_unqualified_pct=50),
              rules(max_ee_micro=7 * 10 ** 6), rules(min_complexity_pct=75), rules(qual_base=0, max_n=20, min_mean_qual=50,
                                                                                    max_unqualified_pct=30, max_ee_micro=10 ** 5,
                                                                                    min_complexity_pct=60)):
        cr = make(F, R)
        got = [cr.verdict(s, q) for s, q in reads]
        assert got == [content_verdict(s, q, R) for s, q in reads]
        assert len(set(got)) > 1
    assert not F.ContentRules().active and F.ContentRules().verdict(b"NNNN", b"!!!!") == 0
    assert F.ContentRules(max_expected_errors=1.0).max_ee_micro == 10 ** 6
    assert F.ContentRules(max_expected_errors=0.0000015).max_ee_micro == int(round(0.0000015 * 1e6))


def test_verdict_pos(F):
    cr = F.ContentRules(max_n=0)
    buf = b"\n@h\nACNT\n+\nIIII\n@w\nAN\nNT\n+\nII\nII\n"
    assert cr.verdict_pos(buf, [1, 3, 4, 8, 11, 15]) == (2, True)
    assert cr.verdict_pos(buf, [1, 3, 4, 6, 11, 13]) == (0, True)
    assert cr.verdict_pos(buf, [16, 18, 19, 24, 27, 32]) == (0, False)           # a wrapped record
    assert cr.verdict_pos(buf, [1, 3, 4, 8, 11, 14]) == (0, False)               # lines of two lengths
    assert cr.verdict_pos(buf, [1, 3, 4, 8, -1, -1]) == (0, False)               # a FASTA row
    assert cr.verdict_pos(buf, [1, 3, 4, 8, len(buf) - 2, len(buf) + 2]) == (0, False)
    with pytest.raises(ValueError):
        cr.verdict(b"ACGT", b"III")


def test_range_errors(F):
    for kw in (dict(max_n=-1), dict(min_mean_quality=0), dict(min_mean_quality=96), dict(qualified_quality=-1), dict(qualified_quality=96),
               dict(max_unqualified_percent=-1), dict(max_unqualified_percent=101), dict(max_expected_errors=-0.5),
               dict(max_expected_errors=float("nan")), dict(min_complexity=0), dict(min_complexity=101), dict(qual_base=-1),
               dict(qual_base=256)):
        with pytest.raises(ValueError):
            F.ContentRules(**kw)
    F.ContentRules(max_n=0, min_mean_quality=95, qualified_quality=0, max_unqualified_percent=100, max_expected_errors=0, min_complexity=100,
                   qual_base=255)
    with pytest.raises(TypeError):
        F.entryfunc_contentfilter(dict(max_n=0))
    with pytest.raises(ValueError):
        F.entryfunc_contentfilter(F.ContentRules(), column="nothing")
    with pytest.raises(TypeError):
        F.filter_fastq(io.BytesIO(b""), io.BytesIO(), content=dict(max_n=0), entrypos=F.entrypos)


# a small mixed file: (header, sequence, quality, wrapped)
def small_file():
    rng = np.random.default_rng(9)
    recs = []
    for i in range(60):
        n = int(rng.integers(1, 90))
        s, q = one_read(rng, n, alphabet=b"ACGTACGTACGTN", qlo=33 + 2, qhi=33 + 42)
        if i % 9 == 4:
            s, q = b"A" * n, q                                                  # no complexity
        if i % 11 == 5:
            q = b"#" * n                                                        # trimmed to length 0 by -q 20
        if i % 13 == 6:
            s = s[:n // 2] + b"NNN" + s[n // 2:]                                 # Ns inside
            q = q[:n // 2] + b"III" + q[n // 2:]
        if i % 7 == 3:
            s, q = s + b"NNNN", q + b"$$$$"                                     # Ns that the trim removes
        recs.append((b"r%d" % i, s, q, False))
    w = 7
    s, q = b"ACGNNNNNACGTACGTACGT", b"IIIIIIIIIIIIIIIIIIII"
    recs.insert(17, (b"wrapped", b"\n".join(s[i:i + w] for i in range(0, 20, w)), b"\n".join(q[i:i + w] for i in range(0, 20, w)), True))
    data = b"".join(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n" for h, s, q, _w in recs)
    return recs, data


def expect(F, recs, cutoff, lo, hi, R):
    """what every record becomes: (reason it is dropped for or None, header, trimmed sequence, trimmed quality)"""
    out = []
    for h, s, q, wrapped in recs:
        if not wrapped and cutoff is not None:
            a, b = F.quality_trim_span(q, cutoff[1], cutoff[0], 33)
            s, q = s[a:b], q[a:b]
        why = None
        if (lo is not None and len(s) < lo) or (hi is not None and len(s) > hi):
            why = "length"
        elif R is not None and not wrapped:
            v = content_verdict(s, q, R)
            why = F.ContentRules.REASONS[v - 1] if v else None
        out.append((why, h, s, q))
    return out


CASES = [((0, 20), 5, None, rules(max_n=0)), ((0, 20), None, 80, rules(max_n=2, max_ee_micro=10 ** 6)), (None, 1, None, rules(min_complexity_pct=30)),
         ((20, 20), 0, None, rules(min_mean_qual=25, max_unqualified_pct=20, qualified_qual=20)), ((0, 20), 5, None, None)]


@pytest.mark.parametrize("fbufsize", (300, 1 << 16))
def test_filter_fastq_with_the_python_scanner(F, fbufsize):
    recs, data = small_file()
    for cutoff, lo, hi, R in CASES:
        want = expect(F, recs, cutoff, lo, hi, R)
        text = b"".join(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n" for why, h, s, q in want if why is None)
        out, report = io.BytesIO(), F.FilterReport(100)
        res = F.filter_fastq(io.BytesIO(data), out, fbufsize, quality_cutoff=cutoff, min_len=lo, max_len=hi, entrypos=F.entrypos,
                             report=report, content=None if R is None else make(F, R))
        assert out.getvalue() == text
        dropped = {r: sum(1 for w in want if w[0] == r) for r in F.ContentRules.REASONS}
        assert report.dropped == dropped and sum(dropped.values()) == len(recs) - res.records_out
        assert res == F.FilterResult(len(recs), sum(1 for w in want if w[0] is None),
                                     sum(len(r[1]) - len(w[2]) for r, w in zip(recs, want)), len(text))
        assert report.before.reads + int(report.before.head[1]) == len(recs)
        assert report.after.reads + int(report.after.head[1]) == res.records_out
    # the trim comes first: a read whose Ns the trim removes passes max_n = 0, and is dropped without the trim
    want = expect(F, recs, (0, 20), 5, None, rules(max_n=0))
    untrimmed = expect(F, recs, None, 5, None, rules(max_n=0))
    assert any(a[0] is None and b[0] == "n" for a, b in zip(want, untrimmed))
    assert any(w[0] == "length" and len(w[2]) == 0 for w in want)              # a read trimmed to length 0
    assert want[17][0] is None and untrimmed[17][0] is None                    # the wrapped record goes by its length alone
    # without a report nothing is counted and the text is the same
    out = io.BytesIO()
    F.filter_fastq(io.BytesIO(data), out, 300, quality_cutoff=(0, 20), min_len=5, entrypos=F.entrypos, content=make(F, rules(max_n=0)))
    assert out.getvalue() == b"".join(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n" for why, h, s, q in want if why is None)


@pytest.mark.parametrize("column", ("sequence", "header", "quality", "entry"))
def test_entryfunc_contentfilter_with_the_python_scanner(F, column):
    recs, data = small_file()
    R = rules(max_n=1, min_complexity_pct=20, max_ee_micro=3 * 10 ** 6)
    want = expect(F, recs, None, 10, 70, R)
    item = {"sequence": lambda w: w[2], "header": lambda w: w[1], "quality": lambda w: w[3], "entry": lambda w: (w[1], w[2], w[3])}[column]
    items = [item(w) if w[0] is None else None for w in want]
    assert any(i is None for i in items) and any(i is not None for i in items)
    ef = F.entryfunc_contentfilter(make(F, R), 10, 70, column)
    assert isinstance(ef, F.entryfunc_lengthfilter) and ef.yield_dropped
    assert list(F.readfastq_iter(io.BytesIO(data), 257, ef, F.entrypos)) == items
    ef = F.entryfunc_contentfilter(make(F, R), 10, 70, column, yield_dropped=False)
    assert list(F.readfastq_iter(io.BytesIO(data), 257, ef, F.entrypos)) == [i for i in items if i is not None]


def test_report_has_dropped_without_content_rules(F):
    recs, data = small_file()
    report = F.FilterReport()
    assert report.dropped == dict.fromkeys(F.ContentRules.REASONS, 0)
    res = F.filter_fastq(io.BytesIO(data), io.BytesIO(), 1 << 12, min_len=40, entrypos=F.entrypos, report=report)
    short = sum(1 for _h, s, _q, _w in recs if len(s) < 40)
    assert report.dropped == dict(dict.fromkeys(F.ContentRules.REASONS, 0), length=short) and res.records_out == len(recs) - short
    assert quantities(b"AN", b"II", OFF)[0] == 1

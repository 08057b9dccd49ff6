"""The overlap of a pair's mates without a GPU: pair_overlap -- the package's host statement of ffq_table_pair_overlap's rule --
against the plain loop of tests/overlap_expect.py over the edge list, and the host route of filter_fastq_paired(overlap=...)
(the Python scanner) against the loop, byte for byte and with every count."""
import numpy as np
import pytest

import overlap_expect as X
import pairs_expect as P

FBUF = 3000


@pytest.fixture(scope="module")
def F(pkg):
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


def edge_pairs():
    """(name, sequence 1, sequence 2, rules)"""
    rng = np.random.default_rng(11)
    D = X.DEFAULT
    out = [("empty", b"", b"", D), ("all A / all T", b"A" * 150, b"T" * 150, D), ("repeat", b"ACGTACGTAC" * 6, X.revcomp(b"ACGTACGTAC" * 5), (20, 0, 0))]
    for n in (29, 30, 31, 15, 16, 17, 32, 33, 150, 511, 512):
        for frag in (n - 7, n, n + 9, 2 * n + 5):
            if frag < 1:
                continue
            s1, s2 = X.mates_of(rng, frag, n, n)
            out.append(("n%d f%d" % (n, frag), s1, s2, D if n >= 30 else (n - 2 if n > 2 else 1, 5, 200)))
    for n1, n2 in ((150, 100), (100, 150), (40, 31), (31, 40)):
        for frag in (35, 90, 120, 200):
            s1, s2 = X.mates_of(rng, frag, n1, n2)
            out.append(("n%d/%d f%d" % (n1, n2, frag), s1, s2, D))
    # mismatches at and one above max_diff (overlap 100: the permille bound is 20), at and above the permille bound (overlap 20: 4)
    for frag, bad in ((100, 5), (100, 6), (20, 4), (20, 5)):
        s1, s2 = X.mates_of(rng, frag, 150, 150)
        s1 = bytearray(s1)
        for i in range(bad):
            s1[2 + 3 * i] = b"ACGT"[(b"ACGT".index(bytes([s1[2 + 3 * i]])) + 1) % 4]
        out.append(("f%d mm%d" % (frag, bad), bytes(s1), s2, (20, 5, 200)))
    # N in one mate, N in both at the same place, lower case
    s1, s2 = X.mates_of(rng, 60, 100, 100)
    for k in range(1, 4):
        a, b = bytearray(s1), bytearray(s2)
        for i in range(k):
            a[5 + 7 * i] = ord("N")
            b[59 - (5 + 7 * i)] = ord("N")
        out.append(("N both x%d" % k, bytes(a), bytes(b), (30, 2, 200)))
        out.append(("N one x%d" % k, bytes(a), s2, (30, 2, 200)))
    out.append(("lower", s1.lower(), s2, D))
    out.append(("lower both", s1.lower(), s2.lower(), D))
    return out


def test_pair_overlap_against_the_loop(F):
    seen = set()
    for name, s1, s2, rules in edge_pairs():
        o = X.loop_overlap(s1, s2, *rules)
        want = None if o is None else len(s2) + o
        assert F.pair_overlap(s1, s2, F.OverlapRules(*rules)) == want, name
        seen.add("none" if o is None else "cut" if o < 0 else "kept")
    assert seen == {"none", "cut", "kept"}
    # the cases the list is there for
    D = F.OverlapRules()
    assert F.pair_overlap(b"A" * 150, b"T" * 150, D) == 150                 # every candidate qualifies: the first, o = 0
    assert F.pair_overlap(b"", b"", D) is None
    r = F.OverlapRules(20, 5, 200)
    byname = {n: (a, b) for n, a, b, _ in edge_pairs()}
    assert F.pair_overlap(*byname["f100 mm5"], r) == 100 and F.pair_overlap(*byname["f100 mm6"], r) != 100
    assert F.pair_overlap(*byname["f20 mm4"], r) == 20 and F.pair_overlap(*byname["f20 mm5"], r) != 20
    assert F.pair_overlap(*byname["N both x2"], F.OverlapRules(30, 2, 200)) == 60
    assert F.pair_overlap(*byname["N both x3"], F.OverlapRules(30, 2, 200)) != 60       # an N does not match an N
    assert F.pair_overlap(*byname["lower"], D) == 60


def test_overlap_rules_ranges(F):
    for bad in ((0, 5, 200), (513, 5, 200), (30, -1, 200), (30, 513, 200), (30, 5, -1), (30, 5, 1001)):
        with pytest.raises(ValueError):
            F.OverlapRules(*bad)
    r = F.OverlapRules()
    assert (r.min_overlap, r.max_diff, r.diff_permille) == X.DEFAULT


def test_host_route_against_the_loop(F):
    r1, r2 = X.records(400, 5)
    want = X.Expected(r1, r2, min_len=(40, 40))
    assert want.kinds == {"none", "cut", "kept"} and want.trimmed > 0 and all(want.bases) and want.dropped["both"] > 0
    res, o1, o2, rep = X.run(F, P.fastq(r1), P.fastq(r2), F.entrypos, FBUF, min_len=40)
    assert (o1, o2) == (want.text[0], want.text[1])
    assert tuple(res) == want.result()
    want.check_report(rep)
    assert rep.insert_peak is not None and rep.pairs_analysed == 400


def test_host_route_order_of_the_stages(F):
    """quality, adapter, overlap, filter"""
    r1, r2 = X.records(300, 6)
    kw = dict(quality_cutoff=(5, 10), adapters=(P.ADAPTER1, P.ADAPTER2), min_len=(40, 35))
    want = X.Expected(r1, r2, **kw)
    res, o1, o2, rep = X.run(F, P.fastq(r1), P.fastq(r2), F.entrypos, FBUF, quality_cutoff=(5, 10), adapter=P.ADAPTER1, adapter2=P.ADAPTER2,
                             min_len=(40, 35))
    assert (o1, o2) == (want.text[0], want.text[1]) and tuple(res) == want.result()
    want.check_report(rep)
    # the overlap still finds work behind the adapter trim, and the stages are not interchangeable
    assert want.trimmed > 0
    assert X.Expected(r1, r2, use_overlap=False, **kw).text != want.text


def test_host_route_without_overlap_is_unchanged(F):
    import io
    r1, r2 = X.records(200, 7)
    d1, d2 = P.fastq(r1), P.fastq(r2)
    res, o1, o2, rep = X.run(F, d1, d2, F.entrypos, FBUF, rules=None, min_len=40)
    assert rep is None
    p1, p2 = io.BytesIO(), io.BytesIO()
    plain = F.filter_fastq_paired(io.BytesIO(d1), io.BytesIO(d2), p1, p2, fbufsize=FBUF, entrypos=F.entrypos, min_len=40)
    assert (o1, o2, tuple(res)) == (p1.getvalue(), p2.getvalue(), tuple(plain))
    want = X.Expected(r1, r2, min_len=(40, 40), use_overlap=False)
    assert (o1, o2) == (want.text[0], want.text[1]) and tuple(res) == want.result()
    with pytest.raises(ValueError):
        F.filter_fastq_paired(io.BytesIO(d1), io.BytesIO(d2), p1, p2, entrypos=F.entrypos, overlap_report=F.OverlapReport())
    with pytest.raises(TypeError):
        F.filter_fastq_paired(io.BytesIO(d1), io.BytesIO(d2), p1, p2, entrypos=F.entrypos, overlap=(30, 5, 200))

"""Paired-end files without a GPU: pair_id, and the host route of filter_fastq_paired (the Python scanner, two readfastq_iter
loops zipped record by record) against the plain loops of tests/pairs_expect.py -- byte for byte, with every count."""
import pytest

import pairs_expect as X

FBUF = 3000


@pytest.fixture(scope="module")
def F(pkg):
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


@pytest.fixture(scope="module")
def recs():
    return X.records(600, 21)


def test_pair_id(F):
    for n in (1, 3, 4, 5, 31, 32, 33, 64, 65, 300):
        i = bytes(65 + (k * 7) % 26 for k in range(n))
        for h, want in ((i, i), (i + b"/1", i), (i + b"/2", i), (i + b"/3", i + b"/3"), (i + b" 1:N:0", i), (i + b"\tx y", i),
                        (i + b"/1 c", i), (i + b"/1/2", i + b"/1"), (i + b"x/1", i + b"x")):
            assert F.pair_id(h) == want == X.id_of(h), h
    for h, want in ((b"/1", b""), (b"/2", b""), (b"/", b"/"), (b"", b""), (b" a", b""), (b"\t", b""), (b"1", b"1"), (b"a\x00b c", b"a\x00b"),
                    (b"a /1", b"a"), (b"a/1\t/2", b"a")):
        assert F.pair_id(h) == want == X.id_of(h), h
    assert F.pair_id(bytearray(b"r/1 x")) == b"r" and F.pair_id(memoryview(b"r/2")) == b"r"


@pytest.mark.parametrize("pair_filter", ("any", "both", "first"))
def test_host_route_against_the_loop(F, recs, pair_filter):
    r1, r2 = recs
    want = X.Expected(r1, r2, pair_filter)
    res, err, o1, o2, rep, rep2 = X.run(F, X.fastq(r1), X.fastq(r2), F.entrypos, FBUF, pair_filter, reports=True)
    assert err is None
    assert (o1, o2) == (want.text[0], want.text[1])
    assert tuple(res) == want.result()
    assert res.pairs_in == res.pairs_out + sum(res.dropped.values())
    assert 0 < res.pairs_out < res.pairs_in
    X.check_reports(rep, rep2, r1, r2, want)
    if pair_filter == "first":
        assert not any(rep2.dropped.values()) and res.dropped["mate2_only"] == res.dropped["both"] == 0
    if pair_filter == "any":
        # every rule fires on either mate, every class of pair is there
        assert all(want.hist[0].values()) and all(want.hist[1].values()) and all(want.dropped.values())


def test_host_route_without_content_rules_or_names(F, recs):
    r1, r2 = recs
    want = X.Expected(r1, r2, "any", with_content=False)
    res, err, o1, o2, _, _ = X.run(F, X.fastq(r1), X.fastq(r2), F.entrypos, FBUF, check_names=False, content=False)
    assert err is None and (o1, o2) == (want.text[0], want.text[1]) and tuple(res) == want.result()


@pytest.mark.parametrize("longer", (1, 2))
def test_host_route_files_of_two_lengths(F, recs, longer):
    """one file a record short: every complete pair is written, then the error names the file that has more"""
    r1, r2 = recs
    n = 200
    a, b = (r1[:n + 1], r2[:n]) if longer == 1 else (r1[:n], r2[:n + 1])
    want = X.Expected(r1, r2, "any", n)
    res, err, o1, o2, _, _ = X.run(F, X.fastq(a), X.fastq(b), F.entrypos, FBUF)
    assert res is None and err is not None
    assert err.startswith("mate %d: the file holds more records than mate %d's" % (longer, 3 - longer)), err
    first_unpaired = len(X.fastq((a if longer == 1 else b)[:n]))
    assert err.endswith("at byte %d" % first_unpaired), err
    assert (o1, o2) == (want.text[0], want.text[1])


def test_host_route_malformed_mate(F, recs):
    """a '+' line with text of another length in the middle of mate 2: the pairs in front of it, then the stream's error with the mate"""
    r1, r2 = recs
    n = 150
    bad = X.fastq(r2[:n]) + b"@" + r2[n][0] + b"\n" + r2[n][1] + b"\n+bad\n" + r2[n][2] + b"\n" + X.fastq(r2[n + 1:300])
    want = X.Expected(r1, r2, "any", n)
    res, err, o1, o2, _, _ = X.run(F, X.fastq(r1[:300]), bad, F.entrypos, FBUF)
    import io
    with pytest.raises(ValueError, match="Entry is invalid at byte") as alone:       # what the file raises on its own
        list(F.readfastq_iter(io.BytesIO(bad), FBUF, F.entryfunc, F.entrypos))
    assert res is None and err == "mate 2: " + str(alone.value), err
    assert (o1, o2) == (want.text[0], want.text[1])
    # cut short inside a header
    cut = X.fastq(r2[:n]) + b"@" + r2[n][0][:3]
    res, err, o1, o2, _, _ = X.run(F, X.fastq(r1[:300]), cut, F.entrypos, FBUF)
    assert res is None and err.startswith("mate 2: Incomplete entry at byte"), err
    assert (o1, o2) == (want.text[0], want.text[1])


def test_host_route_swapped_records(F, recs):
    """two records of mate 2 swapped: the name error with the ordinal and the two ids, behind the pairs in front; none without the check"""
    r1, r2 = recs
    n = 123
    sw = list(r2[:300])
    sw[n], sw[n + 1] = sw[n + 1], sw[n]
    want = X.Expected(r1, r2, "any", n)
    res, err, o1, o2, _, _ = X.run(F, X.fastq(r1[:300]), X.fastq(sw), F.entrypos, FBUF)
    assert res is None
    assert err == "pair %d: the two records are not mates: %r and %r" % (n, X.id_of(r1[n][0]), X.id_of(r2[n + 1][0])), err
    assert (o1, o2) == (want.text[0], want.text[1])
    res, err, o1, o2, _, _ = X.run(F, X.fastq(r1[:300]), X.fastq(sw), F.entrypos, FBUF, check_names=False)
    assert err is None and res.pairs_in == 300


def test_host_route_empty_files_and_arguments(F):
    res, err, o1, o2, _, _ = X.run(F, b"", b"", F.entrypos, FBUF)
    assert err is None and tuple(res) == (0, 0, 0, 0, 0, {"mate1_only": 0, "mate2_only": 0, "both": 0}) and o1 == o2 == b""
    import io
    with pytest.raises(ValueError, match="pair_filter"):
        F.filter_fastq_paired(io.BytesIO(), io.BytesIO(), io.BytesIO(), io.BytesIO(), pair_filter="all", entrypos=F.entrypos)
    with pytest.raises(TypeError):
        F.filter_fastq_paired(io.BytesIO(), io.BytesIO(), io.BytesIO(), io.BytesIO(), content=3, entrypos=F.entrypos)

"""Paired-end files on the device: filter_fastq_paired with the GPU scanner -- two streams walked in lockstep (hip.PairStream,
ffq_pair) -- against the plain loops of tests/pairs_expect.py, byte for byte and with every count; the Python-scanner route
against the same loops.  The fills are a few KiB, so a file is dozens of rounds, some of a handful of pairs, and either mate
is ahead at some time."""
import gzip
import io

import pytest

import pairs_expect as X

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


@pytest.fixture(scope="module")
def small():
    return X.records(600, 21)


def file_opener(tmp_path, name, compress=False):
    def opener(data):
        p = tmp_path / name
        p.write_bytes(gzip.compress(data, 1) if compress else data)
        return gzip.open(p, "rb") if compress else open(p, "rb")
    return opener


def test_main_case_both_routes(F, C, tmp_path):
    """about 3000 pairs from two plain files: the GPU route, the Python-scanner route and the loop agree"""
    r1, r2 = X.records(3000, 20)
    want = X.Expected(r1, r2, "any")
    assert all(want.hist[0].values()) and all(want.hist[1].values()) and all(want.dropped.values())
    d1, d2 = X.fastq(r1), X.fastq(r2)
    res, err, o1, o2, rep, rep2 = X.run(F, d1, d2, C.entrypos, FBUF, reports=True, opener1=file_opener(tmp_path, "r1.fq"),
                                        opener2=file_opener(tmp_path, "r2.fq"))
    assert err is None
    assert o1 == want.text[0] and o2 == want.text[1]
    assert tuple(res) == want.result()
    X.check_reports(rep, rep2, r1, r2, want)
    res, err, o1, o2, rep, rep2 = X.run(F, d1, d2, F.entrypos, FBUF, reports=True)
    assert err is None and (o1, o2) == (want.text[0], want.text[1]) and tuple(res) == want.result()
    X.check_reports(rep, rep2, r1, r2, want)


def test_the_fills_drift_apart(F, C, gpu_ctx, tmp_path):
    """the walk itself: dozens of rounds, small ones among them, each mate ahead at some time, every pair once"""
    from fastqandfurious_amd import hip
    r1, r2 = X.records(3000, 20)
    fh1, fh2 = file_opener(tmp_path, "a.fq")(X.fastq(r1)), file_opener(tmp_path, "b.fq")(X.fastq(r2))
    st1, st2 = C.entrypos.open_stream(fh1, FBUF), C.entrypos.open_stream(fh2, FBUF)
    ps = hip.PairStream(st1, st2, "any", True)
    try:
        with pytest.raises(hip.FFQError) as ei:                    # a stream a pair owns is walked by the pair alone
            st1._next()
        assert ei.value.code == hip.E_ARG
        sizes, ahead, total_in, total_out = [], set(), 0, 0
        for n_in, n_out, end_state, err_mate, err_offset in ps:
            assert end_state in (hip.END_OK, hip.END_REFILL) and err_mate == 0
            idx, pairs = ps.selected()
            assert n_out == pairs[0] == idx.size and pairs[0] + pairs[1] == n_in
            assert (idx[1:] > idx[:-1]).all() and (idx.size == 0 or (0 <= idx[0] and idx[-1] < n_in))
            # no filter on either stream: every pair is kept, and the two mates' rows are the same records
            rows1, fill1, off1 = ps.rows(1)
            rows2, fill2, off2 = ps.rows(2)
            for k in (0, n_out - 1) if n_out else ():
                h1 = bytes(fill1[rows1[k][0] + 1 - off1:rows1[k][1] - off1])
                h2 = bytes(fill2[rows2[k][0] + 1 - off2:rows2[k][1] - off2])
                assert h1 == r1[total_in + int(idx[k])][0] and h2 == r2[total_in + int(idx[k])][0]
            sizes.append(n_in)
            total_in += n_in
            total_out += n_out
            w = hip.lib().ffq_pair_wants(ps._h)
            if w in (1, 2):
                ahead.add(3 - w)                                   # the other mate still has rows: it is ahead
        assert total_in == total_out == 3000
        assert len(sizes) >= 24 and min(s for s in sizes if s) <= 8 and ahead == {1, 2}
    finally:
        ps.close()
        st1.close()
        st2.close()
        fh1.close()
        fh2.close()


@pytest.mark.parametrize("pair_filter", ("any", "both", "first"))
def test_gzip_file_and_pushed_chunks(F, C, small, tmp_path, pair_filter):
    """one mate inflated by the library from a gzip file, the other pushed chunk by chunk from a BytesIO; every pair_filter"""
    r1, r2 = small
    want = X.Expected(r1, r2, pair_filter)
    res, err, o1, o2, rep, rep2 = X.run(F, X.fastq(r1), X.fastq(r2), C.entrypos, FBUF, pair_filter, reports=True,
                                        opener1=file_opener(tmp_path, "r1.fq.gz", True))
    assert err is None
    assert (o1, o2) == (want.text[0], want.text[1])
    assert tuple(res) == want.result()
    X.check_reports(rep, rep2, r1, r2, want)


def test_a_record_longer_than_a_chunk(F, C):
    """mate 1 of one pair has 5000 bases, the chunk has 4096 bytes: fills without a complete record, rounds without a pair"""
    r1, r2 = X.records(300, 22, 140)
    want = X.Expected(r1, r2, "any")
    res, err, o1, o2, _, _ = X.run(F, X.fastq(r1), X.fastq(r2), C.entrypos, 4096)
    assert err is None and (o1, o2) == (want.text[0], want.text[1]) and tuple(res) == want.result()


def test_without_filters_every_pair_is_kept(F, C, small):
    r1, r2 = small
    o1, o2 = io.BytesIO(), io.BytesIO()
    res = F.filter_fastq_paired(io.BytesIO(X.fastq(r1)), io.BytesIO(X.fastq(r2)), o1, o2, fbufsize=FBUF, entrypos=C.entrypos)
    assert tuple(res) == (600, 600, 0, len(X.fastq(r1)), len(X.fastq(r2)), {"mate1_only": 0, "mate2_only": 0, "both": 0})
    assert o1.getvalue() == X.fastq(r1) and o2.getvalue() == X.fastq(r2)


@pytest.mark.parametrize("longer", (1, 2))
def test_files_of_two_lengths(F, C, small, longer):
    """one file a record short: every complete pair is written, then the error names the file that has more"""
    r1, r2 = small
    n = 200
    a, b = (r1[:n + 1], r2[:n]) if longer == 1 else (r1[:n], r2[:n + 1])
    want = X.Expected(r1, r2, "any", n)
    res, err, o1, o2, _, _ = X.run(F, X.fastq(a), X.fastq(b), C.entrypos, FBUF)
    assert res is None and err is not None
    assert err.startswith("mate %d: the file holds more records than mate %d's" % (longer, 3 - longer)), err
    assert err.endswith("at byte %d" % len(X.fastq((a if longer == 1 else b)[:n]))), err
    assert (o1, o2) == (want.text[0], want.text[1])


def test_malformed_mate(F, C, small):
    """a '+' line with text of another length in the middle of mate 2: the pairs in front of it, then the stream's own error"""
    r1, r2 = small
    n = 150
    bad = X.fastq(r2[:n]) + b"@" + r2[n][0] + b"\n" + r2[n][1] + b"\n+bad\n" + r2[n][2] + b"\n" + X.fastq(r2[n + 1:300])
    want = X.Expected(r1, r2, "any", n)
    with pytest.raises(ValueError, match="Entry is invalid at byte") as alone:       # what the file raises on its own
        list(F.readfastq_iter(io.BytesIO(bad), FBUF, F.entryfunc, C.entrypos))
    res, err, o1, o2, _, _ = X.run(F, X.fastq(r1[:300]), bad, C.entrypos, FBUF)
    assert res is None and err == "mate 2: " + str(alone.value), err
    assert (o1, o2) == (want.text[0], want.text[1])
    cut = X.fastq(r2[:n]) + b"@" + r2[n][0][:3]
    res, err, o1, o2, _, _ = X.run(F, X.fastq(r1[:300]), cut, C.entrypos, FBUF)
    assert res is None and err.startswith("mate 2: Incomplete entry at byte"), err
    assert (o1, o2) == (want.text[0], want.text[1])


def test_swapped_records(F, C, small):
    """two records of mate 2 swapped: the name error with the pair's ordinal and the two ids; whole rounds in front of it are
    written, nothing of the round that holds it; no error without the check"""
    r1, r2 = small
    n = 123
    sw = list(r2[:300])
    sw[n], sw[n + 1] = sw[n + 1], sw[n]
    res, err, o1, o2, _, _ = X.run(F, X.fastq(r1[:300]), X.fastq(sw), C.entrypos, FBUF)
    assert res is None
    assert err == "pair %d: the two records are not mates: %r and %r" % (n, X.id_of(r1[n][0]), X.id_of(r2[n + 1][0])), err
    # what was written: the kept pairs among the first k, for some k <= n, the same k for both mates
    want = X.Expected(r1, r2, "any", n)
    ks = [k for k in range(n + 1) if want.prefix(k) == (o1, o2)]
    assert ks, "the output is not a whole number of pairs in front of the error"
    assert n - max(ks) <= 2 * FBUF // 100, "more than a round is missing"
    res, err, o1, o2, _, _ = X.run(F, X.fastq(r1[:300]), X.fastq(sw), C.entrypos, FBUF, check_names=False)
    assert err is None and res.pairs_in == 300


def test_empty_files(F, C):
    res, err, o1, o2, _, _ = X.run(F, b"", b"", C.entrypos, FBUF)
    assert err is None and tuple(res) == (0, 0, 0, 0, 0, {"mate1_only": 0, "mate2_only": 0, "both": 0}) and o1 == o2 == b""
    res, err, o1, o2, _, _ = X.run(F, b"", X.fastq(X.records(600, 21)[1][:3]), C.entrypos, FBUF)
    assert res is None and err.startswith("mate 2: the file holds more records") and err.endswith("at byte 0") and o1 == o2 == b""


def test_pair_open_refuses(C, gpu_ctx):
    """streams that are not fresh, not two, or gather a column"""
    from fastqandfurious_amd import hip
    data = X.fastq(X.records(600, 21)[0][:50])
    sts = [C.entrypos.open_stream(io.BytesIO(data), FBUF) for _ in range(3)]
    try:
        for _ in sts[2]:
            break
        sts[1].set_filter(10, None, "sequence")
        for a, b, mode in ((sts[0], sts[0], "any"), (sts[0], sts[2], "any"), (sts[0], sts[1], "any"), (sts[0], sts[2], 7)):
            with pytest.raises(hip.FFQError) as ei:
                hip.PairStream(a, b, mode)
            assert ei.value.code == hip.E_ARG
        with pytest.raises(ValueError):
            hip.PairStream(sts[0], sts[2], "all")
    finally:
        for st in sts:
            st.close()

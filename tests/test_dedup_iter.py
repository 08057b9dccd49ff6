"""Duplicate removal through the stream front end: filter_fastq(dedup=...), filter_fastq_paired(dedup=...) and
fastq_stats(duplication=True) on the GPU scanner against the host route and against the plain loops of tests/dedup_expect.py --
output bytes, results and DedupReports, all exact.  The input draws 3000 records from 900 distinct reads; header and quality
are every copy's own, so a quality trim cuts the copies of one read differently, and some records are wrapped.  At fbufsize 700
a fill holds two records or one or none, and the copies of a read lie in different fills: the set has to live across them.

Reads without bases are NOT in these files: the device scanners read an empty record and the one behind it as one longer
record (include/ffq.h at ffq_table_render_fastq), so the two routes do not see the same records there.  Empty reads are keyed
on hand-made tables in tests/test_dedup.py and go through the host route in tests/test_dedup_host.py."""
import gzip
import io

import pytest

import dedup_expect as X
import merge_expect as M
import pairs_expect as P

pytestmark = pytest.mark.gpu

SIZES = (700, 1 << 16)


@pytest.fixture(scope="module")
def F(pkg):
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


@pytest.fixture(scope="module")
def C(gpu_ctx):
    from fastqandfurious_amd import _fastqandfurious
    return _fastqandfurious


@pytest.fixture(scope="module")
def recs():
    r = X.records(3000, 900)
    assert X.keys_tell_sequences_apart(r)
    assert sum(1 for _h, s, _q in r if 10 in s) > 50
    return r


@pytest.fixture(scope="module")
def want(recs):
    """(without rules, with trim + adapter + content rules)"""
    w = X.Expected(recs, False), X.Expected(recs, True)
    assert w[0].duplicates > 1500 and w[0].distinct <= 900 and w[0].unkeyed > 50
    assert w[1].first_copy_filtered > 10 and w[1].removed > 0 and 0 < w[1].duplicates < w[0].duplicates
    return w


@pytest.fixture(scope="module")
def host(F, recs):
    """the host route, once per configuration: it does not depend on the size of a fill"""
    data = P.fastq(recs)
    return tuple(X.run(F, data, F.entrypos, 1 << 14, rules) for rules in (False, True))


@pytest.mark.parametrize("rules", (False, True))
@pytest.mark.parametrize("fbufsize", SIZES)
def test_device_and_host_write_the_same_file(F, C, recs, want, host, fbufsize, rules):
    res, out, rep = X.run(F, P.fastq(recs), C.entrypos, fbufsize, rules)
    w = want[rules]
    assert out == w.text
    assert tuple(res) == w.result()
    w.check_report(rep)
    hres, hout, hrep = host[rules]
    assert out == hout and res == hres and rep.__dict__ == hrep.__dict__


@pytest.mark.parametrize("fbufsize", SIZES)
def test_count_only_leaves_the_output_alone(F, C, recs, want, fbufsize):
    data = P.fastq(recs)
    plain, plain_out, _ = X.run(F, data, C.entrypos, fbufsize, True, dedup=False)
    res, out, rep = X.run(F, data, C.entrypos, fbufsize, True, count_only=True)
    assert out == plain_out and res == plain
    assert out == X.Expected(recs, True, drop=False).text
    want[1].check_report(rep)


def test_fastq_stats_counts_the_duplicates(F, C, recs, want):
    data = P.fastq(recs)
    w = want[0]
    for fbufsize in SIZES:
        st = F.fastq_stats(io.BytesIO(data), fbufsize, entrypos=C.entrypos, duplication=True)
        assert (st.keyed, st.distinct, st.duplicates) == (w.keyed, w.distinct, w.duplicates)
        assert st.duplication_rate == w.duplicates / w.keyed
    plain = F.fastq_stats(io.BytesIO(data), 1 << 16, entrypos=C.entrypos)
    assert plain == st and plain.keyed is None and plain.duplication_rate is None
    assert st == F.fastq_stats(io.BytesIO(data), 1 << 14, entrypos=F.entrypos, duplication=True)


def test_a_gzip_file_gives_the_same_bytes(F, C, recs, want, tmp_path):
    z = tmp_path / "reads.fq.gz"
    with gzip.open(str(z), "wb", compresslevel=1) as fh:
        fh.write(P.fastq(recs))
    with F.automagic_open(str(z)) as fh:
        res, out, rep = X.run(F, None, C.entrypos, 1 << 13, True, opened=fh)
    assert out == want[1].text and tuple(res) == want[1].result()
    want[1].check_report(rep)


def test_the_stream_hands_out_what_remains(F, C, gpu_ctx, recs, want):
    """the stream itself: rows, selected() and the counts of every fill add up; the setter's rules"""
    from fastqandfurious_amd import hip
    data = P.fastq(recs)
    st = C.entrypos.open_stream(io.BytesIO(data), 1 << 12)
    try:
        with pytest.raises(hip.FFQError) as ei:                    # not switched on: nothing to report
            st.dedup_counts()
        assert ei.value.code == hip.E_ARG
        st.set_dedup()
        kept_seqs, scanned, last = [], 0, -1
        for rows, fill, off, end_state, _err in st:
            assert end_state in (hip.END_OK, hip.END_REFILL)
            idx, n_scanned, _col, _coff = st.selected()
            assert len(idx) == rows.shape[0] and (len(idx) < 2 or (idx[1:] > idx[:-1]).all()) and (len(idx) == 0 or idx[-1] < n_scanned)
            scanned += n_scanned
            fb = bytes(fill)
            kept_seqs += [fb[r[2] - off:r[3] - off] for r in rows.tolist()]
        w = want[0]
        assert scanned == w.records_in
        seen, first_copies = set(), []
        for _h, sq, _q in recs:
            k = X.key_of_record(sq)
            if k == X.KEY_NONE or k not in seen:
                first_copies.append(sq)
                seen.add(k)
        assert kept_seqs == first_copies and len(kept_seqs) == w.records_out
        c = st.dedup_counts()
        assert c[:4] == [w.records_out, w.duplicates, w.unkeyed, w.distinct] and c[4] >= 2 * c[3] and c[5] >= 1
        with pytest.raises(hip.FFQError) as ei:                    # the stream has handed out a fill
            st.set_dedup()
        assert ei.value.code == hip.E_ARG
    finally:
        st.close()
    st = C.entrypos.open_stream(io.BytesIO(data), 1 << 12)
    try:
        with pytest.raises(hip.FFQError) as ei:                    # a cap below the minimum table
            st.set_dedup(True, 0, 100)
        assert ei.value.code == hip.E_NOMEM
    finally:
        st.close()


# ---- pairs -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs():
    return X.pair_records(1500, 500)


@pytest.fixture(scope="module")
def want_pairs(pairs):
    w = X.ExpectedPairs(*pairs)
    assert w.duplicates > 300 and w.pairs_merged > 100 and w.unkeyed > 3 and sum(w.dropped.values()) > 100
    assert w.first_copy_filtered > 10           # a pair whose first copy the filter dropped keeps its second copy
    assert len(w.text[0]) > 0 and len(w.text[2]) > 0
    return w


@pytest.fixture(scope="module")
def host_pairs(F, pairs):
    return X.run_pairs(F, M.file_of(pairs[0]), M.file_of(pairs[1]), F.entrypos, 1 << 14)


@pytest.mark.parametrize("fbufsize", SIZES)
def test_pairs_device_and_host_write_the_same_three_files(F, C, pairs, want_pairs, host_pairs, fbufsize):
    res, o1, o2, om, rep = X.run_pairs(F, M.file_of(pairs[0]), M.file_of(pairs[1]), C.entrypos, fbufsize)
    w = want_pairs
    assert (o1, o2, om) == tuple(w.text)
    assert tuple(res) == w.result()
    w.check_report(rep)
    hres, h1, h2, hm, hrep = host_pairs
    assert (o1, o2, om) == (h1, h2, hm) and tuple(res) == tuple(hres) and rep.__dict__ == hrep.__dict__
    assert res.pairs_in == res.pairs_out + sum(res.dropped.values()) + rep.duplicates


def test_pairs_count_only_and_the_setters_rules(F, C, pairs, want_pairs):
    from fastqandfurious_amd import hip
    d1, d2 = M.file_of(pairs[0]), M.file_of(pairs[1])
    plain = X.run_pairs(F, d1, d2, C.entrypos, 1 << 15, dedup=False)
    res, o1, o2, om, rep = X.run_pairs(F, d1, d2, C.entrypos, 1 << 15, count_only=True)
    assert (o1, o2, om) == plain[1:4] and res == plain[0]
    assert (o1, o2, om) == tuple(X.ExpectedPairs(pairs[0], pairs[1], dedup=False).text)
    want_pairs.check_report(rep)
    # a stream with a dedup of its own is no mate of a pair; a pair's dedup is set before the walk
    st1, st2 = C.entrypos.open_stream(io.BytesIO(d1), 1 << 14), C.entrypos.open_stream(io.BytesIO(d2), 1 << 14)
    ps = None
    try:
        st1.set_dedup()
        with pytest.raises(hip.FFQError) as ei:
            hip.PairStream(st1, st2)
        assert ei.value.code == hip.E_ARG
    finally:
        st1.close()
        st2.close()
    st1, st2 = C.entrypos.open_stream(io.BytesIO(d1), 1 << 14), C.entrypos.open_stream(io.BytesIO(d2), 1 << 14)
    try:
        ps = hip.PairStream(st1, st2)
        with pytest.raises(hip.FFQError) as ei:
            ps.dedup_counts()
        assert ei.value.code == hip.E_ARG
        ps.set_dedup()
        n_in, n_out, _end, _mate, _err = ps._next()
        idx, pc = ps.selected()
        c = ps.dedup_counts()
        assert pc[0] == n_in == c[0] + c[1] and n_out == c[0] == len(idx) and ps.rows(1)[0].shape == (n_out, 6) == ps.rows(2)[0].shape
        with pytest.raises(hip.FFQError) as ei:
            ps.set_dedup()
        assert ei.value.code == hip.E_ARG
    finally:
        if ps is not None:
            ps.close()
        st1.close()
        st2.close()

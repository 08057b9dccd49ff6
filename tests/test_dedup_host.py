"""Duplicate removal without a GPU: seq_key / pair_key -- the package's host statement of the rule of include/ffq.h -- against the
plain loops of tests/dedup_expect.py, and the host route (the Python scanner, a set of keys) of filter_fastq(dedup=...),
filter_fastq_paired(dedup=...) and fastq_stats(duplication=True) against the loop, byte for byte and with every count."""
import io

import numpy as np
import pytest

import dedup_expect as X
import merge_expect as M
import pairs_expect as P

FBUF = 3000


@pytest.fixture(scope="module")
def F(pkg):
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


@pytest.fixture(scope="module")
def recs():
    r = X.records(1200, 350, 5, empties=True)
    assert X.keys_tell_sequences_apart(r)
    assert sum(1 for _h, s, _q in r if s == b"") > 5 and sum(1 for _h, s, _q in r if 10 in s) > 5
    return r


def test_seq_key_against_the_loop(F):
    rng = np.random.default_rng(3)
    seen = {}
    for n in list(range(0, 71)) + [149, 150, 151, 1000, 4999]:
        for _ in range(3):
            s = bytes(rng.integers(0, 256, n, dtype=np.uint8)) if n % 5 == 0 else bytes(np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, n)])
            k = F.seq_key(s)
            assert k == X.loop_key(s) and 0 < k < 1 << 64, n
            assert F.seq_key(bytearray(s)) == k == F.seq_key(memoryview(s))
            assert seen.setdefault(k, s) == s
    assert F.seq_key(b"") == X.loop_key(b"") != 0
    assert F.seq_key(b"acgt") != F.seq_key(b"ACGT")                      # case is not folded
    assert F.seq_key(b"AAAAA") != F.seq_key(b"AAAAA\x00")                # a zero byte is not the end
    assert F.seq_key(b"ACGTTTTT") != F.seq_key(b"TTTTACGT")              # a word's place counts
    assert len({F.seq_key(b"A" * n) for n in range(600)}) == 600


def test_pair_key_against_the_loop(F):
    rng = np.random.default_rng(4)
    for _ in range(200):
        k1, k2 = (int(x) for x in rng.integers(1, 1 << 63, 2))
        assert F.pair_key(k1, k2) == X.loop_pair_key(k1, k2) != 0
        assert len({F.pair_key(k1, k2), F.pair_key(k2, k1), F.pair_key(k1, k1)}) == 3
        assert F.pair_key(0, k2) == F.pair_key(k1, 0) == F.pair_key(0, 0) == 0
    k1 = 12345
    assert F.pair_key(k1, (-X.sm(k1)) & X.M64) == 1                      # a key of 0 becomes 1


@pytest.mark.parametrize("rules", (False, True))
def test_filter_fastq_host_route_against_the_loop(F, recs, rules):
    want = X.Expected(recs, rules)
    res, out, rep = X.run(F, P.fastq(recs), F.entrypos, FBUF, rules)
    assert out == want.text
    assert tuple(res) == want.result()
    want.check_report(rep)
    assert want.duplicates > 300 and want.unkeyed > 5 and 0 < rep.duplication_rate < 1
    if rules:
        # a read whose first copy the filters dropped keeps a later copy; nothing of this shows in the FilterReport's reasons
        assert want.first_copy_filtered > 3 and want.removed > 0
        frep = F.FilterReport()
        F.filter_fastq(io.BytesIO(P.fastq(recs)), io.BytesIO(), FBUF, entrypos=F.entrypos, report=frep, dedup=F.DedupRules(),
                       content=F.ContentRules(**X.CONTENT), **X.TRIM)
        assert sum(frep.dropped.values()) == want.records_in - want.keyed - want.unkeyed
        assert sorted(frep.dropped) == sorted(F.ContentRules.REASONS)


def test_count_only_writes_what_a_run_without_dedup_writes(F, recs):
    data = P.fastq(recs)
    plain, plain_out, _ = X.run(F, data, F.entrypos, FBUF, True, dedup=False)
    res, out, rep = X.run(F, data, F.entrypos, FBUF, True, count_only=True)
    assert out == plain_out and res == plain
    want = X.Expected(recs, True, drop=False)
    assert out == want.text
    want.check_report(rep)
    assert rep.duplicates == X.Expected(recs, True).duplicates > 0


def test_paired_host_route_against_the_loop(F):
    r1, r2 = X.pair_records(600, 200)
    want = X.ExpectedPairs(r1, r2)
    res, o1, o2, om, rep = X.run_pairs(F, M.file_of(r1), M.file_of(r2), F.entrypos, FBUF)
    assert (o1, o2, om) == tuple(want.text)
    assert tuple(res) == want.result()
    want.check_report(rep)
    assert want.duplicates > 100 and want.pairs_merged > 30 and want.first_copy_filtered > 3 and sum(want.dropped.values()) > 50
    assert res.pairs_in == res.pairs_out + sum(res.dropped.values()) + rep.duplicates
    # count only: the files of a run without dedup, the same numbers
    plain = X.run_pairs(F, M.file_of(r1), M.file_of(r2), F.entrypos, FBUF, dedup=False)
    cres, c1, c2, cm, crep = X.run_pairs(F, M.file_of(r1), M.file_of(r2), F.entrypos, FBUF, count_only=True)
    assert (c1, c2, cm) == plain[1:4] and cres == plain[0]
    assert (c1, c2, cm) == tuple(X.ExpectedPairs(r1, r2, dedup=False).text)
    assert (crep.keyed, crep.unkeyed, crep.distinct, crep.duplicates) == (rep.keyed, rep.unkeyed, rep.distinct, rep.duplicates)


def test_fastq_stats_duplication_on_the_host_route(F, recs):
    data = P.fastq(recs)
    st = F.fastq_stats(io.BytesIO(data), FBUF, entrypos=F.entrypos, duplication=True)
    want = X.Expected(recs, False)
    assert (st.keyed, st.distinct, st.duplicates) == (want.keyed, want.distinct, want.duplicates)
    assert st.duplication_rate == want.duplicates / want.keyed
    plain = F.fastq_stats(io.BytesIO(data), FBUF, entrypos=F.entrypos)
    assert plain == st and plain.keyed is plain.distinct is plain.duplicates is plain.duplication_rate is None


def test_arguments(F):
    with pytest.raises(TypeError):
        F.filter_fastq(io.BytesIO(), io.BytesIO(), dedup=True, entrypos=F.entrypos)
    with pytest.raises(ValueError, match="dedup_report needs dedup"):
        F.filter_fastq(io.BytesIO(), io.BytesIO(), dedup_report=F.DedupReport(), entrypos=F.entrypos)
    with pytest.raises(ValueError):
        F.DedupRules(expected_reads=-1)
    with pytest.raises(TypeError):
        F.filter_fastq_paired(io.BytesIO(), io.BytesIO(), io.BytesIO(), io.BytesIO(), dedup=1, entrypos=F.entrypos)
    rep = F.DedupReport()
    res = F.filter_fastq(io.BytesIO(), io.BytesIO(), dedup=F.DedupRules(), dedup_report=rep, entrypos=F.entrypos)
    assert tuple(res) == (0, 0, 0, 0) and rep.duplication_rate == 0.0 and rep.keyed == 0

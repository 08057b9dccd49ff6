"""How filter_fastq, filter_fastq_paired and readfastq_iter CONFIGURE a native stream, without a GPU: a scanner whose
open_stream hands out recording fakes (tests/plan_fakes.py: the setters and getters of hip._Stream, no fill).  What the three callers ask of
a stream for one parameter set is compared with literals written here: the same setters, in the same order, with the same
arguments; an argument that is switched off calls nothing; a setter that raises leaves no stream open."""
import io

import pytest

from plan_fakes import FakeScanner, no_rounds, paired, single  # noqa: F401

ADAPTER = b"AGATCGGAAGAGC"


@pytest.fixture(scope="module")
def F(pkg):
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


@pytest.fixture(scope="module")
def hip(pkg):
    from fastqandfurious_amd import hip
    return hip


def iterated(F, scanner, entryfunc):
    return list(F.readfastq_iter(io.BytesIO(b""), 4096, entryfunc, scanner))


def test_one_parameter_set_three_callers(F, hip, no_rounds):
    rules = F.ContentRules(max_n=0)
    assert (hip.STATS_IN, hip.STATS_OUT) == (1, 2)
    want = [("set_trim", 20, 20, 33), ("set_adapter", ADAPTER, 100, 3), ("set_content", rules), ("set_filter", 30, 200, None, 0),
            ("set_render",), ("set_stats", 3, 33, 512)]

    sc = FakeScanner()
    res = single(F, sc, quality_cutoff=(20, 20), adapter=ADAPTER, err_permille=100, min_overlap=3, min_len=30, max_len=200,
                 content=rules, report=F.FilterReport())
    assert tuple(res) == (0, 0, 0, 0)
    assert [s.log for s in sc.streams] == [want]
    assert [s.closed for s in sc.streams] == [1]

    sc = FakeScanner()
    res = paired(F, sc, quality_cutoff=(20, 20), adapter=ADAPTER, adapter2=ADAPTER, err_permille=100, min_overlap=3, min_len=30,
                 max_len=200, content=rules, report=F.FilterReport(), report2=F.FilterReport())
    assert tuple(res) == (0, 0, 0, 0, 0, {"mate1_only": 0, "mate2_only": 0, "both": 0})
    assert [s.log for s in sc.streams] == [want, want]
    assert [s.closed for s in sc.streams] == [1, 1]
    assert len(no_rounds.made) == 1 and no_rounds.made[0].mates == tuple(sc.streams) and no_rounds.made[0].closed == 1

    # the iterator's push-down: no render, no statistics, set_filter always and with the entryfunc's column.  One entryfunc
    # trims, another judges by content: the two together ask for what the filters ask for, in their order
    sc = FakeScanner()
    assert iterated(F, sc, F.entryfunc_adaptertrim(ADAPTER, 100, 3, (20, 20), 33, 30, 200, "sequence")) == []
    assert [s.log for s in sc.streams] == [want[:2] + [("set_filter", 30, 200, "sequence", 0)]]
    sc2 = FakeScanner()
    assert iterated(F, sc2, F.entryfunc_contentfilter(rules, 30, 200, "quality")) == []
    assert [s.log for s in sc2.streams] == [want[2:3] + [("set_filter", 30, 200, "quality", 0)]]
    assert [s.closed for s in sc.streams + sc2.streams] == [1, 1]
    # ("entry" is the stream's "no column")
    sc = FakeScanner()
    iterated(F, sc, F.entryfunc_qualitytrim(20, 20, 33, 30, 200))
    assert [s.log for s in sc.streams] == [want[:1] + want[3:4]]


ONE_AT_A_TIME = (
    ({}, []),
    ({"quality_cutoff": 17}, [("set_trim", 17, 0, 33)]),
    ({"quality_cutoff": (5, 17), "qual_base": 64}, [("set_trim", 17, 5, 64)]),
    ({"adapter": ADAPTER, "err_permille": 200, "min_overlap": 5}, [("set_adapter", ADAPTER, 200, 5)]),
    ({"min_len": 30}, [("set_filter", 30, None, None, 0)]),
    ({"max_len": 200}, [("set_filter", None, 200, None, 0)]),
)


@pytest.mark.parametrize("kw,want", ONE_AT_A_TIME)
def test_what_is_switched_off_calls_nothing(F, no_rounds, kw, want):
    sc = FakeScanner()
    single(F, sc, **kw)
    assert [s.log for s in sc.streams] == [want + [("set_render",)]]
    sc = FakeScanner()
    paired(F, sc, **kw)
    # (`adapter` is mate 1's; mate 2's is adapter2)
    want2 = [c for c in want if c[0] != "set_adapter"]
    assert [s.log for s in sc.streams] == [want + [("set_render",)], want2 + [("set_render",)]]
    assert [s.closed for s in sc.streams] == [1, 1]


def test_content_and_report_alone_and_per_mate(F, no_rounds):
    rules = F.ContentRules(min_complexity=30)
    sc = FakeScanner()
    single(F, sc, content=rules)
    assert [s.log for s in sc.streams] == [[("set_content", rules), ("set_render",)]]
    sc = FakeScanner()
    single(F, sc, report=F.FilterReport(100), qual_base=64)
    assert [s.log for s in sc.streams] == [[("set_render",), ("set_stats", 3, 64, 100)]]
    # a pair: bounds, adapter and report of each mate are that mate's
    sc = FakeScanner()
    paired(F, sc, min_len=(30, None), max_len=(None, 99), adapter2=b"ACGT", report2=F.FilterReport(64))
    assert [s.log for s in sc.streams] == [[("set_filter", 30, None, None, 0), ("set_render",)],
                                           [("set_adapter", b"ACGT", 100, 3), ("set_filter", None, 99, None, 0), ("set_render",),
                                            ("set_stats", 3, 33, 64)]]
    # the iterator: its length filter without a bound still sets the filter; an entryfunc it does not know sets nothing
    sc = FakeScanner()
    iterated(F, sc, F.entryfunc_lengthfilter())
    assert [s.log for s in sc.streams] == [[("set_filter", None, None, "sequence", 0)]]
    sc = FakeScanner()
    iterated(F, sc, F.entryfunc)
    assert [s.log for s in sc.streams] == [[]] and sc.streams[0].closed == 1


@pytest.mark.parametrize("setter", ("set_trim", "set_adapter", "set_content", "set_filter", "set_render", "set_stats"))
def test_a_setter_that_raises_closes_every_stream(F, no_rounds, setter):
    rules = F.ContentRules(max_n=0)
    kw = dict(quality_cutoff=20, adapter=ADAPTER, min_len=30, content=rules)
    sc = FakeScanner(fail=(0, setter))
    with pytest.raises(RuntimeError, match=setter + " refused"):
        single(F, sc, report=F.FilterReport(), **kw)
    assert [s.closed for s in sc.streams] == [1]
    for mate in (0, 1):
        sc = FakeScanner(fail=(mate, setter))
        with pytest.raises(RuntimeError, match=setter + " refused"):
            paired(F, sc, adapter2=ADAPTER, report=F.FilterReport(), report2=F.FilterReport(), **kw)
        assert [s.closed for s in sc.streams] == [1, 1]
        assert no_rounds.made == []
    if setter in ("set_trim", "set_adapter", "set_filter"):
        sc = FakeScanner(fail=(0, setter))
        with pytest.raises(RuntimeError, match=setter + " refused"):
            iterated(F, sc, F.entryfunc_adaptertrim(ADAPTER, quality_cutoff=20, min_len=30))
        assert [s.closed for s in sc.streams] == [1]
    if setter in ("set_content", "set_filter"):
        sc = FakeScanner(fail=(0, setter))
        with pytest.raises(RuntimeError, match=setter + " refused"):
            iterated(F, sc, F.entryfunc_contentfilter(rules, 30))
        assert [s.closed for s in sc.streams] == [1]


def test_two_streams_or_none(F, no_rounds):
    """a second mate that cannot be streamed: the first one's stream is closed and the host route is taken"""
    sc = FakeScanner(none_at=1)
    with pytest.raises(AssertionError, match="the host route was taken"):
        paired(F, sc)
    assert [s.closed for s in sc.streams] == [1] and sc.streams[0].log == [] and no_rounds.made == []


# ---- the pair's own ladder (hip.PairStream's setters)
def pair_features(F):
    """every feature of the pair -> (its arguments, the setter calls they alone cause)"""
    overlap, correction = F.OverlapRules(20, 3, 100), F.CorrectionRules(31, 13)
    dedup = F.DedupRules(expected_reads=1000, max_bytes=1 << 20, count_only=True)
    return {
        "overlap": (dict(overlap=overlap), [("set_overlap", overlap, True)]),
        "correction": (dict(overlap=overlap, correction=correction, qual_base=64),
                       [("set_overlap", overlap, True), ("set_correct", correction, 64)]),
        "merge": (dict(overlap=overlap, merged_out=io.BytesIO()), [("set_overlap", overlap, True), ("set_merge", True)]),
        "compress": (dict(compress="bgzf"), []),
        "dedup": (dict(dedup=dedup), [("set_dedup", False, 1000, 1 << 20)]),
    }


def test_the_pairs_ladder_with_everything_on(F, no_rounds):
    overlap, correction, dedup = F.OverlapRules(), F.CorrectionRules(), F.DedupRules()
    sc = FakeScanner()
    paired(F, sc, overlap=overlap, correction=correction, merged_out=io.BytesIO(), compress="bgzf", dedup=dedup)
    assert len(no_rounds.made) == 1
    ps = no_rounds.made[0]
    assert ps.log == [("set_overlap", overlap, True), ("set_correct", correction, 33), ("set_merge", True),
                      ("set_compress", "bgzf"), ("set_dedup", True, 0, 0)]
    assert ps.mates == tuple(sc.streams) and ps.opened == ("any", True) and ps.closed == 1
    # (the mates compress their own text; a pair's duplicates are the pair's, not a mate's)
    assert [s.log for s in sc.streams] == [[("set_render",), ("set_compress", "bgzf")]] * 2
    assert [s.closed for s in sc.streams] == [1, 1]


@pytest.mark.parametrize("feature", ("overlap", "correction", "merge", "compress", "dedup"))
def test_a_pair_feature_alone_calls_its_own_setter(F, no_rounds, feature):
    kw, want = pair_features(F)[feature]
    sc = FakeScanner()
    paired(F, sc, pair_filter="first", check_names=False, **kw)
    ps = no_rounds.made[0]
    assert ps.log == want and ps.opened == ("first", False) and ps.closed == 1
    assert [s.closed for s in sc.streams] == [1, 1]


@pytest.mark.parametrize("setter", ("set_overlap", "set_correct", "set_merge", "set_compress", "set_dedup"))
def test_a_pair_setter_that_raises_closes_everything(F, no_rounds, monkeypatch, setter):
    class Out:
        writes = 0

        def write(self, data):
            Out.writes += 1
    monkeypatch.setattr(no_rounds, "fail", setter)
    sc = FakeScanner()
    with pytest.raises(RuntimeError, match=setter + " refused"):
        F.filter_fastq_paired(io.BytesIO(b""), io.BytesIO(b""), Out(), Out(), 4096, entrypos=sc, overlap=F.OverlapRules(),
                              correction=F.CorrectionRules(), merged_out=Out(), compress="bgzf", dedup=F.DedupRules())
    assert [s.closed for s in sc.streams] == [1, 1]
    assert len(no_rounds.made) == 1 and no_rounds.made[0].closed == 1
    assert Out.writes == 0

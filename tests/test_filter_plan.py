"""How filter_fastq, filter_fastq_paired and readfastq_iter CONFIGURE a native stream, without a GPU: a scanner whose
open_stream hands out recording fakes (the setters and getters of hip._Stream, no fill).  What the three callers ask of
a stream for one parameter set is compared with literals written here: the same setters, in the same order, with the same
arguments; an argument that is switched off calls nothing; a setter that raises leaves no stream open."""
import io

import numpy as np
import pytest

ADAPTER = b"AGATCGGAAGAGC"


@pytest.fixture(scope="module")
def F(pkg):
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


@pytest.fixture(scope="module")
def hip(pkg):
    from fastqandfurious_amd import hip
    return hip


class FakeStream:
    """hip._Stream's surface: every setter call is logged with its arguments as the real signature binds them."""
    decode = False

    def __init__(self, fail=None):
        self.log, self.fail, self.filtered, self.closed, self.cycles = [], fail, False, 0, 1

    def _call(self, name, *args):
        if name == self.fail:
            raise RuntimeError("%s refused" % name)
        self.log.append((name,) + args)

    def set_filter(self, min_seq_len=None, max_seq_len=None, column=None, value_add=0):
        self._call("set_filter", min_seq_len, max_seq_len, column, value_add)
        self.filtered = True

    def set_content(self, rules):
        self._call("set_content", rules)
        self.filtered = True

    def set_trim(self, cutoff_back, cutoff_front=0, qual_base=33):
        self._call("set_trim", cutoff_back, cutoff_front, qual_base)

    def set_adapter(self, adapter, err_permille=100, min_overlap=3):
        self._call("set_adapter", adapter, err_permille, min_overlap)

    def set_stats(self, which, qual_base=33, max_cycles=512):
        self._call("set_stats", which, qual_base, max_cycles)
        self.cycles = max_cycles

    def set_render(self):
        self._call("set_render")

    # what a fill would be asked for; the fake yields none, so only stats() is ever reached
    def rendered(self):
        return np.zeros(0, dtype=np.uint8), (0, 0, 0)

    def filter_counts(self):
        return [0] * 8

    def trimmed(self):
        return 0, 0, 0

    adapter_trimmed = trimmed

    def selected(self):
        return np.zeros(0, dtype=np.int64), 0, None, None

    def stats(self, which):
        from fastqandfurious_amd import hip
        return np.zeros(hip.stats_words(self.cycles), dtype=np.uint64)

    def __iter__(self):
        return iter(())

    def close(self):
        self.closed += 1


class FakeScanner:
    """An `entrypos` with an open_stream attribute; fail: (ordinal of the stream, setter that raises); none_at: the ordinal
    at which open_stream declines (returns None, as the real one does for a source it cannot stream)."""

    def __init__(self, fail=None, none_at=None):
        self.streams, self.fail, self.none_at = [], fail, none_at

    def open_stream(self, fh, fbufsize, decode=False):
        k = len(self.streams)
        if k == self.none_at:
            return None
        self.streams.append(FakeStream(self.fail[1] if self.fail is not None and self.fail[0] == k else None))
        return self.streams[-1]

    def __call__(self, buf, offset, posbuffer):
        raise AssertionError("the host route was taken")


class NoRounds:
    """hip.PairStream's surface, yielding no round."""
    made = []

    def __init__(self, mate1, mate2, pair_filter="any", check_names=True):
        self.mates, self.closed = (mate1, mate2), 0
        NoRounds.made.append(self)

    def set_overlap(self, rules, trim=True):
        pass

    def overlap(self, hist=True):
        from fastqandfurious_amd import hip
        return [0] * 6, np.zeros(hip.OVERLAP_HIST_WORDS, dtype=np.uint64)

    def __iter__(self):
        return iter(())

    def close(self):
        self.closed += 1


@pytest.fixture
def no_rounds(hip, monkeypatch):
    NoRounds.made = []
    monkeypatch.setattr(hip, "PairStream", NoRounds)
    return NoRounds


def single(F, scanner, **kw):
    return F.filter_fastq(io.BytesIO(b""), io.BytesIO(), 4096, entrypos=scanner, **kw)


def paired(F, scanner, **kw):
    return F.filter_fastq_paired(io.BytesIO(b""), io.BytesIO(b""), io.BytesIO(), io.BytesIO(), 4096, entrypos=scanner, **kw)


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

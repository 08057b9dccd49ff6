"""How filter_fastq and filter_fastq_paired ask a native stream for the poly steps, without a GPU: the recording fakes of
tests/test_filter_plan.py (copied, with set_poly and poly_trimmed added).  set_poly is called once, in its place in the ladder
-- behind set_trim and in front of set_adapter, where the first of its two steps works --, only when a setting is on; a
setter that raises leaves no stream open; a range error is raised before a stream is opened."""
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

    def set_poly(self, poly_g=None, poly_x=None):
        self._call("set_poly", poly_g, poly_x)

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

    def poly_trimmed(self):
        return (0, 0, 0), (0, 0, 0)

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
    """An `entrypos` with an open_stream attribute; fail: (ordinal of the stream, setter that raises)."""

    def __init__(self, fail=None):
        self.streams, self.fail = [], fail

    def open_stream(self, fh, fbufsize, decode=False):
        k = len(self.streams)
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


def test_set_poly_in_its_place_in_the_ladder(F, no_rounds):
    rules = F.ContentRules(max_n=0)
    want = [("set_trim", 20, 20, 33), ("set_poly", 10, 12), ("set_adapter", ADAPTER, 100, 3), ("set_content", rules),
            ("set_filter", 30, 200, None, 0), ("set_render",), ("set_stats", 3, 33, 512)]
    kw = dict(quality_cutoff=(20, 20), adapter=ADAPTER, min_len=30, max_len=200, content=rules, poly_g=10, poly_x=12)
    sc = FakeScanner()
    rep = F.PolyReport()
    res = single(F, sc, report=F.FilterReport(), poly_report=rep, **kw)
    assert tuple(res) == (0, 0, 0, 0) and rep.__dict__ == F.PolyReport().__dict__
    assert [s.log for s in sc.streams] == [want] and [s.closed for s in sc.streams] == [1]
    sc = FakeScanner()
    paired(F, sc, adapter2=ADAPTER, report=F.FilterReport(), report2=F.FilterReport(), **kw)
    assert [s.log for s in sc.streams] == [want, want] and [s.closed for s in sc.streams] == [1, 1]
    assert len(no_rounds.made) == 1 and no_rounds.made[0].closed == 1


@pytest.mark.parametrize("kw,call", (
    ({}, None),
    ({"poly_report": "a report"}, None),
    ({"poly_g": 10}, ("set_poly", 10, None)),
    ({"poly_x": 2}, ("set_poly", None, 2)),
    ({"poly_g": 65535, "poly_x": 10}, ("set_poly", 65535, 10)),
))
def test_set_poly_once_and_only_when_a_setting_is_on(F, no_rounds, kw, call):
    kw = dict(kw)
    if "poly_report" in kw:
        kw["poly_report"] = F.PolyReport()
    want = ([call] if call else []) + [("set_render",)]
    sc = FakeScanner()
    single(F, sc, **kw)
    assert [s.log for s in sc.streams] == [want]
    sc = FakeScanner()
    paired(F, sc, **kw)
    assert [s.log for s in sc.streams] == [want, want] and [s.closed for s in sc.streams] == [1, 1]


@pytest.mark.parametrize("setter", ("set_trim", "set_poly", "set_adapter", "set_render"))
def test_a_setter_that_raises_closes_every_stream(F, no_rounds, setter):
    kw = dict(quality_cutoff=20, adapter=ADAPTER, min_len=30, poly_g=10, poly_x=10)
    sc = FakeScanner(fail=(0, setter))
    with pytest.raises(RuntimeError, match=setter + " refused"):
        single(F, sc, **kw)
    assert [s.closed for s in sc.streams] == [1]
    for mate in (0, 1):
        sc = FakeScanner(fail=(mate, setter))
        with pytest.raises(RuntimeError, match=setter + " refused"):
            paired(F, sc, adapter2=ADAPTER, **kw)
        assert [s.closed for s in sc.streams] == [1, 1]
        assert no_rounds.made == []


@pytest.mark.parametrize("name", ("poly_g", "poly_x"))
def test_a_range_error_opens_no_stream(F, no_rounds, name):
    for bad in (1, 65536, 0):
        sc = FakeScanner()
        with pytest.raises(ValueError, match=name):
            single(F, sc, **{name: bad})
        with pytest.raises(ValueError, match=name):
            paired(F, sc, **{name: bad})
        assert sc.streams == [] and no_rounds.made == []

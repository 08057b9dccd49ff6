"""How filter_fastq and filter_fastq_paired ask a native stream for the poly steps, without a GPU: the recording fakes of
tests/plan_fakes.py.  set_poly is called once, in its place in the ladder
-- behind set_trim and in front of set_adapter, where the first of its two steps works --, only when a setting is on; a
setter that raises leaves no stream open; a range error is raised before a stream is opened."""
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

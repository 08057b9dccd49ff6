"""The stream front end's per-fill chain -- scan, ffq_table_trim_quality and ffq_table_trim_adapter in place, table_select,
ffq_table_render_fastq or ffq_table_gather_column, the copies back, carry and refill (ffq_stream_next: stream_take,
stream_scan, stream_chain in csrc/ffq_stream.h) -- on reads as files hold them: short and long ones, some with the 3' adapter, wrapped records between single-line ones, empty headers, '+' lines that repeat the header,
quality lines that begin with '@' and '+', a bad tile, reads above the kernels' short / long split and a record longer
than the buffer.

The stream chooses the buffer address (d_buf = slot + start - mis), `add` (globaloffset - mis, negative on the first fill)
and the fill boundaries itself, so every fill is compared with the same slice of ONE global expectation:

    rows    the oracle's C-variant scan of the whole corpus (stream byte i is file byte i, the sentinel is -1)
    trim    test_trim.loop_rows over those rows
    adapter test_adapter.loop_rows over what that left (cutadapt's order)
    filter  a numpy comparison of pos3 - pos2 of the trimmed rows
    text    test_render.loop_render of the kept rows
    column  test_gather.loop_gather of the kept rows

-- never the package's own trim, adapter, select, gather or render code.  Every comparison is exact.  The corpora come from the
seeded generator below; no corpus holds a read of length 0 (the device scanners do not read one back:
test_empty_reads_are_read_back_by_the_python_scanner_only), and rendered text is rescanned on the device only where the
filter has min_len >= 1.
"""
import contextlib
import gzip
import io
import os

import numpy as np
import pytest

from test_adapter import AD, loop_rows as adapter_loop_rows
from test_gather import loop_gather
from test_render import loop_render
from test_trim import expected_items, loop_rows

END_OK, END_REFILL, END_ERR_FINAL_QUAL, END_ERR_INCOMPLETE, END_ERR_INVALID = range(5)


# ---- the corpora -----------------------------------------------------------------------------------------------------------
COUNTS = {"mixed": 12000, "long": 3000, "small": 500}
SEEDS = {"mixed": 20241, "long": 20242, "small": 20243}
TILE_AT = {"mixed": 5000, "long": 1500}             # first record of the bad tile
TILE = 1100                                         # ... and its records: more than the 1024 of the gather's window walk
ADAPTER_SHARE = 0.3                                 # of the reads: the 3' adapter (test_adapter.AD) from a random base on
LONG_LENGTHS = (4095, 4096, 4097, 9000, 70000)      # either side of TRIM_LONG / RENDER_LONG; longer than every fbufsize below
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_NOISE = np.frombuffer(b"@+#5?I", dtype=np.uint8)
_CORPUS, _EXPECT, _HOST = {}, {}, {}


def _quality(rng, n, kind):
    """good (Q25..40); a bad 3' tail; a bad 5' head; all '#'; noise whose lines begin with '@' and '+'"""
    if kind == 3:
        return b"#" * n
    if kind == 4:
        return _NOISE[rng.integers(0, len(_NOISE), n)].tobytes()
    q = rng.integers(33 + 25, 33 + 41, n, dtype=np.uint8)
    if kind in (1, 2):
        k = int(rng.integers(1, n + 1))
        bad = rng.integers(33 + 2, 33 + 16, k, dtype=np.uint8)
        if kind == 1:
            q[n - k:] = bad
        else:
            q[:k] = bad
    return q.tobytes()


def _wrap(b, w):
    return b"\n".join(b[i:i + w] for i in range(0, len(b), w))


def make_corpus(kind):
    rng = np.random.default_rng(SEEDS[kind])
    arng = np.random.default_rng(SEEDS[kind] + 100)     # (the adapters' own generator: `rng` draws what it drew without them)
    tile = range(TILE_AT[kind], TILE_AT[kind] + TILE) if kind in TILE_AT else range(0)
    parts = []
    for i in range(COUNTS[kind]):
        n = int(rng.integers(1, 40)) if rng.random() < 0.2 else int(rng.integers(40, 321))
        wrapped = rng.random() < 0.15 and n >= 2 and i not in tile
        long_one = kind == "long" and i % 150 == 75
        if long_one:
            n, wrapped = LONG_LENGTHS[(i // 150) % len(LONG_LENGTHS)], False
        head = b"" if rng.random() < 0.03 else b"r%d:%d/%d" % (i, int(rng.integers(0, 10 ** int(rng.integers(1, 9)))), i % 2 + 1)
        plus = b"+" + head if rng.random() < 0.2 else b"+"
        seq = _ACGT[rng.integers(0, 4, n)].tobytes()
        if arng.random() < ADAPTER_SHARE:
            # a short insert: the adapter and what the sequencer read behind it, cut off by the read's end
            p = int(arng.integers(0, n))
            seq = (seq[:p] + AD + _ACGT[arng.integers(0, 4, n)].tobytes())[:n]
        qual = _quality(rng, n, 3 if i in tile else int(rng.choice(5, p=(0.35, 0.25, 0.15, 0.1, 0.15))))
        if wrapped:
            w = int(rng.integers(7, 91))
            if w >= n:
                w = max(1, n // 2)
            seq, qual = _wrap(seq, w), _wrap(qual, w)
        parts.append(b"@" + head + b"\n" + seq + b"\n" + plus + b"\n" + qual + b"\n")
    return b"".join(parts)


def corpus(kind):
    if kind not in _CORPUS:
        _CORPUS[kind] = make_corpus(kind)
    return _CORPUS[kind]


# ---- the expectation -------------------------------------------------------------------------------------------------------
class Expect:
    """The oracle's rows of `data` and what the three loops make of them; computed once, read-only."""

    def __init__(self, oracle, data):
        self.data = data
        self.rows, self.end, _status, self.end_offset = oracle.scan(data)
        self.rows.setflags(write=False)
        self.n = self.rows.shape[0]
        self._trim, self._adapter = {}, {}

    def trimmed(self, trim):
        """(trimmed rows, cum int64[n + 1][3]): cum[b] - cum[a] = loop_rows' [changed, removed, skipped] over rows a..b-1
        (the loop run row by row: its counters are sums over rows).  trim = (front, back) or None."""
        if trim not in self._trim:
            cum = np.zeros((self.n + 1, 3), dtype=np.int64)
            if trim is None:
                t = self.rows
            else:
                out = [loop_rows(self.data, self.rows[i:i + 1], trim[0], trim[1]) for i in range(self.n)]
                t = np.concatenate([r for r, _s in out]) if out else np.zeros((0, 6), dtype=np.int64)
                np.cumsum(np.array([s for _r, s in out], dtype=np.int64).reshape(-1, 3), axis=0, out=cum[1:])
                t.setflags(write=False)
            self._trim[trim] = (t, cum)
        return self._trim[trim]

    def adapted(self, trim):
        """(the trimmed rows cut at the adapter, cum of test_adapter.loop_rows' counters), as trimmed()"""
        if trim not in self._adapter:
            out = [adapter_loop_rows(self.data, r[None, :]) for r in self.trimmed(trim)[0]]
            t = np.concatenate([r for r, _s in out]) if out else np.zeros((0, 6), dtype=np.int64)
            cum = np.zeros((self.n + 1, 3), dtype=np.int64)
            np.cumsum(np.array([s for _r, s in out], dtype=np.int64).reshape(-1, 3), axis=0, out=cum[1:])
            t.setflags(write=False)
            self._adapter[trim] = (t, cum)
        return self._adapter[trim]

    def kept(self, trim, lo=None, hi=None, adapter=False):
        """(trimmed rows -- cut at the adapter too, if `adapter` --, cum of the TRIM, mask of the rows with lo <= pos3 - pos2 <= hi)"""
        t, cum = self.trimmed(trim)
        if adapter:
            t = self.adapted(trim)[0]
        lens = t[:, 3] - t[:, 2]
        keep = np.ones(self.n, dtype=bool)
        if lo is not None:
            keep &= lens >= lo
        if hi is not None:
            keep &= lens <= hi
        return t, cum, keep

    def output(self, trim, lo=None, hi=None):
        """(text, FilterResult as a tuple) of filter_fastq by the loops"""
        t, cum, keep = self.kept(trim, lo, hi)
        text, _off, stats = loop_render(self.data, t[keep])
        assert stats[2] == 0
        return text, (self.n, int(keep.sum()), int(cum[self.n, 1]), len(text))

    def items(self, trim, lo, hi, column):
        """one item per row, None for a dropped one: what readfastq_iter owes for entryfunc_qualitytrim"""
        t, _cum, keep = self.kept(trim, lo, hi)
        d, out = self.data, []
        for (p0, p1, p2, p3, p4, p5), k in zip(t.tolist(), keep.tolist()):
            e = (d[p0 + 1:p1], d[p2:p3], d[p4:p5])
            out.append(None if not k else e if column == "entry" else e[("header", "sequence", "quality").index(column)])
        return out


def expect(oracle, kind):
    if kind not in _EXPECT:
        _EXPECT[kind] = Expect(oracle, corpus(kind))
    return _EXPECT[kind]


def longest_run_of_empty(rows):
    best = run = 0
    for ln in (rows[:, 3] - rows[:, 2]).tolist():
        run = run + 1 if ln == 0 else 0
        best = max(best, run)
    return best


def entries_of(data, rows):
    return [(data[p0 + 1:p1], data[p2:p3], data[p4:p5]) for p0, p1, p2, p3, p4, p5 in np.asarray(rows).tolist()]


# ---- the inputs are what the GPU tests rely on (no GPU) --------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(COUNTS))
def test_corpus_conditions(pkg, oracle, kind):
    from fastqandfurious_amd import fastqandfurious as F
    data = corpus(kind)
    exp = expect(oracle, kind)
    assert exp.end == END_OK and exp.n == COUNTS[kind]
    assert {"mixed": 3000000, "long": 1000000, "small": 100000}[kind] <= len(data) <= {"mixed": 4500000, "long": 2500000, "small": 200000}[kind]
    # the oracle's C variant and the Python scanner give the same records
    got = list(F.readfastq_iter(io.BytesIO(data), 1 << 20, F.entryfunc, F.entrypos))
    assert got == entries_of(data, exp.rows)
    py_rows, py_end, *_ = oracle.scan(data, variant=1)
    assert py_end == END_OK and (py_rows == exp.rows).all()
    assert all(len(s) > 0 for _h, s, _q in got), "a read of length 0"
    # what the corpus holds
    heads = [h for h, _s, _q in got]
    assert heads.count(b"") >= COUNTS[kind] // 100
    assert sum(data[r[3]:r[3] + 3] != b"\n+\n" for r in exp.rows.tolist()) >= COUNTS[kind] // 10       # '+' lines with the header
    qlines = [ln for _h, _s, q in got for ln in q.split(b"\n")]
    assert sum(ln[:1] == b"@" for ln in qlines) >= 10 and sum(ln[:1] == b"+" for ln in qlines) >= 10
    # cutoffs (20, 20), min_len 30
    t, cum, keep = exp.kept((20, 20), 30, None)
    changed, _removed, skipped = cum[exp.n].tolist()
    wrapped = np.array([b"\n" in q for _h, _s, q in got])
    assert skipped == wrapped.sum() and skipped >= exp.n // 20
    assert exp.n // 4 <= keep.sum() <= 3 * exp.n // 4
    assert (t[~wrapped][:, 3] == t[~wrapped][:, 2]).sum() > 0, "no read is trimmed away"
    assert 0 < changed < exp.n - skipped, "every eligible read is trimmed, or none"
    assert (t[wrapped] == exp.rows[wrapped]).all()
    # the adapter behind that trim: found in a share of the eligible reads, neither none nor all; the filter still drops some
    ta, acum = exp.adapted((20, 20))
    a_changed, a_removed, a_skipped = acum[exp.n].tolist()
    assert a_skipped == skipped and (ta[wrapped] == exp.rows[wrapped]).all()
    assert exp.n // 10 <= a_changed <= exp.n // 2 and a_removed > a_changed, (a_changed, a_removed)
    assert a_changed == ((ta[:, 3] != t[:, 3]).sum()) and (ta[:, :3] == t[:, :3]).all()
    keep_a = exp.kept((20, 20), 30, None, adapter=True)[2]
    assert 0 < keep_a.sum() < keep.sum()
    lens = exp.rows[:, 5] - exp.rows[:, 4]
    if kind in TILE_AT:
        assert longest_run_of_empty(t) >= TILE > 1024
        assert longest_run_of_empty(exp.trimmed((0, 20))[0]) >= TILE
    else:
        assert longest_run_of_empty(t) < 1000
    if kind == "long":
        assert (lens[~wrapped] > 65536).any() and (len(data) - 1 > 65536)
        assert ((lens[~wrapped] > 4096) & (lens[~wrapped] < 4200)).any() and ((lens[~wrapped] >= 4000) & (lens[~wrapped] <= 4096)).any()
        assert sorted(set(lens[lens > 4000].tolist())) == sorted(LONG_LENGTHS)
        untiled = np.ones(exp.n, dtype=bool)
        untiled[TILE_AT[kind]:TILE_AT[kind] + TILE] = False
        assert sorted(set(lens[untiled & (lens > 4000)].tolist())) == sorted(LONG_LENGTHS)
    else:
        assert lens.max() <= 320 + 320 // 7


PARAMS = {"cut20-20_min30": (dict(quality_cutoff=(20, 20), min_len=30), ((20, 20), 30, None)),
          "cut20_max140": (dict(quality_cutoff=20, max_len=140), ((0, 20), None, 140))}


def host_filter(F, kind, params):
    """the package's own per-record path (Python scanner) over a corpus: (output, FilterResult); once per corpus"""
    if (kind, params) not in _HOST:
        out = io.BytesIO()
        res = F.filter_fastq(io.BytesIO(corpus(kind)), out, 1 << 20, entrypos=F.entrypos, **PARAMS[params][0])
        _HOST[kind, params] = (out.getvalue(), tuple(res))
    return _HOST[kind, params]


@pytest.mark.parametrize("params", sorted(PARAMS))
@pytest.mark.parametrize("kind", sorted(COUNTS))
def test_filter_fastq_python_scanner(pkg, oracle, kind, params):
    """filter_fastq's host loop (entrypos=F.entrypos) == the loops over the oracle's rows, at two buffer sizes"""
    from fastqandfurious_amd import fastqandfurious as F
    want, counters = expect(oracle, kind).output(*PARAMS[params][1])
    assert 0 < counters[1] < counters[0] and counters[2] > 0
    assert host_filter(F, kind, params) == (want, counters)
    out = io.BytesIO()
    res = F.filter_fastq(io.BytesIO(corpus(kind)), out, 3000, entrypos=F.entrypos, **PARAMS[params][0])
    assert out.getvalue() == want and tuple(res) == counters


EMPTY_READS = b"@a\nACGT\n+\nIIII\n@e\n\n+\n\n@b\nAC\n+\nII\n@c\nACG\n+\nIII\n"


def test_empty_reads_are_read_back_by_the_python_scanner_only(pkg, oracle):
    """A rendered read of length 0 ("@e\\n\\n+\\n\\n"): the Python scanner reads the file back record for record; the
    reference's C scanner -- the oracle's C variant, which the device scanners answer as -- looks for the end of a sequence
    behind its first byte, reads the empty record and its successor as ONE record and reports no error.  min_len >= 1 in
    front of the rendering is what makes a file safe for the GPU scanner and for other tools."""
    from fastqandfurious_amd import fastqandfurious as F
    rows, end, _status, _off = oracle.scan(EMPTY_READS)
    assert end == END_OK and rows.tolist() == [[0, 2, 3, 7, 10, 14], [15, 17, 18, 27, 30, 39]]
    four = [(b"a", b"ACGT", b"IIII"), (b"e", b"", b""), (b"b", b"AC", b"II"), (b"c", b"ACG", b"III")]
    rows, end, _status, _off = oracle.scan(EMPTY_READS, variant=1)
    assert end == END_OK and entries_of(EMPTY_READS, rows) == four
    for fbufsize in (1 << 16, 20):
        assert list(F.readfastq_iter(io.BytesIO(EMPTY_READS), fbufsize, F.entryfunc, F.entrypos)) == four
    # ... and that text is what the loop renders of those four rows
    assert loop_render(EMPTY_READS, rows)[0] == EMPTY_READS


# ---- the stream, fill by fill ----------------------------------------------------------------------------------------------
CONFIGS = {
    "trim20-20": dict(trim=(20, 20)),
    "trim0-20_render": dict(trim=(0, 20), render=True),
    "trim20-20_min30_render": dict(trim=(20, 20), flt=(30, None), render=True),
    "trim10-0_1to140_render": dict(trim=(10, 0), flt=(1, 140), render=True),
    "max60_render": dict(flt=(None, 60), render=True),
    "render": dict(render=True),
    "trim20-20_min30_sequence": dict(trim=(20, 20), flt=(30, None), column="sequence"),
    "trim20-20_min30_quality-33": dict(trim=(20, 20), flt=(30, None), column="quality", value_add=-33),
    "trim20-20_min30_header": dict(trim=(20, 20), flt=(30, None), column="header"),
    "trim20-20_min1_quality": dict(trim=(20, 20), flt=(1, None), column="quality"),
    # (beyond the list: no bound, so the bad tile's rows of length 0 reach the gather between reads of every length)
    "trim20-20_all_quality-33": dict(trim=(20, 20), flt=(None, None), column="quality", value_add=-33),
}
SOURCES = ("file", "gz", "push")
# every editing pass switched on, down either way behind them: the table as edited, and the kept rows of the select
ADAPTER_CONFIGS = {
    "trim20-20_adapter_render": dict(trim=(20, 20), adapter=True, render=True),
    "trim20-20_adapter_min30_quality-33": dict(trim=(20, 20), adapter=True, flt=(30, None), column="quality", value_add=-33),
}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """every corpus in a plain file and as a .gz: {kind: (path, gz path)}"""
    d = tmp_path_factory.mktemp("pipeline")
    out = {}
    for kind in COUNTS:
        p, z = d / (kind + ".fq"), d / (kind + ".fq.gz")
        p.write_bytes(corpus(kind))
        with gzip.open(str(z), "wb", compresslevel=1) as fh:
            fh.write(corpus(kind))
        out[kind] = (str(p), str(z))
    return out


@contextlib.contextmanager
def opened(hip, ctx, source, fbufsize, path=None, gz=None, data=None, start=None):
    fd = None
    try:
        if source == "push":
            st = hip.PushStream(ctx, io.BytesIO(data), fbufsize)
        else:
            fd = os.open(path if source == "file" else gz, os.O_RDONLY)
            st = hip.FileStream(ctx, fd, fbufsize, start=start, gzip=source == "gz")
        try:
            yield st
        finally:
            st.close()
    finally:
        if fd is not None:
            os.close(fd)


def run_stream(st, cfg, exp, tag):
    """Sets `cfg` on the stream, iterates it and compares EVERY fill with the slice of the expectation it covers; then the
    totals.  Returns what was seen: fills, end state, err_offset, the text, the longest run of rows of length 0 handed to
    the render / gather within one fill."""
    trim, flt, column, render = cfg.get("trim"), cfg.get("flt"), cfg.get("column"), cfg.get("render", False)
    value_add, adapter = cfg.get("value_add", 0), cfg.get("adapter", False)
    if trim is not None:
        st.set_trim(trim[1], trim[0])
    if adapter:
        st.set_adapter(AD)
    if flt is not None:
        st.set_filter(flt[0], flt[1], column, value_add)
    if render:
        st.set_render()
    t, cum, keep_all = exp.kept(trim, *(flt or (None, None)), adapter=adapter)
    acum = exp.adapted(trim)[1] if adapter else None
    base = fills = run = 0
    sums = {k: np.zeros(3, dtype=np.int64) for k in ("trim", "adapter", "render")}
    parts, end, err = [], None, None
    for rows, _fill, _off, end, err in st:
        where = (tag, "fill", fills, "records from", base)
        fills += 1
        assert end in (exp.end, END_REFILL), where
        if flt is not None:
            idx, n_scanned, col, coloff = st.selected()
        else:
            n_scanned = rows.shape[0]
        lo, hi = base, base + n_scanned
        assert hi <= exp.n, where
        keep = keep_all[lo:hi]
        want = t[lo:hi][keep]
        assert rows.shape == want.shape, (where, rows.shape, want.shape)
        bad = np.nonzero((rows != want).any(axis=1))[0]
        assert bad.size == 0, (where, bad[:5], rows[bad[:5]], want[bad[:5]])
        run = max(run, longest_run_of_empty(want))
        if flt is not None:
            assert idx.tolist() == np.flatnonzero(keep).tolist(), where
            if column is not None and n_scanned > 0:
                wcol, woff = loop_gather(exp.data, want, column, value_add)
                assert coloff is not None and coloff.tolist() == woff, where
                assert col.shape == wcol.shape and (col == wcol).all(), (where, np.nonzero(col != wcol)[0][:5] if col.shape == wcol.shape else None)
            elif column is None:
                assert col is None and coloff is None, where
        if trim is not None:
            got = st.trimmed()
            assert list(got) == (cum[hi] - cum[lo]).tolist(), (where, got)
            sums["trim"] += got
        if adapter:
            got = st.adapter_trimmed()
            assert list(got) == (acum[hi] - acum[lo]).tolist(), (where, got)
            sums["adapter"] += got
        if render:
            text, stats = st.rendered()
            wtext, _woff, wstats = loop_render(exp.data, want)
            text = text.tobytes()
            if text != wtext:
                at = next((i for i in range(min(len(text), len(wtext))) if text[i] != wtext[i]), min(len(text), len(wtext)))
                raise AssertionError((where, len(text), len(wtext), at, text[max(at - 8, 0):at + 24], wtext[max(at - 8, 0):at + 24]))
            assert list(stats) == wstats == [len(wtext), want.shape[0], 0], (where, stats)
            sums["render"] += stats
            parts.append(text)
        base = hi
    assert fills > 0 and end == exp.end, (tag, end)
    assert base == exp.n, (tag, base, exp.n)
    if trim is not None:
        assert sums["trim"].tolist() == cum[exp.n].tolist(), tag
    if adapter:
        assert sums["adapter"].tolist() == acum[exp.n].tolist(), tag
    text = b"".join(parts)
    if render:
        wtext, _woff, wstats = loop_render(exp.data, t[keep_all])
        assert text == wtext and sums["render"].tolist() == wstats, tag
    return dict(fills=fills, end=end, err=err, text=text, run=run)


def sizes_of(kind, source):
    if kind == "small":
        return (700, 3000)
    return (1 << 16, 1 << 20) + ((4096,) if (kind, source) == ("long", "file") else ())


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("kind", ("small", "mixed", "long"))
def test_stream_fill_by_fill(gpu_ctx, oracle, files, kind, source, config):
    """rows, ordinals, column, counters and text of every fill == the loops over the oracle's rows of that fill; "small" at
    buffer sizes where nearly every fill carries a record over (mis takes every residue), "long" at one below its long
    reads too (every one of them makes the slot grow)"""
    from fastqandfurious_amd import hip
    cfg, exp = CONFIGS[config], expect(oracle, kind)
    path, gz = files[kind]
    for fbufsize in sizes_of(kind, source):
        tag = (kind, source, fbufsize, config)
        with opened(hip, gpu_ctx, source, fbufsize, path, gz, exp.data) as st:
            seen = run_stream(st, cfg, exp, tag)
        print("fills %-5s %-4s fbufsize %7d %-28s %5d" % (kind, source, fbufsize, config, seen["fills"]))
        # a fill takes in at most fbufsize new bytes: this many fills, and a carry between every two of them
        assert seen["fills"] >= -(-len(exp.data) // fbufsize), tag
        if kind == "mixed" and fbufsize == 1 << 20 and cfg.get("trim") in ((20, 20), (0, 20)) and (cfg.get("flt") or (None,))[0] is None:
            # the bad tile, trimmed to rows of length 0, lies inside ONE fill and is handed on unfiltered
            assert seen["run"] > 1024, (tag, seen["run"])
        if cfg.get("render") and (cfg.get("flt") or (None,))[0] is not None and cfg["flt"][0] >= 1 and source == "file":
            # and back: the text (no read of length 0 in it) scanned on the device gives the rendered entries
            t, _cum, keep = exp.kept(cfg.get("trim"), *cfg["flt"])
            want_rows = oracle.scan(seen["text"])[0]
            table, res = gpu_ctx.scan_host(seen["text"])
            assert res.end_state == END_OK and table.shape == want_rows.shape and (table == want_rows).all(), tag
            assert entries_of(seen["text"], table) == entries_of(exp.data, t[keep]), tag


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(ADAPTER_CONFIGS))
@pytest.mark.parametrize("source", ("file", "push"))
@pytest.mark.parametrize("kind,sizes", (("small", (700, 3000)), ("mixed", (1 << 16,))))
def test_stream_fill_by_fill_with_adapter(gpu_ctx, oracle, files, kind, sizes, source, config):
    """the same comparison with the adapter cut behind the quality trim: without a filter (the edited table is counted,
    rendered and copied back) and with one (the kept rows are); at 700 bytes nearly every fill carries and many hold no
    record or one"""
    from fastqandfurious_amd import hip
    cfg, exp = ADAPTER_CONFIGS[config], expect(oracle, kind)
    path, gz = files[kind]
    for fbufsize in sizes:
        tag = (kind, source, fbufsize, config)
        with opened(hip, gpu_ctx, source, fbufsize, path, gz, exp.data) as st:
            seen = run_stream(st, cfg, exp, tag)
        assert seen["fills"] >= -(-len(exp.data) // fbufsize), tag


@pytest.mark.gpu
def test_stream_from_a_file_offset(gpu_ctx, oracle, files):
    """FileStream(start=k), k the offset of record 100 of "small": rows, text and counters are those of the records from
    100 on, with offsets counted from k"""
    from fastqandfurious_amd import hip
    whole = expect(oracle, "small")
    k = int(whole.rows[100, 0])
    exp = Expect(oracle, whole.data[k:])
    assert k > 0 and exp.n == whole.n - 100 and (exp.rows == whole.rows[100:] - k).all()
    for config in ("trim20-20_min30_render", "trim20-20_min30_quality-33", "trim0-20_render"):
        for fbufsize in (700, 1 << 16):
            with opened(hip, gpu_ctx, "file", fbufsize, files["small"][0], start=k) as st:
                seen = run_stream(st, CONFIGS[config], exp, ("start", k, fbufsize, config))
            assert seen["fills"] >= -(-len(exp.data) // fbufsize)


# ---- malformed input behind a trim -----------------------------------------------------------------------------------------
def _cut_in_last_quality(exp):
    p4, p5 = exp.rows[-1, 4:6].tolist()
    assert p5 - p4 >= 2
    return exp.data[:p4 + (p5 - p4) // 2]


def _second_half(exp, ok):
    return next(r for r in exp.rows[exp.n // 2:].tolist() if ok(r))


def _cut_in_header(exp):
    r = _second_half(exp, lambda r: r[1] - r[0] >= 4)
    return exp.data[:r[0] + 3]


def _plus_line_with_text(exp):
    # (an unwrapped record with a bare '+' line, whose header is not as long as "xy")
    r = _second_half(exp, lambda r: exp.data[r[3]:r[3] + 3] == b"\n+\n" and b"\n" not in exp.data[r[2]:r[3]] and r[1] - r[0] - 1 != 2)
    return exp.data[:r[3] + 2] + b"xy" + exp.data[r[3] + 2:]


MALFORMED = {"cut-in-last-quality": (_cut_in_last_quality, END_ERR_FINAL_QUAL), "cut-in-header": (_cut_in_header, END_ERR_INCOMPLETE),
             "plus-line-with-text": (_plus_line_with_text, END_ERR_INVALID)}


def damaged(oracle, name):
    """(the damaged bytes of "small", their expectation: the records the oracle finds in front of the error)"""
    key = ("small", name)
    if key not in _EXPECT:
        _EXPECT[key] = Expect(oracle, MALFORMED[name][0](expect(oracle, "small")))
    return _EXPECT[key]


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_damaged_corpus_conditions(oracle, name):
    exp, whole = damaged(oracle, name), expect(oracle, "small")
    assert exp.end == MALFORMED[name][1]
    assert whole.n // 2 <= exp.n < whole.n and (exp.rows == whole.rows[:exp.n]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("config", ("trim20-20_min30_render", "trim20-20_min30_sequence"))
@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_stream_malformed_input_behind_a_trim(gpu_ctx, oracle, tmp_path, name, config):
    """end state and err_offset of the last fill are those of a stream with nothing set (the refill goes by the scan's end
    offset, not by the table), the oracle's end state; what is delivered is the loops' over the records in front"""
    from fastqandfurious_amd import hip
    exp = damaged(oracle, name)
    p = tmp_path / "bad.fq"
    p.write_bytes(exp.data)
    for source in ("file", "push"):
        for fbufsize in (3000, 1 << 20):
            with opened(hip, gpu_ctx, source, fbufsize, str(p), data=exp.data) as st:
                plain = run_stream(st, {}, exp, (name, source, fbufsize, "plain"))
            with opened(hip, gpu_ctx, source, fbufsize, str(p), data=exp.data) as st:
                seen = run_stream(st, CONFIGS[config], exp, (name, source, fbufsize, config))
            assert plain["end"] == exp.end == MALFORMED[name][1]
            assert (seen["end"], seen["err"], seen["fills"]) == (plain["end"], plain["err"], plain["fills"]), (name, source, fbufsize)


def _until_error(it):
    got = []
    with pytest.raises(ValueError) as e:
        for item in it:
            got.append(item)
    return str(e.value), got


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_python_layer_malformed_input_behind_a_trim(gpu_ctx, oracle, tmp_path, name):
    """filter_fastq and readfastq_iter with entryfunc_qualitytrim raise what the plain GPU iterator raises, behind the
    loops' output for the records in front of the error"""
    from fastqandfurious_amd import fastqandfurious as F, _fastqandfurious as C
    exp = damaged(oracle, name)
    want, _counters = exp.output((20, 20), 30, None)
    p = tmp_path / "bad.fq"
    p.write_bytes(exp.data)
    for fbufsize in (3000, 1 << 20):
        message, got = _until_error(F.readfastq_iter(io.BytesIO(exp.data), fbufsize, F.entryfunc, C.entrypos))
        assert got == entries_of(exp.data, exp.rows)
        for source in ("file", "bytesio"):
            out = io.BytesIO()
            with (open(str(p), "rb") if source == "file" else io.BytesIO(exp.data)) as fh, pytest.raises(ValueError) as e:
                F.filter_fastq(fh, out, fbufsize, quality_cutoff=(20, 20), min_len=30)
            assert str(e.value) == message, (source, fbufsize)
            assert out.getvalue() == want, (source, fbufsize)
            for column in ("entry", "sequence"):
                with (open(str(p), "rb") if source == "file" else io.BytesIO(exp.data)) as fh:
                    text, items = _until_error(F.readfastq_iter(fh, fbufsize, F.entryfunc_qualitytrim(20, 20, min_len=30, column=column), C.entrypos))
                assert text == message, (source, fbufsize, column)
                assert items == exp.items((20, 20), 30, None, column), (source, fbufsize, column)


# ---- the Python layer on the same corpora ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("params", sorted(PARAMS))
@pytest.mark.parametrize("source", ("file", "bytesio", "gz"))
@pytest.mark.parametrize("kind", ("mixed", "long"))
def test_filter_fastq_gpu_scanner(gpu_ctx, oracle, files, kind, source, params):
    """output bytes and FilterResult == the loops' == the package's own per-record path over the Python scanner"""
    from fastqandfurious_amd import fastqandfurious as F
    exp = expect(oracle, kind)
    want, counters = exp.output(*PARAMS[params][1])
    assert host_filter(F, kind, params) == (want, counters)
    for fbufsize in (1 << 16, 1 << 20):
        out = io.BytesIO()
        with (open(files[kind][0], "rb") if source == "file" else io.BytesIO(exp.data) if source == "bytesio"
              else F.automagic_open(files[kind][1])) as fh:
            res = F.filter_fastq(fh, out, fbufsize, **PARAMS[params][0])
        assert out.getvalue() == want, (fbufsize,)
        assert tuple(res) == counters, (fbufsize,)


@pytest.mark.gpu
@pytest.mark.parametrize("column", ("entry", "sequence", "quality"))
@pytest.mark.parametrize("kind,fbufsize", (("small", 3000), ("mixed", 1 << 16)))
def test_readfastq_iter_qualitytrim(gpu_ctx, oracle, files, kind, fbufsize, column):
    """entryfunc_qualitytrim(20, 20, min_len=30, column=c) on the GPU scanner: one item per record, None for a dropped one,
    those of test_trim.expected_items (the Python scanner and the loop) and of the oracle's rows"""
    from fastqandfurious_amd import fastqandfurious as F, _fastqandfurious as C
    exp = expect(oracle, kind)
    if ("items", kind) not in _HOST:
        _HOST["items", kind] = expected_items(F, exp.data, 20, 20, min_len=30, fbufsize=1 << 20)
    j = {"entry": None, "sequence": 1, "quality": 2}[column]
    want = [e if (e is None or j is None) else e[j] for e in _HOST["items", kind]]
    assert want == exp.items((20, 20), 30, None, column) and any(e is None for e in want) and any(e is not None for e in want)
    ef = F.entryfunc_qualitytrim(20, 20, min_len=30, column=column)
    with open(files[kind][0], "rb") as fh:
        got = list(F.readfastq_iter(fh, fbufsize, ef, C.entrypos))
    assert len(got) == len(want) and got == want
    got = list(F.readfastq_iter(io.BytesIO(exp.data), fbufsize, ef, C.entrypos))
    assert got == want
    with F.automagic_open(files[kind][1]) as fh:
        got = list(F.readfastq_iter(fh, fbufsize, ef, C.entrypos))
    assert got == want

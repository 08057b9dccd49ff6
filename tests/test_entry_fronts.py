"""The three batched fronts of readfastq_iter -- the stream front end (_iter_stream), the byte-range iterator
(RangeEntries) and the per-fill buffer loop (_iter_batched) -- build the entries of the reference's own per-record loop
(fastqandfurious.py:241-279) for every kind of entryfunc, whatever the size of a fill or a batch,
with and without the compiled entries module.  CPU only: the device is replaced by host stand-ins over the oracle.

entryfunc_phred is driven only where a front decodes in bulk (a stream opened with the decode, the range iterator):
called per record it goes through the GPU's arrayadd_b."""
import copy
import io
import os
import types
from array import array

import numpy as np
import pytest

COLS = {"header": (0, 1, 1), "sequence": (2, 0, 3), "quality": (4, 0, 5)}
FILLS = (5000, 70000, 1 << 22)
BATCHES = (7, 64, 1 << 15)


class FakeStream:
    """Host stand-in for hip._Stream: b"\\n" + data cut into fills, each scanned by the oracle."""

    def __init__(self, oracle, data, fill_bytes, decode=False):
        self.o, self.data, self.fb, self.decode = oracle, data, fill_bytes, decode
        self.filtered, self.closed, self.flt = False, 0, None

    def set_filter(self, lo, hi, column):
        self.flt, self.filtered = (lo, hi, column), True

    def __iter__(self):
        data = b"\n" + self.data
        start, end = 0, min(len(data), self.fb)
        while True:
            buf = data[start:end]
            table, endst, _st, off = self.o.scan(buf, sentinel=False, offset=0, eof=end >= len(data), add=0)
            table = np.ascontiguousarray(np.asarray(table).reshape(-1, 6))
            self._buf, self._tab = np.frombuffer(buf, np.uint8), table
            rows = table + (start - 1)
            if self.flt:
                lo, hi, _col = self.flt
                ln = table[:, 3] - table[:, 2]
                keep = np.ones(len(table), bool)
                if lo is not None:
                    keep &= ln >= lo
                if hi is not None:
                    keep &= ln <= hi
                self._idx, self._n = np.nonzero(keep)[0].astype(np.int64), len(table)
                rows, self._kept = np.ascontiguousarray(rows[keep]), table[keep]
            yield rows, self._buf, start - 1, int(endst), start - 1 + int(off)
            if int(endst) != 1:
                return
            start += int(off)
            end = min(len(data), end + self.fb)

    def quals(self):
        q, qo = self.o.decode_quals(self._buf, self._tab)
        return np.asarray(q), np.asarray(qo)

    def selected(self):
        col = off = None
        c = self.flt[2]
        if c is not None:
            ca, sh, cb = COLS[c]
            parts = [self._buf[r[ca] + sh:r[cb]] for r in self._kept]
            off = np.zeros(len(parts) + 1, np.int64)
            np.cumsum([len(p) for p in parts], out=off[1:])
            col = np.concatenate(parts).view(np.int8) if parts else np.zeros(0, np.int8)
        return self._idx, self._n, col, off

    def close(self):
        self.closed += 1


class FakeShard:
    """Host stand-in for sharded.FileShard: the rank's rows are the oracle's rows whose '@' lies in [lo, hi)."""

    def __init__(self, oracle, path, data, lo, hi, resident=True, decoded=False, slab=0):
        self.o, self.fd, self.data = oracle, os.open(path, os.O_RDONLY), np.frombuffer(data, np.uint8)
        table, *_ = oracle.scan(self.data)
        t = np.ascontiguousarray(np.asarray(table).reshape(-1, 6))
        own = (t[:, 0] >= lo) & (t[:, 0] < hi)
        self.t, self.bounds = np.ascontiguousarray(t[own]), [0, lo, hi, len(data)]
        self.out = types.SimpleNamespace(record_base=int(np.nonzero(own)[0][0]) if own.any() else 0, total_records=len(t),
                                         row_lo=0, row_hi=len(self.t), halo_source=1, rounds=0, regathers=0, allgather_ms=0.0)
        self.sh = types.SimpleNamespace(transport=lambda: "fake")
        self.resident, self.decoded, self.slab_bytes, self.closed = resident, decoded, slab, 0

    def rows(self, i0=None, i1=None):
        return np.ascontiguousarray(self.t[i0:i1])

    def quals(self, i0, i1, rows):
        q, qo = self.o.decode_quals(self.data, self.t[i0:i1])
        return np.asarray(q), np.asarray(qo)

    def quals_from_file(self, rows):
        q, qo = self.o.decode_quals(self.data, rows)
        return np.asarray(q), np.asarray(qo)

    def select(self, lo, hi):
        ln = self.t[:, 3] - self.t[:, 2]
        keep = np.ones(len(ln), bool)
        if lo is not None:
            keep &= ln >= lo
        if hi is not None:
            keep &= ln <= hi
        self.kept = np.ascontiguousarray(self.t[keep])
        idx = np.nonzero(keep)[0].astype(np.int64)
        return len(idx), idx

    def kept_rows(self, k0, k1):
        return np.ascontiguousarray(self.kept[k0:k1])

    def kept_column(self, k0, k1, column, rows):
        if not self.resident:
            return None                     # (as slabs do: the iterator cuts the column out of the file)
        ca, sh, cb = COLS[column]
        parts = [self.data[r[ca] + sh:r[cb]] for r in rows]
        off = np.zeros(len(parts) + 1, np.int64)
        np.cumsum([len(p) for p in parts], out=off[1:])
        return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), off

    def close(self):
        if self.fd is not None:
            os.close(self.fd)
            self.fd = None
        self.closed += 1


def _scanner(oracle):
    class Scanner:
        def __call__(self, *a):
            raise AssertionError("per-record protocol not expected")

        def scan_buffer(self, buf, offset, eof):
            table, end, _st, off = oracle.scan(buf, sentinel=False, offset=offset, eof=eof, add=0)
            rows = array("q")
            rows.frombytes(np.ascontiguousarray(table).tobytes())
            return rows, int(end), int(off)
    return Scanner()


def plain(buf, pos, globaloffset):
    return (type(buf) is bytes, type(pos) is array and len(pos) == 6, buf[pos[0]:pos[5]], pos[0] + globaloffset)


def _entryfuncs(F):
    class EvenOnly(F.entryfunc_lengthfilter):           # (keeps() of its own: not pushed down, called per record)
        def keeps(self, length):
            return length % 2 == 0

    efs = [F.entryfunc, F.entryfunc_namedtuple, F.entryfunc_abspos, plain]
    efs += [F.entryfunc_lengthfilter(120, column=c, yield_dropped=y)
            for c in ("sequence", "header", "quality", "entry") for y in (True, False)]
    efs += [EvenOnly(120, yield_dropped=True), EvenOnly(120, column="entry", yield_dropped=False)]
    assert not F._pushes_down(efs[-1]) and F._pushes_down(efs[-3])
    return efs


def _listed(F, ef, it):
    return [list(x) if ef is F.entryfunc_abspos else x for x in it]


def reference(F, data, ef, first=0, count=None):
    """What the reference's per-record loop over the pure-Python scanner yields, records [first, first + count)."""
    every = ef
    if isinstance(ef, F.entryfunc_lengthfilter) and not ef.yield_dropped:
        every = copy.copy(ef)
        every.yield_dropped = True
    out = _listed(F, ef, F.readfastq_iter(io.BytesIO(data), 3000, every, F.entrypos))
    out = out[first:] if count is None else out[first:first + count]
    return [x for x in out if x is not None] if every is not ef else out


def phred_reference(F, data, first=0, count=None):
    return [(h, s, array("b", [x - 33 for x in q])) for h, s, q in reference(F, data, F.entryfunc, first, count)]


@pytest.fixture(scope="module")
def F(pkg):
    from fastqandfurious_amd import build, entries, fastqandfurious
    build.build_entries()
    assert entries.native() is not None, "csrc/_ffq_entries.so did not build / load"
    return fastqandfurious


@pytest.fixture(params=("single", "wrapped"))
def data(request, pkg):
    from fastqandfurious_amd import synth
    return (synth.single(0, 900, seed=42) if request.param == "single" else synth.wrapped(0, 400, seed=43)[0]).tobytes()


@pytest.fixture(params=("native", "python"))
def native(request, F, monkeypatch):
    from fastqandfurious_amd import entries
    if request.param == "python":
        monkeypatch.setattr(entries, "_native", None)
    assert (entries.native() is not None) == (request.param == "native")
    return request.param == "native"


def _set_filter(F, st, ef):
    if F._pushes_down(ef):              # (as readfastq_iter does)
        st.set_filter(ef.min_len, ef.max_len, None if ef.column == "entry" else ef.column)


def _shard(oracle, tmp_path, data, **kw):
    p = tmp_path / "range.fq"
    if not p.exists():
        p.write_bytes(data)
    return FakeShard(oracle, str(p), data, len(data) // 3, 2 * len(data) // 3, **kw)


def test_stream_front(F, oracle, data, native):
    n = len(reference(F, data, F.entryfunc))
    assert n in (900, 400)
    for fb in FILLS:
        for ef in _entryfuncs(F):
            st = FakeStream(oracle, data, fb)
            _set_filter(F, st, ef)
            got = _listed(F, ef, F._iter_stream(st, ef))
            assert got == reference(F, data, ef) and st.closed == 1, (fb, ef)
        st = FakeStream(oracle, data, fb, decode=True)
        got = list(F._iter_stream(st, F.entryfunc_phred))
        assert got == phred_reference(F, data) and st.closed == 1, fb
        assert all(type(e[2]) is array and e[2].typecode == "b" for e in got)


def test_stream_front_with_fills_that_hold_no_record(F, oracle, data, native):
    """A fill smaller than a record comes with an empty table (and grows with the next read)."""
    for ef in (F.entryfunc, F.entryfunc_abspos, F.entryfunc_lengthfilter(120), F.entryfunc_lengthfilter(120, column="entry", yield_dropped=False)):
        st = FakeStream(oracle, data, 150)
        _set_filter(F, st, ef)
        assert _listed(F, ef, F._iter_stream(st, ef)) == reference(F, data, ef) and st.closed == 1, ef
    st = FakeStream(oracle, data, 150, decode=True)
    assert list(F._iter_stream(st, F.entryfunc_phred)) == phred_reference(F, data) and st.closed == 1


def test_range_front(F, oracle, data, native, tmp_path):
    for batch in BATCHES:
        for resident in (True, False):
            for ef in _entryfuncs(F):
                sh = _shard(oracle, tmp_path, data, resident=resident)
                b, n = sh.out.record_base, len(sh.t)
                assert n > 100 and b > 0
                r = F.RangeEntries(sh, ef, batch)
                assert (r.record_base, r.n_records, r.total_records) == (b, n, sh.out.total_records)
                got = _listed(F, ef, r)
                assert got == reference(F, data, ef, b, n) and sh.closed >= 1, (batch, resident, ef)


@pytest.mark.parametrize("decoded, slab", ((True, 0), (False, 1 << 20)))
def test_range_front_phred(F, oracle, data, tmp_path, decoded, slab):
    """entryfunc_phred from the step's own decode, or (slabs) decoded batch by batch: the native entries_phred."""
    for batch in BATCHES:
        sh = _shard(oracle, tmp_path, data, decoded=decoded, slab=slab)
        got = list(F.RangeEntries(sh, F.entryfunc_phred, batch))
        assert got == phred_reference(F, data, sh.out.record_base, len(sh.t)) and sh.closed >= 1, batch
        assert all(type(e[2]) is array and e[2].typecode == "b" for e in got)


@pytest.mark.parametrize("decoded, slab", ((True, 0), (False, 1 << 20)))
def test_range_front_phred_without_the_native_module(F, oracle, data, tmp_path, monkeypatch, decoded, slab):
    """... and the same entries from the Python fall-back when csrc/ffq_entries.c is not built: the bulk decode is
    still the one the shard hands over, no call per record."""
    from fastqandfurious_amd import entries
    monkeypatch.setattr(entries, "_native", None)
    for batch in BATCHES:
        sh = _shard(oracle, tmp_path, data, decoded=decoded, slab=slab)
        got = list(F.RangeEntries(sh, F.entryfunc_phred, batch))
        assert got == phred_reference(F, data, sh.out.record_base, len(sh.t)) and sh.closed >= 1, batch
        assert all(type(e[2]) is array and e[2].typecode == "b" for e in got)


def test_batched_front(F, oracle, data, native):
    for fb in FILLS:
        for ef in _entryfuncs(F):
            got = _listed(F, ef, F.readfastq_iter(io.BytesIO(data), fb, ef, _scanner(oracle)))
            assert got == reference(F, data, ef), (fb, ef)


class Boom(Exception):
    pass


def _fronts(F, oracle, tmp_path, data, ef):
    """(name, iterator, object whose close() is counted or None) of every front over `data`."""
    st = FakeStream(oracle, data, 70000)
    yield "stream", F._iter_stream(st, ef), st
    sh = _shard(oracle, tmp_path, data)
    yield "range", F.RangeEntries(sh, ef, 64), sh
    yield "batched", F.readfastq_iter(io.BytesIO(data), 70000, ef, _scanner(oracle)), None


def test_per_record_entryfuncs_are_called_lazily(F, oracle, data, native, tmp_path):
    """entryfunc is not called for record k + 1 before record k has been handed out: one that raises at record 10 lets
    exactly 10 items through, and what the iterator holds is closed all the same."""
    for front in ("stream", "range", "batched"):
        calls = [0]

        def ef(buf, pos, globaloffset):
            if calls[0] == 10:
                raise Boom()
            calls[0] += 1
            return calls[0]

        name, it, closer = [f for f in _fronts(F, oracle, tmp_path, data, ef) if f[0] == front][0]
        got = []
        with pytest.raises(Boom):
            for e in it:
                assert calls[0] == e == len(got) + 1, (name, calls, e)       # (called for this record and no further)
                got.append(e)
        assert got == list(range(1, 11)), name
        if name == "stream":
            assert closer.closed == 1
        elif name == "range":
            assert closer.closed >= 1


def test_fronts_close_what_they_hold_when_the_consumer_stops_early(F, oracle, data, native, tmp_path):
    for ef in (F.entryfunc, F.entryfunc_abspos, F.entryfunc_lengthfilter(120)):
        for name, it, closer in _fronts(F, oracle, tmp_path, data, ef):
            if name == "stream":
                _set_filter(F, closer, ef)
            next(it)
            it.close()
            if name == "stream":
                assert closer.closed == 1, (name, ef)
            elif name == "range":
                assert closer.closed >= 1 and closer.fd is None, (name, ef)

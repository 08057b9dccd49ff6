"""Scans of a context that REMEMBERS another kind of input (InputMemory, csrc/ffq_scanwalk.h:59-72).

Which tier a scan starts on is decided by what the context met before: the fast path is skipped while fast4_remember
holds, a PROBE scan queues its row kernels in front of the general ones when fast4_skip has run out, ranked_skip /
dense_skip / lite_skip send the next HOLD_OFF scans to the tier the last verdict chose, dense4_remember picks the row
kernel's dense instantiation, fused_skip / fz_in_place steer the single pass.  The consumers that matter (readfastq_iter,
FileStream, build_index, the shard step) run ONE context over every fill of a file; tests/conftest.py forgets before
every test and most tests forget before every scan.  Here the state is set on purpose -- forget(), then a known sequence
of scans -- and every scan of the sequence is compared with the oracle: rows, n_records, end_state, last_status,
end_offset, the quality offsets and every decoded byte (oracle.scan / oracle.decode_quals, never a second GPU run).

The comparer below asserts what check_same / decode_same (tests/test_gpu_parity.py) and wide_same (tests/test_wide.py)
assert together, on arrays and from oracle results computed once per (input, keyword set): the sequences here are
thousands of scans long, and the suite's own comparers run the oracle (and build Python lists of the rows) per call.
"""
import io
import os

import numpy as np
import pytest

from test_gpu_parity import _mess, random_records

pytestmark = pytest.mark.gpu

HOLD_OFF = 15                    # csrc/ffq_scanwalk.h:56 -- how many scans a verdict about the input holds
COUNTDOWN = HOLD_OFF + 3         # crosses every hold-off and includes the probe scan, however its off-by-one reads
TILE = 16384

KINDS = ("four", "tiny", "wrap", "wrap80", "wrap45", "long", "longline", "mess", "messfatal")
MODES = (1, 2, 3, 4)
ADD = 7 * (1 << 32) + 12345

# records per kind (`long`: bytes)
COUNTS = {"four": 8000, "tiny": 30000, "wrap": 20000, "wrap80": 20000, "wrap45": 6000, "long": 8 << 20, "mess": 4000}

ROUTES = {}                      # (A, B, mode) -> [res.path of every scan of B], filled by the matrix


def _long_lines():
    """the 12 unwrapped records of test_long_records (tests/test_gpu_parity.py)"""
    rng = np.random.default_rng(5)
    parts = []
    for i in range(12):
        L = int(rng.integers(20000, 200000))
        seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=L).tobytes()
        qual = rng.choice(np.frombuffer(bytes(range(33, 74)), dtype=np.uint8), size=L).tobytes()
        parts.append(b"@long%d\n" % i + seq + b"\n+\n" + qual + b"\n")
    return b"".join(parts)


def _build_kinds():
    """Every kind of input once, from fixed seeds; the shapes are those of tests that assert the route on a fresh context."""
    from fastqandfurious_amd import synth
    rng, N = np.random.default_rng, COUNTS
    kinds = {
        "four": random_records(rng(100), N["four"], 100, 160),
        "tiny": b"".join(b"@r%d\nACGT\n+\nIIII\n" % i for i in range(N["tiny"])),
        "wrap": synth.wrapped(0, N["wrap"], seed=43)[0],
        "wrap80": random_records(rng(77), N["wrap80"], 100, 100, wrap=80, hdr_hi=12),
        "wrap45": random_records(rng(45), N["wrap45"], 50, 300, wrap=45, hdr_hi=40),
        "long": random_records(rng(20000), N["long"] // 40000, 10000, 20000, wrap=80, hdr_hi=10),
        "longline": _long_lines(),
        "mess": _mess(rng(1), N["mess"], fatal=False),
        "messfatal": _mess(rng(2), N["mess"], fatal=True),
    }
    return {k: np.frombuffer(v, dtype=np.uint8) if not isinstance(v, np.ndarray) else v for k, v in kinds.items()}


def variants(n):
    """(bytes cut off the end, keywords): the keyword sets of test_fast_path_edits, `add`, and the two cuts"""
    return ((0, {}), (0, dict(eof=False)), (0, dict(offset=n // 3)), (0, dict(sentinel=False, offset=5)), (0, dict(add=ADD)),
            (1, {}), (n - n * 2 // 3, {}))


class Expected:
    """What the oracle says about one (input, keyword set)."""

    def __init__(self, oracle, data, kw):
        self.rows, self.end_state, self.last_status, self.end_offset = oracle.scan(data, **kw)
        sentinel = kw.get("sentinel", True)
        add = kw.get("add", -1 if sentinel else 0)
        self.in_buf = self.rows - add - (1 if sentinel else 0)              # the rows as offsets into `data`
        self.qual, self.qoff = oracle.decode_quals(data, self.in_buf)
        self.lens = self.in_buf[:, 5] - self.in_buf[:, 4]
        self._not_quality = self._arange = None

    @property
    def not_quality(self):
        """True at every byte of the buffer that no record's quality covers (in-place layout: only the others count)"""
        if self._not_quality is None:
            end = int(self.in_buf[-1, 5]) if len(self.in_buf) else 0
            m = np.zeros(end + 1, dtype=np.int8)
            m[self.in_buf[:, 4]] += 1
            m[self.in_buf[:, 5]] -= 1
            self._not_quality = np.cumsum(m, dtype=np.int8)[:end] == 0
        return self._not_quality

    @property
    def arange(self):
        if self._arange is None:
            self._arange = np.arange(self.qual.size)
        return self._arange


class World:
    """The inputs, their decoded images and the oracle's results, built once for the module."""

    def __init__(self, oracle, hip):
        self.oracle, self.hip = oracle, hip
        self.data = _build_kinds()
        self.decoded = {k: (v.view(np.int8) - 33).astype(np.int8) for k, v in self.data.items()}    # arrayadd_b(-33) of every byte
        self._exp = {}

    def mode(self, mode):
        """(flags, qual_room): 1 rows only, 2 packed decode, 3 single pass with room for the in-place layout, 4 with segments only"""
        h = self.hip
        return {1: (0, None), 2: (h.F_DECODE_QUAL, None), 3: (h.F_DECODE_QUAL | h.F_SINGLE_PASS, h.INPLACE_STRIDE),
                4: (h.F_DECODE_QUAL | h.F_SINGLE_PASS, None)}[mode]

    def view(self, kind, cut=0):
        d = self.data[kind]
        return d[:d.size - cut]

    def expected(self, kind, cut=0, kw=None):
        kw = kw or {}
        key = (kind, cut, tuple(sorted(kw.items())))
        if key not in self._exp:
            self._exp[key] = Expected(self.oracle, self.view(kind, cut), kw)
        return self._exp[key]

    def same(self, ctx, kind, mode, cut=0, kw=None):
        """One scan_host of `kind` on `ctx` as it is, against the oracle; returns the ScanResult."""
        kw = kw or {}
        hip = self.hip
        data, w = self.view(kind, cut), self.expected(kind, cut, kw)
        flags, room = self.mode(mode)
        n = len(w.rows)
        out = ctx.scan_host(data, flags=flags, qual_room=room, table_cap=n + 8, **kw)       # (one call, one scan: no retry for a larger table)
        table, res = out[0], out[1]
        assert int(res.n_records) == n, "n_records %d, the oracle has %d" % (res.n_records, n)
        assert table.shape == w.rows.shape and (table == w.rows).all(), "rows differ"
        assert int(res.end_state) == w.end_state, "end_state %d, the oracle has %d" % (res.end_state, w.end_state)
        assert int(res.last_status) == w.last_status, "last_status %d, the oracle has %d" % (res.last_status, w.last_status)
        assert int(res.end_offset) == w.end_offset, "end_offset %d, the oracle has %d" % (res.end_offset, w.end_offset)
        if not flags & hip.F_DECODE_QUAL:
            assert res.path not in (6,) and not res.path & hip.PATH_IN_PLACE, res.path
            return res
        qual, qoff = out[2], out[3]
        assert qoff.shape[0] == n + 1
        if n:
            assert int(qoff[n]) == int(qoff[n - 1] + w.lens[n - 1]) == int(res.n_qual_bytes)
        ntiles = (data.size + TILE - 1) // TILE
        qual_cap = max(data.size, ntiles * (room or hip.SEG_STRIDE)) if flags & hip.F_SINGLE_PASS else data.size    # (scan_host's)
        if res.path & hip.PATH_IN_PLACE:
            assert flags & hip.F_SINGLE_PASS and qual_cap >= ntiles * TILE, "in place without the room for it"
            assert (qoff[:n] == w.in_buf[:, 4]).all(), "in place: qoff[i] must be pos4's offset in the buffer"
            if n:
                k = int(w.in_buf[n - 1, 5])
                assert int(res.n_qual_bytes) == k == qual.shape[0]
                assert ((qual == self.decoded[kind][:k]) | w.not_quality).all(), "decoded bytes differ (in place)"
        elif res.path == 6:
            assert flags & hip.F_SINGLE_PASS, "segments without FFQ_F_SINGLE_PASS"
            if n:
                assert (qoff[1:n] >= qoff[:n - 1] + w.lens[:n - 1]).all(), "records overlap or are out of order"
                assert int(qoff[0]) >= 0 and int(qoff[n]) <= qual_cap
                idx = np.repeat(qoff[:n] - w.qoff[:n], w.lens) + w.arange
                assert (qual[idx] == w.qual).all(), "decoded bytes differ (segments)"
        else:
            assert (qoff == w.qoff).all(), "packed: the offsets differ"
            assert int(res.n_qual_bytes) == w.qual.size and (qual == w.qual).all(), "decoded bytes differ (packed)"
        return res


@pytest.fixture(scope="module")
def world(oracle, pkg):
    from fastqandfurious_amd import hip
    return World(oracle, hip)


def fresh_route(kind, mode):
    """res.path (without FFQ_PATH_IN_PLACE) of the first two scans of `kind` on a context that has forgotten, where a test
    of the suite asserts it; None: not asserted."""
    single_pass = mode in (3, 4)
    return {"four": (6,) if single_pass else (3,),          # test_fused_shapes / test_decode_record_shapes
            # the row kernel's DENSE instantiation (test_very_short_reads_every_tile_dense); behind a single pass that was
            # refused the driver does not try it today: the general kernels, and the context remembers THAT
            "tiny": (0, 3) if single_pass else (3,),
            "wrap": (0,),                                   # test_synth_wrapped; test_a_context_that_has_met_wrapped_records_takes_the_one_pass
            "wrap80": (2,),                                 # the dense configuration of the group kernels
            "wrap45": (0, 2, 5),
            "long": (5,),                                   # test_long_wrapped_records_take_the_ranked_tier
            "longline": (6,) if mode == 3 else (3,),        # test_fused_shapes: 3 with segments only; with the room: in place
            }.get(kind)


def warm_up(world, ctx, kind, mode):
    """forget(), then `kind` twice, compared; the routes prove that the state was set"""
    ctx.forget()
    for scan in range(2):
        res = world.same(ctx, kind, mode)
        want = fresh_route(kind, mode)
        if want is not None:
            assert res.path & ~world.hip.PATH_IN_PLACE in want, "%s, mode %d, scan %d: path %d" % (kind, mode, scan, res.path)
        if kind == "tiny" and scan == 0 and mode in (1, 2):
            assert res.retries >= 1                          # (the plain row kernel met a dense tile: dense4_remember)
        if kind == "wrap" and scan == 1 and mode == 3:
            assert res.path & world.hip.PATH_IN_PLACE       # started on the general kernels: fast4_remember
        if kind == "long" and scan == 1 and mode == 3:
            assert res.path & world.hip.PATH_IN_PLACE       # started on the ranked tier: ranked_skip


# ---- 1. the matrix ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("A", KINDS)
def test_scan_after_other_input(gpu_ctx, world, A, mode):
    """Every kind B, HOLD_OFF + 3 times in a row, on a context whose last two scans were A."""
    for B in KINDS:
        warm_up(world, gpu_ctx, A, mode)
        paths = ROUTES.setdefault((A, B, mode), [])
        del paths[:]
        for k in range(COUNTDOWN):
            try:
                paths.append(int(world.same(gpu_ctx, B, mode).path))
            except AssertionError as e:
                raise AssertionError("after %s twice, mode %d: scan %d of %s (paths so far %r): %s" % (A, mode, k, B, paths, e)) from None


def _runs(paths):
    out, i = [], 0
    while i < len(paths):
        j = i
        while j < len(paths) and paths[j] == paths[i]:
            j += 1
        out.append("%d" % paths[i] if j - i == 1 else "%dx%d" % (paths[i], j - i))
        i = j
    return " ".join(out)


def test_matrix_reached_the_routes(world, capsys):
    """The matrix is only worth its time if history did steer it: the union of its routes, and the return of a context
    that met wrapped records to the fast path."""
    assert len(ROUTES) == len(KINDS) ** 2 * len(MODES), "the whole module has to run: the matrix fills the table"
    with capsys.disabled():
        print("\nres.path of every scan of B after A twice (path x count):")
        for mode in MODES:
            for A in KINDS:
                print("  mode %d  %-9s | " % (mode, A) + " | ".join("%s: %s" % (B, _runs(ROUTES[A, B, mode])) for B in KINDS))
    in_place = world.hip.PATH_IN_PLACE
    plain = {p for (A, B, mode), v in ROUTES.items() if mode in (1, 2) for p in v}
    one_pass = {p for (A, B, mode), v in ROUTES.items() if mode in (3, 4) for p in v}
    assert {0, 2, 3, 5} <= plain, sorted(plain)
    assert 6 in one_pass and any(p & in_place for p in one_pass), sorted(one_pass)
    back = [v for (A, B, mode), v in ROUTES.items() if (A, B) == ("wrap", "four")]
    assert any(v[0] & ~in_place in (0, 2) and v[-1] in (3, 6) for v in back), back


# ---- 2. keyword variants on a warm context ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (1, 3))
@pytest.mark.parametrize("A", ("wrap", "long", "wrap80"))
def test_probe_scan_with_offsets_and_cuts(gpu_ctx, world, A, mode):
    """The countdown and the probe scan with eof=False, a search offset, no sentinel, `add` and truncated input: the 7
    keyword sets cycled over the 18 scans.  The probe scan falls on the same scan of every countdown that follows the same
    A, so the cycle is started at each of its 7 entries in turn: every set meets the probe scan."""
    for B in ("four", "wrap", "mess"):
        var = variants(world.data[B].size)
        for shift in range(len(var)):
            warm_up(world, gpu_ctx, A, mode)
            for k in range(COUNTDOWN):
                cut, kw = var[(k + shift) % len(var)]
                try:
                    world.same(gpu_ctx, B, mode, cut, kw)
                except AssertionError as e:
                    raise AssertionError("after %s twice, mode %d: scan %d of %s (cycle from %d), cut %d, %r: %s"
                                         % (A, mode, k, B, shift, cut, kw, e)) from None


# ---- 3. seeded walk -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_random_walk_of_inputs(gpu_ctx, world, seed):
    """One context, 150 scans: kind, mode and keyword set drawn anew for each.  A failure names the seed and the steps so
    far: replay them as a fixed sequence."""
    rng = np.random.default_rng(4200 + seed)
    gpu_ctx.forget()
    steps = []
    for _ in range(150):
        kind = KINDS[int(rng.integers(len(KINDS)))]
        mode = MODES[int(rng.integers(len(MODES)))]
        v = int(rng.integers(7))
        cut, kw = variants(world.data[kind].size)[v]
        steps.append((kind, mode, v))
        try:
            world.same(gpu_ctx, kind, mode, cut, kw)
        except AssertionError as e:
            raise AssertionError("seed %d, steps (kind, mode, variant) %r: %s" % (seed, steps, e)) from None


# ---- 4. exactly sized outputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (1, 2, 3))
@pytest.mark.parametrize("A,B", (("wrap", "four"), ("wrap", "wrap"), ("wrap", "mess"), ("long", "four")))
def test_warm_fronts_stay_inside_the_callers_buffers(gpu_ctx, world, A, B, mode):
    """A table of exactly n_records rows, a quality buffer of exactly the mode's room and n_records + 1 offsets, each with
    guards behind it, through the countdown: the probe front has two writers of the table (the fast path's row kernel,
    then the general kernels), the refused ranked start hands its index to the fast path.  Then one row short:
    E_TABLE_FULL, the rows that fit, nothing behind them."""
    import torch
    hip = world.hip
    data, w = world.data[B], world.expected(B)
    flags, room = world.mode(mode)
    decode = bool(flags & hip.F_DECODE_QUAL)
    n = len(w.rows)
    ntiles = (data.size + TILE - 1) // TILE
    qual_cap = (ntiles * room if room else w.qual.size) if decode else 0
    dbuf = torch.from_numpy(data.copy()).cuda()
    table = torch.empty((n + 64, 6), dtype=torch.int64, device="cuda")
    qual = torch.empty(qual_cap + 256, dtype=torch.int8, device="cuda")
    qoff = torch.empty(n + 1 + 8, dtype=torch.int64, device="cuda")

    def scan(cap):
        table.fill_(-7)
        qual.fill_(99)
        qoff.fill_(-7)
        torch.cuda.synchronize()                      # (torch's stream is not the context's)
        rc, res = gpu_ctx.scan_device(dbuf.data_ptr(), data.size, table.data_ptr(), cap, flags=flags,
                                      d_qual=qual.data_ptr() if decode else None, qual_cap=qual_cap,
                                      d_qoff=qoff.data_ptr() if decode else None)
        return rc, res, table.cpu().numpy(), qual.cpu().numpy(), qoff.cpu().numpy()

    warm_up(world, gpu_ctx, A, mode)
    for k in range(COUNTDOWN):
        rc, res, t, q, qo = scan(n)
        where = "after %s twice, mode %d: scan %d of %s, path %d" % (A, mode, k, B, res.path)
        assert rc == hip.OK and int(res.n_records) == n, where
        assert (int(res.end_state), int(res.last_status), int(res.end_offset)) == (w.end_state, w.last_status, w.end_offset), where
        assert (t[:n] == w.rows).all(), where
        assert (t[n:] == -7).all(), "rows written behind the table, " + where
        if not decode:
            continue
        assert (q[qual_cap:] == 99).all(), "bytes written behind the quality buffer, " + where
        assert (qo[n + 1:] == -7).all(), "offsets written behind qoff, " + where
        if res.path & hip.PATH_IN_PLACE:
            assert mode == 3, where
            assert (qo[:n] == w.in_buf[:, 4]).all(), where
            end = int(w.in_buf[n - 1, 5])
            assert int(qo[n]) == int(res.n_qual_bytes) == end, where
            assert ((q[:end] == world.decoded[B][:end]) | w.not_quality).all(), where
        elif res.path == 6:
            assert mode == 3, where
            assert (qo[1:n] >= qo[:n - 1] + w.lens[:n - 1]).all() and int(qo[0]) >= 0 and int(qo[n]) <= qual_cap, where
            assert int(qo[n]) == int(qo[n - 1] + w.lens[n - 1]) == int(res.n_qual_bytes), where
            assert (q[np.repeat(qo[:n] - w.qoff[:n], w.lens) + w.arange] == w.qual).all(), where
        else:
            assert (qo[:n + 1] == w.qoff).all() and int(res.n_qual_bytes) == w.qual.size, where
            assert (q[:w.qual.size] == w.qual).all(), where
            if mode == 2:
                assert (q[w.qual.size:] == 99).all(), where
    # one row short, as test_table_too_small_with_decode has it on a context without memory
    cap = n - 1
    rc, res, t, q, qo = scan(cap)
    assert rc == hip.E_TABLE_FULL and int(res.n_records) == n
    assert (t[:cap] == w.rows[:cap]).all() and (t[cap:] == -7).all()
    if decode:
        assert (qo[cap + 1:] == -7).all()
        assert (q[qual_cap:] == 99).all()


# ---- 5. a file that changes character -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def changing_file(world, tmp_path_factory):
    """four + wrap + tiny + long + wrap80 + wrap45 + four: every part ends in a newline, the whole is valid"""
    blob = b"".join(world.data[k].tobytes() for k in ("four", "wrap", "tiny", "long", "wrap80", "wrap45", "four"))
    a = np.frombuffer(blob, dtype=np.uint8)
    rows, end, _status, _off = world.oracle.scan(a)
    assert end == 0
    qual, qoff = world.oracle.decode_quals(a, rows)
    path = str(tmp_path_factory.mktemp("changing") / "changing.fq")
    with open(path, "wb") as fh:
        fh.write(blob)
    return blob, a, rows, qual, qoff, path


@pytest.mark.parametrize("bufsize", (1 << 20, 1 << 22))
def test_file_that_changes_character(gpu_ctx, world, changing_file, bufsize):
    """One context over every fill of a file whose parts are of different kinds, through readfastq_iter and the native
    stream, plain and with the decode: every header, sequence, quality and decoded quality is the oracle's, in order."""
    from fastqandfurious_amd import fastqandfurious as fqf, _fastqandfurious as gpu
    hip = world.hip
    blob, a, rows, wq, wqoff, path = changing_file
    n = len(rows)
    gpu_ctx.forget()
    got = list(fqf.readfastq_iter(io.BytesIO(blob), bufsize, fqf.entryfunc, gpu.entrypos))
    assert len(got) == n
    for i, (r, e) in enumerate(zip(rows.tolist(), got)):
        assert e == (blob[r[0] + 1:r[1]], blob[r[2]:r[3]], blob[r[4]:r[5]]), "entry %d" % i
    for decode, single_pass in ((False, False), (True, False), (True, True)):
        gpu_ctx.forget()
        fd = os.open(path, os.O_RDONLY)
        try:
            st = hip.FileStream(gpu_ctx, fd, bufsize, decode=decode, single_pass=single_pass)
            base, paths = 0, []
            for t, fill, off, end_state, _err in st:
                where = "decode %r, single_pass %r: fill at %d, path %d" % (decode, single_pass, off, st.path())
                paths.append(st.path())
                k = t.shape[0]
                assert end_state in (hip.END_OK, hip.END_REFILL), where
                assert base + k <= n and (t == rows[base:base + k]).all(), where
                # the fill's bytes are the file's: with the rows equal, every header, sequence and quality slice is
                # (the first fill begins with the sentinel, stream byte -1)
                lead = max(0, -off)
                assert lead <= 1 and (fill[:lead] == 10).all() and (fill[lead:] == a[off + lead:off + fill.size]).all(), where
                assert k == 0 or (int(t[0, 0]) >= off and int(t[-1, 5]) <= off + fill.size), where
                if decode:
                    q, qo = st.quals()
                    ln = t[:, 5] - t[:, 4]
                    assert qo.shape[0] == k + 1 and qo[-1] == q.shape[0], where
                    if k:
                        assert (qo[1:k] >= qo[:k - 1] + ln[:k - 1]).all() and qo[k] == qo[k - 1] + ln[k - 1], where
                        if not single_pass:
                            assert qo[0] == 0 and (np.diff(qo) == ln).all(), "gaps the caller did not accept, " + where
                        w0, w1 = int(wqoff[base]), int(wqoff[base + k])
                        idx = np.repeat(qo[:k] - (wqoff[base:base + k] - w0), ln) + np.arange(w1 - w0)
                        assert (q[idx] == wq[w0:w1]).all(), "decoded bytes differ, " + where
                base += k
            assert base == n and end_state == hip.END_OK, (decode, single_pass, paths)
        finally:
            st.close()
            os.close(fd)

"""One component of every row as a packed stream: ffq_table_gather_column on tables written by hand.

The expectation of every test is the loop below -- the contract as include/ffq.h states it -- never the package's host
code and never the oracle's gather.  Coordinates: a position minus `add` minus the sentinel (0 / 1) is an offset into the
bytes handed over.  The bytes lie in the middle of a larger device tensor whose margins hold 0xEE, and the output in the
middle of one that holds guard bytes: a read outside the buffer shows up as a wrong byte, a write outside the output as a
guard byte that changed.

The copy kernel (k_decode_stream, also the Phred decode of every scan) walks its 64 KiB output block in windows of at
most 1023 consecutive records; more than 1021 EMPTY records under one 16-byte chunk are what no window covers (the
walk's slow step: csrc/ffq_dqwalk.h, driven on the host by tests/dq_windows_host.cpp).  A quality trim produces exactly
that out of a bad tile, so the zero-run cases here are rows a documented pair of calls yields.
"""
import io
import os
import subprocess

import numpy as np
import pytest

from test_render import hand_buffer
from test_trim import expected_items, loop_rows, scan_on_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
GUARD, MOAT_BYTE, MOAT = 0x5A, 0xEE, 256
COLUMNS = {"header": (0, 1, 1), "sequence": (2, 0, 3), "quality": (4, 0, 5)}
E_TABLE_FULL = -5


# ---- the window walk on the host ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("san", ("", "address,undefined"))
def test_window_walk_on_the_host(tmp_path, san):
    """tests/dq_windows_host.cpp over csrc/ffq_dqwalk.h -- the functions k_decode_stream calls: the walk ends, hands out
    every chunk once, from a window that caches its records; plain and under AddressSanitizer + UBSan"""
    if not os.path.exists(CLANG):
        pytest.skip("no clang++")
    if san:
        # (looked for BEFORE anything is compiled: a build line that breaks is a failure, not a skip)
        res = subprocess.run([CLANG, "-print-resource-dir"], capture_output=True, text=True).stdout.strip()
        if not any(f.startswith("libclang_rt.asan") and f.endswith(".a")
                   for _d, _s, fs in os.walk(os.path.join(res, "lib")) for f in fs):
            pytest.skip("this clang++ has no AddressSanitizer runtime for the host")
    exe = tmp_path / "dq_windows_host"
    cmd = [CLANG, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "fastq-and-furious_amd", "csrc"),
           os.path.join(ROOT, "tests", "dq_windows_host.cpp"), "-o", str(exe)]
    if san:
        cmd[1:1] = ["-fsanitize=" + san, "-fno-sanitize-recover=undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1"))
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert " 0 failures" in p.stdout and " 0 slow steps" not in p.stdout


# ---- the rule ------------------------------------------------------------------------------------------------------------
def loop_gather(data, rows, which, value_add=0, add=0, sentinel=False):
    """(int8 stream, offsets [n + 1]) of buf[p_begin + shift : p_end] + value_add (mod 256) for every row; positions
    - add - sentinel index `data` (bytes).  A component that does not lie inside the bytes, or whose end is not above its
    beginning, is empty."""
    ca, sh, cb = COLUMNS[which] if isinstance(which, str) else which
    s = int(bool(sentinel))
    out, off = [], [0]
    for row in rows:
        b, e = int(row[ca]) + sh - add - s, int(row[cb]) - add - s
        piece = data[b:e] if (e > b and b >= 0 and e <= len(data)) else b""
        out.append(piece)
        off.append(off[-1] + len(piece))
    raw = np.frombuffer(b"".join(out), dtype=np.uint8).astype(np.int64)
    return ((raw + value_add) % 256).astype(np.uint8).view(np.int8), off


# ---- the device ------------------------------------------------------------------------------------------------------------
def moated(data):
    """CUDA tensor MOAT_BYTE * MOAT + data + MOAT_BYTE * MOAT; the data begin at [MOAT]"""
    import torch
    h = np.full(len(data) + 2 * MOAT, MOAT_BYTE, dtype=np.uint8)
    h[MOAT:MOAT + len(data)] = np.frombuffer(data, dtype=np.uint8)
    return torch.from_numpy(h).cuda()


def device_gather(ctx, data, rows, which, value_add=0, add=0, sentinel=False, misalign=0, cap=None, dbuf=None):
    """rows (host int64[n][6]) gathered by ffq_table_gather_column over `data` into an output that begins `misalign` bytes
    behind a 16-byte boundary and has `cap` bytes (None: the sizing call is asked first).  Returns (rc, bytes needed,
    int8 array [cap], offsets); asserts that no byte around the output was written."""
    import torch
    big = moated(data) if dbuf is None else dbuf
    t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 6)).cuda()
    n = t.shape[0]
    d_buf = big.data_ptr() + MOAT
    off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    if cap is None:
        rc, cap = ctx.table_gather_column(d_buf, len(data), t.data_ptr(), n, which, None, 0, off.data_ptr(), sentinel=sentinel,
                                          add=add, value_add=value_add)
        assert rc == (E_TABLE_FULL if cap else 0)
        off.fill_(-7)
    out = torch.full((misalign + cap + 64,), GUARD, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    rc, need = ctx.table_gather_column(d_buf, len(data), t.data_ptr(), n, which, out.data_ptr() + misalign, cap, off.data_ptr(),
                                       sentinel=sentinel, add=add, value_add=value_add)
    h = out.cpu().numpy()
    assert (h[:misalign] == GUARD).all() and (h[misalign + cap:] == GUARD).all(), "bytes outside the output were written"
    return rc, need, h[misalign:misalign + cap].view(np.int8), off.cpu().numpy()


def check(ctx, data, rows, which, **kw):
    """device == loop for rows that index `data`, handed over with the sentinel / add of kw"""
    s, add = int(bool(kw.get("sentinel", False))), kw.get("add", 0)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
    want, off = loop_gather(data, rows, which, kw.get("value_add", 0))
    shifted = rows + s + add
    shifted[rows < 0] = rows[rows < 0]            # (the -1 of a FASTA row is not a position: it does not move)
    rc, need, got, goff = device_gather(ctx, data, shifted, which, **kw)
    assert rc == 0 and need == len(want) == len(got), (rc, need, len(want), kw)
    assert goff.tolist() == off, kw
    if not (got == want).all():
        bad = int(np.nonzero(got != want)[0][0])
        raise AssertionError("first difference at output byte %d of %d (row %d): %r != %r; %r"
                             % (bad, len(want), np.searchsorted(off, bad, side="right") - 1, got[max(bad - 8, 0):bad + 24].tolist(),
                                want[max(bad - 8, 0):bad + 24].tolist(), kw))
    return want.view(np.uint8).tobytes()


@pytest.mark.gpu
def test_hand_vectors(gpu_ctx):
    buf, rows, names = hand_buffer()
    buf = bytes(buf)
    n = len(buf)
    assert names[1] == "an empty header" and names[2] == "a read of length 0"
    # one row: the formula, spelled out
    rc, need, got, off = device_gather(gpu_ctx, buf, rows[:1], "quality", value_add=-33)
    assert (rc, need, off.tolist()) == (0, 10, [0, 10]) and got.tolist() == [40] * 5 + [39] * 4 + [2]
    assert check(gpu_ctx, buf, rows[:1], "header") == b"read/1 x"
    assert check(gpu_ctx, buf, rows[:1], "sequence") == b"ACGTACGTAC"
    # no rows: nothing, and off[0] = 0
    rc, need, got, off = device_gather(gpu_ctx, buf, np.zeros((0, 6), dtype=np.int64), "sequence", cap=0)
    assert (rc, need, off.tolist()) == (0, 0, [0])
    # a row of length 0, alone and between others
    for which in COLUMNS:
        assert check(gpu_ctx, buf, rows[2:3], which) == (b"e" if which == "header" else b"")
        for i in range(len(rows)):
            check(gpu_ctx, buf, rows[i:i + 1], which)
        check(gpu_ctx, buf, rows, which)
        check(gpu_ctx, buf, [rows[2]] * 3 + rows[:1] + [rows[2]] * 40 + rows[3:4] + [rows[2]] * 2, which, misalign=3)
    # the header column, with shift 1, over an empty header: buf[p0 + 1 : p1] is empty, not -1 bytes long
    assert check(gpu_ctx, buf, rows[1:2], "header") == b""
    assert check(gpu_ctx, buf, [rows[1], rows[0], rows[1]], "header") == b"read/1 x"
    # FASTA rows (-1, -1) in the quality column, p_end < p_begin
    r = rows[0]
    odd = [[r[0], r[1], r[2], r[3], -1, -1], [r[0], r[1], r[3], r[2], r[5], r[4]], [r[1], r[0], r[2], r[3], r[4], r[5]]]
    mixed = [rows[0], odd[0], rows[1], odd[1], odd[2], rows[3]] + odd + [rows[5]]
    for which in COLUMNS:
        check(gpu_ctx, buf, mixed, which)
        check(gpu_ctx, buf, odd, which)
    assert check(gpu_ctx, buf, odd[:2], "quality") == b"" and check(gpu_ctx, buf, odd[1:2], "sequence") == b"" == check(gpu_ctx, buf, odd[2:], "header")
    # a component may begin at the buffer's first byte and end at its last
    check(gpu_ctx, buf, [[0, 2, 0, 5, n - 4, n]], "quality")
    check(gpu_ctx, buf, [[0, 2, 0, 5, n - 4, n]], "sequence")
    # repeated, reversed, overlapping
    for which in COLUMNS:
        check(gpu_ctx, buf, rows[::-1], which, misalign=9)
        check(gpu_ctx, buf, [rows[0]] * 5 + rows + [rows[3]] * 40, which)
    check(gpu_ctx, buf, [[rows[0][0], rows[2][1], rows[0][2], rows[1][3], rows[0][4], rows[3][5]]], "quality")
    check(gpu_ctx, buf, [[0, 0, 0, n, 3, n - 3]] * 7, "sequence", misalign=1)
    # the explicit (begin column, shift, end column) triple: any pair of columns, any shift
    assert check(gpu_ctx, buf, rows, (4, 0, 5)) == check(gpu_ctx, buf, rows, "quality")
    assert check(gpu_ctx, buf, rows[:1], (0, 0, 5)) == buf[rows[0][0]:rows[0][5]]
    assert check(gpu_ctx, buf, rows[:1], (2, 3, 3)) == b"TACGTAC"
    assert check(gpu_ctx, buf, rows[:1], (2, -2, 3)) == b"x\nACGTACGTAC"
    check(gpu_ctx, buf, rows, (1, 1, 4), value_add=7)
    # sentinel and add: the same bytes
    for which in COLUMNS:
        check(gpu_ctx, buf, rows, which, sentinel=True, add=0)
        check(gpu_ctx, buf, rows, which, sentinel=True, add=-1, misalign=7)
        check(gpu_ctx, buf, rows, which, sentinel=False, add=(1 << 40) + 3)


_SWEEP = {}
CORNERS = [(0, 0, 0), (40, 40, 40), (0, 40, 0), (40, 0, 40), (0, 0, 40), (10, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (16, 16, 16)]


def sweep():
    """3000 rows whose three component lengths run over 0..40 independently (fixed seed, the corners first) over bytes
    that take every value 0..255; a FASTA-style row now and then.  (bytes, rows) -- computed once."""
    if not _SWEEP:
        rng = np.random.default_rng(20240611)
        rows, at = [], 1
        for i in range(3000):
            h, s, q = (int(x) for x in rng.integers(0, 41, 3))
            if i < len(CORNERS):
                h, s, q = CORNERS[i]
            p0, p2 = at, at + h + 2
            p4 = p2 + s + 3
            rows.append([p0, p0 + 1 + h, p2, p2 + s, p4, p4 + q] if i % 97 != 50 else [p0, p0 + 1 + h, p2, p2 + s, -1, -1])
            at = p4 + q + 1
        data = np.concatenate([np.arange(256, dtype=np.uint8), rng.integers(0, 256, at - 256, dtype=np.uint8)]).tobytes()
        _SWEEP["v"] = (data, np.array(rows, dtype=np.int64), {})
    return _SWEEP["v"]


@pytest.mark.gpu
@pytest.mark.parametrize("sentinel", (False, True))
@pytest.mark.parametrize("add", (0, (1 << 32) + 5))
def test_length_and_alignment_sweep(gpu_ctx, sentinel, add):
    """component lengths 0..40 at every residue of the output address (d_out 0..15 bytes behind a 16-byte boundary), every
    value_add over every byte value; the quality stream is a little under one output block, the three together are more"""
    data, rows, memo = sweep()
    dbuf = moated(data)
    shifted = rows + int(sentinel) + add
    shifted[rows < 0] = -1
    for which, values in (("quality", (0, -33, 7, -128)), ("sequence", (0, -33)), ("header", (0, 7)), ((0, 0, 5), (-128,))):
        for value_add in values:
            key = (str(which), value_add)
            if key not in memo:
                memo[key] = loop_gather(data, rows, which, value_add)
            want, off = memo[key]
            assert len(want) > (50000 if which != (0, 0, 5) else 2 * 65536) and len(set(want.tolist())) == 256
            for mis in range(16):
                rc, need, got, goff = device_gather(gpu_ctx, data, shifted, which, value_add=value_add, add=add, sentinel=sentinel,
                                                    misalign=mis, cap=len(want), dbuf=dbuf)
                assert rc == 0 and need == len(want) and goff.tolist() == off, (which, value_add, mis)
                if not (got == want).all():
                    bad = int(np.nonzero(got != want)[0][0])
                    raise AssertionError((which, value_add, mis, bad, np.searchsorted(off, bad, side="right") - 1,
                                          got[max(bad - 8, 0):bad + 24].tolist(), want[max(bad - 8, 0):bad + 24].tolist()))


# ---- runs of empty rows ----------------------------------------------------------------------------------------------------
def table_of_lengths(lens, seed=5):
    """(bytes, rows): row i's quality is lens[i] bytes of its own (its header 3 bytes, its sequence as long as the quality);
    a row of length 0 keeps positions in line with its neighbours', as a trim leaves them"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    p4 = 8 + np.concatenate([[0], np.cumsum(lens + 1)[:-1]])
    rows = np.stack([p4 - 7, p4 - 4, p4 - 3, p4 - 3 + np.minimum(lens, 2), p4, p4 + lens], axis=1)
    data = rng.integers(33, 127, int(p4[-1] + lens[-1] + 4), dtype=np.uint8).tobytes()
    return data, rows


TAIL = [20] + [30] * 50


def fill(total):
    return [32] * (total // 32) + ([total % 32] if total % 32 else [])


def _zero_run_check(ctx, lens, misaligns=(0, 5), which="quality"):
    data, rows = table_of_lengths(lens)
    dbuf = moated(data)
    want, off = loop_gather(data, rows, which, -33)
    assert which != "quality" or len(want) == sum(lens)
    for mis in misaligns:
        rc, need, got, goff = device_gather(ctx, data, rows, which, value_add=-33, misalign=mis, cap=len(want), dbuf=dbuf)
        assert rc == 0 and need == len(want) and goff.tolist() == off
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (mis, bad[:5], np.searchsorted(off, bad[:5], side="right") - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("z", (1021, 1022, 1023, 1024, 3000))
def test_runs_of_empty_rows(gpu_ctx, z):
    """a row that ends inside (or at the end of) a 16-byte chunk, z empty rows, more bytes in the same output block: at
    z >= 1022 no window of 1023 consecutive records reaches across the run (tests/dq_windows_host.cpp walks these on the
    host; the walk's slow step writes the chunk).  Also with the run in front of every byte, behind the last one, and on
    the boundary between two output blocks."""
    for first in (1, 16, 20, 33):
        _zero_run_check(gpu_ctx, [first] + [0] * z + TAIL)
    _zero_run_check(gpu_ctx, [0] * z + TAIL)                                       # at the start of the table
    _zero_run_check(gpu_ctx, [20] + [30] * 50 + [0] * z)                           # at its end
    _zero_run_check(gpu_ctx, [20] + [0] * z + [7] + [0] * (z + 1) + TAIL)          # two runs in one block
    _zero_run_check(gpu_ctx, [3] + [0] * z + [2] + [0] * z + [1] + [0] * z + TAIL)   # ... under one chunk
    for first in (1, 20):                                                          # on the 65536 boundary, and beside it
        _zero_run_check(gpu_ctx, fill(65536 - first) + [first] + [0] * z + TAIL)
        _zero_run_check(gpu_ctx, fill(65536 - first - 40) + [40] + [0] * z + [first] + TAIL)
        _zero_run_check(gpu_ctx, fill(65536) + [first] + [0] * z + TAIL)
    # another pair of columns walks the same way: the sequence of these rows is 0..2 bytes long
    _zero_run_check(gpu_ctx, [1] + [0] * z + TAIL, which="sequence")


_BAD_TILE = {}
QUAL_BYTES = np.array([c for c in range(35, 74) if c not in b"+@"], dtype=np.uint8)       # Q2..Q40


def bad_tile():
    """3000 single-line reads of 60 bases; reads 200..1500 have quality all '#' (a bad tile), the others Q2..Q40 at random
    (fixed seed)"""
    if not _BAD_TILE:
        rng = np.random.default_rng(31)
        parts = []
        for i in range(3000):
            seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 60).tobytes()
            q = b"#" * 60 if 200 <= i <= 1500 else rng.choice(QUAL_BYTES, 60).tobytes()
            parts.append(b"@tile:%d\n" % i + seq + b"\n+\n" + q + b"\n")
        _BAD_TILE["v"] = b"".join(parts)
    return _BAD_TILE["v"]


def longest_run_of_empty(rows):
    best = run = 0
    for ln in (rows[:, 3] - rows[:, 2]).tolist():
        run = run + 1 if ln == 0 else 0
        best = max(best, run)
    return best


@pytest.mark.gpu
def test_trim_then_gather_without_a_filter(gpu_ctx):
    """ffq_table_trim_quality then ffq_table_gather_column, the pair include/ffq.h recommends, with nothing in between: the
    gather sees what the trim made of a bad tile -- 1301 consecutive rows of length 0"""
    from fastqandfurious_amd import index as X
    data = bad_tile()
    dbuf, table = scan_on_device(gpu_ctx, data)
    rows = table.cpu().numpy()
    assert rows.shape[0] == 3000
    want_rows, stats = loop_rows(data, rows, 20, 20)
    assert longest_run_of_empty(want_rows) >= 1301 and (want_rows[:200, 3] > want_rows[:200, 2]).any()
    trimmed, tstats = X.trim_rows_device(gpu_ctx, dbuf, table, 20, 20)
    assert (trimmed.cpu().numpy() == want_rows).all() and list(tstats) == stats
    for which, value_add in (("sequence", 0), ("quality", -33), ("header", 0)):
        want, off = loop_gather(data, want_rows, which, value_add)
        assert len(want) > 16 * 1024
        # through the wrapper ...
        got, goff = X.select_column_device(gpu_ctx, dbuf, trimmed, which, value_add=value_add)
        assert goff.cpu().numpy().tolist() == off and (got.cpu().numpy() == want).all(), which
        # ... and with the guards around input and output
        for mis in (0, 5):
            rc, need, got, goff = device_gather(gpu_ctx, data, want_rows, which, value_add=value_add, misalign=mis, cap=len(want))
            assert rc == 0 and need == len(want) and goff.tolist() == off and (got == want).all(), (which, mis)


@pytest.mark.gpu
def test_trimmed_column_through_readfastq_iter(gpu_ctx, tmp_path):
    """the same file through readfastq_iter with entryfunc_qualitytrim(20, column="sequence") on the GPU scanner: no
    min_len, so the stream front end gathers the rows trimmed to length 0 too.  The items are the per-record path's."""
    from fastqandfurious_amd import fastqandfurious as F, _fastqandfurious as C
    data = bad_tile()
    p = tmp_path / "tile.fq"
    p.write_bytes(data)
    want = expected_items(F, data, 0, 20, column="sequence", fbufsize=1 << 20)
    assert len(want) == 3000 and all(w == b"" for w in want[200:1501]) and sum(len(w) for w in want) > 50000
    for column in ("sequence", "quality"):
        ef = F.entryfunc_qualitytrim(20, column=column)
        exp = want if column == "sequence" else expected_items(F, data, 0, 20, column=column, fbufsize=1 << 20)
        with open(p, "rb") as fh:
            got = list(F.readfastq_iter(fh, 1 << 20, ef, C.entrypos))
        assert got == exp, column
        with open(p, "rb") as fh:
            per_record = list(F.readfastq_iter(fh, 1 << 20, ef, F.entrypos))
        assert per_record == exp, column
    got = list(F.readfastq_iter(io.BytesIO(data), 1 << 20, F.entryfunc_qualitytrim(20, column="sequence"), C.entrypos))
    assert got == want


@pytest.mark.gpu
def test_scan_with_decode_over_empty_reads(gpu_ctx, oracle):
    """one read, 1100 empty reads ("@h\\n\\n+\\n\\n"), 50 reads, scanned with FFQ_F_DECODE_QUAL: table, qualities and qoff
    are the oracle's, as tests/test_gpu_parity.py::test_decode_quals compares them.  (The reference's C scanner -- the
    oracle, and the device scanners that answer as it does -- looks for the end of a sequence and of a quality BEHIND
    their first byte: it reads this buffer as fewer, longer records and never yields a quality of length 0.  The Python
    scanner does yield them; a device table gets rows of length 0 from ffq_table_trim_quality, not from a scan.)"""
    from fastqandfurious_amd import hip
    from test_gpu_parity import decode_same
    rng = np.random.default_rng(3)

    def read(i, n):
        return b"@r%d\n" % i + rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes() + b"\n+\n" + \
            rng.choice(QUAL_BYTES, n).tobytes() + b"\n"
    for first in (20, 16):
        data = read(0, first) + b"".join(b"@e%d\n\n+\n\n" % i for i in range(1100)) + b"".join(read(i, 30) for i in range(1, 51))
        want, *_ = oracle.scan(data)
        assert len(want) > 400 and want[0, 5] - want[0, 4] == first
        decode_same(gpu_ctx, hip, oracle, data)


@pytest.mark.gpu
def test_capacity(gpu_ctx):
    data, rows, _memo = sweep()
    rows = rows[:700]
    want, off = loop_gather(data, rows, "quality", -33)
    total = len(want)
    assert total > 10000
    for mis in (0, 3):
        rc, need, got, goff = device_gather(gpu_ctx, data, rows, "quality", value_add=-33, misalign=mis, cap=total)
        assert rc == 0 and need == total and (got == want).all() and goff.tolist() == off
        # one byte short: the need comes back, the offsets are written, nothing past cap is touched (device_gather asserts
        # the guards), what fits is there
        rc, need, got, goff = device_gather(gpu_ctx, data, rows, "quality", value_add=-33, misalign=mis, cap=total - 1)
        assert rc == E_TABLE_FULL and need == total and goff.tolist() == off
        assert (got == want[:-1]).all()
        rc, need, got, goff = device_gather(gpu_ctx, data, rows, "quality", value_add=-33, misalign=mis, cap=total // 2 + 1)
        assert rc == E_TABLE_FULL and need == total and goff.tolist() == off and (got == want[:total // 2 + 1]).all()
    # the sizing call: no output at all
    import torch
    t = torch.from_numpy(rows).cuda()
    offs = torch.full((len(rows) + 1,), -7, dtype=torch.int64, device="cuda")
    dbuf = moated(data)
    rc, need = gpu_ctx.table_gather_column(dbuf.data_ptr() + MOAT, len(data), t.data_ptr(), len(rows), "quality", None, 0,
                                           offs.data_ptr(), sentinel=False, add=0)
    assert rc == E_TABLE_FULL and need == total and offs.cpu().numpy().tolist() == off
    # room for bytes but no output, or no buffer, to copy them: FFQ_E_ARG, before anything is launched
    from fastqandfurious_amd import hip
    for d_buf, d_out in ((dbuf.data_ptr() + MOAT, None), (None, t.data_ptr())):
        with pytest.raises(hip.FFQError) as e:
            gpu_ctx.table_gather_column(d_buf, len(data), t.data_ptr(), len(rows), "quality", d_out, 16, offs.data_ptr(),
                                        sentinel=False, add=0)
        assert e.value.code == hip.E_ARG


@pytest.mark.gpu
def test_rows_outside_the_buffer_gather_as_nothing(gpu_ctx):
    """include/ffq.h: a component that does not lie inside [d_buf, d_buf + n_bytes) is empty -- no byte outside is read.
    Positions up to 48 bytes beyond either end (inside the moat of 0xEE around the buffer), lengths 1..20, among rows that
    lie inside, some of them touching the ends."""
    rng = np.random.default_rng(9)
    data = rng.integers(33, 127, 600, dtype=np.uint8).tobytes()         # (no 0xEE among them)
    n = len(data)
    inside = [[0, 0, 0, 0, 100 + 7 * i, 100 + 7 * i + 1 + i] for i in range(20)]

    def rows_with(spans, add):
        rows = []
        for i, (b, e) in enumerate(spans):
            rows.append([x + add for x in inside[i % 20]])
            rows.append([0, 0, 0, 0, b, e])
        return np.array(rows + [[x + add for x in r] for r in inside[:3]], dtype=np.int64)

    def run(spans, sentinel=False, add=0, n_outside=None):
        rows = rows_with(spans, add)
        want, off = loop_gather(data, rows, "quality", 0, add=add, sentinel=sentinel)
        empty = [off[2 * i + 2] == off[2 * i + 1] for i in range(len(spans))]
        assert sum(empty) == (len(spans) if n_outside is None else n_outside)
        for mis in (0, 11):
            rc, need, got, goff = device_gather(gpu_ctx, data, rows, "quality", sentinel=sentinel, add=add, misalign=mis, cap=len(want))
            assert rc == 0 and need == len(want) and goff.tolist() == off, (spans[:3], sentinel, add)
            assert MOAT_BYTE not in got.view(np.uint8).tolist(), "a byte outside the buffer was read"
            assert (got == want).all()
    lens = range(1, 21)
    run([(-1, -1 + L) for L in lens])                                    # begins one byte in front of the buffer
    run([(0, L) for L in lens], sentinel=True)                           # coordinate 0 with a sentinel: the virtual "\n"
    run([(1, 1 + L) for L in lens], sentinel=True, n_outside=0)          # (coordinate 1 is the first byte)
    run([(n + 1 - L, n + 1) for L in lens])                              # ends one byte behind it
    run([(n - L, n) for L in lens], n_outside=0)                         # (may end at its end)
    run([(0, L) for L in lens], n_outside=0)                             # (may begin at its beginning)
    run([(-48, -48 + L) for L in lens] + [(-L, 0) for L in lens] + [(-5, 5), (-16, 16), (-20, 0)])
    run([(n, n + L) for L in lens] + [(n + 48 - L, n + 48) for L in lens] + [(n - 5, n + 5), (n - 16, n + 16)])
    run([(5000 + 3, 5000 + 3 + L) for L in lens], add=5000, n_outside=0)
    run([(5000 - 1, 5000 - 1 + L) for L in lens] + [(5000 + n + 1 - L, 5000 + n + 1) for L in lens], add=5000)
    run([(-1, n + 1), (-48, n + 48), (0, n + 1), (-1, n)])               # around the whole buffer
    # the wrapper sizes its output from the rows' own lengths: with rows outside it returns the shorter stream
    import torch
    from fastqandfurious_amd import index as X
    rows = rows_with([(-1, 4), (n - 3, n + 1), (n + 48 - 7, n + 48)], 0)
    want, off = loop_gather(data, rows, "quality", -33)
    assert 0 < len(want) < int((rows[:, 5] - rows[:, 4]).sum())
    big = moated(data)
    got, goff = X.select_column_device(gpu_ctx, big[MOAT:MOAT + n], torch.from_numpy(rows).cuda(), "quality", sentinel=False,
                                       add=0, value_add=-33)
    assert goff.cpu().numpy().tolist() == off and got.numel() == len(want) and (got.cpu().numpy() == want).all()

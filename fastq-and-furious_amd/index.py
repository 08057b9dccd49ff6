"""Offset-index files: store the table of record positions once, replay it without parsing.

The reference keeps such an index as the concatenation of `pos.tofile(fh_index)` over
`readfastq_iter(fh, bufsize, entryfunc=entryfunc_abspos, ...)`
(/root/reference/src/demo/benchmark.py:268-287): raw native int64 x 6 per record, ABSOLUTE
stream offsets (pos0 = the '@').  It replays it record by record with `array.fromfile`,
`fh.seek`, `fh.read` and `arrayadd_q(posarray, -offset)`
(/root/reference/src/demo/benchmark.py:47-83, doc/user-guide.rst:182-204).

The GPU scan already produces exactly this table for a whole buffer fill, so the index is
written table by table (`build_index`) and replayed in chunks of rows (`iter_indexed`).
Filtering or trimming reads is editing rows (`select_rows`), as the user guide suggests.
"""

import numpy as np

from . import entries as _entries
from . import fastqandfurious as _F
from . import hip as _hip

ROW_BYTES = 48          # 6 x int64 per record


def _fileno(fh):
    """(fd, start) of a plain binary file object -- its descriptor and the position the object is
    at -- else None.  The descriptor itself is not touched: the native stream reads it with pread
    from `start` (start None: it cannot seek and is read in order)."""
    import io
    # only plain files: a GzipFile also has a fileno() -- that of the COMPRESSED file
    raw = fh.raw if isinstance(fh, io.BufferedReader) else fh
    if not isinstance(raw, io.FileIO):
        return None
    try:
        fd = fh.fileno()
    except (AttributeError, OSError, ValueError):
        return None
    try:
        start = fh.tell() if fh.seekable() else None
    except (OSError, ValueError, AttributeError):
        start = None
    if start is None and fh is not raw:
        return None              # a buffered pipe: bytes may already sit in the object's buffer, past the descriptor
    return fd, start


def _leave_at(fh, st):
    """Leave a shared file object where the stream stopped reading (the reference's loop leaves
    `fh` behind the last chunk it read, /root/reference/src/fastqandfurious.py:274-277)."""
    try:
        if fh.seekable():
            fh.seek(st.tell())
    except (OSError, ValueError, AttributeError):
        pass


iter_tables = _F.iter_tables        # one (buf, rows, globaloffset) per buffer fill: the refill loop of readfastq_iter's batched front


def build_index(fh, fh_index, fbufsize=1 << 24, entrypos=None):
    """Write the offset index of the FASTQ stream `fh` to `fh_index`; returns the number of
    records.  `entrypos` is a scanner as readfastq_iter takes it; one that offers
    `scan_buffer` (the GPU scanner of this package, the default) writes a whole table per
    buffer fill, any other goes record by record exactly like the reference
    (benchmark.py:277-283).  The bytes written are the same either way."""
    if entrypos is None:
        from . import _fastqandfurious
        entrypos = _fastqandfurious.entrypos
        f = _fileno(fh)
        if f is not None:
            # a real file and the GPU scanner: the native stream front end (ffq_stream_*) reads
            # ahead into pinned memory and hands back whole tables; no per-fill Python copies
            n = 0
            st = _hip.FileStream(_hip.default_context(), f[0], fbufsize, start=f[1])
            try:
                for rows, _fill, _off, end_state, err in st:
                    if rows.shape[0]:
                        fh_index.write(memoryview(rows).cast("B"))
                        n += rows.shape[0]
                    if end_state not in (_F._END_OK, _F._END_REFILL):
                        _F._raise_for_end(end_state, err)
            finally:
                _leave_at(fh, st)
                st.close()
            return n
    scan_buffer = getattr(entrypos, 'scan_buffer', None)
    n = 0
    if scan_buffer is None:
        for pos in _F.readfastq_iter(fh, fbufsize, _F.entryfunc_abspos, entrypos):
            pos.tofile(fh_index)
            n += 1
        return n
    for _buf, rows, globaloffset in iter_tables(fh, fbufsize, scan_buffer):
        t = np.frombuffer(rows, dtype=np.int64) + np.int64(globaloffset)     # entryfunc_abspos, all rows
        fh_index.write(t.tobytes())
        n += t.size // 6
    return n


def read_index(fh_index, count=-1):
    """The index as int64[n][6] (count = -1: all of it)."""
    raw = fh_index.read() if count < 0 else fh_index.read(count * ROW_BYTES)
    if len(raw) % ROW_BYTES:
        raise ValueError('The index must hold 6 int64 per entry.')
    return np.frombuffer(raw, dtype=np.int64).reshape(-1, 6)


def iter_indexed(fh, fh_index, chunk_records=1 << 16):
    """Replay: yields (header, sequence, quality) per index row, read from `fh` by position
    without parsing.  As in the reference's replay loop (benchmark.py:62-71) the slices are
    `buf[pos0:pos1]`, `buf[pos2:pos3]`, `buf[pos4:pos5]` -- pos0 is the '@', so the header
    slice starts with it.  Rows may have been filtered or edited; they must be in stream
    order within a chunk only if `fh` cannot seek backwards."""
    while True:
        t = read_index(fh_index, chunk_records)
        if t.shape[0] == 0:
            return
        lo = int(t[:, 0].min())
        hi = int(t[:, 5].max())
        fh.seek(lo)
        buf = fh.read(hi - lo + 1)
        if _entries.native() is not None:
            # arrayadd_q(posarray, -offset) and the three slices of every row, natively
            # (csrc/ffq_entries.c; a thousand rows per call so that consumed tuples are reused)
            t = np.ascontiguousarray(t)
            for at in range(0, t.shape[0], 1024):
                yield from _entries.entries(buf, t[at:at + 1024], lo, 0)
            continue
        rel = (t - lo).tolist()                 # arrayadd_q(posarray, -offset), whole chunk
        for p0, p1, p2, p3, p4, p5 in rel:
            yield (buf[p0:p1], buf[p2:p3], buf[p4:p5])


def select_rows(table, min_seq_len=None, max_seq_len=None):
    """Rows whose sequence length pos3 - pos2 lies in [min_seq_len, max_seq_len]: the length
    filter of doc/user-guide.rst:153-180 evaluated on the table, before any per-record
    object exists."""
    t = np.asarray(table, dtype=np.int64).reshape(-1, 6)
    ln = t[:, 3] - t[:, 2]
    keep = np.ones(t.shape[0], dtype=bool)
    if min_seq_len is not None:
        keep &= ln >= min_seq_len
    if max_seq_len is not None:
        keep &= ln <= max_seq_len
    return t[keep]


def select_rows_device(ctx, table, min_seq_len=None, max_seq_len=None):
    """select_rows on the GPU: `table` is a CUDA int64[n][6] torch tensor (e.g. the output of a
    device scan); returns a new tensor with the kept rows, in order.  One C-ABI call
    (ffq_table_select_seqlen: count, scan, scatter kernels)."""
    import torch
    n = int(table.shape[0])
    out = torch.empty_like(table)
    lo, hi = _hip.length_bounds(min_seq_len, max_seq_len)
    k = ctx.table_select_seqlen(table.data_ptr(), n, lo, hi, out.data_ptr()) if n else 0
    return out[:k]


def trim_rows(buf, table, cutoff_back, cutoff_front=0, qual_base=33, shift=0):
    """Quality-trimmed copy of a table, on the host: pos2..pos5 of every row the rule applies to (_F.trimmable: positions
    minus `shift` index `buf`) moved inwards by the running-sum rule (_F.quality_trim_span); the same rows, none dropped
    -- select_rows then drops what became too short.  The user guide's "modifying the values in a table of indices"
    (doc/user-guide.rst:196-204)."""
    t = np.array(table, dtype=np.int64).reshape(-1, 6)
    buf = bytes(buf) if not isinstance(buf, bytes) else buf
    for row in t:
        rel = (row - shift).tolist()
        if _F.trimmable(buf, rel):
            start, stop = _F.quality_trim_span(buf[rel[4]:rel[5]], cutoff_back, cutoff_front, qual_base)
            row[2:6] = (row[2] + start, row[2] + stop, row[4] + start, row[4] + stop)
    return t


def trim_rows_device(ctx, buf, table, cutoff_back, cutoff_front=0, qual_base=33, sentinel=True, add=None, out=None):
    """trim_rows on the GPU: `buf` is the CUDA uint8 tensor the rows of `table` (CUDA int64[n][6]) were scanned from,
    sentinel / add as that scan had them.  Returns (tensor with the trimmed rows -- a new one, or `out`, which may be
    `table` itself: in place --, (rows changed, bases removed, rows skipped)).  One C-ABI call
    (ffq_table_trim_quality)."""
    import torch
    n = int(table.shape[0])
    if out is None:
        out = torch.empty_like(table)
    stats = ctx.table_trim_quality(buf.data_ptr(), buf.numel(), table.data_ptr(), n, cutoff_back, cutoff_front, qual_base,
                                   d_out=out.data_ptr(), sentinel=sentinel, add=add)
    return out, stats


def trim_adapter_rows(buf, table, adapter, err_permille=100, min_overlap=3, shift=0):
    """Copy of a table cut at a 3' adapter, on the host: pos3 and pos5 of every row the rule applies to
    (_F.adapter_trimmable: positions minus `shift` index `buf`) moved to the leftmost place the adapter matches
    (_F.adapter_cut); the same rows, none dropped.  Run it behind trim_rows (cutadapt's order: -q first)."""
    t = np.array(table, dtype=np.int64).reshape(-1, 6)
    buf = bytes(buf) if not isinstance(buf, bytes) else buf
    _F._adapter_args(adapter, err_permille, min_overlap)
    for row in t:
        rel = (row - shift).tolist()
        if _F.adapter_trimmable(buf, rel):
            cut = _F.adapter_cut(buf[rel[2]:rel[3]], adapter, err_permille, min_overlap)
            row[3], row[5] = row[2] + cut, row[4] + cut
    return t


def trim_adapter_rows_device(ctx, buf, table, adapter, err_permille=100, min_overlap=3, sentinel=True, add=None, out=None):
    """trim_adapter_rows on the GPU: `buf` is the CUDA uint8 tensor the rows of `table` (CUDA int64[n][6]) were scanned from,
    sentinel / add as that scan had them.  Returns (tensor with the trimmed rows -- a new one, or `out`, which may be
    `table` itself: in place --, (rows changed, bases removed, rows skipped)).  One C-ABI call (ffq_table_trim_adapter)."""
    import torch
    n = int(table.shape[0])
    if out is None:
        out = torch.empty_like(table)
    stats = ctx.table_trim_adapter(buf.data_ptr(), buf.numel(), table.data_ptr(), n, adapter, err_permille, min_overlap,
                                   d_out=out.data_ptr(), sentinel=sentinel, add=add)
    return out, stats


def poly_rows(buf, table, base=None, min_len=10, shift=0):
    """Copy of a table with the poly tails cut off, on the host: pos3 and pos5 of every row the rule applies to
    (_F.poly_trimmable: positions minus `shift` index `buf`) moved to where _F.poly_tail_cut says (base: b"A", b"C", b"G",
    b"T", or None for any of the four); the same rows, none dropped.  Poly-G runs behind trim_rows and in front of
    trim_adapter_rows, poly-X behind that.  On the GPU: hip.Context.table_trim_poly."""
    t = np.array(table, dtype=np.int64).reshape(-1, 6)
    buf = bytes(buf) if not isinstance(buf, bytes) else buf
    _F.poly_tail_cut(b"", base, min_len)                # (checks the arguments)
    for row in t:
        rel = (row - shift).tolist()
        if _F.poly_trimmable(buf, rel):
            cut = _F.poly_tail_cut(buf[rel[2]:rel[3]], base, min_len)
            row[3], row[5] = row[2] + cut, row[4] + cut
    return t


def umi_rows(buf, table, rules, shift=0):
    """Copy of a table with the UMIs taken off, on the host: pos2 and pos4 of every row the rule applies to (_F.umi_takable:
    positions minus `shift` index `buf`) and that is at least rules.length long moved inwards by min(length + skip, the
    read's length) (rules: an _F.UmiRules; its loc does not matter here); the same rows, none dropped.  pos1 stays: the UMI
    is buf[pos1 + 1:pos1 + 1 + length].  It runs in front of ends_rows and every other trim.  On the GPU:
    hip.Context.table_take_umi."""
    t = np.array(table, dtype=np.int64).reshape(-1, 6)
    buf = bytes(buf) if not isinstance(buf, bytes) else buf
    rules._check()
    for row in t:
        rel = (row - shift).tolist()
        if _F.umi_takable(buf, rel) and rel[3] - rel[2] >= rules.length:
            cut = min(rules.length + rules.skip, rel[3] - rel[2])
            row[2] += cut
            row[4] += cut
    return t


def ends_rows(buf, table, rules, qual_base=33, shift=0):
    """Copy of a table with the fixed trims and sliding windows of `rules` (an _F.EndRules) applied, on the host: pos2..pos5 of
    every row the rule applies to (_F.ends_trimmable: positions minus `shift` index `buf`) moved to where _F.ends_cut says;
    the same rows, none dropped.  It runs in front of trim_rows and every other trim.  On the GPU:
    hip.Context.table_trim_ends."""
    t = np.array(table, dtype=np.int64).reshape(-1, 6)
    buf = bytes(buf) if not isinstance(buf, bytes) else buf
    _F.ends_cut(b"", rules, qual_base)                  # (checks the arguments)
    for row in t:
        rel = (row - shift).tolist()
        if _F.ends_trimmable(buf, rel):
            a, b = _F.ends_cut(buf[rel[4]:rel[5]], rules, qual_base)
            row[2:6] = (row[2] + a, row[2] + b, row[4] + a, row[4] + b)
    return t


def stats_rows(buf, table, qual_base=33, max_cycles=512, shift=0):
    """Per-cycle base and quality statistics of the rows of a table, on the host (_F.FastqStats.add_rows: positions minus
    `shift` index `buf`; a row the rule does not apply to counts as skipped)."""
    return _F.FastqStats(max_cycles, qual_base).add_rows(buf, table, shift)


def stats_rows_device(ctx, buf, table, qual_base=33, max_cycles=512, sentinel=True, add=None, out=None, accumulate=False):
    """stats_rows on the GPU: `buf` is the CUDA uint8 tensor the rows of `table` (CUDA int64[n][6]) were scanned from,
    sentinel / add as that scan had them.  out: a CUDA int64 tensor of hip.stats_words(max_cycles) elements to count into
    (overwritten, or added to with accumulate); None: a new one.  Returns (_F.FastqStats of what `out` holds after the call,
    out).  One C-ABI call (ffq_table_stats) and one copy back."""
    import torch
    words = _hip.stats_words(max_cycles)
    if out is None:
        out = torch.zeros(words, dtype=torch.int64, device=buf.device)
        torch.cuda.current_stream(buf.device).synchronize()      # (the call runs on the context's stream, not on torch's)
    ctx.table_stats(buf.data_ptr(), buf.numel(), table.data_ptr(), int(table.shape[0]), out.data_ptr(), qual_base, max_cycles,
                    accumulate=accumulate, sentinel=sentinel, add=add)
    return _F.FastqStats.from_words(out.cpu().numpy().view(np.uint64), max_cycles, qual_base), out


def select_column_device(ctx, buf, table, which, sentinel=True, add=None, value_add=0):
    """One component of every row, packed, on the GPU: `buf` is the CUDA uint8 tensor the rows of
    `table` (CUDA int64[n][6]) were scanned from; which = "header" | "sequence" | "quality".
    Returns (int8 tensor with the bytes, int64 tensor with n + 1 offsets): what an entryfunc that
    builds only that component returns for every entry (doc/user-guide.rst:153-180), before any
    per-record Python object exists.  With value_add = -33 on "quality": the Phred decode."""
    import torch
    n = int(table.shape[0])
    off = torch.empty(n + 1, dtype=torch.int64, device=table.device)
    ca, sh, cb = ctx.COLUMNS[which] if isinstance(which, str) else which
    total = int((table[:, cb] - table[:, ca] - sh).clamp_(min=0).sum().item()) if n else 0
    out = torch.empty(max(total, 16), dtype=torch.int8, device=table.device)
    rc, nb = ctx.table_gather_column(buf.data_ptr(), buf.numel(), table.data_ptr(), n, which, out.data_ptr(), total,
                                     off.data_ptr(), sentinel=sentinel, add=add, value_add=value_add)
    # (fewer than `total`: rows that do not lie inside `buf` gather as nothing, include/ffq.h)
    if rc != 0 or nb > total:
        raise RuntimeError("select_column_device: gathered %d of %d bytes (code %d)" % (nb, total, rc))
    return out[:nb], off


def render_rows(buf, table, shift=0):
    """FASTQ text of a table, on the host: row p renders as b"@" + buf[p0 + 1:p1] + b"\\n" + buf[p2:p3] + b"\\n+\\n" +
    buf[p4:p5] + b"\\n" (positions minus `shift` index `buf`) -- the three slices of entryfunc and a bare '+' line, in table
    order; a row that is not renderable (a position below 0, a slice that ends in front of its beginning or behind the
    buffer: FASTA rows, rows that point elsewhere) renders as nothing.  What a pipeline that deleted and edited rows
    "to avoid saving a FASTQ file after each filtering or read-trimming step" (doc/user-guide.rst:196-204) saves at its
    end.  A read of length 0 renders as b"@h\\n\\n+\\n\\n": a file with such records is read back record for record by the
    Python scanner only (the GPU scanner answers as the reference's C scanner does and joins an empty record with the one
    behind it) -- filter with min_seq_len >= 1 in front of a file the GPU scanner or other tools will read."""
    t = np.asarray(table, dtype=np.int64).reshape(-1, 6)
    buf = bytes(buf) if not isinstance(buf, bytes) else buf
    n = len(buf)
    out = []
    for p0, p1, p2, p3, p4, p5 in (t - shift).tolist():
        if min(p0, p1, p2, p3, p4, p5) < 0 or p0 + 1 > p1 or p2 > p3 or p4 > p5 or max(p1, p3, p5) > n:
            continue
        out += (b"@", buf[p0 + 1:p1], b"\n", buf[p2:p3], b"\n+\n", buf[p4:p5], b"\n")
    return b"".join(out)


def render_rows_device(ctx, buf, table, sentinel=True, add=None):
    """render_rows on the GPU: `buf` is the CUDA uint8 tensor the rows of `table` (CUDA int64[n][6]) were scanned from,
    sentinel / add as that scan had them.  Returns (uint8 tensor with the text, int64 tensor with n + 1 offsets -- row i's
    record is text[off[i]:off[i + 1]], empty for a row that is not renderable --, (bytes rendered, rows rendered, rows
    skipped)).  Two C-ABI calls (ffq_table_render_fastq): the first, without an output, says how many bytes there are."""
    import torch
    n = int(table.shape[0])
    off = torch.empty(n + 1, dtype=torch.int64, device=table.device)
    _, (need, _, _) = ctx.table_render_fastq(buf.data_ptr(), buf.numel(), table.data_ptr(), n, None, 0, None,
                                             sentinel=sentinel, add=add)
    out = torch.empty(max(need, 16), dtype=torch.uint8, device=table.device)
    rc, stats = ctx.table_render_fastq(buf.data_ptr(), buf.numel(), table.data_ptr(), n, out.data_ptr(), need, off.data_ptr(),
                                       sentinel=sentinel, add=add)
    if rc != 0 or stats[0] != need:
        raise RuntimeError("render_rows_device: rendered %d of %d bytes (code %d)" % (stats[0], need, rc))
    return out[:need], off, stats

"""Duplicate removal on the device: ffq_table_seq_keys and ffq_dedup_select against the plain loops and the dict of
tests/dedup_expect.py.  Every comparison is exact: every key, the kept rows of both tables, d_idx, all six counts.  Coordinates:
a row minus `add` indexes the buffer the scanner saw; with a sentinel that buffer is b'\\n' + bytes.  The buffer lies at the END
of a device allocation of whole pages and begins at a multiple of 16, so that a read past its end leaves the allocation and a
sequence's address modulo 16 is what the table builder says it is."""
import ctypes

import numpy as np
import pytest

import dedup_expect as X

pytestmark = pytest.mark.gpu

GROUP_BYTES = 32        # bytes of a row that its 8 lanes take per round (csrc/ffq_dedup.h: SEQKEY_G * 4)
TILE = 160              # bases above which a row goes onto the long list and gets a wave of its own (SEQKEY_TILE)
WAVE_BYTES = 256        # bytes of a row that the 64 lanes of the long rows' kernel take per step


def band(x):
    return [x - 1, x, x + 1]


LENGTHS = sorted(set(list(range(0, 41)) + band(GROUP_BYTES) + band(2 * GROUP_BYTES) + band(TILE) + band(WAVE_BYTES) + band(2 * WAVE_BYTES)))


# ---- tables by hand ------------------------------------------------------------------------------------------------
def place(buf, rows, seq, qual=None, mod16=None):
    """append a four-line record whose sequence begins at an offset = mod16 modulo 16 (junk in front of the record)"""
    qual = b"I" * len(seq) if qual is None else qual
    if mod16 is not None:
        buf += b"#" * ((mod16 - (len(buf) + 3)) % 16)
    p0 = len(buf)
    buf += b"@h\n"
    p2 = len(buf)
    buf += seq + b"\n+\n"
    p4 = len(buf)
    buf += qual + b"\n"
    rows.append([p0, p2 - 1, p2, p2 + len(seq), p4, p4 + len(qual)])


def read_of(rng, n):
    return np.frombuffer(b"ACGTNacgt", dtype=np.uint8)[rng.integers(0, 9, n)].tobytes()


def finish(buf, rows):
    """the buffer with junk in front so that its length is a multiple of 16 (it ENDS where the allocation ends), the rows moved"""
    pad = (-len(buf)) % 16
    return b"%" * pad + bytes(buf), np.array(rows, dtype=np.int64).reshape(-1, 6) + pad


class Dev:
    def __init__(self, ctx, data):
        assert len(data) % 16 == 0
        self.ctx, self.n = ctx, len(data)
        self.size = (len(data) + 4095) // 4096 * 4096 + 4096
        self.base = ctx.dev_alloc(self.size)
        self.ptr = self.base + self.size - len(data)
        if len(data):
            ctx.h2d(self.ptr, np.frombuffer(data, dtype=np.uint8).copy())
        ctx.sync()

    def close(self):
        self.ctx.dev_free(self.base)

    def keys(self, rows, sentinel=False, add=0):
        """ffq_table_seq_keys -> (keys as Python ints, counts)"""
        import torch
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 6)
        n = rows.shape[0]
        t = torch.from_numpy(rows.copy()).cuda() if n else torch.zeros((1, 6), dtype=torch.int64, device="cuda")
        k = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        counts = self.ctx.table_seq_keys(self.ptr, self.n, t.data_ptr(), n, k.data_ptr(), sentinel=sentinel, add=add)
        got = k.cpu().numpy()
        assert got[n] == -7, "a key behind the last row was written"
        return [int(x) for x in got[:n].view(np.uint64)], counts


def check_keys(dev, buf, rows, combos=((0, 0),)):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
    wants = []
    for sentinel, add in combos:
        seen = (b"\n" if sentinel else b"") + buf
        want = [X.row_key(seen, r, bool(sentinel)) for r in (rows + sentinel).tolist()]
        got, counts = dev.keys(rows + sentinel + add, bool(sentinel), add)
        bad = [i for i in range(len(want)) if got[i] != want[i]]
        assert not bad, (sentinel, add, bad[:10], [rows[i].tolist() for i in bad[:3]])
        assert counts == (sum(1 for k in want if k != X.KEY_NONE), sum(1 for k in want if k == X.KEY_NONE)), (sentinel, add)
        wants.append(want)
    return wants[0]


@pytest.fixture(scope="module")
def lengths_table(gpu_ctx):
    """one read per length of LENGTHS, the SAME bytes at every address modulo 16; a read of 10 007 bases at two"""
    rng = np.random.default_rng(17)
    buf, rows, reads = bytearray(b"#"), [], {}
    for n in LENGTHS:
        reads[n] = read_of(rng, n)
        for a in range(16):
            place(buf, rows, reads[n], None, a)
    big = read_of(rng, 10007)
    for a in (3, 14):
        place(buf, rows, big, None, a)
    buf, rows = finish(buf, rows)
    assert sorted(set(int(r[2]) % 16 for r in rows)) == list(range(16))
    dev = Dev(gpu_ctx, buf)
    yield dev, buf, rows
    dev.close()


def test_keys_at_every_length_and_alignment(lengths_table):
    dev, buf, rows = lengths_table
    want = check_keys(dev, buf, rows, ((0, 0), (1, 0), (0, 1000003), (1, -77)))
    # copies of one read at different addresses have one key; different reads have different keys
    per_len = [set(want[16 * i:16 * i + 16]) for i in range(len(LENGTHS))]
    assert all(len(s) == 1 for s in per_len) and len(set.union(*per_len)) == len(LENGTHS)
    assert want[-1] == want[-2] != X.KEY_NONE and X.KEY_NONE not in want
    # any order, repeated rows
    rng = np.random.default_rng(2)
    check_keys(dev, buf, rows[rng.integers(0, len(rows), 700)])


def test_keys_of_rows_the_rule_does_not_apply_to(gpu_ctx):
    rng = np.random.default_rng(23)
    buf, rows = bytearray(b"#"), []
    for n in (20, 150, 170, 300, 1000):                      # wrapped: a newline inside the sequence (short rows and long ones)
        s = bytearray(read_of(rng, n))
        for at in (0, n // 2, n - 1):
            w = bytes(s[:at]) + b"\n" + bytes(s[at + 1:])
            place(buf, rows, w, None, int(rng.integers(0, 16)))
        place(buf, rows, bytes(s), None, 5)
    n_good = len(rows)
    good = [list(r) for r in rows]
    # a sequence and a quality of two lengths; FASTA rows; rows that point outside, backwards, below zero
    r = good[3]
    rows.append(r[:5] + [r[5] - 1])
    rows.append(r[:4] + [-1, -1])
    rows.append([r[0], r[1], r[2], 1 << 40, r[4], r[4] + (1 << 40) - r[2]])
    rows.append([r[0], r[1], r[3], r[2], r[4], r[4] + r[2] - r[3]])
    rows.append([r[0], r[1], -5, -5 + r[3] - r[2], r[4], r[5]])
    rows.append([r[0], r[1], r[2], r[3], -(1 << 62), -(1 << 62) + r[3] - r[2]])
    rows.append([-1] * 6)
    # a read that ends with the buffer's last byte (its quality lies in front of it); an empty one there
    tail = read_of(rng, 37)
    q4 = len(buf)
    buf += b"J" * 37 + b"\n"
    buf += b"#" * ((-(len(buf) + 37)) % 16)
    s2 = len(buf)
    buf += tail
    assert len(buf) % 16 == 0
    rows.append([0, 1, s2, s2 + 37, q4, q4 + 37])
    rows.append([0, 1, s2 + 37, s2 + 37, q4, q4])
    rows.append([0, 1, s2 + 1, s2 + 38, q4, q4 + 37])         # one byte too far
    buf, rows = finish(buf, rows)
    dev = Dev(gpu_ctx, buf)
    try:
        want = check_keys(dev, buf, rows, ((0, 0), (1, 0), (1, 12345)))
        assert sum(1 for k in want[:n_good] if k == X.KEY_NONE) == 15 and all(k == X.KEY_NONE for k in want[n_good:n_good + 7])
        assert want[-3] == X.loop_key(tail) and want[-2] == X.loop_key(b"") and want[-1] == X.KEY_NONE
        # with a sentinel, coordinate 0 is the virtual newline: a sequence with bytes in it that begins there has no key, an empty one has
        first = [[0, 0, 0, 4, 8, 12], [0, 0, 0, 0, 8, 8], [0, 0, 1, 5, 0, 4]]
        got, counts = dev.keys(first, True, 0)
        seen = b"\n" + buf
        assert got == [X.KEY_NONE, X.loop_key(b""), X.loop_key(seen[1:5])] == [X.row_key(seen, r, True) for r in first]
        assert counts == (2, 1)
        assert dev.keys(np.zeros((0, 6), dtype=np.int64)) == ([], (0, 0))
    finally:
        dev.close()


# ---- the set ---------------------------------------------------------------------------------------------------------------
def u64(keys):
    return np.array([int(k) for k in keys], dtype=np.uint64)


def dev_select(dd, keys1, keys2=None, ord_=None, n_tables=1, drop=True, idx=True):
    """ffq_dedup_select on arrays made here -> (d_idx list, out table 1, out table 2, counts, the input tables)"""
    import torch
    n_keys = len(keys1)
    n = n_keys if ord_ is None else len(ord_)

    def dev(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int64).copy() if a.dtype == np.uint64 else a.copy()).cuda() if a.size else \
            torch.zeros((2,), dtype=torch.int64, device="cuda")
    k1 = dev(u64(keys1))
    k2 = dev(u64(keys2)) if keys2 is not None else None
    od = dev(np.asarray(ord_, dtype=np.int64)) if ord_ is not None else None
    tabs = [(np.arange(6 * n, dtype=np.int64).reshape(n, 6) * 3 + 1000003 * (t + 1)) for t in range(n_tables)]
    dt = [dev(t) for t in tabs]
    outs = [torch.full((n + 1, 6), -7, dtype=torch.int64, device="cuda") for _ in range(n_tables)]
    di = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    p = [x.data_ptr() for x in dt] + [None, None]
    o = [x.data_ptr() for x in outs] + [None, None]
    k, counts = dd.select(k1.data_ptr(), n, k2.data_ptr() if k2 is not None else None, od.data_ptr() if od is not None else None,
                          p[0], p[1], o[0], o[1], di.data_ptr() if idx else None, drop)
    d = di.cpu().numpy()
    assert (d[k if idx else 0:] == -7).all()
    got = []
    for x in outs:
        h = x.cpu().numpy()
        assert (h[k:] == -7).all(), "rows behind the kept ones were written"
        got.append(h[:k])
    return d[:k].tolist(), got, counts, tabs, k


def check_call(dd, model, keys1, keys2=None, ord_=None, n_tables=1, drop=True):
    """one call against the dict, exact; returns the counts"""
    n_keys = len(keys1)
    order = list(range(n_keys)) if ord_ is None else [int(j) for j in ord_]
    eff = [(X.loop_pair_key(keys1[j], keys2[j]) if keys2 is not None else keys1[j]) for j in order]
    kept, counts = model.select(eff, drop)
    idx, got, gc, tabs, k = dev_select(dd, keys1, keys2, ord_, n_tables, drop)
    assert gc == counts, (gc, counts)
    assert k == len(kept) and gc[0] + gc[1] == len(order)
    assert idx == [order[i] for i in kept]
    for t, g in zip(tabs, got):
        assert (g == t[kept]).all()
    return gc


@pytest.fixture
def fresh(gpu_ctx):
    from fastqandfurious_amd import hip
    made = []

    def make(expected=0, max_bytes=0):
        dd = hip.Dedup(gpu_ctx, expected, max_bytes)
        made.append(dd)
        return dd, X.LoopSet(expected)
    yield make
    for dd in made:
        dd.close()


def rand_keys(rng, n):
    return [int(x) | 1 for x in rng.integers(1, 1 << 63, n)]


@pytest.mark.parametrize("drop", (True, False))
def test_first_copy_wins(fresh, drop):
    rng = np.random.default_rng(31)
    dd, model = fresh()
    pool = rand_keys(rng, 150)
    # duplicates inside one call
    a = [pool[int(i)] for i in rng.integers(0, 100, 400)]
    check_call(dd, model, a, drop=drop)
    # across three calls: earlier keys, new ones
    for lo in (50, 100):
        b = [pool[int(i)] for i in rng.integers(lo - 50, lo + 50, 300)]
        check_call(dd, model, b, drop=drop)
    # d_ord a permutation: the call's order decides, not the keys' places
    keys = [pool[int(i)] for i in rng.integers(100, 150, 200)] + rand_keys(rng, 56)
    gc = check_call(dd, model, keys, ord_=rng.permutation(256), drop=drop)
    assert gc[3] == len(model.first) and gc[4] == 1024 and gc[5] == 0
    # d_ord a selection (what a filter kept), no table
    check_call(dd, model, rand_keys(rng, 64) + keys[:64], ord_=[1, 5, 64, 65, 66, 100, 127], n_tables=0, drop=drop)
    assert check_call(dd, model, [], drop=drop)[:3] == [0, 0, 0]


@pytest.mark.parametrize("drop", (True, False))
def test_contention_probing_and_wrap_around(fresh, drop):
    dd, model = fresh(70000)
    # 65 536 rows with one key: exactly row 0 is kept
    gc = check_call(dd, model, [0xDEADBEEFCAFEF00D] * 65536, drop=drop)
    assert gc[:4] == [1, 65535, 0, 1]
    # equal home slots in the minimum table: keys whose low 10 bits are equal, a chain of 200
    dd, model = fresh()
    chain = [(i + 1) << 10 | 0x155 for i in range(200)]
    assert check_call(dd, model, chain + chain[::-1], drop=drop)[:2] == [200, 200]
    # homes slots - 1, slots - 2, ...: the chain wraps to slot 0
    dd, model = fresh()
    wrap = [((i + 1) << 10) | (1023 - i % 3) for i in range(120)]
    gc = check_call(dd, model, wrap, drop=drop)
    assert gc[:2] == [120, 0] and gc[4] == 1024
    assert check_call(dd, model, wrap[::-1] + chain[:50], drop=drop)[:2] == [50, 120]


@pytest.mark.parametrize("drop", (True, False))
def test_growth_keeps_every_key_and_its_first_ordinal(fresh, drop):
    rng = np.random.default_rng(37)
    dd, model = fresh(0)
    calls = []
    for c in range(3):
        new = rand_keys(rng, 4096)
        old = [k for call in calls for k in call[:300]]
        keys = new + old
        keys = [keys[int(i)] for i in rng.permutation(len(keys))]
        gc = check_call(dd, model, keys, drop=drop)
        assert gc[1] == len(old)
        calls.append(new)
    assert gc[5] >= 2 and gc[3] == 3 * 4096 and gc[4] >= 2 * gc[3]
    # every key is still known: all of them again, in reverse, are duplicates (a first ordinal lost in a rehash would be re-entered)
    everything = [k for call in calls for k in call][::-1]
    gc = check_call(dd, model, everything, drop=drop)
    assert gc[:4] == [0, len(everything), 0, 3 * 4096]


@pytest.mark.parametrize("drop", (True, False))
def test_rows_without_a_key_and_pair_keys(fresh, drop):
    rng = np.random.default_rng(41)
    dd, model = fresh()
    k = rand_keys(rng, 40)
    keys = [X.KEY_NONE if i % 3 == 0 else k[i % 40] for i in range(300)]
    gc = check_call(dd, model, keys, drop=drop)
    assert gc[2] == 100 and gc[3] <= 40 and gc[0] == 100 + gc[3]
    assert check_call(dd, model, [X.KEY_NONE] * 70, drop=drop)[:3] == [70, 0, 70]
    # pairs: (k1, k2), (k2, k1) and (k1, k1) are three pairs; a pair with a mate without a key has none
    dd, model = fresh()
    k1, k2 = k[0], k[1]
    a = [k1, k2, k1, k1, k2, k1, X.KEY_NONE, k1, X.KEY_NONE, k1]
    b = [k2, k1, k1, k2, k1, k1, k2, X.KEY_NONE, X.KEY_NONE, k2]
    gc = check_call(dd, model, a, b, n_tables=2, drop=drop)
    assert gc[:4] == [6, 4, 3, 3]
    many1, many2 = [k[int(i)] for i in rng.integers(0, 12, 500)], [k[int(i)] for i in rng.integers(0, 12, 500)]
    gc = check_call(dd, model, many1, many2, ord_=rng.permutation(500)[:400], n_tables=2, drop=drop)
    assert gc[3] <= 3 + 144


def test_a_cap_that_is_too_small_and_bad_arguments(gpu_ctx, fresh):
    import torch
    from fastqandfurious_amd import hip
    rng = np.random.default_rng(43)
    with pytest.raises(hip.FFQError) as ei:                  # the minimum table has 16 KiB
        hip.Dedup(gpu_ctx, 0, 1000)
    assert ei.value.code == hip.E_NOMEM
    dd, model = fresh(0, 1024 * 16)
    first = rand_keys(rng, 400)
    check_call(dd, model, first)
    with pytest.raises(hip.FFQError) as ei:                  # 400 keys and 200 rows need 2048 slots: refused before any launch
        dev_select(dd, rand_keys(rng, 200))
    assert ei.value.code == hip.E_NOMEM and "32768 bytes" in str(ei.value)
    # ... and the set is as it was: the refused rows were never submitted
    check_call(dd, model, first[:50] + rand_keys(rng, 50))
    # arguments
    k = torch.zeros((16,), dtype=torch.int64, device="cuda")
    t = torch.zeros((4, 6), dtype=torch.int64, device="cuda")
    o = torch.zeros((5, 6), dtype=torch.int64, device="cuda")
    o2 = torch.zeros((5, 6), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    dd, model = fresh()

    def refused(*a, **kw):
        with pytest.raises(hip.FFQError) as ei:
            dd.select(*a, **kw)
        assert ei.value.code == hip.E_ARG

    refused(k.data_ptr(), 4, d_table1=t.data_ptr() + 8, d_out1=o.data_ptr())                 # tables are 16-byte aligned
    refused(k.data_ptr(), 4, d_table1=t.data_ptr(), d_out1=o.data_ptr() + 8)
    refused(k.data_ptr(), 4, d_table1=t.data_ptr(), d_table2=t.data_ptr(), d_out1=o.data_ptr(), d_out2=o2.data_ptr())    # no second keys
    refused(k.data_ptr(), 4, d_table1=t.data_ptr(), d_out1=t.data_ptr())                    # not the input table
    refused(k.data_ptr(), 4, d_table1=t.data_ptr())                                         # nowhere to put the rows
    refused(None, 4)
    refused(k.data_ptr(), -1)
    n_out, counts = ctypes.c_int64(), (ctypes.c_int64 * 6)()
    rc = hip.lib().ffq_dedup_select(None, k.data_ptr(), None, None, 4, None, None, None, None, None, ctypes.byref(n_out), 1, counts)
    assert rc == hip.E_ARG                                                                  # a NULL set
    # a scan pending on the context
    data = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, b"ACGT" * 9, b"I" * 36) for i in range(50))
    d2 = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    d_tab = torch.empty((64, 6), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.scan_submit(d2.data_ptr(), len(data), d_tab.data_ptr(), 64)
    try:
        refused(k.data_ptr(), 4)
        with pytest.raises(hip.FFQError) as ei:
            gpu_ctx.table_seq_keys(d2.data_ptr(), len(data), d_tab.data_ptr(), 4, k.data_ptr())
        assert ei.value.code == hip.E_ARG
    finally:
        gpu_ctx.scan_wait()
    with pytest.raises(hip.FFQError) as ei:                  # the table is 16-byte aligned
        gpu_ctx.table_seq_keys(d2.data_ptr(), len(data), d_tab.data_ptr() + 8, 4, k.data_ptr())
    assert ei.value.code == hip.E_ARG
    # the set is untouched by all of this, and the library's host statement agrees with the loop
    assert check_call(dd, model, [5, 5, 7])[:4] == [2, 1, 0, 2]
    for s in (b"", b"A", b"ACGTN" * 31, bytes(range(256))):
        assert hip.seq_key_host(s) == X.loop_key(s)
    assert hip.pair_key_host(5, 7) == X.loop_pair_key(5, 7) and hip.pair_key_host(0, 7) == 0

"""Duplicate removal on the device: ffq_table_seq_keys and ffq_dedup_select against the plain loops and the dict of
tests/dedup_expect.py.  Every comparison is exact: every key, the kept rows of both tables, d_idx, all six counts.  Coordinates:
a row minus `add` indexes the buffer the scanner saw; with a sentinel that buffer is b'\\n' + bytes.  The buffer lies at the END
of a device allocation of whole pages and begins at a multiple of 16, so that a read past its end leaves the allocation and a
sequence's address modulo 16 is what the table builder says it is."""
import ctypes
import functools

import numpy as np
import pytest

import dedup_expect as X
import grid_expect as GE


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


@pytest.mark.gpu
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


@pytest.mark.gpu
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


# ---- more rows than one pass of the grid (tests/grid_expect.py) -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def keys_pool():
    """(bytes, rows, idle, long, keys by the loop without and with a sentinel): a read of every length of LENGTHS at four
    addresses modulo 16, reads just above TILE and of a few thousand bases, empty reads, and the rows without a key -- wrapped
    (short and long), lines of two lengths, a FASTA row, rows that point outside"""
    rng = np.random.default_rng(29)
    buf, rows = bytearray(b"#"), []
    for n in LENGTHS:
        s = read_of(rng, n)
        for a in (0, 5, 10, 15):
            place(buf, rows, s, None, a)
    for n in (TILE + 1, TILE + 2, TILE + 3, 1000, 3001, 5000):
        place(buf, rows, read_of(rng, n), None, int(rng.integers(0, 16)))
    idle = [i for i, r in enumerate(rows) if r[3] == r[2]]
    good = [list(r) for r in rows]
    for src in (good[4 * 30], good[-2]):                                       # a short row and a long one, wrapped
        s = bytearray(buf[src[2]:src[3]])
        s[len(s) // 2] = 10
        idle.append(len(rows))
        place(buf, rows, bytes(s), None, 7)
    r = good[4 * 20]
    n0 = len(rows)
    rows.append(r[:5] + [r[5] - 1])
    rows.append(r[:4] + [-1, -1])
    rows.append([r[0], r[1], r[2], 1 << 40, r[4], r[4] + (1 << 40) - r[2]])
    rows.append([r[0], r[1], r[3], r[2], r[4], r[4] + r[2] - r[3]])
    rows.append([r[0], r[1], -5, -5 + r[3] - r[2], r[4], r[5]])
    rows.append([-1] * 6)
    idle += list(range(n0, len(rows)))
    buf, rows = finish(buf, rows)
    rows[n0 + 1, 4:] = -1                                                      # (finish moved them)
    rows[n0 + 5] = -1
    long = [i for i, r in enumerate(rows.tolist()) if i < n0 and r[3] - r[2] > TILE]
    keys = []
    for sentinel in (0, 1):
        seen = (b"\n" if sentinel else b"") + buf
        keys.append(np.array([X.row_key(seen, r, bool(sentinel)) for r in (rows + sentinel).tolist()], dtype=np.uint64))
    return buf, rows, tuple(idle), tuple(long), keys


def keys_table(arrangement, long_rows=False):
    _buf, rows, idle, long, _keys = keys_pool()
    if long_rows:
        return GE.long_idx(long, [i for i in range(len(rows)) if i not in long], seed=47)
    return GE.table_idx(arrangement, GE.n_above(GE.P_SHORT), GE.P_SHORT, len(rows), idle, seed=47)


def check_keys_above(dev, idx, sentinel, add, P, what):
    import torch
    _buf, rows, _idle, _long, keys = keys_pool()
    want = keys[sentinel][idx]
    t = torch.from_numpy(rows[idx] + sentinel + add).cuda()
    k = torch.full((len(idx) + 1,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    counts = dev.ctx.table_seq_keys(dev.ptr, dev.n, t.data_ptr(), len(idx), k.data_ptr(), sentinel=bool(sentinel), add=add)
    got = k.cpu().numpy()
    assert got[-1] == -7, "a key behind the last row was written"
    GE.same_rows(got[:-1].view(np.uint64), want, P, what)
    assert tuple(counts) == (int((want != X.KEY_NONE).sum()), int((want == X.KEY_NONE).sum())), what


@pytest.mark.parametrize("long_rows", (False, True))
def test_the_table_above_one_pass_is_what_the_loop_says(long_rows):
    buf, rows, idle, long, keys = keys_pool()
    lengths = rows[:, 3] - rows[:, 2]
    assert len(rows) < 300 and len(buf) < 1 << 20 and len(long) >= 6 and sorted(lengths[list(long)])[:3] == [TILE + 1, TILE + 1, TILE + 1]
    assert (keys[0][list(idle)] == X.KEY_NONE).sum() == 8 and (keys[1][list(idle)] == X.KEY_NONE).sum() == 7     # ([-1] * 6 + 1: an empty read)
    P = GE.P_LONG if long_rows else GE.P_SHORT
    for arrangement in ("random",) if long_rows else GE.ARRANGEMENTS:
        idx = keys_table(arrangement, long_rows)
        n = len(idx)
        assert (n == 2 * GE.N_LONG and int(np.isin(idx, long).sum()) == GE.N_LONG > 2 * 1024 * 4 and n >= 4096) if long_rows else n > 2 * 2048 * 32
        at = GE.sample_rows(n, P)
        for sentinel in (0, 1):
            seen = (b"\n" if sentinel else b"") + buf
            want = [X.row_key(seen, r, bool(sentinel)) for r in (rows[idx[at]] + sentinel).tolist()]
            assert len(at) >= 2000 and want == keys[sentinel][idx[at]].tolist()
        order = np.flatnonzero(np.isin(idx, long)) if long_rows else np.arange(n)
        for k, s in enumerate(GE.passes(len(order), P)):
            part = idx[order[s]]
            if (arrangement, k > 0) in (("late work", False), ("early work", True)):
                assert set(part.tolist()) <= set(idle)
            elif long_rows:
                assert set(part.tolist()) == set(long)
            else:
                assert (keys[0][part] == X.KEY_NONE).any() and (lengths[part] == 0).any() and (lengths[part] > TILE).any() and \
                    ((lengths[part] > 0) & (lengths[part] <= TILE)).any()


@pytest.mark.gpu
def test_more_rows_than_one_pass_of_the_grid(gpu_ctx):
    """three steps of every workgroup of k_seqkey_rows, the last for 1001 of the 2048 with five rows for the last of those: every
    key and both counts, in the three arrangements; "late work" with a sentinel and add = 1000003"""
    buf = keys_pool()[0]
    dev = Dev(gpu_ctx, buf)
    try:
        for arrangement in GE.ARRANGEMENTS:
            sentinel, add = (1, 1000003) if arrangement == "late work" else (0, 0)
            idx = keys_table(arrangement)
            assert len(idx) > 2 * 2048 * 32
            check_keys_above(dev, idx, sentinel, add, GE.P_SHORT, arrangement)
    finally:
        dev.close()


@pytest.mark.gpu
def test_more_long_rows_than_one_pass_of_the_grid(gpu_ctx):
    """9195 rows above TILE among as many others: the long launch's 1024 workgroups take three steps over the list"""
    buf, _rows, _idle, long, _keys = keys_pool()
    dev = Dev(gpu_ctx, buf)
    try:
        idx = keys_table("random", long_rows=True)
        assert int(np.isin(idx, long).sum()) > 2 * 1024 * 4 and len(idx) >= 4096
        check_keys_above(dev, idx, 0, 0, GE.P_SHORT, "long rows among short ones")
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


@pytest.mark.gpu
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


@pytest.mark.gpu
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


@pytest.mark.gpu
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


# ---- more rows than one pass of the grid: the set ---------------------------------------------------------------------------------
N_SET = GE.n_above(GE.P_WIDE)         # rows of either call: two steps of k_dedup_insert / k_dedup_resolve's 2048 workgroups of 256
P_TABLE = 4096 * 256                  # slots k_dedup_clear / k_dedup_rehash take in one pass


def np_pair_key(k1, k2):
    """X.loop_pair_key over arrays (uint64 arithmetic wraps as the loop's masks do)"""
    def sm(z):
        z = z ^ (z >> np.uint64(30))
        z = z * np.uint64(0xbf58476d1ce4e5b9)
        z = z ^ (z >> np.uint64(27))
        z = z * np.uint64(0x94d049bb133111eb)
        return z ^ (z >> np.uint64(31))
    with np.errstate(over="ignore"):
        k = sm(sm(k1) + k2)
    k[k == 0] = 1
    k[(k1 == X.KEY_NONE) | (k2 == X.KEY_NONE)] = X.KEY_NONE
    return k


@functools.lru_cache(maxsize=None)
def set_calls(pairs=False):
    """[(keys 1, keys 2 or None)] of two calls of N_SET rows on a set made for no keys at all.  Call 1: 560 000 distinct keys,
    copies of some of them, rows without a key -- the set grows from 1024 to 2^21 slots (k_dedup_clear strides).  Call 2: 200 000
    new keys, 50 000 more that come twice in this call, copies of call 1's keys, rows without a key -- 2^21 to 2^22
    (k_dedup_rehash strides over more than 2^20 slots).  Every call is shuffled, so every kind lies in every pass and a key's
    second copy often belongs to a workgroup that runs before the one of its first."""
    rng = np.random.default_rng(53)
    n_none = 11095

    def fresh_keys(m):
        return rng.integers(1, 1 << 63, m, dtype=np.uint64) | np.uint64(1)
    d1 = fresh_keys(560000)
    call1 = np.concatenate([d1, d1[rng.integers(0, len(d1), N_SET - len(d1) - n_none)], np.zeros(n_none, dtype=np.uint64)])
    new, twice = fresh_keys(200000), fresh_keys(50000)
    call2 = np.concatenate([new, twice, twice, d1[rng.integers(0, len(d1), N_SET - 300000 - n_none)], np.zeros(n_none, dtype=np.uint64)])
    out = []
    for c in (call1, call2):
        rng.shuffle(c)
        assert len(c) == N_SET
        # (pairs: mate 2's key is drawn from a few values, so that equal mate 1 keys make equal and unequal pairs)
        out.append((c, (rng.integers(1, 4, N_SET).astype(np.uint64) * np.uint64(977)) if pairs else None))
    return out


def test_the_calls_above_one_pass_are_what_they_should_be():
    assert N_SET == 601095 and N_SET > 2048 * 256 and (1 << 21) > P_TABLE
    for pairs in (False, True):
        model = X.LoopSet(0)
        seen = set()
        for c, (k1, k2) in enumerate(set_calls(pairs)):
            eff = k1 if k2 is None else np_pair_key(k1, k2)
            if k2 is not None:
                at = GE.sample_rows(N_SET, GE.P_WIDE)
                assert len(at) >= 2000 and [X.loop_pair_key(a, b) for a, b in zip(k1[at].tolist(), k2[at].tolist())] == eff[at].tolist()
            kept, counts = model.select(eff.tolist(), True)
            assert counts[4] == 1 << (21 + c) and counts[5] == c + 1 and counts[0] + counts[1] == N_SET
            is_kept = np.zeros(N_SET, dtype=bool)
            is_kept[kept] = True
            for s in GE.passes(N_SET, GE.P_WIDE):                            # every kind in every pass
                e = eff[s]
                assert (e == X.KEY_NONE).sum() > 100 and (~is_kept[s]).sum() > 1000 and (is_kept[s] & (e != X.KEY_NONE)).sum() > 1000
            if c == 1:
                # a key of THIS call alone with two copies: the first in pass 1 and the second in pass 2 in an EARLIER workgroup's
                # place; both in pass 2
                fresh = ~np.isin(eff, np.fromiter(seen, dtype=np.uint64, count=len(seen))) & (eff != X.KEY_NONE)
                order = np.argsort(eff[fresh], kind="stable")
                pos, key = np.flatnonzero(fresh)[order], eff[fresh][order]
                two = (key[:-1] == key[1:]) & np.concatenate([[True], key[1:-1] != key[:-2]])      # a key's first two copies
                i, j = pos[:-1][two], pos[1:][two]
                P = GE.P_WIDE
                assert ((i < P) & (j >= P) & ((j - P) // 256 < i // 256)).sum() > 100 and ((i >= P) & (j > i)).sum() > 100
                assert (~is_kept[j]).all() and is_kept[i].all()
            seen.update(eff.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("drop,pairs", ((True, False), (False, False), (True, True)))
def test_more_rows_than_one_pass_of_the_grid_in_the_set(fresh, drop, pairs):
    """two calls of 601 095 rows on a set made for no keys: two steps of the insert and the resolve, the clear striding over
    2^21 slots and the rehash over 2^21 old ones; kept rows, d_idx and all six counts against the dict"""
    dd, model = fresh(0)
    for c, (k1, k2) in enumerate(set_calls(pairs)):
        eff = k1 if k2 is None else np_pair_key(k1, k2)
        kept, counts = model.select(eff.tolist(), drop)
        idx, got, gc, tabs, k = dev_select(dd, k1, k2, None, 2 if pairs else 1, drop)
        assert gc == counts, (c, gc, counts)
        assert gc[4] == 1 << (21 + c) and gc[5] == c + 1 and k == len(kept)
        GE.same_kept(idx, kept, GE.P_WIDE, "call %d" % (c + 1))
        for t, g in zip(tabs, got):
            GE.same_rows(g, t[kept], GE.P_WIDE, "call %d: the kept rows (row: among the kept)" % (c + 1))


@pytest.mark.gpu
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


@pytest.mark.gpu
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

"""The stable compaction behind every selecting table call (csrc/ffq_compact.h), through its four front doors on ONE table and
ONE keep set: ffq_table_select_seqlen_idx, ffq_table_select_reads, ffq_table_select_pairs and ffq_dedup_select must all hand
back the same rows, the same ordinals and the same count -- the host's list.

The table is hand-made: four-line records in a buffer, every row at positions of its own, so a row says which it is.  A kept
row has KEEP_LEN bases and no N; a dropped one is too short or too long AND holds an N: the length bounds pick the set, and so
does the content rule max_n = 0.  The set has kept and dropped rows on both sides of every edge of a wave (64 rows) and of a
block (256 rows).  Sizes: around a wave, around a block, several blocks and a row."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 3 * 256 + 1)
KEEP_LEN = 12
FILL = -7
RULES = dict(qual_base=33, max_n=0, min_mean_qual=0, qualified_qual=15, max_unqualified_pct=-1, min_complexity_pct=0, max_ee_micro=-1)
SEEN, MATE2 = 7, 5           # the key the dedup set holds before the call: every dropped row has it; with two tables every
                             # row's second key, which makes pair keys of them


def kept_row(i):
    """last row of a wave kept, the one before dropped; first row of a wave kept, the next dropped; a mix between"""
    edge = {62: False, 63: True, 0: True, 1: False}
    return edge.get(i % 64, (i * 7 + i // 64) % 5 < 2)


@pytest.fixture(scope="module")
def world():
    """(buffer bytes, int64[n][6] rows, bool[n] keep) for the largest size; a smaller size takes the first rows"""
    n = max(SIZES)
    buf, rows, keep = bytearray(b"#"), [], []
    for i in range(n):
        k = kept_row(i)
        ln = KEEP_LEN if k else (KEEP_LEN - 6, KEEP_LEN + 8)[i % 2]
        seq = bytearray(b"ACGT"[(i + j) % 4] for j in range(ln))
        if not k:
            seq[i % ln] = ord("N")
        p0 = len(buf)
        buf += b"@r%d\n" % i
        p2 = len(buf)
        buf += bytes(seq) + b"\n+\n"
        p4 = len(buf)
        buf += b"I" * ln + b"\n"
        rows.append([p0, p2 - 1, p2, p2 + ln, p4, p4 + ln])
        keep.append(k)
    keep = np.array(keep)
    for e in range(64, n - 1, 64):
        for side in (keep[e - 2:e], keep[e:e + 2]):
            assert side.any() and not side.all()
    return bytes(buf), np.array(rows, dtype=np.int64), keep


class Case:
    """the first n rows on the device, and the outputs of a call: filled, a row longer than the table"""

    def __init__(self, world, n):
        import torch
        self.torch = torch
        buf, rows, keep = world
        self.n, self.rows = n, rows[:n]
        self.kept = np.flatnonzero(keep[:n])
        self.n_bytes = len(buf)
        self.d_buf = torch.from_numpy(np.frombuffer(buf + bytes(64), dtype=np.uint8).copy()).cuda()
        self.d_table = self.dev(self.rows)

    def dev(self, a):
        a = np.ascontiguousarray(a, dtype=np.int64)
        return self.torch.from_numpy(a.copy()).cuda() if a.size else self.torch.zeros((6,), dtype=self.torch.int64, device="cuda")

    def outputs(self, n_tables):
        t = self.torch
        outs = [t.full((self.n + 1, 6), FILL, dtype=t.int64, device="cuda") for _ in range(n_tables)]
        idx = t.full((self.n + 1,), FILL, dtype=t.int64, device="cuda")
        t.cuda.synchronize()
        return outs, idx

    def check(self, k, outs, idx, ordinals=None):
        """the count, the kept rows of every table, their ordinals; nothing written behind them"""
        want = self.kept if ordinals is None else ordinals
        assert k == len(self.kept)
        for o in outs:
            h = o.cpu().numpy()
            assert (h[:k] == self.rows[self.kept]).all()
            assert (h[k:] == FILL).all(), "rows behind the kept ones were written"
        if idx is not None:
            h = idx.cpu().numpy()
            assert h[:k].tolist() == [int(j) for j in want]
            assert (h[k:] == FILL).all(), "ordinals behind the kept ones were written"


@pytest.mark.parametrize("n", SIZES)
def test_every_front_door_keeps_the_host_list(gpu_ctx, world, n):
    from fastqandfurious_amd import hip
    c = Case(world, n)
    rules = hip.ContentRulesStruct(*(RULES[name] for name, _ in hip.ContentRulesStruct._fields_))
    table, buf = c.d_table.data_ptr(), c.d_buf.data_ptr()
    n_kept, n_drop = len(c.kept), n - len(c.kept)

    # by length, read from the table
    (out,), idx = c.outputs(1)
    k = gpu_ctx.table_select_seqlen_idx(table, n, KEEP_LEN, KEEP_LEN, out.data_ptr(), idx.data_ptr())
    c.check(k, [out], idx)

    # by content, read from the verdict bytes (no length bound: the N alone drops a row)
    (out,), idx = c.outputs(1)
    k, counts = gpu_ctx.table_select_reads(buf, c.n_bytes, table, n, out.data_ptr(), rules=rules, d_idx=idx.data_ptr(), sentinel=False, add=0)
    c.check(k, [out], idx)
    assert counts[0] == n_kept and sum(counts[1:7]) == n_drop and counts[7] == 0

    # the table paired with itself: mate 1 judged by content, mate 2 by its length; both fail or neither, so every mode agrees
    view = hip.table_view(buf, c.n_bytes, table, sentinel=False, add=0)
    for mode in ("any", "both", "first"):
        outs, idx = c.outputs(2)
        k, _h1, _h2, pairs = gpu_ctx.table_select_pairs(view, view, n, outs[0].data_ptr(), outs[1].data_ptr(), rules1=rules,
                                                        min_len=(None, KEEP_LEN), max_len=(None, KEEP_LEN), pair_filter=mode,
                                                        d_idx=idx.data_ptr())
        c.check(k, outs, idx)
        assert pairs == [n_kept, n_drop, n_drop if mode == "first" else 0, 0, 0 if mode == "first" else n_drop]

    # by key: a kept row's key is new, a dropped row's is in the set already.  Straight, and through a permutation: row i of
    # the call has the key at ord[i] and hands back ord[i]
    perm = np.random.default_rng(n).permutation(n)
    for ord_ in (None, perm):
        keys = np.zeros(max(n, 1), dtype=np.int64)
        at = np.arange(n) if ord_ is None else ord_
        keys[at] = SEEN
        keys[at[c.kept]] = 1000 + c.kept
        d_keys, d_ord, d_seen = c.dev(keys), None if ord_ is None else c.dev(ord_), c.dev([SEEN])
        d_keys2 = c.dev(np.full(max(n, 1), MATE2))
        for n_tables in (0, 1, 2):
            dd = hip.Dedup(gpu_ctx)
            try:
                k2 = d_keys2.data_ptr() if n_tables == 2 else None           # (a second table needs a second mate's keys)
                assert dd.select(d_seen.data_ptr(), 1, k2)[0] == 1
                outs, idx = c.outputs(n_tables)
                t = [table] * n_tables + [None, None]
                o = [x.data_ptr() for x in outs] + [None, None]
                k, counts = dd.select(d_keys.data_ptr(), n, k2, d_ord.data_ptr() if d_ord is not None else None, t[0], t[1], o[0], o[1],
                                      idx.data_ptr())
            finally:
                dd.close()
            c.check(k, outs, idx, ordinals=at[c.kept])
            assert counts[:3] == [n_kept, n_drop, 0]

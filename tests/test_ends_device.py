"""Fixed trims and sliding-window quality cutting by editing rows of the offset table on the device: ffq_table_trim_ends.

The expectation of every test is the loop of tests/ends_expect.py -- the rule as include/ffq.h states it, written out there --
never the package's own host implementation.  Coordinates: a row minus `add` indexes the buffer the scanner saw; with a
sentinel that buffer is b'\\n' + bytes.
"""
import functools

import numpy as np
import pytest

import ends_expect as E
import grid_expect as GE


@pytest.fixture(scope="module")
def F(pkg):
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


def device_ends(ctx, F, data, rows, r, qual_base=33, sentinel=False, add=0, in_place=False):
    """rows (int64[n][6]) through ffq_table_trim_ends over `data` (bytes) -> (rows, stats)"""
    import torch
    dbuf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 6)).cuda()
    out = t if in_place else torch.full_like(t, -77)
    stats = ctx.table_trim_ends(dbuf.data_ptr(), dbuf.numel(), t.data_ptr(), t.shape[0], E.pkg_rules(F, r), qual_base,
                                d_out=out.data_ptr(), sentinel=sentinel, add=add)
    return out.cpu().numpy(), list(stats)


def same(got, want, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, bad.size, bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(E.SETTINGS))
def test_hand_table_device(gpu_ctx, F, setting):
    r = E.SETTINGS[setting]
    buf, rows, names = E.hand_table()
    rows = np.array(rows, dtype=np.int64)
    want, stats, _spans = E.loop_rows(buf, rows, r)
    assert stats[2] == len(names)
    for in_place in (False, True):
        got, gstats = device_ends(gpu_ctx, F, buf, rows, r, in_place=in_place)
        same(got, want, (setting, in_place))
        assert gstats == stats
        # add != 0, and with a sentinel: the rows index b"\n" + bytes
        got, gstats = device_ends(gpu_ctx, F, buf, rows + 1000, r, add=1000, in_place=in_place)
        assert (got == want + 1000).all() and gstats == stats
        w2, s2, _l = E.loop_rows(b"\n" + buf, rows + 1, r)
        assert (w2 == want + 1).all() and s2 == stats
        got, gstats = device_ends(gpu_ctx, F, buf, rows + 1, r, sentinel=True, add=0, in_place=in_place)
        assert (got == want + 1).all() and gstats == stats
        got, gstats = device_ends(gpu_ctx, F, buf, rows + 1001, r, sentinel=True, add=1000, in_place=in_place)
        assert (got == want + 1001).all() and gstats == stats
    assert device_ends(gpu_ctx, F, buf, np.zeros((0, 6), dtype=np.int64), r)[1] == [0, 0, 0]


@pytest.mark.gpu
def test_the_hand_values_device(gpu_ctx, F):
    """every hand line under its own rules"""
    buf, rows, _names = E.hand_table()
    for i, (text, r, want) in enumerate(E.HAND):
        got, gstats = device_ends(gpu_ctx, F, buf, [rows[i]], r)
        assert (int(got[0, 4] - rows[i][4]), int(got[0, 5] - rows[i][4])) == want, (text, r, got.tolist())
        assert (int(got[0, 2] - rows[i][2]), int(got[0, 3] - rows[i][2])) == want
        n = len(text)
        assert gstats == [int(want[1] - want[0] != n), n - (want[1] - want[0]), 0]
    # with a sentinel, coordinate 0 is the virtual newline: a quality line that begins there is left alone, an empty one is not skipped
    data = b"#" * 30 + b"\n"
    sub = np.array([[0, 1, 14, 26, 0, 12], [0, 1, 14, 26, 1, 13], [0, 1, 5, 5, 0, 0]], dtype=np.int64)
    want, stats, _l = E.loop_rows(b"\n" + data, sub, E.ALL3)
    assert stats == [1, 12, 1] and (want[0] == sub[0]).all()
    got, gstats = device_ends(gpu_ctx, F, data, sub, E.ALL3, sentinel=True, add=0)
    assert (got == want).all() and gstats == stats


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(E.SETTINGS))
def test_seeded_table_device(gpu_ctx, F, setting):
    buf, rows = E.seeded_table()
    want, stats, _spans = E.seeded_want(setting)
    got, gstats = device_ends(gpu_ctx, F, buf, rows, E.SETTINGS[setting])
    same(got, want, setting)
    assert gstats == stats
    got, gstats = device_ends(gpu_ctx, F, buf, rows, E.SETTINGS[setting], in_place=True)
    assert (got == want).all() and gstats == stats
    got, gstats = device_ends(gpu_ctx, F, buf, np.array(rows, dtype=np.int64) + 1001, E.SETTINGS[setting], sentinel=True, add=1000)
    assert (got == want + 1001).all() and gstats == stats


@pytest.mark.gpu
def test_another_qual_base_device(gpu_ctx, F):
    buf, rows = E.seeded_table()
    r = E.Rules(front=(5, 3), right=(7, 2), tail=(3, 4))
    want, stats, _spans = E.loop_rows(buf, rows[:1200], r, qual_base=64)      # (the values go negative)
    got, gstats = device_ends(gpu_ctx, F, buf, rows[:1200], r, qual_base=64)
    same(got, want, "qual_base 64")
    assert gstats == stats and stats[0] > 100


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", (1, 31, 32, 33))
def test_row_counts_around_one_workgroup_step(gpu_ctx, F, n_rows):
    buf, rows = E.seeded_table()
    want = E.seeded_want("all three")[0]
    first = 480                                       # (into the first run of ineligible rows)
    got, gstats = device_ends(gpu_ctx, F, buf, np.array(rows[first:first + n_rows], dtype=np.int64).reshape(-1, 6), E.ALL3)
    assert (got == want[first:first + n_rows]).all()
    assert gstats == E.loop_rows(buf, rows[first:first + n_rows], E.ALL3)[1]


@pytest.mark.gpu
@pytest.mark.parametrize("stage", ("front", "right", "tail"))
def test_the_decisive_window_on_the_chunk_edges(gpu_ctx, F, stage):
    """200-byte rows whose cut lies at every offset 50..80 and 118..138, for windows {1, 4, 8, 9, 63, 64}"""
    buf, rows, what = E.edge_table(stage)
    for W in E.EDGE_WINDOWS:
        sub = np.array([r for r, w in zip(rows, what) if w[1] == W], dtype=np.int64)
        want, stats, _spans = E.loop_rows(buf, sub, E.edge_rules(stage, W))
        got, gstats = device_ends(gpu_ctx, F, buf, sub, E.edge_rules(stage, W))
        same(got, want, (stage, W))
        assert gstats == stats and stats[0] == len(sub)
        # the other two stages beside it, with windows of their own
        r = E.edge_rules(stage, W)._replace(**{s: (5, 12) for s in ("front", "right", "tail") if s != stage})
        want, stats, _spans = E.loop_rows(buf, sub, r)
        got, gstats = device_ends(gpu_ctx, F, buf, sub, r)
        same(got, want, (stage, W, "all three"))
        assert gstats == stats


@pytest.mark.gpu
def test_long_rows_device(gpu_ctx, F):
    buf, rows, names = E.long_table()
    assert sum(1 for r in rows if r[5] - r[4] > E.LONG) >= 24 and sum(1 for r in rows if r[5] - r[4] <= 220) >= 40
    for setting in ("front", "right", "tail", "all three", "window 64", "window 1", "fixed"):
        r = E.SETTINGS[setting]
        want, stats, _spans = E.loop_rows(buf, rows, r)
        assert stats[2] == 1
        for in_place in (False, True):
            got, gstats = device_ends(gpu_ctx, F, buf, rows, r, in_place=in_place)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (setting, [names[i] for i in bad], got[bad].tolist(), want[bad].tolist())
            assert gstats == stats


# ---- more rows than one pass of the grid (tests/grid_expect.py) -------------------------------------------------------------
GRID_SETTINGS = ("all three", "window 64", "fixed")


@functools.lru_cache(maxsize=None)
def grid_parts(setting, sentinel=False, add=0):
    """the loop's answer for every pool row ALONE: (rows in, rows out, [changed, bases removed, skipped] each)"""
    buf, rows, _idle, _long = E.grid_pool()
    seen, shift = (b"\n" if sentinel else b"") + buf, add + (1 if sentinel else 0)
    rows = np.array(rows, dtype=np.int64) + shift
    per = [E.loop_rows(seen, [r], E.SETTINGS[setting], add=add) for r in rows]
    return rows, np.array([w[0] for w, _s, _l in per], dtype=np.int64), np.array([s for _w, s, _l in per], dtype=np.int64)


def grid_table(arrangement, setting, sentinel=False, add=0, long_rows=False):
    """(rows in, rows out, stats, idx) of pool[idx]"""
    _buf, rows, idle, long = E.grid_pool()
    if long_rows:
        idx = GE.long_idx(long, [i for i in range(len(rows)) if i not in long], seed=43)
    else:
        idx = GE.table_idx(arrangement, GE.n_above(GE.P_SHORT), GE.P_SHORT, len(rows), idle, seed=43)
    rin, rout, stats = grid_parts(setting, sentinel, add)
    return rin[idx], rout[idx], stats[idx].sum(axis=0).tolist(), idx


@pytest.mark.parametrize("long_rows", (False, True))
def test_the_table_above_one_pass_is_what_the_loop_says(long_rows):
    buf, rows, idle, long = E.grid_pool()
    lengths = np.array([r[5] - r[4] for r in rows])
    assert len(rows) < 400 and len(buf) < 1 << 20 and {E.LONG, E.LONG + 1} <= set(lengths.tolist()) and len(long) >= 6
    assert (lengths[list(long)] > E.LONG).all() and max(lengths) <= 5000
    for setting in GRID_SETTINGS:                       # (an idle row has nothing to do under any of them)
        assert (grid_parts(setting)[2][list(idle)][:, :2] == 0).all()
    P = GE.P_LONG if long_rows else GE.P_SHORT
    for arrangement in ("random",) if long_rows else GE.ARRANGEMENTS:
        for setting, sentinel, add in (("all three", False, 0), ("window 64", True, 500)):
            rin, rout, stats, idx = grid_table(arrangement, setting, sentinel, add, long_rows)
            n = len(idx)
            assert (n == 2 * GE.N_LONG and int(np.isin(idx, long).sum()) == GE.N_LONG > 2 * 1024 * 4 and n >= 4096) if long_rows else n > 2 * 2048 * 32
            _r, _rout1, stats1 = grid_parts(setting, sentinel, add)
            # the expansion against the loop over the table's own rows
            at = GE.sample_rows(n, P, 300)
            want, wstats, _l = E.loop_rows((b"\n" if sentinel else b"") + buf, rin[at], E.SETTINGS[setting], add=add)
            GE.same_rows(rout[at], want, P, "rows")
            assert stats1[idx[at]].sum(axis=0).tolist() == wstats
            # what every pass holds: changed rows, skipped rows, rows left as they are
            order = np.flatnonzero(np.isin(idx, long)) if long_rows else np.arange(n)        # (the list's entries, in row order)
            for k, s in enumerate(GE.passes(len(order), P)):
                part = idx[order[s]]
                c = stats1[part].sum(axis=0)
                if (arrangement, k > 0) in (("late work", False), ("early work", True)):
                    assert c[0] == c[1] == 0 and c[2] > 0 and set(part.tolist()) <= set(idle)
                else:
                    assert (c[:2] > 0).all() and (c[2] > 0 or long_rows) and (stats1[part][:, 0] == 0).any(), (arrangement, k, c)
                    assert long_rows or ((lengths[part] == 0).any() and (lengths[part] > E.LONG).any())


@pytest.mark.gpu
@pytest.mark.parametrize("setting", GRID_SETTINGS)
def test_more_rows_than_one_pass_of_the_grid(gpu_ctx, F, setting):
    """three steps of every workgroup, the last for 1001 of the 2048 with five rows for the last of those; every row and the
    three counts, out of place and in place; "late work" with a sentinel and add = 500"""
    buf = E.grid_pool()[0]
    for arrangement in GE.ARRANGEMENTS:
        sentinel, add = (True, 500) if arrangement == "late work" else (False, 0)
        rin, want, stats, idx = grid_table(arrangement, setting, sentinel, add)
        assert len(idx) > 2 * 2048 * 32
        for in_place in (False, True):
            got, gstats = device_ends(gpu_ctx, F, buf, rin, E.SETTINGS[setting], sentinel=sentinel, add=add, in_place=in_place)
            GE.same_rows(got, want, GE.P_SHORT, "%s, in place %s" % (arrangement, in_place))
            assert gstats == stats, (arrangement, in_place)


@pytest.mark.gpu
@pytest.mark.parametrize("setting", GRID_SETTINGS[:2])
def test_more_long_rows_than_one_pass_of_the_grid(gpu_ctx, F, setting):
    """9195 rows above LONG among as many short ones: the long launch's 1024 workgroups take three steps over the list"""
    buf, _rows, _idle, long = E.grid_pool()
    rin, want, stats, idx = grid_table("random", setting, long_rows=True)
    is_long = np.isin(idx, long)
    assert int(is_long.sum()) > 2 * 1024 * 4 and len(idx) >= 4096
    for in_place in (False, True):
        got, gstats = device_ends(gpu_ctx, F, buf, rin, E.SETTINGS[setting], in_place=in_place)
        GE.same_rows(got[is_long], want[is_long], GE.P_LONG, "long rows (list entries), in place %s" % in_place)
        GE.same_rows(got, want, GE.P_SHORT, "all rows, in place %s" % in_place)
        assert gstats == stats


@pytest.mark.gpu
def test_argument_errors_device(gpu_ctx, F):
    import torch
    from fastqandfurious_amd import hip
    buf, rows, _names = E.hand_table()
    dbuf = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).cuda()
    t = torch.from_numpy(np.array(rows, dtype=np.int64)).cuda()
    raw = torch.zeros(t.numel() + 1, dtype=torch.int64, device="cuda")
    S = hip.EndsRulesStruct

    def call(rules, **kw):
        return gpu_ctx.table_trim_ends(dbuf.data_ptr(), dbuf.numel(), t.data_ptr(), t.shape[0], rules, d_out=raw.data_ptr(), sentinel=False,
                                       add=0, **kw)
    good = dict(trim_front=0, trim_tail=0, keep_len=0, qual_base=33, front_window=4, front_quality=20, right_window=0, right_quality=0,
                tail_window=0, tail_quality=0)
    for bad in (dict(front_window=65), dict(front_window=-1), dict(right_window=65, right_quality=20), dict(tail_window=4, tail_quality=0),
                dict(tail_window=4, tail_quality=94), dict(front_quality=0), dict(front_quality=94), dict(trim_front=-1), dict(trim_tail=-1),
                dict(keep_len=-1), dict(qual_base=-1), dict(qual_base=256), dict(front_window=0)):
        with pytest.raises(hip.FFQError, match="ffq_table_trim_ends"):
            call(S(**dict(good, **bad)))
    with pytest.raises(hip.FFQError, match="ffq_table_trim_ends"):
        call(None)
    with pytest.raises(hip.FFQError, match="16-byte aligned"):
        gpu_ctx.table_trim_ends(dbuf.data_ptr(), dbuf.numel(), t.data_ptr(), t.shape[0], S(**good), d_out=raw.data_ptr() + 8)
    # a scan pending on the context
    data = E.fastq(E.single_records()[:50])
    d2 = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    t2 = torch.empty((64, 6), dtype=torch.int64, device="cuda")
    gpu_ctx.scan_submit(d2.data_ptr(), len(data), t2.data_ptr(), 64)
    try:
        with pytest.raises(hip.FFQError) as e:
            call(S(**good))
        assert e.value.code == hip.E_ARG and "pending" in str(e.value)
    finally:
        gpu_ctx.scan_wait()
    # the quality of a window that is off is not looked at; the C ABI's own struct passes as it is
    want, stats, _l = E.loop_rows(buf, rows, E.FRONT)
    assert list(call(S(**dict(good, right_quality=500, tail_quality=-3)))) == stats
    assert (raw[:t.numel()].cpu().numpy().reshape(-1, 6) == want).all()

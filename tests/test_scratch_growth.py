"""Scans and table calls on a context whose scratch has JUST been reallocated.

The session's shared context grows once and stays large: no other test scans on a context that regrew a moment ago.
The context owns its scratch in self-freeing buffers (csrc/ffq_mem.h) and hands the kernels raw-pointer views of them
(ChainBufs, RankBufs: csrc/ffq_hip.hip); a view that still pointed at the block a regrow freed would show here and
nowhere else.  So: a NEW context, a small input (small scratch), a large one (every tile-sized and record-sized buffer
regrows), the small one again -- each scan compared with the oracle by World.same (tests/test_input_memory.py: rows, end
state, offsets, every decoded byte), and forget() in between, so that each starts on the tier a fresh context takes.
"""
import numpy as np
import pytest

from test_gather import device_gather, loop_gather
from test_input_memory import TILE, World
from test_render import device_render, loop_render
from test_trim import device_trim, loop_rows

pytestmark = pytest.mark.gpu

KINDS = ("four", "tiny", "wrap", "wrap80", "long", "longline", "mess")
MODES = (1, 2, 3)
TINY_LARGE = 70000               # records: more than the 65536-element floor of the table utilities' scratch (grow_dev)


@pytest.fixture(scope="module")
def world(oracle, pkg):
    from fastqandfurious_amd import hip
    w = World(oracle, hip)
    big = b"".join(b"@r%d\nACGT\n+\nIIII\n" % i for i in range(TINY_LARGE))            # "tiny", more of it
    w.data["tiny70k"] = np.frombuffer(big, dtype=np.uint8)
    w.decoded["tiny70k"] = (w.data["tiny70k"].view(np.int8) - 33).astype(np.int8)
    return w


def grow_and_shrink(world, ctx, kind):
    """two-tile prefix, the whole input, the prefix again; in every mode"""
    size = world.data[kind].size
    assert 4 * TILE < size < 10 << 20
    cut = size - 2 * TILE - 100
    for mode in MODES:
        for c in (cut, 0, cut):
            ctx.forget()
            try:
                world.same(ctx, kind, mode, c)
            except AssertionError as e:
                raise AssertionError("%s, mode %d, %d bytes: %s" % (kind, mode, size - c, e)) from None


@pytest.mark.parametrize("kind", KINDS)
def test_scans_around_a_regrow(world, kind):
    ctx = world.hip.Context(0)
    try:
        grow_and_shrink(world, ctx, kind)
    finally:
        ctx.close()


def test_scans_around_a_regrow_on_a_shared_stream(world):
    """... on a context that uses another one's stream (ffq_ctx_create_shared); the child is closed first, and the parent
    scans after that"""
    hip = world.hip
    parent = hip.Context(0)
    try:
        child = hip.Context(share=parent)
        try:
            world.same(parent, "wrap", 2, world.data["wrap"].size - 2 * TILE - 100)
            grow_and_shrink(world, child, "wrap")
            grow_and_shrink(world, child, "four")
        finally:
            child.close()
        parent.forget()
        world.same(parent, "wrap", 2)
        world.same(parent, "four", 3)
    finally:
        parent.close()


def _select(ctx, oracle, rows):
    """ffq_table_select_seqlen_idx == the oracle's filter and the ordinals of the rows it keeps (every read of "tiny" has 4 bases)"""
    import torch
    n = rows.shape[0]
    t = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    lens = rows[:, 3] - rows[:, 2]
    for lo, hi in ((4, 4), (5, 1 << 62), (-(1 << 62), 3)):
        out = torch.full((n, 6), -7, dtype=torch.int64, device="cuda")
        idx = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        k = ctx.table_select_seqlen_idx(t.data_ptr(), n, lo, hi, out.data_ptr(), idx.data_ptr())
        exp = oracle.select_seqlen(rows, lo, hi)
        assert k == len(exp) and (out[:k].cpu().numpy() == exp).all(), (n, lo, hi)
        assert (idx[:k].cpu().numpy() == np.nonzero((lens >= lo) & (lens <= hi))[0]).all(), (n, lo, hi)
        assert (out[k:] == -7).all() and (idx[k:] == -7).all(), (n, lo, hi)


def _gather(ctx, data, rows):
    for which in ("header", "quality"):
        want, off = loop_gather(data, rows, which, -33 if which == "quality" else 0)
        rc, need, got, goff = device_gather(ctx, data, rows, which, value_add=-33 if which == "quality" else 0)
        assert rc == 0 and need == len(want) and goff.tolist() == off and (got == want).all(), (len(rows), which)


def _trim(ctx, data, rows):
    for cf, cb in ((0, 41), (0, 20)):           # every quality of "tiny" is 40: all of a read goes, or none of it
        want, stats = loop_rows(data, rows, cf, cb)
        got, gstats = device_trim(ctx, data, rows, cf, cb)
        assert (got == want).all() and gstats == stats, (len(rows), cf, cb, gstats, stats)


def _render(ctx, data, rows):
    want, off, stats = loop_render(data, rows)
    rc, text, goff, gstats = device_render(ctx, data, rows)
    assert rc == 0 and gstats == stats and goff.tolist() == off and text == want, (len(rows), gstats, stats)


@pytest.mark.parametrize("call", ("select", "gather", "trim", "render"))
def test_table_utilities_around_a_regrow(world, oracle, call):
    """Each table call on a context of its own: about 1000 rows of "tiny", then all 30000 -- the per-record scratch of the
    gather (p4s, qdir) regrows; the row lists of the trim and the render lie behind grow_dev's 65536-element floor and
    regrow only with the 70000-record input, which those two get as well."""
    w = world.expected("tiny")
    cut = world.data["tiny"].size - int(w.in_buf[1000, 0])          # (the first 1000 records, whole)
    inputs = [("tiny", cut, 1000), ("tiny", 0, 30000)] + ([("tiny70k", 0, TINY_LARGE)] if call in ("trim", "render") else [])
    ctx = world.hip.Context(0)
    try:
        for kind, c, n in inputs:
            ctx.forget()
            world.same(ctx, kind, 1, c)                              # the scan: the table is the oracle's (asserted)
            rows = world.expected(kind, c).in_buf
            assert rows.shape[0] == n
            if call == "select":
                _select(ctx, oracle, rows)
            else:
                {"gather": _gather, "trim": _trim, "render": _render}[call](ctx, world.view(kind, c).tobytes(), rows)
    finally:
        ctx.close()

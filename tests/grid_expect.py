"""What the tests named ..._than_one_pass_of_the_grid share: a kernel under a capped grid strides by one
PASS of P rows (workgroups x rows per workgroup) and carries state from step to step -- prefetched rows, counters, LDS that is
set up once -- which a table below P never exercises.  No package code in here.

The table is pool[idx]: a pool of a few hundred distinct rows whose expectation the module's own plain loop gives once per
pool row, and a seeded idx of length n > P through which numpy expands it.  Three arrangements:
    "random"      idx drawn from the whole pool: the row a workgroup meets in pass k differs from the one it met in pass k - 1
    "late work"   rows [0, P) drawn from the pool's IDLE rows (nothing to do: empty or ineligible), the whole pool behind them
    "early work"  the reverse: the whole pool in [0, P), idle rows behind
A workgroup that leaves its loop early, or drops what it counted after its first step, shows in the last two even where
"random" averages it away.
"""
import numpy as np

ARRANGEMENTS = ("random", "late work", "early work")
P_SHORT = 2048 * 32           # one pass of the row kernels with a group of lanes per row: 2048 workgroups of 32 rows
P_WIDE = 2048 * 256           # ... of those with a lane per row


def n_above(P):
    """P_SHORT: three steps, the last one with rows for the first 1001 workgroups only, and five rows (a partial wave) for
    the last of those.  P_WIDE: two steps, the second for 301 workgroups, seven rows for the last."""
    assert P in (P_SHORT, P_WIDE)
    n = 2 * P + 1000 * 32 + 5 if P == P_SHORT else P + 300 * 256 + 7
    assert n > (2 if P == P_SHORT else 1) * P and (n % P) % (32 if P == P_SHORT else 256) in (5, 7)
    return n


def table_idx(arrangement, n, P, n_pool, idle, seed):
    """idx[n] into a pool of n_pool rows, `idle` the pool rows with nothing to do"""
    assert arrangement in ARRANGEMENTS and n > P and len(idle) > 0
    rng = np.random.default_rng([seed, ARRANGEMENTS.index(arrangement)])
    idx = rng.integers(0, n_pool, n)
    lazy = np.asarray(idle)[rng.integers(0, len(idle), n)]
    if arrangement == "late work":
        idx[:P] = lazy[:P]
    elif arrangement == "early work":
        idx[P:] = lazy[P:]
    return idx


P_LONG = 1024 * 4             # one pass of a long-row launch over its list: 1024 workgroups of 4 entries
N_LONG = 2 * P_LONG + 1000 + 3


def long_idx(long, short, seed, n_long=N_LONG):
    """idx of a table with n_long rows drawn from the pool's `long` rows and as many from its `short` ones, shuffled: the long
    launch takes three steps over its list, the last one partial.  (Its grid is sized from the table's rows: 4096 rows or more
    give it all its 1024 workgroups.)"""
    assert n_long > 2 * P_LONG and len(long) >= 2 and len(short) >= 2
    rng = np.random.default_rng([seed, 77])
    idx = np.concatenate([np.asarray(long)[rng.integers(0, len(long), n_long)], np.asarray(short)[rng.integers(0, len(short), n_long)]])
    rng.shuffle(idx)
    return idx


def passes(n, P):
    return [slice(a, min(a + P, n)) for a in range(0, n, P)]


def sample_rows(n, P, k=2000, seed=1):
    """k table rows or more, seeded, the first and the last row of every pass among them"""
    edges = [x for s in passes(n, P) for x in (s.start, s.stop - 1)]
    return np.unique(np.concatenate([np.array(edges), np.random.default_rng(seed).choice(n, k, replace=False)]))


def same_kept(got, want, P, what):
    """the ordinals a selecting pass kept (d_idx), exact; on a mismatch: the first row kept or dropped wrongly, and its pass"""
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    k = min(len(got), len(want))
    bad = np.flatnonzero(got[:k] != want[:k])
    if bad.size or len(got) != len(want):
        at = int(bad[0]) if bad.size else k
        r = int(min(got[at] if at < len(got) else 1 << 62, want[at] if at < len(want) else 1 << 62))
        raise AssertionError("%s: %d rows kept, %d expected; the first difference is at kept ordinal %d: row %d, pass %d (row %d of it)"
                             % (what, len(got), len(want), at, r, r // P, r % P))


def same_rows(got, want, P, what):
    """exact, row by row; on a mismatch: the first bad row and the pass it lies in"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1)) if got.size else np.zeros(0, dtype=np.int64)
    if bad.size:
        r = int(bad[0])
        raise AssertionError("%s: %d rows differ, the first is row %d in pass %d (row %d of it): got %s, expected %s; bad rows per pass %s"
                             % (what, bad.size, r, r // P, r % P, got[r].tolist(), want[r].tolist(),
                                np.bincount(bad // P).tolist()))

"""The scan of an array behind the table calls (csrc/ffq_scan.h: k_scan_one, k_scan_blksum, k_scan_blkapply; launch_scan in
csrc/ffq_hip.hip) at the EDGES of its levels.  The levels switch at compile-time constants -- a thread of the one-workgroup
kernel owns 32 values, a round of it has 32 768, one workgroup serves up to 32 768 counts or 65 536 int64 values, the outer
levels take 2048 values a workgroup -- so the numbers of values below are the smallest that reach each branch, and each is
taken with a full last block of 256 rows and with a single row in it.

  counts (u32 -> int64)   ffq_table_select_seqlen_idx: a value per block of 256 rows = the rows kept in it.  The call reads the
                          table alone.  A wrong base moves rows, so the kept rows, their ordinals and the fill behind them
                          are compared with torch's own selection by the same mask.
  int64, in place         ffq_table_gather_column as a sizing call (out_cap = 0, no buffer): a value per block = the bytes of
                          its rows' components; d_off must be torch's exclusive int64 cumsum of the clamped lengths.  Lengths
                          up to 2^30: a block's sum passes 2^32, the total 2^40 within a few thousand rows.

Tables are made on the device, results are compared there and reduced to one boolean."""
import pytest

E_TABLE_FULL = -5
FILL = -7
ROWS = 256                                   # rows per value of either scan

# ---- counts ----------------------------------------------------------------------------------------------------------------
U32_NBLK = (1, 31, 32, 33, 1024, 1025, 32767, 32768, 32769, 17 * 2048, 17 * 2048 + 1)
LEN_LO, LEN_HI = 100, 200                    # a kept row's length lies in [LEN_LO, LEN_HI]

# ---- int64 -----------------------------------------------------------------------------------------------------------------
I64_NBLK = (1, 32, 33, 65536, 65537, 65536 + 2048 + 1)
N_BYTES = 1 << 30
COL_LEN_CLAMP = 0x7FFFFFF0                   # col_len's clamp (csrc/ffq_kernels.h)


def sizes(nblk):
    """a full last block, and a last block of one row"""
    return (ROWS * nblk, ROWS * nblk - (ROWS - 1))


def keep_plan(i):
    """bool per row index i (a tensor): which rows the length filter is to keep.

    Every row on its own by a hash of i, then whole blocks of 256 over that: block b is kept whole for b % 7 == 3 and dropped
    whole for b % 7 == 5; and around every multiple of 32 blocks -- the edge of a thread's 32 values, and with it every edge
    of a wave's or an outer block's 2048 values and of a round's 32 768 -- the four blocks [-2, +2) are one run, kept or dropped
    whole by the edge's number: kept across 32 * 1024 (the round), dropped across 2048 * 3, kept across 2048 * 1, ..."""
    b = i // ROWS
    keep = ((i * 2654435761) >> 7) % 5 < 2
    keep = keep | (b % 7 == 3)
    keep = keep & ~(b % 7 == 5)
    edge = (b + 2) // 32
    near = ((b + 2) % 32 < 4) & (edge > 0)
    return (keep & ~near) | (near & (edge % 3 != 0))


def select_world(torch, n, device):
    """int64[n][6] rows: pos2 = 0, pos3 = a seeded length inside [LEN_LO, LEN_HI] for the rows of keep_plan and outside it for
    the others; the other four positions say which row it is"""
    g = torch.Generator(device=device).manual_seed(20240611)
    i = torch.arange(n, dtype=torch.int64, device=device)
    r = torch.randint(0, 1 << 20, (n,), generator=g, dtype=torch.int64, device=device)
    inside = LEN_LO + r % (LEN_HI - LEN_LO + 1)
    outside = torch.where(r % 2 == 0, r % LEN_LO, LEN_HI + 1 + r % 1000)
    ln = torch.where(keep_plan(i), inside, outside)
    t = torch.stack((i, i + 1, torch.zeros_like(i), ln, 7 * i, -i), dim=1).contiguous()
    return t


def gather_world(torch, n, device):
    """int64[n][6] rows whose component (pos2, pos3) has a seeded length in [0, 2^30] at a seeded place inside the N_BYTES the
    call declares; one row in 16 ends below its start, one in 16 ends past N_BYTES, and every fifth block of 256 is such rows
    throughout.  Returns (table, lengths as col_len counts them)."""
    g = torch.Generator(device=device).manual_seed(20240612)
    i = torch.arange(n, dtype=torch.int64, device=device)
    ln = torch.randint(0, (1 << 30) + 1, (n,), generator=g, dtype=torch.int64, device=device)
    start = torch.randint(0, 1 << 30, (n,), generator=g, dtype=torch.int64, device=device) % (N_BYTES - ln + 1)
    kind = torch.randint(0, 16, (n,), generator=g, dtype=torch.int64, device=device)
    kind = torch.where((i // ROWS) % 5 == 2, kind % 2, kind)
    end = start + ln
    end = torch.where(kind == 0, start - 1 - ln, end)                     # below its start
    start = torch.where(kind == 1, N_BYTES - ln + 1 + start % 1000, start)    # ... past the end of the buffer
    end = torch.where(kind == 1, start + ln, end)
    t = torch.stack((i, i, start, end, i, i), dim=1).contiguous()
    # the reference arithmetic of col_len (sentinel 0, add 0), nothing else
    raw = end - start
    valid = (raw > 0) & (start >= 0) & (start <= N_BYTES) & (raw <= N_BYTES - start)
    return t, torch.where(valid, raw, torch.zeros_like(raw))


def test_gather_lengths_stay_inside_the_clamp():
    """what makes torch's cumsum the whole expectation: no length reaches col_len's clamp, nor the 2^31 the column kernels'
    wave scan is exact below (COL_LEN_BITS)"""
    import torch
    t, ln = gather_world(torch, 64 * ROWS + 1, "cpu")
    raw = t[:, 3] - t[:, 2]
    assert int(raw.max()) <= 1 << 30 < COL_LEN_CLAMP < 1 << 31 and int(ln.max()) <= 1 << 30 and int(ln.min()) == 0
    assert int((ln == 0).sum()) > 64 * ROWS // 10 and int((raw < 0).sum()) > 0 and int((t[:, 3] > N_BYTES).sum()) > 0
    b = ln[:64 * ROWS].view(64, ROWS).sum(dim=1)
    assert int(b.max()) > 1 << 32 and int((b == 0).sum()) >= 64 // 5 and int(ln.sum()) > 1 << 40


def test_keep_plan_has_the_runs():
    """whole blocks kept and dropped, and runs of either across the edges of 32, 2048 and 32 768 values"""
    import torch
    n = ROWS * max(U32_NBLK)
    cnt = keep_plan(torch.arange(n, dtype=torch.int64)).view(-1, ROWS).sum(dim=1)
    assert int((cnt == ROWS).sum()) > 0 and int((cnt == 0).sum()) > 0 and int(((cnt > 0) & (cnt < ROWS)).sum()) > 0
    seen = set()
    for edge in (32, 64, 96, 2048, 3 * 2048, 32768):
        run = cnt[edge - 2:edge + 2]
        assert bool((run == ROWS).all()) or bool((run == 0).all())
        seen.add((edge % 2048 == 0, int(run[0]) == ROWS))
    assert seen == {(False, True), (False, False), (True, True), (True, False)}
    assert int(cnt[32768 - 2]) == ROWS


@pytest.fixture(scope="module")
def select_rows(gpu_ctx):
    import torch
    t = select_world(torch, ROWS * max(U32_NBLK), "cuda")
    ln = t[:, 3] - t[:, 2]
    return t, (ln >= LEN_LO) & (ln <= LEN_HI)


@pytest.fixture(scope="module")
def gather_rows(gpu_ctx):
    import torch
    t, ln = gather_world(torch, ROWS * max(I64_NBLK), "cuda")
    assert int(ln.max()) <= 1 << 30 and int((t[:, 3] - t[:, 2]).max()) < COL_LEN_CLAMP
    return t, ln


@pytest.mark.gpu
@pytest.mark.parametrize("nblk", U32_NBLK)
@pytest.mark.parametrize("last", ("full", "one"))
def test_counts_scan_places_the_kept_rows(gpu_ctx, select_rows, nblk, last):
    import torch
    n = sizes(nblk)[last == "one"]
    table, mask = select_rows[0][:n], select_rows[1][:n]
    out = torch.full((n + 1, 6), FILL, dtype=torch.int64, device="cuda")
    idx = torch.full((n + 1,), FILL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    k = gpu_ctx.table_select_seqlen_idx(table.data_ptr(), n, LEN_LO, LEN_HI, out.data_ptr(), idx.data_ptr())
    want = torch.nonzero(mask).flatten()
    assert k == want.numel()
    ok = (out[:k] == table[want]).all() & (idx[:k] == want).all() & (out[k:] == FILL).all() & (idx[k:] == FILL).all()
    assert bool(ok)


@pytest.mark.gpu
@pytest.mark.parametrize("nblk", I64_NBLK)
@pytest.mark.parametrize("last", ("full", "one"))
def test_int64_scan_gives_the_offsets(gpu_ctx, gather_rows, nblk, last):
    import torch
    n = sizes(nblk)[last == "one"]
    table, ln = gather_rows[0][:n], gather_rows[1][:n]
    off = torch.full((n + 1,), FILL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc, nbytes = gpu_ctx.table_gather_column(None, N_BYTES, table.data_ptr(), n, (2, 0, 3), None, 0, off.data_ptr(), sentinel=False, add=0)
    incl = torch.cumsum(ln, dim=0)
    total = int(incl[-1])
    assert nbytes == total and rc == (E_TABLE_FULL if total > 0 else 0)
    if n > 4096:
        assert total > 1 << 40
    ok = (off[:n] == incl - ln).all() & (off[n] == total)
    assert bool(ok)

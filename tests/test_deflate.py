"""Device bytes written as BGZF members deflated on the GPU: Context.deflate_bgzf (ffq_deflate_bgzf, include/ffq.h).

The judge is zlib (tests/deflate_expect.py: no package code): gzip.decompress gives the input back, and every member is
walked by its BSIZE -- header bytes, size, a raw deflate stream that ends where the member says, CRC-32, ISIZE.  S is the
segment a match may not leave, R the positions of a round, B the bytes of a member, G the blocks deflated at a time: all
read from the binding.
"""
import gzip

import numpy as np
import pytest

import deflate_expect as E

GUARD = 0xEE
PHRASE = bytes(range(32, 132))               # 100 bytes no four of which come twice


def consts():
    from fastqandfurious_amd import hip
    return hip.DEFLATE_SEG_BYTES, hip.DEFLATE_ROUND_POSITIONS, hip.BGZF_BLOCK_BYTES


def sizes():
    S, _R, B = consts()
    return [0, 1, 3, 4, S - 1, S, S + 1, B - 1, B, B + 1, 2 * B + 1]


def noise(n, seed=5):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def phrase_twice(n, first, dist, quiet=False):
    """the phrase at `first` and again `dist` behind it; around them noise, or with `quiet` one repeated byte: nothing
    between the two then takes the phrase's places in the hash table, and the second is SURE to be offered the first"""
    v = bytearray(b"x" * n if quiet else noise(n))
    v[first:first + 100] = PHRASE
    v[first + dist:first + dist + 100] = PHRASE
    return bytes(v)


def fibonacci_bytes():
    a, b, out = 1, 1, []
    for i in range(22):                       # 46367 bytes, and a Huffman code over these counts is 21 deep
        out.append(np.full(a, i * 11 + 1, dtype=np.uint8))
        a, b = b, a + b
    v = np.concatenate(out)
    np.random.default_rng(3).shuffle(v)
    return v.tobytes()


def deflate(ctx, src, misalign_src=0, misalign_out=3, cap=None):
    """(rc, stats, out bytes or None, member offsets, guard intact) of one call on a fresh output buffer"""
    import torch
    from fastqandfurious_amd import hip
    n = len(src)
    dsrc = torch.zeros(misalign_src + n + 16, dtype=torch.uint8, device="cuda")
    if n:
        dsrc[misalign_src:misalign_src + n] = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).cuda()
    bound = hip.deflate_bgzf_bound(n)
    cap = bound if cap is None else cap
    n_members = (n + hip.BGZF_BLOCK_BYTES - 1) // hip.BGZF_BLOCK_BYTES
    out = torch.full((misalign_out + max(cap, 0) + 64,), GUARD, dtype=torch.uint8, device="cuda")
    off = torch.full((n_members + 1,), -7, dtype=torch.int64, device="cuda")
    rc, stats = ctx.deflate_bgzf(dsrc.data_ptr() + misalign_src, n, out.data_ptr() + misalign_out, cap, off.data_ptr())
    h = out.cpu().numpy()
    got = h[misalign_out:misalign_out + stats[1]].tobytes() if rc == hip.OK else None
    untouched = h[:misalign_out].tolist() == [GUARD] * misalign_out and \
        bool((h[misalign_out + (stats[1] if rc == hip.OK else 0):] == GUARD).all())
    return rc, stats, got, off.cpu().numpy().tolist(), untouched


def check_case(ctx, src, want_stored=None, from_isize=0, **kw):
    """want_stored: what every member of from_isize bytes or more must be -- one answer for all, or one per member"""
    from fastqandfurious_amd import hip
    B = hip.BGZF_BLOCK_BYTES
    n = len(src)
    assert hip.deflate_bgzf_bound(n) == n + 31 * ((n + B - 1) // B)
    rc, stats, out, off, untouched = deflate(ctx, src, **kw)
    assert rc == hip.OK and untouched, (rc, stats, untouched)
    assert gzip.decompress(out) == src
    text, members = E.walk(out, B)
    assert text == src
    assert [m[2] for m in members] == [min(B, n - a) for a in range(0, n, B)]
    assert stats == (n, len(out), len(members), sum(m[3] for m in members)), (stats, len(out), len(members))
    assert off == [m[0] for m in members] + [len(out)]
    assert all(m[1] <= m[2] + 31 for m in members) and len(out) <= hip.deflate_bgzf_bound(n)
    if want_stored is not None:
        want = list(want_stored) if isinstance(want_stored, (list, tuple)) else [want_stored] * len(members)
        assert len(want) == len(members)
        bad = [(i, m[2:]) for i, (m, w) in enumerate(zip(members, want)) if m[2] >= from_isize and m[3] != w]
        assert not bad, bad[:8]
    # the same bytes on a second call
    rc2, stats2, out2, off2, _u = deflate(ctx, src, **kw)
    assert (rc2, stats2, off2) == (rc, stats, off) and out2 == out
    # an output one byte short: refused, the need reported, nothing written
    if n:
        rc3, stats3, out3, off3, untouched3 = deflate(ctx, src, cap=len(out) - 1, **kw)
        assert rc3 == hip.E_TABLE_FULL and stats3 == stats and out3 is None and untouched3 and off3 == off
        assert "members have %d" % len(out) in hip.lib().ffq_last_error().decode()
    return out, members


@pytest.mark.gpu
@pytest.mark.parametrize("n", sizes())
def test_one_byte_repeated(gpu_ctx, n):
    """a chain of matches of length 258 at distance 1: one distance symbol, a code of length 1"""
    S, _R, B = consts()
    out, members = check_case(gpu_ctx, b"F" * n, want_stored=False, from_isize=64)
    if n >= B:
        assert members[0][1] < 1000, members[0]        # 255 segments of (a literal, a 255-byte match)


@pytest.mark.gpu
@pytest.mark.parametrize("n", sizes())
def test_two_bytes_alternating(gpu_ctx, n):
    # (from 256 bytes: all code lengths are 0, 1 or 2, so the header is under 75 bytes and the literals under 2 bits each)
    out, members = check_case(gpu_ctx, (b"AC" * (n // 2 + 1))[:n], want_stored=False, from_isize=256)


@pytest.mark.gpu
@pytest.mark.parametrize("n", sizes())
def test_noise_is_stored(gpu_ctx, n):
    S, _R, B = consts()
    src = noise(n)
    if n >= B:
        assert set(range(144, 256)) <= set(src)
    out, members = check_case(gpu_ctx, src, want_stored=True, misalign_src=n % 4)
    assert len(out) == n + 31 * len(members)


@pytest.mark.gpu
def test_fibonacci_counts(gpu_ctx):
    """counts whose Huffman code is deeper than deflate's 15 bits: the lengths are cut to the limit"""
    check_case(gpu_ctx, fibonacci_bytes(), want_stored=False)


@pytest.mark.gpu
def test_a_repeat_farther_than_a_distance_reaches(gpu_ctx):
    """65280 bytes offer candidates up to 65279 back; deflate's distances end at 32768"""
    _S, _R, B = consts()
    check_case(gpu_ctx, phrase_twice(B, 1000, 40000))
    far, _m = check_case(gpu_ctx, phrase_twice(B, 1024, 40000, quiet=True), want_stored=False)
    edge, _m = check_case(gpu_ctx, phrase_twice(B, 1024, 32768, quiet=True), want_stored=False)
    past, _m = check_case(gpu_ctx, phrase_twice(B, 1024, 32769, quiet=True), want_stored=False)
    check_case(gpu_ctx, phrase_twice(B, 1024, 32768))
    check_case(gpu_ctx, phrase_twice(B, 1024, 32769))
    # at 32768 the second phrase is one match; a byte farther it is a hundred literals
    assert len(edge) + 40 < len(past) and len(edge) + 40 < len(far), (len(edge), len(past), len(far))


@pytest.mark.gpu
def test_repeats_across_a_round_and_a_segment(gpu_ctx):
    S, R, _B = consts()
    check_case(gpu_ctx, phrase_twice(8 * R, R - 50, 2 * R))
    check_case(gpu_ctx, phrase_twice(8 * R, R - 50, 2 * R, quiet=True), want_stored=False)
    check_case(gpu_ctx, phrase_twice(8 * R, 3 * S - 50, 2 * R + 17))
    check_case(gpu_ctx, phrase_twice(8 * R, 3 * S - 50, 2 * R + 17, quiet=True), want_stored=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("synth.single", "illumina-like"))
def test_fastq_text(gpu_ctx, kind):
    """20000 records: no member stored, and the whole within 2 % of what zlib's Huffman-only coding gives for the same
    blocks (the header's lengths are written without run-length codes: at most about 280 bytes a block)"""
    from fastqandfurious_amd import hip, synth
    B = hip.BGZF_BLOCK_BYTES
    src = synth.single(0, 20000).tobytes() if kind == "synth.single" else E.illumina_like(20000)
    out, members = check_case(gpu_ctx, src, want_stored=False)
    huff = E.huffman_only_bytes(src, B)
    l1, l6 = E.zlib_level_bytes(src, B, 1), E.zlib_level_bytes(src, B, 6)
    print("%s: %d bytes -> %d (ratio %.3f); zlib per block: Huffman-only %d (%.3f), level 1 %d (%.3f), level 6 %d (%.3f); "
          "against level 1: %.3f" % (kind, len(src), len(out), len(src) / len(out), huff, len(src) / huff, l1, len(src) / l1,
                                     l6, len(src) / l6, len(out) / l1))
    assert len(out) <= 1.02 * huff, (len(out), huff)


def grid_consts():
    from fastqandfurious_amd import hip
    return hip.DEFLATE_GRID_BLOCKS, hip.BGZF_BLOCK_BYTES


def test_the_grid_source_is_what_it_says():
    """zlib's own compression of every block alone stores the noise blocks and no others; copies are copies"""
    import zlib
    G, B = grid_consts()
    src, kinds, twin = E.grid_source(G, B)
    n = len(kinds)
    assert n == len(twin) == 2 * G + 3 and n > 2 * G and len(src) == (n - 1) * B + E.GRID_LAST
    blocks = [src[a:a + B] for a in range(0, len(src), B)]
    assert len(set(blocks[:G])) == G                                       # no two alike
    for k in range(G):
        assert blocks[G + k] == blocks[(k + 1) % G] and twin[G + k] == (k + 1) % G
    assert blocks[2 * G] == blocks[2] and blocks[2 * G + 1] == blocks[3] and blocks[2 * G + 2] == blocks[4][:E.GRID_LAST]
    for p in range(0, n, G):                                               # every kind in every pass of the grid
        assert set(kinds[p:p + G]) == set(E.GRID_KINDS)
    assert kinds[-1] == "text"
    for k in list(range(G)) + [n - 1]:
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        raw = c.compress(blocks[k]) + c.flush()
        stored = (raw[0] & 6) == 0
        assert stored == (kinds[k] == "noise"), (k, kinds[k], len(raw))
        assert stored or len(raw) < len(blocks[k]) // 2, (k, kinds[k], len(raw))


@pytest.mark.gpu
def test_more_blocks_than_one_pass_of_the_grid(gpu_ctx):
    """2 * G + 3 blocks under a grid of G workgroups: the workgroup of block k takes blocks G + k and 2 * G + k behind it,
    on the LDS and the scratch it used before.  Members do not depend on one another and the call is deterministic, so the
    member of a copied block IS the member of the block it copies, byte for byte -- which the round trip cannot see: stale
    counts give a legal stream under another code."""
    from fastqandfurious_amd import hip
    G, B = grid_consts()
    src, kinds, twin = E.grid_source(G, B)
    n = len(kinds)
    assert n == 2 * G + 3 and n > 2 * G and len(src) == (n - 1) * B + E.GRID_LAST
    out, members = check_case(gpu_ctx, src, want_stored=[k == "noise" for k in kinds])
    assert len(members) == n and sum(m[3] for m in members) == kinds.count("noise")      # (stats[3]: check_case)
    blob = [out[m[0]:m[0] + m[1]] for m in members]
    for i in range(G, n - 1):
        assert blob[i] == blob[twin[i]], "block %d (pass %d of its workgroup, %s behind %s) is not the member of block %d" % (
            i, i // G, kinds[i], kinds[i - G], twin[i])
    rc, stats, alone, _off, untouched = deflate(gpu_ctx, src[(n - 1) * B:])
    assert rc == hip.OK and untouched and stats[2] == 1
    assert blob[n - 1] == alone, "the short last block (%s behind %s)" % (kinds[n - 1], kinds[n - 1 - G])


@pytest.mark.gpu
def test_arguments(gpu_ctx):
    import torch
    from fastqandfurious_amd import hip
    d = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    with pytest.raises(hip.FFQError):
        gpu_ctx.deflate_bgzf(d.data_ptr(), -1, d.data_ptr(), 10)
    with pytest.raises(hip.FFQError):
        gpu_ctx.deflate_bgzf(None, 10, d.data_ptr(), 100)
    assert hip.bgzf_eof_block() == E.EOF_MEMBER and E.walk(hip.bgzf_eof_block(), hip.BGZF_BLOCK_BYTES, eof_marker=True)[0] == b""
    assert hip.deflate_bgzf_bound(0) == 0
    # refused while a scan is pending on the context
    data = b"@a\nACGT\n+\nIIII\n" * 8
    buf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    table = torch.empty((16, 6), dtype=torch.int64, device="cuda")
    gpu_ctx.scan_submit(buf.data_ptr(), len(data), table.data_ptr(), 16)
    try:
        with pytest.raises(hip.FFQError) as ei:
            gpu_ctx.deflate_bgzf(buf.data_ptr(), len(data), d.data_ptr(), 1024)
        assert ei.value.code == hip.E_ARG and "pending" in str(ei.value)
    finally:
        gpu_ctx.scan_wait()

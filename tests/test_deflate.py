"""Device bytes written as BGZF members deflated on the GPU: Context.deflate_bgzf (ffq_deflate_bgzf, include/ffq.h).

The judge is zlib (tests/deflate_expect.py: no package code): gzip.decompress gives the input back, and every member is
walked by its BSIZE -- header bytes, size, a raw deflate stream that ends where the member says, CRC-32, ISIZE.  S is the
segment a match may not leave, R the positions of a round, B the bytes of a member: all three read from the binding.
"""
import gzip

import numpy as np
import pytest

import deflate_expect as E

pytestmark = pytest.mark.gpu
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
    """want_stored: what every member of from_isize bytes or more must be"""
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
        assert all(m[3] == want_stored for m in members if m[2] >= from_isize), [m[2:] for m in members]
    # the same bytes on a second call
    rc2, stats2, out2, off2, _u = deflate(ctx, src, **kw)
    assert (rc2, stats2, off2) == (rc, stats, off) and out2 == out
    # an output one byte short: refused, the need reported, nothing written
    if n:
        rc3, stats3, out3, off3, untouched3 = deflate(ctx, src, cap=len(out) - 1, **kw)
        assert rc3 == hip.E_TABLE_FULL and stats3 == stats and out3 is None and untouched3 and off3 == off
        assert "members have %d" % len(out) in hip.lib().ffq_last_error().decode()
    return out, members


@pytest.mark.parametrize("n", sizes())
def test_one_byte_repeated(gpu_ctx, n):
    """a chain of matches of length 258 at distance 1: one distance symbol, a code of length 1"""
    S, _R, B = consts()
    out, members = check_case(gpu_ctx, b"F" * n, want_stored=False, from_isize=64)
    if n >= B:
        assert members[0][1] < 1000, members[0]        # 255 segments of (a literal, a 255-byte match)


@pytest.mark.parametrize("n", sizes())
def test_two_bytes_alternating(gpu_ctx, n):
    # (from 256 bytes: all code lengths are 0, 1 or 2, so the header is under 75 bytes and the literals under 2 bits each)
    out, members = check_case(gpu_ctx, (b"AC" * (n // 2 + 1))[:n], want_stored=False, from_isize=256)


@pytest.mark.parametrize("n", sizes())
def test_noise_is_stored(gpu_ctx, n):
    S, _R, B = consts()
    src = noise(n)
    if n >= B:
        assert set(range(144, 256)) <= set(src)
    out, members = check_case(gpu_ctx, src, want_stored=True, misalign_src=n % 4)
    assert len(out) == n + 31 * len(members)


def test_fibonacci_counts(gpu_ctx):
    """counts whose Huffman code is deeper than deflate's 15 bits: the lengths are cut to the limit"""
    check_case(gpu_ctx, fibonacci_bytes(), want_stored=False)


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


def test_repeats_across_a_round_and_a_segment(gpu_ctx):
    S, R, _B = consts()
    check_case(gpu_ctx, phrase_twice(8 * R, R - 50, 2 * R))
    check_case(gpu_ctx, phrase_twice(8 * R, R - 50, 2 * R, quiet=True), want_stored=False)
    check_case(gpu_ctx, phrase_twice(8 * R, 3 * S - 50, 2 * R + 17))
    check_case(gpu_ctx, phrase_twice(8 * R, 3 * S - 50, 2 * R + 17, quiet=True), want_stored=False)


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

"""What a BGZF stream must be (SAM specification 4.1), checked with zlib alone -- no package code in here -- and the seeded
generator of Illumina-like records the deflate tests and tools share.

walk(blob, block_bytes): member by member by BSIZE.  Of every member: the fixed header bytes, at most 65536 bytes, ISIZE at
most block_bytes, a raw deflate stream that zlib.decompressobj(-15) takes whole with nothing left over, CRC-32 and ISIZE of
what came out; with one_block (what the device writes, not zlib) the stream is one final block, stored or dynamic.  Returns
(text, members), members = [(offset, size, isize, stored)].
"""
import struct
import zlib

import numpy as np

HEAD = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0])
EOF_MEMBER = HEAD + bytes([0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def walk(blob, block_bytes, eof_marker=False, one_block=True):
    blob = bytes(blob)
    text, members, at = [], [], 0
    while at < len(blob):
        assert len(blob) - at >= 26, "a member cut short at %d" % at
        assert blob[at:at + 16] == HEAD, "member at %d: header bytes %s" % (at, blob[at:at + 16].hex())
        size = struct.unpack_from("<H", blob, at + 16)[0] + 1
        assert 26 <= size <= 65536 and at + size <= len(blob), "member at %d: BSIZE + 1 = %d" % (at, size)
        crc, isize = struct.unpack_from("<II", blob, at + size - 8)
        assert isize <= block_bytes, "member at %d: ISIZE %d" % (at, isize)
        d = zlib.decompressobj(-15)
        stream = blob[at + 18:at + size - 8]
        out = d.decompress(stream)
        assert d.eof and not d.unused_data and not d.unconsumed_tail, "member at %d: the stream does not end where the member says" % at
        assert len(out) == isize and zlib.crc32(out) == crc, "member at %d: ISIZE / CRC-32" % at
        stored = (stream[0] & 6) == 0          # BTYPE 0
        if one_block and not (eof_marker and blob[at:at + size] == EOF_MEMBER):       # (the marker is an empty fixed block)
            # what the device writes: ONE block with BFINAL set, stored or dynamic
            assert (stream[0] & 7) in (1, 5), "member at %d: not one final stored or dynamic block (%#x)" % (at, stream[0] & 7)
            assert not stored or size == isize + 31, "member at %d: a stored block of %d bytes in %d" % (at, isize, size)
        members.append((at, size, isize, stored))
        text.append(out)
        at += size
    if eof_marker:
        assert blob.endswith(EOF_MEMBER) and members and members[-1][2] == 0, "no EOF marker at the end"
        assert all(m[2] > 0 for m in members[:-1]), "an empty member inside the file"
    else:
        assert all(m[2] > 0 for m in members), "an empty member"
    return b"".join(text), members


def illumina_like(n_records, seed=7):
    """n_records records as a patterned-flowcell NovaSeq writes them: header
    @A00123:45:HXXXXDSXY:1:1101:x:y 1:N:0:ATCACGTT+AGGCTATA with x, y creeping upwards, 150 bases, binned qualities from
    'F', ':', ',', '#' at .9 / .06 / .03 / .01.  bytes."""
    rng = np.random.default_rng(seed)
    x = 1000 + np.cumsum(rng.integers(0, 30, n_records))
    y = 1000 + rng.integers(0, 36000, n_records)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n_records, 150))]
    qual = np.frombuffer(b"F:,#", dtype=np.uint8)[rng.choice(4, (n_records, 150), p=(.9, .06, .03, .01))]
    out = []
    for i in range(n_records):
        out.append(b"@A00123:45:HXXXXDSXY:1:1101:%d:%d 1:N:0:ATCACGTT+AGGCTATA\n" % (x[i], y[i]))
        out.append(seq[i].tobytes())
        out.append(b"\n+\n")
        out.append(qual[i].tobytes())
        out.append(b"\n")
    return b"".join(out)


GRID_KINDS = ("noise", "text", "byte")     # a stored member, a dynamic one, a tiny one
GRID_LAST = 1000                           # bytes of grid_source's last block


def grid_source(grid, block_bytes, seed=11):
    """2 * grid + 3 blocks for a device that deflates `grid` blocks at a time, so that whoever took block k takes blocks
    grid + k and 2 * grid + k behind it.  Blocks [0, grid) cycle through GRID_KINDS, seeded per block: no two are alike.
    Block grid + k is a COPY of block (k + 1) % grid and block 2 * grid + k one of block (k + 2) % grid -- of the next kind
    after the block in front of it in the same place of the grid, save where k + 1 or k + 2 wraps --, the last one cut to GRID_LAST bytes.
    -> (bytes, kind of every block, twin: the block of [0, grid) every block holds the bytes of)"""
    assert grid >= 3 and grid <= 256 and block_bytes > GRID_LAST
    first = []
    for k in range(grid):
        kind = GRID_KINDS[k % 3]
        if kind == "noise":
            first.append(np.random.default_rng((seed, k)).integers(0, 256, block_bytes, dtype=np.uint8).tobytes())
        elif kind == "text":
            first.append(illumina_like(block_bytes // 300, seed=seed * 1000 + k)[:block_bytes])
        else:
            first.append(bytes([k]) * block_bytes)
        assert len(first[-1]) == block_bytes
    twin = list(range(grid)) + [(k + 1) % grid for k in range(grid)] + [(k + 2) % grid for k in range(3)]
    blocks = [first[t] for t in twin]
    blocks[-1] = blocks[-1][:GRID_LAST]
    return b"".join(blocks), [GRID_KINDS[t % 3] for t in twin], twin


def huffman_only_bytes(data, block_bytes):
    """What zlib's Z_HUFFMAN_ONLY makes of the same blocks as BGZF members: the raw streams plus 26 bytes each."""
    total = 0
    for a in range(0, len(data), block_bytes):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        total += len(c.compress(data[a:a + block_bytes]) + c.flush()) + 26
    return total


def zlib_level_bytes(data, block_bytes, level):
    total = 0
    for a in range(0, len(data), block_bytes):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(c.compress(data[a:a + block_bytes]) + c.flush()) + 26
    return total

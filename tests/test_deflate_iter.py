"""filter_fastq(compress="bgzf") and filter_fastq_paired(compress="bgzf"): the text of every fill deflated on the device behind
the render (ffq_stream_set_compress) and written as a BGZF file.  What is asked of it: inflated (zlib alone,
tests/deflate_expect.py), the file is byte for byte what the same call writes without `compress`; the counters are the same;
the file ends with the EOF marker; and the package's own readers read it back.  The host route (another scanner) writes
other members with the same text."""
import gzip
import io
import os

import numpy as np
import pytest

import deflate_expect as E
import merge_expect as M

KW = dict(quality_cutoff=(20, 20), min_len=30)


@pytest.fixture(scope="module")
def F(pkg):
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """synth.single(0, 20000) in a file and as a .gz"""
    from fastqandfurious_amd import synth
    data = synth.single(0, 20000).tobytes()
    d = tmp_path_factory.mktemp("deflate")
    (d / "s.fq").write_bytes(data)
    with gzip.open(str(d / "s.fq.gz"), "wb", compresslevel=1) as fh:
        fh.write(data)
    return data, str(d / "s.fq"), str(d / "s.fq.gz"), d


@pytest.fixture(scope="module")
def plain(F, reads, gpu_ctx):
    """the same call without `compress`, once: (text, result)"""
    out = io.BytesIO()
    with open(reads[1], "rb") as fh:
        res = F.filter_fastq(fh, out, 1 << 20, **KW)
    assert 0 < res.records_out < res.records_in == 20000 and res.bytes_out == len(out.getvalue())
    return out.getvalue(), res


def check_file(blob, want, rep, B, one_block=True):
    text, members = E.walk(blob, B, eof_marker=True, one_block=one_block)
    assert text == want and gzip.decompress(blob) == want
    body = members[:-1]
    assert (rep.bytes_in, rep.bytes_out, rep.members, rep.members_stored) == \
        (len(want), sum(m[1] for m in body), len(body), sum(m[3] for m in body))
    assert rep.ratio == pytest.approx(len(want) / (len(blob) - 28))
    return members


@pytest.mark.gpu
@pytest.mark.parametrize("source", ("file", "gz"))
@pytest.mark.parametrize("fbufsize", (1 << 20, 3000))
def test_the_compressed_file_inflates_to_the_plain_one(F, reads, plain, source, fbufsize):
    """fbufsize 3000: many tiny members, and fills that keep no row and write none"""
    from fastqandfurious_amd import hip
    want, want_res = plain
    out, rep = io.BytesIO(), F.CompressReport()
    with (open(reads[1], "rb") if source == "file" else gzip.open(reads[2], "rb")) as fh:
        res = F.filter_fastq(fh, out, fbufsize, compress="bgzf", compress_report=rep, **KW)
    assert tuple(res) == tuple(want_res)
    members = check_file(out.getvalue(), want, rep, hip.BGZF_BLOCK_BYTES)
    assert rep.members_stored == 0 and rep.ratio > 1.5
    if fbufsize == 3000:
        assert len(members) > 1000


@pytest.mark.gpu
def test_the_package_reads_its_own_file_back(F, reads, plain):
    from fastqandfurious_amd import hip
    want, _res = plain
    path = str(reads[3] / "out.fq.gz")
    with open(reads[1], "rb") as fh, open(path, "wb") as out:
        F.filter_fastq(fh, out, 1 << 20, compress="bgzf", **KW)
    size = os.path.getsize(path)
    fd = os.open(path, os.O_RDONLY)
    try:
        got, n_parallel = hip.gunzip_fd(fd, len(want) + 16)
        assert got.tobytes() == want and n_parallel >= 0
        # two ranges that meet in the middle of the file: every member belongs to one of them
        parts, at = [], 0
        for lo, hi in ((0, size // 2), (size // 2, size)):
            c_first, c_end, n_bytes, n_members = hip.bgzf_range(fd, lo, hi)
            buf = np.empty(max(n_bytes, 1), dtype=np.uint8)
            assert hip.bgzf_range(fd, lo, hi, out=buf) == (c_first, c_end, n_bytes, n_members)
            assert c_first == at and n_members > 0
            at = c_end
            parts.append(buf[:n_bytes].tobytes())
        assert at == size and b"".join(parts) == want
    finally:
        os.close(fd)
    with F.automagic_open(path) as fh:
        back = [tuple(bytes(x) for x in e) for e in F.readfastq_iter(fh, 1 << 20)]
    assert back == [tuple(bytes(x) for x in e) for e in F.readfastq_iter(io.BytesIO(want), 1 << 20, F.entryfunc, F.entrypos)]


@pytest.mark.gpu
def test_pairs_three_compressed_files(F, gpu_ctx):
    from fastqandfurious_amd import hip, _fastqandfurious as C
    r1, r2 = M.records(600)
    d1, d2 = M.file_of(r1), M.file_of(r2)
    res, o1, o2, om, rep, _reps = M.run(F, d1, d2, C.entrypos, 1 << 15, min_len=40)
    assert rep.pairs_merged > 100 and len(o1) > 0 and len(om) > 0
    crep = F.CompressReport()
    zres, z1, z2, zm, zrep, _zreps = M.run(F, d1, d2, C.entrypos, 1 << 15, min_len=40, compress="bgzf", compress_report=crep)
    assert tuple(zres) == tuple(res) and zrep.__dict__ == rep.__dict__
    B = hip.BGZF_BLOCK_BYTES
    n_members = 0
    for z, want in ((z1, o1), (z2, o2), (zm, om)):
        text, members = E.walk(z, B, eof_marker=True)
        assert text == want
        n_members += len(members) - 1
    assert (crep.bytes_in, crep.members) == (len(o1) + len(o2) + len(om), n_members)
    assert crep.bytes_out == len(z1) + len(z2) + len(zm) - 3 * 28


@pytest.mark.gpu
def test_compress_needs_a_render(reads, gpu_ctx):
    from fastqandfurious_amd import hip
    fd = os.open(reads[1], os.O_RDONLY)
    try:
        st = hip.FileStream(gpu_ctx, fd, 1 << 20)
        try:
            with pytest.raises(hip.FFQError) as ei:
                st.set_compress("bgzf")
            assert ei.value.code == hip.E_ARG and "render" in str(ei.value)
            with pytest.raises(ValueError):
                st.set_compress("gzip")
            # a stream that renders and was not asked to compress hands out text, as before
            st.set_render()
            next(iter(st))
            text, (nb, rendered, _skipped) = st.rendered()
            assert text is not None and nb == text.size > 0 and text[:1].tobytes() == b"@" and rendered > 0
            with pytest.raises(hip.FFQError):
                st.compressed()
        finally:
            st.close()
    finally:
        os.close(fd)


# ---- the host route (no GPU) -------------------------------------------------------------------------------------------
def test_host_route_writes_the_same_text(F, pkg):
    from fastqandfurious_amd import hip, synth
    data = synth.single(0, 2000).tobytes()
    want = io.BytesIO()
    want_res = F.filter_fastq(io.BytesIO(data), want, 1 << 16, entrypos=F.entrypos, **KW)
    for fbufsize in (1 << 16, 3000):
        out, rep = io.BytesIO(), F.CompressReport()
        res = F.filter_fastq(io.BytesIO(data), out, fbufsize, entrypos=F.entrypos, compress="bgzf", compress_report=rep, **KW)
        assert tuple(res) == tuple(want_res)
        members = check_file(out.getvalue(), want.getvalue(), rep, hip.BGZF_BLOCK_BYTES, one_block=False)
        assert [m[2] for m in members[:-2]] == [hip.BGZF_BLOCK_BYTES] * (len(members) - 2)
    # nothing kept: the EOF marker alone
    out = io.BytesIO()
    F.filter_fastq(io.BytesIO(data), out, 1 << 16, entrypos=F.entrypos, min_len=1000, compress="bgzf")
    assert out.getvalue() == E.EOF_MEMBER == hip.BGZF_EOF


def test_unknown_compress_values(F, pkg):
    for bad in ("gzip", "zstd", 1, True):
        with pytest.raises(ValueError):
            F.filter_fastq(io.BytesIO(b""), io.BytesIO(), entrypos=F.entrypos, compress=bad)
        with pytest.raises(ValueError):
            F.filter_fastq_paired(io.BytesIO(b""), io.BytesIO(b""), io.BytesIO(), io.BytesIO(), entrypos=F.entrypos, compress=bad)
    with pytest.raises(ValueError):
        F.filter_fastq(io.BytesIO(b""), io.BytesIO(), entrypos=F.entrypos, compress_report=F.CompressReport())
    with pytest.raises(TypeError):
        F.filter_fastq(io.BytesIO(b""), io.BytesIO(), entrypos=F.entrypos, compress="bgzf", compress_report=object())

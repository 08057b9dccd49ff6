"""FASTQ text out of the stream front end (ffq_stream_set_render / ffq_stream_rendered) and fastqandfurious.filter_fastq.

The expectation is the loop below: the records the Python scanner finds, trimmed by the rule written out in test_trim.py,
filtered by length, and rendered by the formula of include/ffq.h -- never the package's own renderer.
"""
import gzip
import io
import os

import pytest

from test_trim import loop_span


def expected_output(F, data, cf=None, cb=None, min_len=None, max_len=None):
    """(text, (records_in, records_out, bases_removed, bytes_out)): cf / cb None: no trimming"""
    out, n_in, removed = [], 0, 0
    for h, s, q in F.readfastq_iter(io.BytesIO(data), 1 << 20, F.entryfunc, F.entrypos):
        n_in += 1
        if cf is not None and len(s) == len(q) and b"\n" not in q:
            a, b = loop_span(q, cf, cb)
            removed += len(s) - (b - a)
            s, q = s[a:b], q[a:b]
        if (min_len is not None and len(s) < min_len) or (max_len is not None and len(s) > max_len):
            continue
        out.append(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n")
    text = b"".join(out)
    return text, (n_in, len(out), removed, len(text))


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """synth.single(0, 20000) in a file and as a .gz; the loop's output for (20, 20), min_len 30"""
    from fastqandfurious_amd import synth, fastqandfurious as F
    data = synth.single(0, 20000).tobytes()
    d = tmp_path_factory.mktemp("render")
    p = d / "s.fq"
    p.write_bytes(data)
    with gzip.open(str(d / "s.fq.gz"), "wb", compresslevel=1) as fh:
        fh.write(data)
    return data, str(p), str(d / "s.fq.gz"), expected_output(F, data, 20, 20, min_len=30)


# ---- the host loop (no GPU) ------------------------------------------------------------------------------------------
def test_filter_fastq_python_scanner(pkg):
    from fastqandfurious_amd import synth, fastqandfurious as F
    data = synth.single(0, 2000).tobytes()
    want, counters = expected_output(F, data, 20, 20, min_len=30)
    assert 0 < counters[1] < 2000 and counters[2] > 2000
    for fbufsize in (1 << 20, 3000):
        out = io.BytesIO()
        res = F.filter_fastq(io.BytesIO(data), out, fbufsize, quality_cutoff=(20, 20), min_len=30, entrypos=F.entrypos)
        assert out.getvalue() == want
        assert tuple(res) == counters and res.records_in == 2000 and res.bytes_out == len(want)
    # an int is the 3' end; bounds on either side
    for kw, loop in ((dict(quality_cutoff=20), dict(cf=0, cb=20)), (dict(quality_cutoff=(10, 0), max_len=140), dict(cf=10, cb=0, max_len=140)),
                     (dict(min_len=151), dict(min_len=151))):
        out = io.BytesIO()
        res = F.filter_fastq(io.BytesIO(data), out, 1 << 16, entrypos=F.entrypos, **kw)
        want, counters = expected_output(F, data, **loop)
        assert out.getvalue() == want and tuple(res) == counters, kw
    # untouched: the file itself
    out = io.BytesIO()
    res = F.filter_fastq(io.BytesIO(data), out, 1 << 16, entrypos=F.entrypos)
    assert out.getvalue() == data and tuple(res) == (2000, 2000, 0, len(data))
    with pytest.raises(ValueError):
        F.filter_fastq(io.BytesIO(data), io.BytesIO(), quality_cutoff=128, entrypos=F.entrypos)


MALFORMED = [("cut inside the last quality", lambda d: d[:-40]), ("cut inside a header", lambda d: d[:322 * 50 + 5]),
             ("a '+' line with other text", lambda d: d[:322 * 10 + 169] + b"+xy" + d[322 * 10 + 170:])]


def _iterator_error(F, bad, entrypos, fbufsize=4096):
    got = []
    with pytest.raises(ValueError) as e:
        for item in F.readfastq_iter(io.BytesIO(bad), fbufsize, F.entryfunc, entrypos):
            got.append(item)
    return str(e.value), got


@pytest.mark.parametrize("name,damage", MALFORMED)
def test_filter_fastq_malformed_input_python_scanner(pkg, name, damage):
    from fastqandfurious_amd import synth, fastqandfurious as F
    bad = damage(synth.single(0, 100).tobytes())
    text, got = _iterator_error(F, bad, F.entrypos)
    out = io.BytesIO()
    with pytest.raises(ValueError) as e:
        F.filter_fastq(io.BytesIO(bad), out, 4096, entrypos=F.entrypos)
    assert str(e.value) == text
    assert out.getvalue() == b"".join(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n" for h, s, q in got)


# ---- the stream ------------------------------------------------------------------------------------------------------
def _stream_text(hip, ctx, path, fbufsize, setup, last=0):
    """(concatenated text, summed stats, fills) of a FileStream over `path`; last: the end state its last fill must have"""
    fd = os.open(path, os.O_RDONLY)
    try:
        st = hip.FileStream(ctx, fd, fbufsize)
        setup(st)
        parts, total, fills = [], [0, 0, 0], 0
        for rows, fill, off, end, err in st:
            assert end in (last, hip.END_REFILL)
            ends = end
            text, stats = st.rendered()
            assert stats[0] == len(text) and stats[1] == rows.shape[0]
            parts.append(text.tobytes())
            total = [a + b for a, b in zip(total, stats)]
            fills += 1
        st.close()
        assert ends == last
    finally:
        os.close(fd)
    return b"".join(parts), total, fills


@pytest.mark.gpu
def test_stream_trim_filter_render(gpu_ctx, reads):
    """several fills and a carry between them; the concatenated text is the loop's"""
    from fastqandfurious_amd import hip
    data, path, _gz, (want, counters) = reads

    def setup(st):
        st.set_trim(20, 20)
        st.set_filter(30, None)
        st.set_render()
    text, total, fills = _stream_text(hip, gpu_ctx, path, 1 << 20, setup)
    assert fills > 3
    assert text == want
    assert total == [len(want), counters[1], 0] and 0 < counters[1] < 20000


@pytest.mark.gpu
def test_stream_render_alone_is_the_file(gpu_ctx, reads):
    from fastqandfurious_amd import hip
    data, path, _gz, _ = reads
    text, total, fills = _stream_text(hip, gpu_ctx, path, 1 << 20, lambda st: st.set_render())
    assert fills > 3 and text == data and total == [len(data), 20000, 0]


@pytest.mark.gpu
def test_stream_last_record_without_a_final_newline(gpu_ctx, reads, tmp_path):
    """A last quality line that no newline ends.  The scanner takes such a record when a byte follows its quality (the
    reference's loop, fastqandfurious.py:256-266: as many quality bytes as bases) and the text ends it with a newline;
    when the file ends with the quality's last byte it is 'Incomplete final quality string at byte' for the iterator and
    for the stream alike, and the records in front of it are rendered."""
    from fastqandfurious_amd import hip, fastqandfurious as F
    data = reads[0][:322 * 500]
    p = tmp_path / "cut.fq"
    p.write_bytes(data[:-1] + b"I")
    assert [len(q) for _h, _s, q in F.readfastq_iter(io.BytesIO(data[:-1] + b"I"), 1 << 20, F.entryfunc, F.entrypos)] == [150] * 500
    for fbufsize in (1 << 20, 1 << 16):
        text, total, fills = _stream_text(hip, gpu_ctx, str(p), fbufsize, lambda st: st.set_render())
        assert text == data and total == [len(data), 500, 0]
    p.write_bytes(data[:-1])
    with pytest.raises(ValueError, match="Incomplete final quality string at byte"):
        list(F.readfastq_iter(io.BytesIO(data[:-1]), 1 << 20, F.entryfunc, F.entrypos))
    for fbufsize in (1 << 20, 1 << 16):
        text, total, fills = _stream_text(hip, gpu_ctx, str(p), fbufsize, lambda st: st.set_render(), last=hip.END_ERR_FINAL_QUAL)
        assert text == data[:322 * 499] and total == [322 * 499, 499, 0]
    out = io.BytesIO()
    with open(str(p), "rb") as fh, pytest.raises(ValueError, match="Incomplete final quality string at byte"):
        F.filter_fastq(fh, out, 1 << 16)
    assert out.getvalue() == data[:322 * 499]


@pytest.mark.gpu
def test_stream_refused_combinations(gpu_ctx, reads):
    from fastqandfurious_amd import hip
    fd = os.open(reads[1], os.O_RDONLY)
    try:
        st = hip.FileStream(gpu_ctx, fd, 1 << 20, decode=True)
        with pytest.raises(hip.FFQError) as e:
            st.set_render()
        assert e.value.code == hip.E_ARG and "FFQ_F_DECODE_QUAL" in str(e.value)
        st.close()
        st = hip.FileStream(gpu_ctx, fd, 1 << 20)
        st.set_filter(30, None, "sequence")
        with pytest.raises(hip.FFQError) as e:
            st.set_render()
        assert e.value.code == hip.E_ARG and "column" in str(e.value)
        st.close()
        st = hip.FileStream(gpu_ctx, fd, 1 << 20)
        with pytest.raises(hip.FFQError):
            st.rendered()                   # (a stream that does not render has no text)
        st.set_render()
        with pytest.raises(hip.FFQError) as e:
            st.set_filter(30, None, "quality")
        assert e.value.code == hip.E_ARG and "column" in str(e.value)
        st.close()
    finally:
        os.close(fd)


# ---- filter_fastq on the GPU scanner -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("source", ("file", "bytesio", "gz"))
def test_filter_fastq_gpu_scanner(gpu_ctx, reads, source):
    """the same file and the same counters as the per-record loop over the Python scanner; fh is left where readfastq_iter
    leaves it"""
    from fastqandfurious_amd import fastqandfurious as F, _fastqandfurious as C
    data, path, gz, (want, counters) = reads

    def opened():
        if source == "file":
            return open(path, "rb")
        if source == "bytesio":
            return io.BytesIO(data)
        return F.automagic_open(gz)
    host = io.BytesIO()
    with opened() as fh:
        res_host = F.filter_fastq(fh, host, 1 << 20, quality_cutoff=(20, 20), min_len=30, entrypos=F.entrypos)
    assert host.getvalue() == want and tuple(res_host) == counters
    out = io.BytesIO()
    with opened() as fh:
        res = F.filter_fastq(fh, out, 1 << 20, quality_cutoff=(20, 20), min_len=30)
        where = fh.tell()
    assert out.getvalue() == want
    assert tuple(res) == counters
    with opened() as fh:
        assert sum(1 for _ in F.readfastq_iter(fh, 1 << 20, F.entryfunc, C.entrypos)) == 20000
        assert fh.tell() == where
    # untouched: the file comes back
    out = io.BytesIO()
    with opened() as fh:
        res = F.filter_fastq(fh, out, 1 << 20)
    assert out.getvalue() == data and tuple(res) == (20000, 20000, 0, len(data))


@pytest.mark.gpu
@pytest.mark.parametrize("name,damage", MALFORMED)
def test_filter_fastq_malformed_input_gpu_scanner(gpu_ctx, name, damage):
    from fastqandfurious_amd import synth, fastqandfurious as F, _fastqandfurious as C
    bad = damage(synth.single(0, 100).tobytes())
    text, got = _iterator_error(F, bad, C.entrypos)
    out = io.BytesIO()
    with pytest.raises(ValueError) as e:
        F.filter_fastq(io.BytesIO(bad), out, 4096)
    assert str(e.value) == text
    assert out.getvalue() == b"".join(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n" for h, s, q in got)

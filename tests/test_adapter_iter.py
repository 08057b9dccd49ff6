"""3' adapter trimming through the stream front end (ffq_stream_set_adapter / ffq_stream_adapter_trimmed), filter_fastq and
readfastq_iter on the GPU scanner.  The expectation is the per-record path worked out by the loops of test_adapter.py and
test_trim.py over the records the Python scanner finds."""
import gzip
import io
import os

import pytest

from test_adapter import AD, expected_items, expected_output, expected_records, mixed_file


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """a few thousand mixed records in a file and as a .gz; the loops' records with the quality rule (0, 20) in front of the
    adapter, and with the adapter alone"""
    from fastqandfurious_amd import fastqandfurious as F
    data = mixed_file(4000, seed=17)
    d = tmp_path_factory.mktemp("adapter")
    p = d / "m.fq"
    p.write_bytes(data)
    with gzip.open(str(d / "m.fq.gz"), "wb", compresslevel=1) as fh:
        fh.write(data)
    return data, str(p), str(d / "m.fq.gz"), expected_records(F, data, quality=(0, 20)), expected_records(F, data)


@pytest.mark.gpu
@pytest.mark.parametrize("fbufsize", (1 << 16, 1 << 20))
def test_stream_trim_adapter_filter_render(gpu_ctx, reads, fbufsize):
    """byte-identical text and equal summed stats to the per-record path; adapter_trimmed() is the loop's, fill by fill"""
    from fastqandfurious_amd import hip
    data, path, _gz, recs, _plain = reads
    want, counters = expected_output(recs, min_len=30)
    fd = os.open(path, os.O_RDONLY)
    try:
        st = hip.FileStream(gpu_ctx, fd, fbufsize)
        st.set_trim(20)
        st.set_adapter(AD, 100, 3)
        st.set_filter(30, None)
        st.set_render()
        parts, at, fills, removed, rendered = [], 0, 0, 0, 0
        for rows, fill, off, end, err in st:
            assert end in (hip.END_OK, hip.END_REFILL)
            text, stats = st.rendered()
            parts.append(text.tobytes())
            n = st.selected()[1]
            part = recs[at:at + n]
            assert list(st.adapter_trimmed()) == [sum(1 for r in part if r[4] > 0), sum(r[4] for r in part),
                                                  sum(1 for r in part if r[5])], fills
            assert st.trimmed()[1] == sum(r[3] for r in part)
            removed += st.trimmed()[1] + st.adapter_trimmed()[1]
            rendered += stats[1]
            at += n
            fills += 1
        st.close()
    finally:
        os.close(fd)
    assert fills > (3 if fbufsize == 1 << 16 else 0) and at == len(recs) == 4000
    assert b"".join(parts) == want
    assert (at, rendered, removed, len(want)) == counters and 0 < counters[1] < 4000


@pytest.mark.gpu
@pytest.mark.parametrize("source", ("file", "gz"))
def test_filter_fastq_gpu_scanner(gpu_ctx, reads, source):
    from fastqandfurious_amd import fastqandfurious as F
    data, path, gz, recs, plain = reads

    def opened():
        return open(path, "rb") if source == "file" else F.automagic_open(gz)
    for kw, rr, bounds in ((dict(adapter=AD, quality_cutoff=20, min_len=30), recs, dict(min_len=30)),
                           (dict(adapter=AD, min_len=1, max_len=140), plain, dict(min_len=1, max_len=140))):
        want, counters = expected_output(rr, **bounds)
        host = io.BytesIO()
        with opened() as fh:
            res_host = F.filter_fastq(fh, host, 1 << 18, entrypos=F.entrypos, **kw)
        assert host.getvalue() == want and tuple(res_host) == counters
        out = io.BytesIO()
        with opened() as fh:
            res = F.filter_fastq(fh, out, 1 << 18, **kw)
        assert out.getvalue() == want
        assert res == res_host


@pytest.mark.gpu
@pytest.mark.parametrize("column", ("entry", "sequence", "quality", "header"))
def test_readfastq_iter_gpu_scanner(gpu_ctx, reads, column):
    from fastqandfurious_amd import fastqandfurious as F, _fastqandfurious as C
    data, path, _gz, recs, plain = reads
    for ef, rr, bounds in ((F.entryfunc_adaptertrim(AD, quality_cutoff=20, min_len=30, column=column), recs, dict(min_len=30)),
                           (F.entryfunc_adaptertrim(AD, 100, 3, min_len=10, max_len=120, column=column), plain, dict(min_len=10, max_len=120))):
        want = expected_items(rr, column=column, **bounds)
        assert any(e is None for e in want) and any(e is not None for e in want)
        with open(path, "rb") as fh:
            got = list(F.readfastq_iter(fh, 1 << 17, ef, C.entrypos))
        assert got == want
        with open(path, "rb") as fh:
            assert list(F.readfastq_iter(fh, 1 << 17, ef, F.entrypos)) == want


@pytest.mark.gpu
def test_a_subclassed_trimmer_is_called_per_record(gpu_ctx, reads):
    from fastqandfurious_amd import fastqandfurious as F, _fastqandfurious as C
    data, recs = reads[0][:reads[0].index(b"@r300 x")], reads[3][:300]
    calls = []

    class Mine(F.entryfunc_adaptertrim):
        def trimmed_pos(self, buf, pos):
            calls.append(1)
            return super().trimmed_pos(buf, pos)
    got = list(F.readfastq_iter(io.BytesIO(data), 20000, Mine(AD, quality_cutoff=20, min_len=30), C.entrypos))
    assert got == expected_items(recs, min_len=30) and len(calls) == len(got) == 300


@pytest.mark.gpu
def test_misuse(gpu_ctx, reads):
    from fastqandfurious_amd import hip
    fd = os.open(reads[1], os.O_RDONLY)
    try:
        st = hip.FileStream(gpu_ctx, fd, 1 << 16, decode=True)
        with pytest.raises(hip.FFQError) as e:
            st.set_adapter(AD)
        assert e.value.code == hip.E_ARG and "FFQ_F_DECODE_QUAL" in str(e.value)
        st.close()
        st = hip.FileStream(gpu_ctx, fd, 1 << 16)
        for bad in (dict(adapter=b""), dict(adapter=b"A" * 65), dict(adapter=AD, min_overlap=14), dict(adapter=AD, err_permille=1001)):
            with pytest.raises(hip.FFQError) as e:
                st.set_adapter(**bad)
            assert e.value.code == hip.E_ARG
        with pytest.raises(hip.FFQError):
            st.adapter_trimmed()            # (a stream that trims no adapter has no counters)
        next(iter(st))
        with pytest.raises(hip.FFQError) as e:
            st.set_adapter(AD)
        assert e.value.code == hip.E_ARG and "already" in str(e.value)
        st.close()
    finally:
        os.close(fd)

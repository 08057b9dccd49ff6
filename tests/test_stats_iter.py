"""Statistics through the stream front end (ffq_stream_set_stats / ffq_stream_stats), fastq_stats and filter_fastq(report=)
on the GPU scanner.  The expectation is the loop of test_stats.py over the records the Python scanner finds in the input
file -- and, for what was written, in the OUTPUT file --, or over the rows the stream handed out.  Every comparison is exact
over every word."""
import gzip
import io
import os

import numpy as np
import pytest

from test_adapter import AD, expected_records
from test_stats import check_invariants, file_records, mixed_corpus, n_words, np_words, records_of


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """mixed records, a few of them longer than the small buffers below, in a file and as a .gz, and the same without
    wrapped records and with adapters; (data, path, gz path, the loop's records)"""
    from fastqandfurious_amd import fastqandfurious as F
    d = tmp_path_factory.mktemp("stats")
    out = {}
    for name, kw in (("mixed", dict(count=2500, seed=31, long_every=500)), ("single", dict(count=2500, seed=32, wrap=False, adapter=AD)),
                     ("small", dict(count=300, seed=33))):
        data = mixed_corpus(**kw)
        p, z = d / (name + ".fq"), d / (name + ".fq.gz")
        p.write_bytes(data)
        with gzip.open(str(z), "wb", compresslevel=1) as fh:
            fh.write(data)
        out[name] = (data, str(p), str(z), file_records(F, data))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("source", ("file", "gz", "bytesio"))
def test_fastq_stats(gpu_ctx, reads, source):
    """the whole file, whatever the buffer size: at least five fills with records straddling them, and one fill"""
    from fastqandfurious_amd import fastqandfurious as F
    data, path, gz, recs = reads["mixed"]
    assert len(data) > 5 * (1 << 17) and sum(r is None for r in recs) > 100

    def opened():
        return open(path, "rb") if source == "file" else F.automagic_open(gz) if source == "gz" else io.BytesIO(data)
    want = np_words(recs, 512)
    check_invariants(want, 512)
    for fbufsize in (1 << 16, 1 << 17, 1 << 24):
        with opened() as fh:
            s = F.fastq_stats(fh, fbufsize)
        assert (s.words == want).all(), (source, fbufsize, np.flatnonzero(s.words != want)[:8])
        assert s.max_cycles == 512 and s.qual_base == 33 and s.reads == int(want[0])
    with opened() as fh:
        s = F.fastq_stats(fh, 1 << 17, qual_base=64, max_cycles=100)
    assert (s.words == np_words(recs, 100, 64)).all()
    # malformed input raises what readfastq_iter raises
    with pytest.raises(ValueError, match="Incomplete final quality"):
        F.fastq_stats(io.BytesIO(data + b"@x\nACGTACGT\n+\nIII"), 1 << 17)


@pytest.mark.gpu
@pytest.mark.parametrize("source", ("file", "bytesio"))
def test_filter_fastq_report(gpu_ctx, reads, source):
    from fastqandfurious_amd import fastqandfurious as F
    data, path, _gz, recs = reads["single"]
    assert all(r is not None for r in recs)
    kw = dict(quality_cutoff=(20, 20), adapter=AD, min_len=30)

    def opened():
        return open(path, "rb") if source == "file" else io.BytesIO(data)
    plain = io.BytesIO()
    with opened() as fh:
        res0 = F.filter_fastq(fh, plain, 1 << 17, **kw)
    rep, out = F.FilterReport(200), io.BytesIO()
    with opened() as fh:
        res = F.filter_fastq(fh, out, 1 << 17, report=rep, **kw)
    assert res == res0 and out.getvalue() == plain.getvalue()           # the report changes nothing
    assert 0 < res.records_out < res.records_in == len(recs) and res.bases_removed > 0
    assert (rep.before.words == np_words(recs, 200)).all()
    after = file_records(F, out.getvalue())                             # the OUTPUT file's records, by the Python scanner
    want = np_words(after, 200)
    check_invariants(want, 200)
    assert (rep.after.words == want).all()
    assert rep.after.reads == res.records_out == len(after)
    # what is gone: the bases the trims removed, and the rest of the reads that were dropped
    final = expected_records(F, data, quality=(20, 20))
    dropped = sum(len(r[1]) for r in final if len(r[1]) < 30)
    assert dropped > 0 and rep.before.bases - rep.after.bases == res.bases_removed + dropped
    # the Python scanner's branch fills the same report
    rep2 = F.FilterReport(200)
    assert F.filter_fastq(io.BytesIO(data), io.BytesIO(), 1 << 17, entrypos=F.entrypos, report=rep2, **kw) == res
    assert rep2.before == rep.before and rep2.after == rep.after


@pytest.mark.gpu
def test_filter_fastq_report_wrapped_records_and_qual_base(gpu_ctx, reads):
    """wrapped records are written but not counted: skipped, before and after"""
    from fastqandfurious_amd import fastqandfurious as F
    data, path, _gz, recs = reads["mixed"]
    rep, out = F.FilterReport(150), io.BytesIO()
    with open(path, "rb") as fh:
        res = F.filter_fastq(fh, out, 1 << 17, quality_cutoff=20, qual_base=64, min_len=10, report=rep)
    assert rep.before.qual_base == rep.after.qual_base == 64
    assert (rep.before.words == np_words(recs, 150, 64)).all()
    after = file_records(F, out.getvalue())
    assert (rep.after.words == np_words(after, 150, 64)).all()
    assert rep.after.reads + int(rep.after.head[1]) == res.records_out and rep.after.head[1] > 50


def _stream(hip, ctx, source, fd, data, fbufsize, decode=False):
    return hip.PushStream(ctx, io.BytesIO(data), fbufsize, decode=decode) if source == "push" else hip.FileStream(ctx, fd, fbufsize, decode=decode)


CONFIGS = {
    "in": dict(which=1),
    "out": dict(which=2),
    "both": dict(which=3),
    "both_trim_min30_render": dict(which=3, trim=(20, 20), flt=(30, None), render=True),
    "both_trim_adapter_max200": dict(which=3, trim=(0, 20), adapter=AD, flt=(None, 200)),
    "out_trim": dict(which=2, trim=(20, 20)),
    "in_min30_sequence": dict(which=1, flt=(30, None), column="sequence"),
    "both_min30_quality": dict(which=3, trim=(20, 20), flt=(30, None), column="quality", value_add=-33),
    "both_decode": dict(which=3, decode=True),
    "out_decode": dict(which=2, decode=True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("source", ("file", "push"))
def test_stream_totals_after_every_fill(gpu_ctx, reads, source, config):
    """ffq_stream_stats after each fill == the loop over the records scanned (IN) and over the rows handed out (OUT) so far"""
    from fastqandfurious_amd import hip
    cfg = CONFIGS[config]
    data, path, _gz, recs = reads["small"]
    C, qbase = 150, 33
    fd = os.open(path, os.O_RDONLY)
    try:
        st = _stream(hip, gpu_ctx, source, fd, data, 3000, cfg.get("decode", False))
        try:
            if "trim" in cfg:
                st.set_trim(cfg["trim"][1], cfg["trim"][0])
            if "adapter" in cfg:
                st.set_adapter(cfg["adapter"])
            if "flt" in cfg:
                st.set_filter(cfg["flt"][0], cfg["flt"][1], cfg.get("column"), cfg.get("value_add", 0))
            if cfg.get("render"):
                st.set_render()
            st.set_stats(cfg["which"], qbase, C)
            scanned, handed, fills = 0, [], 0
            for rows, _fill, _off, end, _err in st:
                assert end in (hip.END_OK, hip.END_REFILL)
                fills += 1
                scanned += st.selected()[1] if "flt" in cfg else rows.shape[0]
                handed.append(np.array(rows, dtype=np.int64).reshape(-1, 6))
                if cfg["which"] & hip.STATS_IN:
                    got = st.stats(hip.STATS_IN)
                    assert got.dtype == np.uint64 and got.shape == (n_words(C),)
                    assert (got == np_words(recs[:scanned], C, qbase)).all(), (config, source, fills)
                else:
                    with pytest.raises(hip.FFQError) as e:
                        st.stats(hip.STATS_IN)
                    assert e.value.code == hip.E_ARG
                if cfg["which"] & hip.STATS_OUT:
                    want = np_words(records_of(data, np.concatenate(handed)), C, qbase)     # (a stream's rows index the file)
                    assert (st.stats(hip.STATS_OUT) == want).all(), (config, source, fills)
                else:
                    with pytest.raises(hip.FFQError) as e:
                        st.stats(hip.STATS_OUT)
                    assert e.value.code == hip.E_ARG
                for which in (0, 3, 4):
                    with pytest.raises(hip.FFQError):
                        st.stats(which)
            assert fills >= 5 and scanned == len(recs)
            # after the last fill: the totals stay
            if cfg["which"] & hip.STATS_IN:
                assert (st.stats(hip.STATS_IN) == np_words(recs, C, qbase)).all()
            if cfg["which"] == hip.STATS_OUT and "trim" not in cfg and "flt" not in cfg:
                assert (st.stats(hip.STATS_OUT) == np_words(recs, C, qbase)).all()
        finally:
            st.close()
    finally:
        os.close(fd)


@pytest.mark.gpu
def test_misuse(gpu_ctx, reads):
    import ctypes
    from fastqandfurious_amd import hip
    fd = os.open(reads["small"][1], os.O_RDONLY)
    try:
        st = hip.FileStream(gpu_ctx, fd, 3000)
        for bad in (dict(which=0), dict(which=4), dict(which=1, max_cycles=0), dict(which=1, max_cycles=4097), dict(which=3, qual_base=256),
                    dict(which=2, qual_base=-1)):
            with pytest.raises(hip.FFQError) as e:
                st.set_stats(**bad)
            assert e.value.code == hip.E_ARG, bad
        with pytest.raises(hip.FFQError):
            st.stats(hip.STATS_IN)                   # (nothing was set)
        st.set_stats(hip.STATS_IN, 33, 150)
        next(iter(st))
        # an output that is too small
        small = np.zeros(n_words(150) - 1, dtype=np.uint64)
        assert hip.lib().ffq_stream_stats(st._h, 1, ctypes.c_void_p(small.ctypes.data), small.size) == hip.E_ARG and not small.any()
        with pytest.raises(hip.FFQError) as e:
            st.set_stats(hip.STATS_OUT)
        assert e.value.code == hip.E_ARG and "already" in str(e.value)
        assert st.stats(hip.STATS_IN)[0] > 0
        st.close()
    finally:
        os.close(fd)

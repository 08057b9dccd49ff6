"""entryfunc_qualitytrim through readfastq_iter on the GPU scanner: the stream front end trims every fill's table on the
device (ffq_stream_set_trim), filters it and gathers the column -- the items are those of the per-record path."""
import io
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, golden_file
from test_trim import expected_items, loop_rows


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """synth.single(0, 20000) in a file; the per-record expectation for (20, 20), min_len 30, by column"""
    from fastqandfurious_amd import synth, fastqandfurious as F
    data = synth.single(0, 20000).tobytes()
    p = tmp_path_factory.mktemp("trim") / "s.fq"
    p.write_bytes(data)
    entries = expected_items(F, data, 20, 20, min_len=30)
    return data, str(p), entries


def _column(entries, c):
    j = {"header": 0, "sequence": 1, "quality": 2}.get(c)
    return [e if (e is None or j is None) else e[j] for e in entries]


@pytest.mark.gpu
@pytest.mark.parametrize("column", ["entry", "sequence", "quality"])
def test_stream_of_20000_records(gpu_ctx, reads, column):
    """several fills and a carry between them; the same items as the per-record path, in the same order"""
    from fastqandfurious_amd import fastqandfurious as F, _fastqandfurious as C
    data, path, entries = reads
    ef = F.entryfunc_qualitytrim(20, 20, min_len=30, column=column)
    with open(path, "rb") as fh:
        got = list(F.readfastq_iter(fh, 1 << 20, ef, C.entrypos))
    want = _column(entries, column)
    assert len(got) == len(want) == 20000
    assert got == want
    # the per-record path of the package says the same (Python scanner, the entryfunc called for every record)
    with open(path, "rb") as fh:
        per_record = list(F.readfastq_iter(fh, 1 << 20, ef, F.entrypos))
    assert per_record == want


@pytest.mark.gpu
def test_stream_counters(gpu_ctx, reads):
    """ffq_stream_trimmed over the fills of a FileStream opened directly == the loop's totals; the rows are the trimmed
    ones, without a filter too"""
    from fastqandfurious_amd import hip
    data, path, _ = reads
    rows = np.array([[b, b + 17, b + 18, b + 168, b + 171, b + 321] for b in range(0, len(data), 322)], dtype=np.int64)
    want, stats = loop_rows(data, rows, 20, 20)
    fd = os.open(path, os.O_RDONLY)
    try:
        st = hip.FileStream(gpu_ctx, fd, 1 << 20)
        st.set_trim(20, 20)
        total, got, fills = [0, 0, 0], [], 0
        for r, fill, off, end, err in st:
            assert end in (hip.END_OK, hip.END_REFILL)
            t = st.trimmed()
            total = [a + b for a, b in zip(total, t)]
            got.append(r.copy())
            fills += 1
        st.close()
    finally:
        os.close(fd)
    assert fills > 3
    assert (np.concatenate(got) == want).all()
    assert total == stats and stats[0] > 10000


@pytest.mark.gpu
def test_stream_small_fills_golden_file(gpu_ctx):
    """tests/golden/data/test.fq at fbufsize 300: nearly every fill carries an unfinished record over"""
    from fastqandfurious_amd import fastqandfurious as F, _fastqandfurious as C
    data = golden_file("test.fq")
    for column in ("entry", "sequence", "quality"):
        want = expected_items(F, data, 20, 20, min_len=30, column=column)
        with open(os.path.join(GOLDEN_DIR, "data", "test.fq"), "rb") as fh:
            got = list(F.readfastq_iter(fh, 300, F.entryfunc_qualitytrim(20, 20, min_len=30, column=column), C.entrypos))
        assert got == want, column
        # a source the library cannot read itself (chunks pushed by the host), and the batched scanner's front
        got = list(F.readfastq_iter(io.BytesIO(data), 300, F.entryfunc_qualitytrim(20, 20, min_len=30, column=column), C.entrypos))
        assert got == want, column


@pytest.mark.gpu
def test_a_subclassed_trimmer_is_called_per_record(gpu_ctx):
    from fastqandfurious_amd import fastqandfurious as F, _fastqandfurious as C
    data = golden_file("test.fq")
    calls = []

    class Mine(F.entryfunc_qualitytrim):
        def __call__(self, buf, pos, globaloffset=None):
            calls.append(1)
            return super().__call__(buf, pos, globaloffset)
    got = list(F.readfastq_iter(io.BytesIO(data), 20000, Mine(20, 20, min_len=30), C.entrypos))
    assert got == expected_items(F, data, 20, 20, min_len=30) and len(calls) == len(got)


@pytest.mark.gpu
def test_a_decoding_stream_refuses_to_trim(gpu_ctx, reads):
    from fastqandfurious_amd import hip
    fd = os.open(reads[1], os.O_RDONLY)
    try:
        st = hip.FileStream(gpu_ctx, fd, 1 << 20, decode=True)
        with pytest.raises(hip.FFQError) as e:
            st.set_trim(20, 20)
        assert e.value.code == hip.E_ARG
        st.close()
        st = hip.FileStream(gpu_ctx, fd, 1 << 20)
        with pytest.raises(hip.FFQError):
            st.set_trim(128)
        with pytest.raises(hip.FFQError):
            st.trimmed()                    # (a stream that does not trim has no counters)
        st.close()
    finally:
        os.close(fd)

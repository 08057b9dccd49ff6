"""filter_fastq_paired(merged_out=...) on the device: two streams walked in lockstep (hip.PairStream, ffq_pair_set_merge)
against the host route and against the plain loops of tests/merge_expect.py -- three output files, result, MergeReport and
FilterReports.  About 2000 pairs: short, middling and long fragments, Ns, a few wrapped records.  The fills are small and
mate 2's headers are longer than mate 1's, so the two files' fills drift and the rounds cut them at different places."""
import io

import pytest

import merge_expect as M

pytestmark = pytest.mark.gpu

N_PAIRS = 2000
MIN_LEN = 40


@pytest.fixture(scope="module")
def F(pkg):
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


@pytest.fixture(scope="module")
def C(gpu_ctx):
    from fastqandfurious_amd import _fastqandfurious
    return _fastqandfurious


@pytest.fixture(scope="module")
def files():
    r1, r2 = M.records(N_PAIRS)
    return M.file_of(r1), M.file_of(r2)


@pytest.fixture(scope="module")
def want():
    r1, r2 = M.records(N_PAIRS)
    w = M.Expected(r1, r2, min_len=(MIN_LEN, MIN_LEN))
    assert w.kinds >= {"wrapped", "none", "merged"} and w.pairs_merged > 500 and w.written[0] > 300 and w.taken > 0
    assert sum(w.dropped.values()) > 0
    return w


@pytest.fixture(scope="module")
def host(F, files):
    """the host route, once: it does not depend on the size of a fill"""
    return M.run(F, files[0], files[1], F.entrypos, 1 << 14, min_len=MIN_LEN)


def same_reports(a, b):
    for x, y in zip(a, b):
        assert x.before == y.before and x.after == y.after and x.dropped == y.dropped


@pytest.mark.parametrize("fbufsize", (1 << 14, 1 << 15))
def test_device_and_host_write_the_same_three_files(F, C, files, want, host, fbufsize):
    res, o1, o2, om, rep, reps = M.run(F, files[0], files[1], C.entrypos, fbufsize, min_len=MIN_LEN)
    assert (o1, o2, om) == tuple(want.text)
    assert tuple(res) == want.result()
    want.check_report(rep)
    hres, h1, h2, hm, hrep, hreps = host
    assert (o1, o2, om) == (h1, h2, hm) and tuple(res) == tuple(hres)
    assert rep.__dict__ == hrep.__dict__
    same_reports(reps, hreps)
    assert int(reps[0].after.head[0]) + int(reps[0].after.head[1]) == want.written[0]


def test_the_merged_file_scans_back(F, C, gpu_ctx, files, want):
    """the merged text is FASTQ: scanned again on the GPU it yields pairs_merged records, of bases_merged bases"""
    res, _o1, _o2, om, rep, _reps = M.run(F, files[0], files[1], C.entrypos, 1 << 15, min_len=MIN_LEN)
    table, sres = gpu_ctx.scan_host(om)[:2]
    assert int(sres.n_records) == rep.pairs_merged == want.pairs_merged
    assert int((table[:, 3] - table[:, 2]).sum()) == rep.bases_merged


def test_the_rounds_hand_out_the_unmerged_pairs(F, C, files, want):
    """the walk itself: rows(), selected() and merged() of every round add up; the setter's order is enforced"""
    from fastqandfurious_amd import hip
    st1, st2 = C.entrypos.open_stream(io.BytesIO(files[0]), 1 << 14), C.entrypos.open_stream(io.BytesIO(files[1]), 1 << 14)
    for st in (st1, st2):
        st.set_filter(MIN_LEN, None, None)
    ps = hip.PairStream(st1, st2, "any", True)
    try:
        with pytest.raises(hip.FFQError) as ei:                    # needs the overlap
            ps.set_merge()
        assert ei.value.code == hip.E_ARG
        with pytest.raises(hip.FFQError) as ei:                    # not switched on: nothing to report
            ps.merged()
        assert ei.value.code == hip.E_ARG
        ps.set_overlap(F.OverlapRules())
        ps.set_merge()
        total, kept, rounds, text = [0] * 6, 0, 0, bytearray()
        for n_in, n_out, end_state, _mate, _err in ps:
            assert end_state in (hip.END_OK, hip.END_REFILL)
            t, counts = ps.merged()
            idx, pairs = ps.selected()
            assert counts[0] + counts[1] == pairs[0] and counts[1] == n_out and len(t) == counts[2]
            assert len(idx) == n_out and (n_out < 2 or (idx[1:] > idx[:-1]).all()) and (n_out == 0 or idx[-1] < n_in)
            assert ps.rows(1)[0].shape == (n_out, 6) == ps.rows(2)[0].shape
            text += bytes(t)
            total = [a + b for a, b in zip(total, counts)]
            kept += pairs[0]
            rounds += 1
        assert bytes(text) == want.text[2] and kept == want.pairs_out and rounds > 20
        assert total == [want.pairs_merged, want.pairs_out - want.pairs_merged, len(want.text[2]), want.bases_merged, want.overlap_positions,
                         want.taken]
        with pytest.raises(hip.FFQError) as ei:                    # the walk has begun
            ps.set_merge(False)
        assert ei.value.code == hip.E_ARG
    finally:
        ps.close()
        st1.close()
        st2.close()


def test_without_merged_out_nothing_differs(F, C, files):
    """merged_out omitted: the outputs are those of the same call without the argument -- the loop's, with the overlap alone"""
    r1, r2 = M.records(N_PAIRS)
    plain = M.Expected(r1, r2, min_len=(MIN_LEN, MIN_LEN), merge=False)
    assert plain.text[2] == b""
    runs = [M.run(F, files[0], files[1], C.entrypos, 1 << 14, merge=False, min_len=MIN_LEN) for _ in range(2)]
    for res, o1, o2, om, _rep, _reps in runs:
        assert (o1, o2, om) == (plain.text[0], plain.text[1], b"") and tuple(res) == plain.result()
    same_reports(runs[0][5], runs[1][5])

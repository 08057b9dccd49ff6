"""The CPU oracle against the reference: committed golden vectors (captured by
tests/golden/make_golden.py and make_golden_live.py from the reference's Python
module and its C extension)."""
import os
from array import array

import numpy as np
import pytest

from conftest import GOLDEN_DIR, end_matches, golden_file, rows_of

FILES = ("test.fq", "test_longqualityheader.fq", "test_multiline.fq")


@pytest.mark.parametrize("fn", FILES)
def test_files_abspos(golden, oracle, fn):
    data = golden_file(fn)
    for variant, key in ((oracle.VARIANT_C, "c"), (oracle.VARIANT_PY, "py")):
        table, end, status, off = oracle.scan(data, variant=variant)
        for bs, runs in golden["files"][fn]["bufsizes"].items():
            assert rows_of(table) == runs[key]["rows"], (fn, bs, key)
            assert runs[key]["error"] is None and end == 0


def test_survey_known_tables(oracle):
    # SURVEY.md 8c / BASELINE.md section 4
    t, *_ = oracle.scan(golden_file("test.fq"))
    assert rows_of(t) == [[0, 29, 30, 115, 118, 203], [204, 233, 234, 646, 649, 1061],
                          [1062, 1091, 1092, 1225, 1228, 1361], [1362, 1391, 1392, 1446, 1449, 1503]]
    t, *_ = oracle.scan(golden_file("test_multiline.fq"))
    assert rows_of(t)[-1] == [349, 379, 380, 417, 420, 457]


def test_template_prefix_curves(golden, oracle):
    n = 0
    for tpl in golden["templates"]:
        buf = bytes.fromhex(tpl["buf"])
        for rec in tpl["curve"]:
            b = buf[:rec["cut"]]
            st, pos = oracle.entrypos(b, 0, oracle.VARIANT_PY)
            assert [st, [int(x) for x in pos]] == rec["py"], (tpl["name"], rec["cut"])
            if "c" in rec:
                st, pos = oracle.entrypos(b, 0, oracle.VARIANT_C)
                assert [st, [int(x) for x in pos]] == rec["c"], (tpl["name"], rec["cut"])
                n += 1
    assert n > 300


def test_reference_live_test_expectations(oracle):
    """The expectations of the reference's own live tests (tests.py:110-166)."""
    H, S, Q = "foo#2", "AATTGCCG", "3425@!#!"
    MS, MQ = "AATTGCCG\nGCCGTA", "3425@!#!\n255212"
    FINAL = "\n@{header}\n{sequence}\n+\n{quality}\n"
    QUALHEAD = "\n@{header}\n{sequence}\n+\n{quality}\n@bar{header}\n"
    NOQUAL = "\n@{header}\n{sequence}\n+\n"
    for variant in (oracle.VARIANT_C, oracle.VARIANT_PY):
        for tpl in (FINAL, QUALHEAD):
            for s, q in ((S, Q), (MS, MQ)):
                e = tpl.format(header=H, sequence=s, quality=q).encode()
                for cut, want in ((len(H) - 2, 1), (len(H) + len(s) - 1, 3), (len(H) + len(s) + len(q), 5)):
                    st, _ = oracle.entrypos(e[:cut], 0, variant)
                    assert st == want
        # tests.py:56-80 (shadowed there, still the documented behaviour)
        for tpl, want in ((FINAL, 5), (QUALHEAD, 6)):
            for s, q in ((S, Q), (MS, MQ)):
                e = tpl.format(header=H, sequence=s, quality=q).encode()
                st, pos = oracle.entrypos(e, 0, variant)
                assert st == want
                assert e[pos[0] + 1:pos[1]] == H.encode() and e[pos[2]:pos[3]] == s.encode()
                if want == 6:
                    assert e[pos[4]:pos[5]] == q.encode()
    # tests.py:110-138: Python gives 4, C gives 7 (the reference's xfail)
    for s in (S, MS):
        e = NOQUAL.format(header=H, sequence=s).encode()
        assert oracle.entrypos(e, 0, oracle.VARIANT_PY)[0] == 4
        assert oracle.entrypos(e, 0, oracle.VARIANT_C)[0] == 7


def test_edge_corpus(golden, oracle):
    for name, ent in golden["edge"].items():
        data = bytes.fromhex(ent["data"])
        for variant, key in ((oracle.VARIANT_C, "c"), (oracle.VARIANT_PY, "py")):
            table, end, status, off = oracle.scan(data, variant=variant)
            for bs, runs in ent["runs"].items():
                run = runs[key]
                assert rows_of(table) == run["rows"], (name, bs, key)
                assert end_matches(run, end, off), (name, bs, key, run, end, off)


def test_fuzz_corpus(golden, oracle):
    nc = 0
    for i, ent in enumerate(golden["fuzz"]):
        data = bytes.fromhex(ent["data"])
        for variant, key in ((oracle.VARIANT_C, "c"), (oracle.VARIANT_PY, "py")):
            if key not in ent:
                continue
            table, end, status, off = oracle.scan(data, variant=variant)
            assert rows_of(table) == ent[key]["rows"], (i, key)
            assert end_matches(ent[key], end, off), (i, key, ent[key]["error"], end, off)
            nc += key == "c"
    assert nc > 350


def test_arrayadd_known_answers(golden, oracle):
    for k in golden["arrayadd"]["b"]:
        a = np.frombuffer(bytes.fromhex(k["in"]), dtype=np.int8).copy()
        oracle.arrayadd_b(a, k["value"])
        assert a.tobytes().hex() == k["out"]
    for k in golden["arrayadd"]["q"]:
        a = np.array(k["in"], dtype=np.int64)
        oracle.arrayadd_q(a, k["value"])
        assert [int(x) for x in a] == k["out"]
    # SURVEY.md 8c
    a = np.frombuffer(b"!I~5@+\n", dtype=np.int8).copy()
    oracle.arrayadd_b(a, -33)
    assert a.tolist() == [0, 40, 93, 20, 31, 10, -23]


def test_synthetic_tables(oracle, pkg):
    from fastqandfurious_amd import synth
    import os
    from conftest import GOLDEN_DIR
    want = np.load(os.path.join(GOLDEN_DIR, "synth_single_table.npy"))
    data = synth.single(0, 2000, seed=42)
    t, end, st, off = oracle.scan(data)
    assert end == 0 and (t == want).all()
    # closed form on clean 4-line input
    k = np.arange(2000, dtype=np.int64) * 322
    assert (t[:, 0] == k).all() and (t[:, 1] == k + 17).all() and (t[:, 3] == k + 168).all()
    assert (t[:, 4] == k + 171).all() and (t[:, 5] == k + 321).all()
    want = np.load(os.path.join(GOLDEN_DIR, "synth_wrapped_table.npy"))
    data, start = synth.wrapped(0, 2000, seed=43)
    t, end, st, off = oracle.scan(data)
    assert end == 0 and (t == want).all()
    assert (t[:, 0] == start[:-1]).all()


def test_decode_quals(oracle, pkg):
    from fastqandfurious_amd import synth
    data, _ = synth.wrapped(5, 50, seed=43)
    t, *_ = oracle.scan(data)
    q, qoff = oracle.decode_quals(data, t)
    for i in range(len(t)):
        a = array("b")
        a.frombytes(data[t[i, 4]:t[i, 5]].tobytes())
        want = [(x - 33 + 128) % 256 - 128 for x in a]
        assert q[qoff[i]:qoff[i + 1]].tolist() == want
    assert qoff[-1] == q.size


def test_nonsentinel_and_offset(oracle):
    buf = b"\n" + golden_file("test.fq")
    t0, end, st, off = oracle.scan(buf, sentinel=False, eof=True, add=-1)
    t1, *_ = oracle.scan(golden_file("test.fq"))
    assert (t0 == t1).all()
    # start in the middle: search from the second record on
    t2, *_ = oracle.scan(buf, sentinel=False, offset=int(t1[0, 5]), add=-1)
    assert (t2 == t1[1:]).all()
    # not eof: the last record cannot be COMPLETE (needs 2 bytes after pos5)
    t3, end, st, off = oracle.scan(buf, sentinel=False, eof=False, add=-1)
    assert (t3 == t1[:-1]).all() and end == 1 and st == 5 and off == t1[-2, 5] + 1 - 1


# ---- the reference's outputs on seeded random inputs -------------------------
# (captured from the reference's Python module and C extension by tests/golden/make_golden_live.py)
@pytest.fixture(scope="module")
def live():
    with np.load(os.path.join(GOLDEN_DIR, "live_reference.npz"), allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


def test_live_reference_random_prefixes(oracle, live):
    start, data = live["prefix_start"], live["prefix_bytes"]
    n = 0
    for k in range(len(live["prefix_off"])):
        b = data[start[k]:start[k + 1]].tobytes()
        off = int(live["prefix_off"][k])
        so, po = oracle.entrypos(b, off, oracle.VARIANT_PY)
        assert live["prefix_py"][k].tolist() == [so] + po.tolist(), (b, off)
        if not live["prefix_c_ok"][k]:
            continue   # the C scanner reads out of bounds here (_fastqandfurious.c:70-71): not captured
        so, po = oracle.entrypos(b, off, oracle.VARIANT_C)
        assert live["prefix_c"][k].tolist() == [so] + po.tolist(), (b, off)
        n += 1
    assert n > 2500


def test_live_reference_iterator_bufsize_independence(oracle, live):
    data = live["iter_data"].tobytes()
    want, end, st, off = oracle.scan(data)
    assert len(live["iter_bufsizes"]) == 3
    for bs in live["iter_bufsizes"]:
        got = live["iter_rows_%d" % bs].tolist()
        assert got == rows_of(want)


def test_live_reference_arrayadd(oracle, live):
    start = live["aa_start"]
    assert len(start) == 51
    for k in range(len(start) - 1):
        s = slice(start[k], start[k + 1])
        b = live["aa_b_src"][s].copy()
        oracle.arrayadd_b(b, int(live["aa_b_v"][k]))
        assert live["aa_b_out"][s].tolist() == b.tolist()
        b = live["aa_q_src"][s].copy()
        oracle.arrayadd_q(b, int(live["aa_q_v"][k]))
        assert live["aa_q_out"][s].tolist() == b.tolist()

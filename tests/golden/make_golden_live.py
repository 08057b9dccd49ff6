"""Golden vectors for the oracle-vs-reference tests that used to call the reference live.

Run in the build container only (needs /root/reference and oracle/_ref):

    make -C oracle && python tests/golden/make_golden_live.py

tests/test_oracle.py::test_live_reference_* compared the oracle with the reference's Python module
and C extension at test time, so they could only run where the reference was mounted.  This script
runs the same seeded inputs through the reference once and stores inputs and outputs in
live_reference.npz (no reference source is stored):
  prefix_*   3000 random short buffers over "\\n@+ACGT!I#" (seed 7): the buffer, the search offset,
             entrypos' (status, pos[6]) from the Python scanner and from the C scanner (prefix_c_ok
             False where the C scanner would read past the buffer and was not called)
  iter_*     300 wrapped synthetic records (synth.wrapped(100, 300, seed=43)): the abspos rows the
             reference's readfastq_iter yields with its C scanner at fbufsize 700 / 4096 / 65536
  aa_b_*, aa_q_*
             50 random cases (seed 3) of arrayadd_b / arrayadd_q: source, value, result
"""
import io
import os
import sys
from array import array

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import refload  # noqa: E402
import fastqandfurious_amd  # noqa: E402,F401
from fastqandfurious_amd import synth  # noqa: E402

py = refload.load_py()
ext = refload.load_ext()

N_PREFIX = 3000
ITER_BUFSIZES = (700, 4096, 65536)
N_ARRAYADD = 50


def prefixes():
    rng = np.random.default_rng(7)
    alpha = np.frombuffer(b"\n\n@+ACGT!I#", dtype=np.uint8)
    bufs, offs, res_py, res_c, c_ok = [], [], [], [], []
    for _ in range(N_PREFIX):
        L = int(rng.integers(0, 80))
        b = b"\n" + rng.choice(alpha, size=L).tobytes()
        off = int(rng.integers(0, max(L, 1)))
        pp = array("q", [-1] * 6)
        st = py.entrypos(b, off, pp)
        res_py.append([st] + list(pp))
        i = b.find(b"\n@", off)
        ok = not (i >= 0 and i + 2 >= len(b))          # the C scanner reads out of bounds otherwise (_fastqandfurious.c:70-71)
        pc = array("q", [-1] * 6)
        st = ext.entrypos(b, off, pc) if ok else -1
        res_c.append([st] + list(pc))
        bufs.append(b)
        offs.append(off)
        c_ok.append(ok)
    start = np.zeros(N_PREFIX + 1, dtype=np.int64)
    np.cumsum([len(b) for b in bufs], out=start[1:])
    return {"prefix_bytes": np.frombuffer(b"".join(bufs), dtype=np.uint8), "prefix_start": start,
            "prefix_off": np.array(offs, dtype=np.int64), "prefix_py": np.array(res_py, dtype=np.int64),
            "prefix_c": np.array(res_c, dtype=np.int64), "prefix_c_ok": np.array(c_ok, dtype=bool)}


def iterator_rows():
    data, _ = synth.wrapped(100, 300, seed=43)
    data = data.tobytes()
    out = {"iter_data": np.frombuffer(data, dtype=np.uint8), "iter_bufsizes": np.array(ITER_BUFSIZES, dtype=np.int64)}
    for bs in ITER_BUFSIZES:
        rows = [list(p) for p in py.readfastq_iter(io.BytesIO(data), bs, entryfunc=py.entryfunc_abspos, entrypos=ext.entrypos)]
        out["iter_rows_%d" % bs] = np.array(rows, dtype=np.int64).reshape(-1, 6)
    return out


def arrayadd():
    rng = np.random.default_rng(3)
    cols = {k: [] for k in ("b_src", "b_v", "b_out", "q_src", "q_v", "q_out")}
    for _ in range(N_ARRAYADD):
        n = int(rng.integers(0, 200))
        src = rng.integers(-128, 128, size=n, dtype=np.int8)
        v = int(rng.integers(-300, 300))
        a = array("b", src.tolist())
        ext.arrayadd_b(a, v)
        cols["b_src"].append(src)
        cols["b_v"].append(v)
        cols["b_out"].append(np.array(a.tolist(), dtype=np.int8))
        src = rng.integers(-2**62, 2**62, size=n, dtype=np.int64)
        v = int(rng.integers(-2**40, 2**40))
        a = array("q", src.tolist())
        ext.arrayadd_q(a, v)
        cols["q_src"].append(src)
        cols["q_v"].append(v)
        cols["q_out"].append(np.array(a.tolist(), dtype=np.int64))
    start = np.zeros(N_ARRAYADD + 1, dtype=np.int64)
    np.cumsum([len(s) for s in cols["b_src"]], out=start[1:])
    return {"aa_start": start,
            "aa_b_src": np.concatenate(cols["b_src"]), "aa_b_v": np.array(cols["b_v"], dtype=np.int64),
            "aa_b_out": np.concatenate(cols["b_out"]),
            "aa_q_src": np.concatenate(cols["q_src"]), "aa_q_v": np.array(cols["q_v"], dtype=np.int64),
            "aa_q_out": np.concatenate(cols["q_out"])}


if __name__ == "__main__":
    out = {}
    out.update(prefixes())
    out.update(iterator_rows())
    out.update(arrayadd())
    path = os.path.join(HERE, "live_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))

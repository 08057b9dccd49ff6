"""bench.py's own contract: a plain run times the steps and prints the headline line, --dump-outputs writes what the
last timed step computed (the offset table's rows, decoded qualities), --full adds the rest of the line."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
SINGLE_COLS = (0, 17, 18, 168, 171, 321)          # S-single: 322-byte records (synthshard.SyntheticShard.rec_cols)


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


@pytest.mark.parametrize("n, row_lo, sampled", [(700, 0, False), (5000, 37, True)])
def test_dump_outputs_rows_and_qualities(tmp_path, monkeypatch, n, row_lo, sampled):
    """dump_outputs on host tensors: the rows of this rank's records (all of them, or the seeded sample), their quality
    offsets, and the decoded bytes qual[qoff[i] : qoff[i] + pos5 - pos4] of every k-th of them, in float64 / float32."""
    import torch
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_ROWS", 1000)
    monkeypatch.setattr(bench, "DUMP_QUAL_RECORDS", 100)
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 40, size=n + row_lo + 8)
    table = np.zeros((len(lens), 6), dtype=np.int64)
    table[:, 4] = np.arange(len(lens)) * 1000
    table[:, 5] = table[:, 4] + lens
    qoff = np.zeros(len(lens) + 1, dtype=np.int64)
    qoff[1:] = np.cumsum(lens + rng.integers(0, 3, size=len(lens)))       # (segmented: gaps between records)
    qual = rng.integers(-128, 128, size=int(qoff[-1]) + 16, dtype=np.int8)
    out = types.SimpleNamespace(n_own_records=n, row_lo=row_lo)
    bench.dump_outputs(str(tmp_path), torch.from_numpy(table), out, torch.from_numpy(qual), torch.from_numpy(qoff), True)
    got = {f[:-4]: np.load(str(tmp_path / f)) for f in os.listdir(str(tmp_path))}
    assert sorted(got) == ["n_records", "qoff", "qual", "row_index", "rows"]
    assert got["qual"].dtype == np.float32 and all(got[k].dtype == np.float64 for k in got if k != "qual")
    assert got["n_records"].tolist() == [n]
    idx = got["row_index"].astype(np.int64)
    if sampled:
        assert 900 < len(idx) <= 1000 and (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < n
        again = tmp_path / "again"
        bench.dump_outputs(str(again), torch.from_numpy(table), out, torch.from_numpy(qual), torch.from_numpy(qoff), True)
        assert (np.load(str(again / "row_index.npy")) == got["row_index"]).all(), "the sample must not change from run to run"
    else:
        assert idx.tolist() == list(range(n))
    assert (got["rows"] == table[row_lo + idx]).all()
    assert (got["qoff"] == qoff[row_lo + idx]).all()
    sub = (row_lo + idx)[::max(1, len(idx) // 100)][:100]
    want = np.concatenate([qual[qoff[i]:qoff[i] + lens[i]] for i in sub])
    assert (got["qual"] == want).all()


def _run(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_last_step(gpu_ctx, tmp_path):
    """A plain run: the headline line with --steps timed steps, none of the --full extras, and the last step's rows (every
    one of them, 64 MiB of S-single has fewer than DUMP_ROWS records) equal to the generator's closed form."""
    line = _run(["--workload", "single-64m", "--steps", "5", "--warmup", "2", "--dump-outputs", str(tmp_path)])
    assert all(k in line for k in HEADLINE) and "error" not in line
    assert line["steps"] == 5 and line["value"] > 0 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert line["cpu_baseline"] is None
    for k in ("roofline", "path_roofline", "hbm_read_probe", "host_inclusive", "other_workloads", "shapes"):
        assert k not in line, k
    n = line["config"]["records_per_gpu"]
    assert np.load(str(tmp_path / "n_records.npy")).tolist() == [n]
    rows = np.load(str(tmp_path / "rows.npy"))
    assert rows.dtype == np.float64 and rows.shape == (n, 6)
    k = np.arange(n, dtype=np.float64)[:, None] * 322
    assert (rows == k + np.array(SINGLE_COLS, dtype=np.float64)[None, :]).all()
    assert sum(os.path.getsize(str(tmp_path / f)) for f in os.listdir(str(tmp_path))) <= 64 << 20


@pytest.mark.gpu
def test_bench_dumps_decoded_qualities(gpu_ctx, tmp_path):
    """decode-64m (packed stream): qual.npy holds the decoded qualities of every k-th dumped row -- the buffer's quality
    bytes - 33, the buffer regenerated on the host from the same seed."""
    from fastqandfurious_amd import synth
    line = _run(["--workload", "decode-64m", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    n = line["config"]["records_per_gpu"]
    idx = np.load(str(tmp_path / "row_index.npy")).astype(np.int64)
    rows = np.load(str(tmp_path / "rows.npy")).astype(np.int64)
    qoff = np.load(str(tmp_path / "qoff.npy"))
    qual = np.load(str(tmp_path / "qual.npy"))
    assert qual.dtype == np.float32 and len(idx) == n and (np.diff(qoff) == rows[:-1, 5] - rows[:-1, 4]).all()
    data = synth.single(0, n, seed=42)
    sel = np.arange(len(idx))[::max(1, len(idx) // 4096)][:4096]
    want = np.concatenate([data[rows[i, 4]:rows[i, 5]].astype(np.int16) - 33 for i in sel])
    assert qual.shape == want.shape and (qual == want).all()


@pytest.mark.gpu
def test_bench_full_run_carries_the_extras(gpu_ctx):
    """--full: the roofline figures (marked and unpipelined steps after the timed region), the parity check and the read
    probe are back in the line."""
    line = _run(["--workload", "single-64m", "--steps", "4", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-others"])
    assert all(k in line for k in HEADLINE) and line["steps"] == 4 and "error" not in line
    assert line["roofline"]["kernel"] == "k_scan_lines" and line["roofline"]["launches_timed"] >= 20
    assert line["path_roofline"]["device_span_ms"] > 0
    assert "hbm_read_probe" in line

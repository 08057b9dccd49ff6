"""Time of rendering a table as FASTQ text (ffq_table_render_fastq) on the table of the 1 GiB S-single buffer:
  (a) the untouched table,
  (b) the table after a (20, 20) trim and the length filter min_len = 30,
beside (c) the yardstick -- the three ffq_table_gather_column calls (header, sequence, quality) on the untouched table,
summed: the same bytes moved in three passes -- and (d) a device-to-device copy of as many bytes as (a) wrote.  One
process, the four alternating; medians of REPS rounds, wall clock around the blocking calls (each has one host wait).

    python tools/bench_render.py [--bytes N] [--reps 25]
    python tools/bench_render.py --trace       five calls of (a), (b), (c) and nothing else, to run under rocprofv3 --kernel-trace
    python tools/bench_render.py --e2e DIR     fastqandfurious.filter_fastq over the buffer as a file in DIR (page cache) beside
                                               readfastq_iter + entryfunc_qualitytrim(column="entry") + a write per record
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import fastqandfurious_amd
from fastqandfurious_amd import hip, index
from fastqandfurious_amd.sharded import SyntheticShard

COPY_RATE = 6.29e12         # bytes moved per second (read + written) by the device-to-device copy of DESIGN.md

ap = argparse.ArgumentParser()
ap.add_argument("--bytes", type=int, default=1 << 30)
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--e2e", metavar="DIR")
args = ap.parse_args()

ctx = hip.Context(0)
sh = SyntheticShard(ctx, "single", args.bytes, 0, 1, torch.device("cuda:0"))
nbytes = sh.ext_scanned_bytes

if args.e2e:
    from fastqandfurious_amd import fastqandfurious as F, _fastqandfurious as C
    src, dst = os.path.join(args.e2e, "bench_render_in.fq"), os.path.join(args.e2e, "bench_render_out.fq")
    sh.ext[:nbytes].cpu().numpy().tofile(src)
    result = {"bytes": nbytes}
    try:
        for name in ("filter_fastq", "iterator_and_write_loop", "filter_fastq", "iterator_and_write_loop"):
            t0 = time.perf_counter()
            with open(src, "rb") as fh, open(dst, "wb") as fo:
                if name == "filter_fastq":
                    res = F.filter_fastq(fh, fo, 1 << 24, quality_cutoff=(20, 20), min_len=30)
                    n_out = res.records_out
                else:
                    n_out = 0
                    for e in F.readfastq_iter(fh, 1 << 24, F.entryfunc_qualitytrim(20, 20, min_len=30, column="entry"), C.entrypos):
                        if e is not None:
                            fo.write(b"@%s\n%s\n+\n%s\n" % e)
                            n_out += 1
            dt = time.perf_counter() - t0
            r = result.setdefault(name, {"s": [], "records_out": n_out, "bytes_out": os.path.getsize(dst)})
            r["s"].append(dt)
            assert (r["records_out"], r["bytes_out"]) == (n_out, os.path.getsize(dst))
        for name in ("filter_fastq", "iterator_and_write_loop"):
            result[name]["GB_per_s_in"] = nbytes / min(result[name]["s"]) / 1e9
        assert result["filter_fastq"]["bytes_out"] == result["iterator_and_write_loop"]["bytes_out"]
        result["speedup"] = min(result["iterator_and_write_loop"]["s"]) / min(result["filter_fastq"]["s"])
    finally:
        for p in (src, dst):
            if os.path.exists(p):
                os.unlink(p)
    print(json.dumps(result))
    sys.exit(0)

table = torch.empty((sh.max_records, 6), dtype=torch.int64, device="cuda")
rc, res = ctx.scan_device(sh.ext.data_ptr(), nbytes, table.data_ptr(), sh.max_records)
n = int(res.n_records)
table = table[:n]
trimmed, tstats = index.trim_rows_device(ctx, sh.ext[:nbytes], table, 20, 20)
kept = index.select_rows_device(ctx, trimmed, 30, None)
k = int(kept.shape[0])
out = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda")
out2 = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda")
off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
col = {c: torch.empty(int((table[:, b] - table[:, a] - s).sum().item()) + 16, dtype=torch.int8, device="cuda")
       for c, (a, s, b) in hip.Context.COLUMNS.items()}
torch.cuda.synchronize()


def render(t, rows):
    rc, stats = ctx.table_render_fastq(sh.ext.data_ptr(), nbytes, t.data_ptr(), rows, out.data_ptr(), out.numel(), off.data_ptr())
    assert rc == 0
    return stats


def gathers():
    total = 0
    for c, buf in col.items():
        rc, nb = ctx.table_gather_column(sh.ext.data_ptr(), nbytes, table.data_ptr(), n, c, buf.data_ptr(), buf.numel(), off.data_ptr())
        assert rc == 0
        total += nb
    return total


stats_a, stats_b, gathered = render(table, n), render(kept, k), gathers()
assert stats_a[0] == nbytes and stats_a[1] == n and gathered == nbytes - 6 * n


def d2d():
    out2[:stats_a[0]].copy_(out[:stats_a[0]])
    torch.cuda.synchronize()


calls = {"render_all": lambda: render(table, n), "render_trimmed_filtered": lambda: render(kept, k), "three_gathers": gathers,
         "copy_d2d": d2d}
if args.trace:
    for name in ("render_all", "render_trimmed_filtered", "three_gathers"):
        for _ in range(5):
            calls[name]()
    print(json.dumps({"rows": n, "kept": k}))
    sys.exit(0)

ts = {name: [] for name in calls}
for name, call in calls.items():
    call()
for _ in range(args.reps):
    for name, call in calls.items():             # alternating: every round times each once
        t0 = time.perf_counter()
        call()
        ts[name].append(time.perf_counter() - t0)
ms = {name: statistics.median(v) * 1e3 for name, v in ts.items()}
result = {"rows": n, "bytes": nbytes, "reps": args.reps, "kept_rows": k, "trim_stats": list(tstats)}
for name, stats in (("render_all", stats_a), ("render_trimmed_filtered", stats_b)):
    rows = stats[1]
    # bytes the algorithm moves: the slices read and the text written, the 48-byte rows read twice (lengths, copy), the offsets
    traffic = (stats[0] - 6 * rows) + stats[0] + 2 * 48 * rows + 8 * (rows + 1)
    result[name] = {"ms": ms[name], "bytes_out": stats[0], "rows": rows, "traffic_bytes": traffic,
                    "traffic_TB_per_s": traffic / ms[name] / 1e9, "of_copy_rate": traffic / (ms[name] * 1e-3) / COPY_RATE,
                    "x_three_gathers": ms[name] / ms["three_gathers"]}
result["three_gathers"] = {"ms": ms["three_gathers"], "bytes_out": gathered}
result["copy_d2d"] = {"ms": ms["copy_d2d"], "bytes": stats_a[0], "TB_per_s": 2 * stats_a[0] / ms["copy_d2d"] / 1e9}
result["render_all"]["x_copy_d2d"] = ms["render_all"] / ms["copy_d2d"]
result["render_no_slower_than_three_gathers"] = ms["render_all"] <= ms["three_gathers"]
print(json.dumps(result))

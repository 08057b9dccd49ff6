"""Time of the quality trimming of a table (ffq_table_trim_quality) on the table of the 1 GiB S-single buffer, beside the
length filter keeping every row of the same table (ffq_table_select_seqlen_idx: the yardstick) and a device-to-device copy
of the table.  Medians of REPS calls, wall clock around the blocking call (each has one host wait).

    python tools/bench_trim.py [--bytes N] [--reps 25] [--trace]     (--trace: five calls per pair of cutoffs and nothing
                                                                       else, to run under rocprofv3 --kernel-trace)
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import fastqandfurious_amd
from fastqandfurious_amd import hip
from fastqandfurious_amd.sharded import SyntheticShard

ap = argparse.ArgumentParser()
ap.add_argument("--bytes", type=int, default=1 << 30)
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()

ctx = hip.Context(0)
sh = SyntheticShard(ctx, "single", args.bytes, 0, 1, torch.device("cuda:0"))
table = torch.empty((sh.max_records, 6), dtype=torch.int64, device="cuda")
rc, res = ctx.scan_device(sh.ext.data_ptr(), sh.ext_scanned_bytes, table.data_ptr(), sh.max_records)
n = int(res.n_records)
out = torch.empty_like(table)
idx = torch.empty(sh.max_records, dtype=torch.int64, device="cuda")
torch.cuda.synchronize()


def median_ms(call):
    call()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def trim(cf, cb):
    return ctx.table_trim_quality(sh.ext.data_ptr(), sh.ext_scanned_bytes, table.data_ptr(), n, cb, cf, d_out=out.data_ptr())


if args.trace:
    print(json.dumps({"rows": n, "stats": [[trim(cf, cb) for _ in range(5)][-1] for cf, cb in ((0, 10), (20, 20), (30, 30))]}))
    sys.exit(0)

result = {"rows": n, "bytes": sh.ext_scanned_bytes, "reps": args.reps}
result["select_all_ms"] = median_ms(lambda: ctx.table_select_seqlen_idx(table.data_ptr(), n, 0, 1 << 40, out.data_ptr(), idx.data_ptr()))


def d2d():
    out[:n].copy_(table[:n])
    torch.cuda.synchronize()


result["copy_d2d_ms"] = median_ms(d2d)
for cf, cb in ((0, 10), (20, 20), (30, 30)):
    ms = median_ms(lambda: trim(cf, cb))
    changed, removed, skipped = trim(cf, cb)
    result["trim_%d_%d" % (cf, cb)] = {"ms": ms, "x_select": ms / result["select_all_ms"], "rows_changed": changed,
                                       "bases_removed": removed, "rows_skipped": skipped,
                                       "G_rows_per_s": n / ms / 1e6}
print(json.dumps(result))

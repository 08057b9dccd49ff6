"""Time of the ends pass over a table (ffq_table_trim_ends with front, right and tail windows of 4 at quality 20) on the table of
the S-single buffer (150-base reads) beside, in the same process and on the same table, the yardstick: the quality trimming at
(20, 20) (ffq_table_trim_quality: the same frame, the quality line of every row read once, the same rows stored).  hipEvent
times on the context's stream around each call (a call has a host wait inside: its second event is recorded when that wait has
returned); median, minimum and maximum of REPS calls, the two passes in alternating calls.

    python tools/bench_ends.py [--bytes 1073741824] [--reps 25]
    python tools/bench_ends.py --trace            five calls of each and nothing else, to run under rocprofv3 --kernel-trace
"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import fastqandfurious_amd
from fastqandfurious_amd import fastqandfurious as F, hip
from fastqandfurious_amd.sharded import SyntheticShard

ap = argparse.ArgumentParser()
ap.add_argument("--bytes", type=int, default=1 << 30)
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()

ctx = hip.Context(0)
sh = SyntheticShard(ctx, "single", args.bytes, 0, 1, torch.device("cuda:0"))
nb = sh.ext_scanned_bytes
table = torch.empty((sh.max_records, 6), dtype=torch.int64, device="cuda")
rc, res = ctx.scan_device(sh.ext.data_ptr(), nb, table.data_ptr(), sh.max_records)
n = int(res.n_records)
out = torch.empty_like(table)
torch.cuda.synchronize()
stream = torch.cuda.ExternalStream(ctx.stream())
RULES = hip.ends_rules_struct(F.EndRules(front=(4, 20), right=(4, 20), tail=(4, 20)), 33)


def quality():
    return ctx.table_trim_quality(sh.ext.data_ptr(), nb, table.data_ptr(), n, 20, 20, d_out=out.data_ptr())


def ends():
    return ctx.table_trim_ends(sh.ext.data_ptr(), nb, table.data_ptr(), n, RULES, d_out=out.data_ptr())


CALLS = (("trim_quality_20_20", quality), ("trim_ends_4_20", ends))

if args.trace:
    print(json.dumps({"rows": n, "stats": {name: [call() for _ in range(5)][-1] for name, call in CALLS}}))
    sys.exit(0)

for _name, call in CALLS:                               # (warm-up: code objects, the long list's room)
    call()
ctx.sync()
ts = {name: [] for name, _call in CALLS}
for _ in range(args.reps):
    for name, call in CALLS:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        ts[name].append(e0.elapsed_time(e1))
result = {"rows": n, "bytes": nb, "reps": args.reps}
for name, call in CALLS:
    t = ts[name]
    result[name] = {"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "stats": list(call()),
                    "G_rows_per_s": n / statistics.median(t) / 1e6}
result["ends_over_quality"] = result["trim_ends_4_20"]["ms"] / result["trim_quality_20_20"]["ms"]
print(json.dumps(result))

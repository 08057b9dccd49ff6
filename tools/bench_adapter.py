"""Time of the 3' adapter trimming of a table (ffq_table_trim_adapter) on the table of the 1 GiB S-single buffer, beside -- in
the same process, on the same table -- the length filter keeping every row (ffq_table_select_seqlen_idx) and the quality
trimming at (0, 10) (ffq_table_trim_quality: the yardstick, it moves about the same bytes).  The adapter is implanted on the
device into `--share` of the reads (every 1 / share-th), at seeded uniform positions of the read, the part that overhangs
the 3' end cut off.  Medians of REPS calls, wall clock around the blocking call (each has one host wait).

    python tools/bench_adapter.py [--bytes N] [--reps 25] [--share 0.5] [--trace]     (--trace: five adapter calls and nothing
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
ap.add_argument("--share", type=float, default=0.5)
ap.add_argument("--adapter", default="AGATCGGAAGAGC")
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
adapter = args.adapter.encode()

ctx = hip.Context(0)
sh = SyntheticShard(ctx, "single", args.bytes, 0, 1, torch.device("cuda:0"))
table = torch.empty((sh.max_records, 6), dtype=torch.int64, device="cuda")
rc, res = ctx.scan_device(sh.ext.data_ptr(), sh.ext_scanned_bytes, table.data_ptr(), sh.max_records)
n = int(res.n_records)

# ---- the adapter into every `every`-th read: bytes [p, min(p + m, length)) of its sequence, p uniform in [0, length) ----
every = max(1, round(1 / args.share))
g = torch.Generator(device="cuda")
g.manual_seed(args.seed)
n_implanted = 0
for lo in range(0, n, 1 << 20):                         # (a million rows at a time: the index tensors stay small)
    sel = table[lo:min(lo + (1 << 20), n)][::every]
    length = sel[:, 3] - sel[:, 2]
    p = (torch.rand(sel.shape[0], generator=g, device="cuda") * length).long()
    j = torch.arange(len(adapter), device="cuda")
    inside = (p[:, None] + j[None, :]) < length[:, None]
    at = (sel[:, 2:3] + p[:, None] + j[None, :])[inside]
    sh.ext[at] = torch.tensor(list(adapter), dtype=torch.uint8, device="cuda").expand(sel.shape[0], -1)[inside]
    n_implanted += int(sel.shape[0])
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


def cut():
    return ctx.table_trim_adapter(sh.ext.data_ptr(), sh.ext_scanned_bytes, table.data_ptr(), n, adapter, 100, 3, d_out=out.data_ptr())


if args.trace:
    print(json.dumps({"rows": n, "stats": [cut() for _ in range(5)][-1]}))
    sys.exit(0)

result = {"rows": n, "bytes": sh.ext_scanned_bytes, "reps": args.reps, "adapter": args.adapter, "err_permille": 100, "min_overlap": 3,
          "rows_implanted": n_implanted, "seed": args.seed}
result["select_all_ms"] = median_ms(lambda: ctx.table_select_seqlen_idx(table.data_ptr(), n, 0, 1 << 40, out.data_ptr(), idx.data_ptr()))
ms_q = median_ms(lambda: ctx.table_trim_quality(sh.ext.data_ptr(), sh.ext_scanned_bytes, table.data_ptr(), n, 10, 0, d_out=out.data_ptr()))
result["trim_quality_0_10_ms"] = ms_q
ms = median_ms(cut)
changed, removed, skipped = cut()
result["trim_adapter"] = {"ms": ms, "x_trim_quality": ms / ms_q, "x_select": ms / result["select_all_ms"], "rows_changed": changed,
                          "bases_removed": removed, "rows_skipped": skipped, "G_rows_per_s": n / ms / 1e6}
print(json.dumps(result))

"""Time of the poly-tail trimming of a table (ffq_table_trim_poly: poly-G, and poly-X) on the table of the S-single buffer
(150-base reads) -- as generated, and with G tails of 20..100 bases planted on a share of the reads -- beside, in the same
process and on the same table, the yardstick: the quality trimming at (20, 20) (ffq_table_trim_quality: the same frame, one
line of every row read once, the same rows stored).  hipEvent times on the context's stream around each call (a call has a
host wait inside: its second event is recorded when that wait has returned); median, minimum and maximum of REPS calls.

    python tools/bench_poly.py [--bytes 1073741824] [--reps 25] [--share 0.2]
    python tools/bench_poly.py --trace            five calls of each on the planted table and nothing else, to run under
                                                  rocprofv3 --kernel-trace
    python tools/bench_poly.py --e2e DIR [--runs 5]
                                                  fastqandfurious.filter_fastq(quality_cutoff=(20, 20), min_len=30) over the
                                                  planted buffer as a file in DIR (page cache), without and with poly_g=10, in
                                                  alternating runs behind a warm-up of each
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
ap.add_argument("--share", type=float, default=0.2)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--e2e", metavar="DIR")
ap.add_argument("--runs", type=int, default=5)
args = ap.parse_args()

ctx = hip.Context(0)
sh = SyntheticShard(ctx, "single", args.bytes, 0, 1, torch.device("cuda:0"))
nb = sh.ext_scanned_bytes
table = torch.empty((sh.max_records, 6), dtype=torch.int64, device="cuda")
rc, res = ctx.scan_device(sh.ext.data_ptr(), nb, table.data_ptr(), sh.max_records)
n = int(res.n_records)
out = torch.empty_like(table)
torch.cuda.synchronize()


def plant(share, seed=1):
    """G over the last 20..100 bases of `share` of the reads (the rows index the buffer's bytes)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    pick = torch.rand(n, generator=g, device="cuda") < share
    length = torch.randint(20, 101, (n,), generator=g, device="cuda")
    end = table[:n, 3][pick]
    begin = torch.maximum(end - length[pick], table[:n, 2][pick])
    delta = torch.zeros(nb + 1, dtype=torch.int32, device="cuda")
    delta.index_add_(0, begin, torch.ones_like(begin, dtype=torch.int32))
    delta.index_add_(0, end, -torch.ones_like(end, dtype=torch.int32))
    sh.ext[:nb][torch.cumsum(delta[:nb], 0) > 0] = ord("G")
    torch.cuda.synchronize()
    return int(pick.sum())


if args.e2e:
    from fastqandfurious_amd import fastqandfurious as F
    planted = plant(args.share)
    src, dst = os.path.join(args.e2e, "bench_poly_in.fq"), os.path.join(args.e2e, "bench_poly_out.fq")
    sh.ext[:nb].cpu().numpy().tofile(src)
    del sh, table, out
    legs = {"plain": {}, "poly_g": {"poly_g": 10}}
    result = {"bytes": nb, "runs": args.runs, "planted_reads": planted, "legs": {k: {"s": []} for k in legs}}
    try:
        for run in range(args.runs + 1):                     # (the first run of each leg is a warm-up and is not kept)
            for name, kw in legs.items():
                t0 = time.perf_counter()
                with open(src, "rb") as fh, open(dst, "wb") as fo:
                    r = F.filter_fastq(fh, fo, 1 << 24, quality_cutoff=(20, 20), min_len=30, **kw)
                dt = time.perf_counter() - t0
                leg = result["legs"][name]
                assert leg.setdefault("result", list(r)) == list(r)
                if run:
                    leg["s"].append(dt)
        for leg in result["legs"].values():
            s = leg["s"]
            leg.update(median_s=statistics.median(s), min_s=min(s), max_s=max(s), GB_per_s_in=nb / statistics.median(s) / 1e9)
        result["poly_g_over_plain"] = result["legs"]["poly_g"]["median_s"] / result["legs"]["plain"]["median_s"]
    finally:
        for p in (src, dst):
            if os.path.exists(p):
                os.unlink(p)
    print(json.dumps(result))
    sys.exit(0)

stream = torch.cuda.ExternalStream(ctx.stream())


def timed(call, reps):
    call()
    ctx.sync()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def quality():
    return ctx.table_trim_quality(sh.ext.data_ptr(), nb, table.data_ptr(), n, 20, 20, d_out=out.data_ptr())


def poly(base):
    return ctx.table_trim_poly(sh.ext.data_ptr(), nb, table.data_ptr(), n, base, 10, d_out=out.data_ptr())


CALLS = (("trim_quality_20_20", quality), ("poly_g", lambda: poly(b"G")), ("poly_x", lambda: poly(None)))

if args.trace:
    plant(args.share)
    print(json.dumps({"rows": n, "stats": {name: [call() for _ in range(5)][-1] for name, call in CALLS}}))
    sys.exit(0)

result = {"rows": n, "bytes": nb, "reps": args.reps, "mixes": {}}
for mix, share in (("as_generated", 0.0), ("planted", args.share)):
    planted = plant(share) if share else 0
    r = {"planted_reads": planted}
    for name, call in CALLS:
        r[name] = timed(call, args.reps)
        r[name]["stats"] = list(call())
        r[name]["G_rows_per_s"] = n / r[name]["ms"] / 1e6
    q = r["trim_quality_20_20"]
    for name in ("poly_g", "poly_x"):
        r[name]["x_quality"] = r[name]["ms"] / q["ms"]
        # the aim: inside the quality trim's own min - max, widened by a quarter
        r[name]["inside_quality_band"] = q["min_ms"] - 0.25 * (q["max_ms"] - q["min_ms"]) <= r[name]["ms"] <= q["max_ms"] + 0.25 * (q["max_ms"] - q["min_ms"])
    result["mixes"][mix] = r
print(json.dumps(result))

"""Time of the two UMI table calls on the table of the S-single buffer (150-base reads), each beside its yardstick in the same
process and on the same table:

    ffq_table_take_umi (8, 0)                       against   ffq_table_trim_quality (0, 10): the row-edit yardstick (the same
                                                              frame, lines of every row read once, the same rows stored)
    ffq_table_render_fastq_umi (read1, the rendered  against   ffq_table_render_fastq on the same table (the rows with their UMI
    table its own source)                                     taken: the same bytes to copy but for the insert)

hipEvent times on the context's stream around each call (a call has a host wait inside: its second event is recorded when that
wait has returned); median, minimum and maximum of REPS calls.

    python tools/bench_umi.py [--bytes 1073741824] [--reps 25]
    python tools/bench_umi.py --trace              five calls of each and nothing else, to run under rocprofv3 --kernel-trace
    python tools/bench_umi.py --e2e DIR [--runs 5]
                                                   fastqandfurious.filter_fastq(min_len=30) over the buffer as a file in DIR
                                                   (page cache), without and with umi=UmiRules("read1", 8), in alternating runs
                                                   behind a warm-up of each
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
ap.add_argument("--e2e", metavar="DIR")
ap.add_argument("--runs", type=int, default=5)
args = ap.parse_args()

ctx = hip.Context(0)
sh = SyntheticShard(ctx, "single", args.bytes, 0, 1, torch.device("cuda:0"))
nb = sh.ext_scanned_bytes

if args.e2e:
    from fastqandfurious_amd import fastqandfurious as F
    src, dst = os.path.join(args.e2e, "bench_umi_in.fq"), os.path.join(args.e2e, "bench_umi_out.fq")
    sh.ext[:nb].cpu().numpy().tofile(src)
    del sh
    legs = {"plain": {}, "umi": {"umi": F.UmiRules("read1", 8)}}
    result = {"bytes": nb, "runs": args.runs, "legs": {k: {"s": []} for k in legs}}
    try:
        for run in range(args.runs + 1):                     # (the first run of each leg is a warm-up and is not kept)
            for name, kw in legs.items():
                t0 = time.perf_counter()
                with open(src, "rb") as fh, open(dst, "wb") as fo:
                    r = F.filter_fastq(fh, fo, 1 << 24, min_len=30, **kw)
                dt = time.perf_counter() - t0
                leg = result["legs"][name]
                assert leg.setdefault("result", list(r)) == list(r)
                if run:
                    leg["s"].append(dt)
        for leg in result["legs"].values():
            s = leg["s"]
            leg.update(median_s=statistics.median(s), min_s=min(s), max_s=max(s), GB_per_s_in=nb / statistics.median(s) / 1e9)
        result["umi_over_plain"] = result["legs"]["umi"]["median_s"] / result["legs"]["plain"]["median_s"]
    finally:
        for p in (src, dst):
            if os.path.exists(p):
                os.unlink(p)
    print(json.dumps(result))
    sys.exit(0)

table = torch.empty((sh.max_records, 6), dtype=torch.int64, device="cuda")
rc, res = ctx.scan_device(sh.ext.data_ptr(), nb, table.data_ptr(), sh.max_records)
n = int(res.n_records)
out = torch.empty_like(table)
taken = torch.empty_like(table)
rules = hip.UmiRulesStruct(hip.UMI_READ1, 8, 0, ord(":"), 0)
text = torch.empty(nb + 1 + 12 * n, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
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
    return ctx.table_trim_quality(sh.ext.data_ptr(), nb, table.data_ptr(), n, 10, 0, d_out=out.data_ptr())


def take():
    return ctx.table_take_umi(sh.ext.data_ptr(), nb, table.data_ptr(), n, 8, 0, d_out=taken.data_ptr())


def render():
    return ctx.table_render_fastq(sh.ext.data_ptr(), nb, taken.data_ptr(), n, text.data_ptr(), text.numel())[1]


def render_umi():
    v = hip.table_view(sh.ext.data_ptr(), nb, taken.data_ptr())
    return ctx.table_render_fastq_umi(v, n, rules, text.data_ptr(), text.numel(), None, v, None)[1]


take()
CALLS = (("trim_quality_0_10", quality), ("take_umi_8_0", take), ("render_fastq", render), ("render_fastq_umi", render_umi))

if args.trace:
    print(json.dumps({"rows": n, "stats": {name: [call() for _ in range(5)][-1] for name, call in CALLS}}))
    sys.exit(0)

result = {"rows": n, "bytes": nb, "reps": args.reps}
for name, call in CALLS:
    result[name] = timed(call, args.reps)
    result[name]["stats"] = list(call())
    result[name]["G_rows_per_s"] = n / result[name]["ms"] / 1e6
result["take_umi_8_0"]["x_trim_quality"] = result["take_umi_8_0"]["ms"] / result["trim_quality_0_10"]["ms"]
result["render_fastq_umi"]["x_render_fastq"] = result["render_fastq_umi"]["ms"] / result["render_fastq"]["ms"]
print(json.dumps(result))

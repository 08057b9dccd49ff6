"""Time of the statistics of a table (ffq_table_stats, max_cycles 150 and 512) on the table of the S-single buffer at 64 MiB
and 1 GiB, beside -- in the same process, on the same table -- the quality trimming at (20, 20) (ffq_table_trim_quality: it
touches the same quality bytes) and the traffic floor: rows * (2 * 150 + 48) bytes at the device-to-device copy rate of
README.md.  hipEvent times on the context's stream around each call (the trim has a host wait inside: its second event is
recorded when that wait has returned); medians of REPS calls.

    python tools/bench_stats.py [--sizes 67108864,1073741824] [--reps 25]
    python tools/bench_stats.py --trace            five calls of each at 1 GiB and nothing else, to run under rocprofv3 --kernel-trace
    python tools/bench_stats.py --e2e DIR [--runs 5] [--no-report]
                                                   fastqandfurious.filter_fastq(quality_cutoff=(20, 20), min_len=30) over the 1 GiB
                                                   buffer as a file in DIR (page cache), RUNS times without and RUNS times with a
                                                   report, alternating (--no-report: without only -- what an older tree can run)
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import fastqandfurious_amd
from fastqandfurious_amd import hip
from fastqandfurious_amd.sharded import SyntheticShard

COPY_RATE = 6.29e12         # bytes moved per second (read + written) by the device-to-device copy of README.md

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="%d,%d" % (64 << 20, 1 << 30))
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--e2e", metavar="DIR")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--no-report", action="store_true")
args = ap.parse_args()

ctx = hip.Context(0)

if args.e2e:
    from fastqandfurious_amd import fastqandfurious as F
    sh = SyntheticShard(ctx, "single", 1 << 30, 0, 1, torch.device("cuda:0"))
    nbytes = sh.ext_scanned_bytes
    src, dst = os.path.join(args.e2e, "bench_stats_in.fq"), os.path.join(args.e2e, "bench_stats_out.fq")
    sh.ext[:nbytes].cpu().numpy().tofile(src)
    del sh
    result = {"bytes": nbytes, "runs": args.runs}
    try:
        for run in range(args.runs + 1):                     # (the first round is a warm-up and is not kept)
            for name in ("plain",) if args.no_report else ("plain", "report"):
                kw = {"report": F.FilterReport(512)} if name == "report" else {}
                t0 = time.perf_counter()
                with open(src, "rb") as fh, open(dst, "wb") as fo:
                    res = F.filter_fastq(fh, fo, 1 << 24, quality_cutoff=(20, 20), min_len=30, **kw)
                dt = time.perf_counter() - t0
                r = result.setdefault(name, {"s": [], "result": list(res)})
                assert r["result"] == list(res)
                if run:
                    r["s"].append(dt)
                if kw:
                    rep = kw["report"]
                    assert rep.before.reads == res.records_in and rep.after.reads == res.records_out
                    result["report_reads_bases"] = [rep.before.reads, rep.before.bases, rep.after.reads, rep.after.bases]
        for name in ("plain", "report"):
            if name in result:
                s = result[name]["s"]
                result[name].update(median_s=statistics.median(s), min_s=min(s), max_s=max(s), GB_per_s_in=nbytes / statistics.median(s) / 1e9)
        if "report" in result:
            result["report_minus_plain_median_s"] = result["report"]["median_s"] - result["plain"]["median_s"]
    finally:
        for p in (src, dst):
            if os.path.exists(p):
                os.unlink(p)
    print(json.dumps(result))
    sys.exit(0)

stream = torch.cuda.ExternalStream(ctx.stream())


def median_ms(call, reps):
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
    return statistics.median(ts)


results = []
for size in ([1 << 30] if args.trace else [int(x) for x in args.sizes.split(",")]):
    sh = SyntheticShard(ctx, "single", size, 0, 1, torch.device("cuda:0"))
    table = torch.empty((sh.max_records, 6), dtype=torch.int64, device="cuda")
    rc, res = ctx.scan_device(sh.ext.data_ptr(), sh.ext_scanned_bytes, table.data_ptr(), sh.max_records)
    n = int(res.n_records)
    out = torch.empty_like(table)
    blocks = {C: torch.zeros(hip.stats_words(C), dtype=torch.int64, device="cuda") for C in (150, 512)}
    torch.cuda.synchronize()

    def stats(C):
        return ctx.table_stats(sh.ext.data_ptr(), sh.ext_scanned_bytes, table.data_ptr(), n, blocks[C].data_ptr(), 33, C, wait=False)

    def trim():
        return ctx.table_trim_quality(sh.ext.data_ptr(), sh.ext_scanned_bytes, table.data_ptr(), n, 20, 20, d_out=out.data_ptr())

    if args.trace:
        for call in (lambda: stats(150), lambda: stats(512), trim):
            for _ in range(5):
                call()
        ctx.sync()
        print(json.dumps({"rows": n}))
        sys.exit(0)
    floor_ms = n * (2 * 150 + 48) / COPY_RATE * 1e3
    r = {"rows": n, "bytes": sh.ext_scanned_bytes, "reps": args.reps, "traffic_floor_ms": floor_ms}
    r["trim_quality_20_20"] = {"ms": median_ms(trim, args.reps)}
    r["trim_quality_20_20"]["x_floor"] = r["trim_quality_20_20"]["ms"] / floor_ms
    for C in (150, 512):
        ms = median_ms(lambda: stats(C), args.reps)
        ctx.sync()
        head = blocks[C][:8].cpu().tolist()
        r["stats_%d" % C] = {"ms": ms, "x_floor": ms / floor_ms, "x_trim_quality": ms / r["trim_quality_20_20"]["ms"],
                             "G_rows_per_s": n / ms / 1e6, "head": head}
        assert head[0] == n and head[1] == 0
    results.append(r)
    del sh, table, out, blocks
    torch.cuda.empty_cache()
print(json.dumps(results))

"""Time of the content filter of a table (ffq_table_select_reads: every rule on, and max_n alone) on the table of the S-single
buffer at 64 MiB and 1 GiB, beside -- in the same process, on the same table -- the yardsticks: the statistics at max_cycles
150 (ffq_table_stats: it reads the same two lines of every row), the quality trimming at (20, 20) (ffq_table_trim_quality),
the length filter (ffq_table_select_seqlen: no buffer read) and the traffic floor: rows * (2 * 150 + 48) bytes at the
device-to-device copy rate of README.md.  hipEvent times on the context's stream around each call (a call with a host wait
inside has its second event recorded when that wait has returned); median, minimum and maximum of REPS calls.

    python tools/bench_filter.py [--sizes 67108864,1073741824] [--reps 25]
    python tools/bench_filter.py --trace           five calls of each at 1 GiB and nothing else, to run under rocprofv3 --kernel-trace
    python tools/bench_filter.py --e2e DIR [--runs 5] [--content]
                                                   fastqandfurious.filter_fastq(quality_cutoff=(20, 20), min_len=30) over the 1 GiB
                                                   buffer as a file in DIR (page cache), RUNS times behind a warm-up; --content: with
                                                   content=ContentRules(max_n=0, max_expected_errors=1.0).  Without --content it
                                                   is what `tools/bench_stats.py --e2e DIR --no-report` times on an older tree.
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
ap.add_argument("--content", action="store_true")
args = ap.parse_args()

ctx = hip.Context(0)

if args.e2e:
    from fastqandfurious_amd import fastqandfurious as F
    sh = SyntheticShard(ctx, "single", 1 << 30, 0, 1, torch.device("cuda:0"))
    nbytes = sh.ext_scanned_bytes
    src, dst = os.path.join(args.e2e, "bench_filter_in.fq"), os.path.join(args.e2e, "bench_filter_out.fq")
    sh.ext[:nbytes].cpu().numpy().tofile(src)
    del sh
    result = {"bytes": nbytes, "runs": args.runs, "content": bool(args.content), "s": []}
    try:
        for run in range(args.runs + 1):                     # (the first run is a warm-up and is not kept)
            kw = {"content": F.ContentRules(max_n=0, max_expected_errors=1.0), "report": F.FilterReport(150)} if args.content else {}
            t0 = time.perf_counter()
            with open(src, "rb") as fh, open(dst, "wb") as fo:
                res = F.filter_fastq(fh, fo, 1 << 24, quality_cutoff=(20, 20), min_len=30, **kw)
            dt = time.perf_counter() - t0
            assert result.setdefault("result", list(res)) == list(res)
            if kw:
                result["dropped"] = kw["report"].dropped
            if run:
                result["s"].append(dt)
        s = result["s"]
        result.update(median_s=statistics.median(s), min_s=min(s), max_s=max(s), GB_per_s_in=nbytes / statistics.median(s) / 1e9)
    finally:
        for p in (src, dst):
            if os.path.exists(p):
                os.unlink(p)
    print(json.dumps(result))
    sys.exit(0)

stream = torch.cuda.ExternalStream(ctx.stream())
ALL_RULES = hip.ContentRulesStruct(33, 5, 20, 15, 40, 30, 10 * 10 ** 6)          # every rule on
MAX_N = hip.ContentRulesStruct(33, 0, 0, 15, -1, 0, -1)                           # --max-n 0


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


results = []
for size in ([1 << 30] if args.trace else [int(x) for x in args.sizes.split(",")]):
    sh = SyntheticShard(ctx, "single", size, 0, 1, torch.device("cuda:0"))
    table = torch.empty((sh.max_records, 6), dtype=torch.int64, device="cuda")
    rc, res = ctx.scan_device(sh.ext.data_ptr(), sh.ext_scanned_bytes, table.data_ptr(), sh.max_records)
    n = int(res.n_records)
    out = torch.empty_like(table)
    idx = torch.empty((sh.max_records,), dtype=torch.int64, device="cuda")
    block = torch.zeros(hip.stats_words(150), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    buf, nb = sh.ext.data_ptr(), sh.ext_scanned_bytes
    last = {}

    def stats():
        return ctx.table_stats(buf, nb, table.data_ptr(), n, block.data_ptr(), 33, 150, wait=False)

    def trim():
        return ctx.table_trim_quality(buf, nb, table.data_ptr(), n, 20, 20, d_out=out.data_ptr())

    def seqlen():
        return ctx.table_select_seqlen_idx(table.data_ptr(), n, 30, 1 << 62, out.data_ptr(), idx.data_ptr())

    def reads(rules, name):
        last[name] = ctx.table_select_reads(buf, nb, table.data_ptr(), n, out.data_ptr(), rules, 30, None, idx.data_ptr())

    calls = (("trim_quality_20_20", trim), ("stats_150", stats), ("select_seqlen", seqlen),
             ("select_reads_all_rules", lambda: reads(ALL_RULES, "all")), ("select_reads_max_n", lambda: reads(MAX_N, "max_n")))
    if args.trace:
        for _name, call in calls:
            for _ in range(5):
                call()
        ctx.sync()
        print(json.dumps({"rows": n}))
        sys.exit(0)
    floor_ms = n * (2 * 150 + 48) / COPY_RATE * 1e3
    r = {"rows": n, "bytes": nb, "reps": args.reps, "traffic_floor_ms": floor_ms}
    for name, call in calls:
        r[name] = timed(call, args.reps)
        r[name]["x_floor"] = r[name]["ms"] / floor_ms
    y = r["stats_150"]
    r["stats_150"]["spread_ms"] = y["max_ms"] - y["min_ms"]
    for name, key in (("select_reads_all_rules", "all"), ("select_reads_max_n", "max_n")):
        r[name].update(x_stats_150=r[name]["ms"] / y["ms"], minus_stats_150_ms=r[name]["ms"] - y["ms"], G_rows_per_s=n / r[name]["ms"] / 1e6,
                       counts=last[key][1])
        assert sum(last[key][1][:7]) == n and last[key][0] == last[key][1][0]
    r["all_rules_within_the_yardsticks_spread"] = r["select_reads_all_rules"]["ms"] - y["ms"] <= r["stats_150"]["spread_ms"]
    results.append(r)
    del sh, table, out, idx, block
    torch.cuda.empty_cache()
print(json.dumps(results))

"""Time of the pair passes on two copies of the S-single workload of tools/bench_filter.py (1 GiB, 3.3 M rows each),
beside -- in the same process, on the same tables -- what they are made of:
    ffq_table_select_pairs, every rule on both mates      against   two calls of ffq_table_select_reads, one per table
    ffq_table_pair_names                                  against   the sizing half of ffq_table_render_fastq (out_cap = 0:
                                                                    k_render_sum and its scan, the one existing pass that looks at
                                                                    every row's header positions)
hipEvent times on the context's stream around each call (a call with a host wait inside has its second event recorded when
that wait has returned); median, minimum and maximum of REPS calls.

    python tools/bench_pairs.py [--size 1073741824] [--reps 25]
    python tools/bench_pairs.py --trace            five calls of each and nothing else, to run under rocprofv3 --kernel-trace
    python tools/bench_pairs.py --e2e DIR [--runs 5]
                                                   fastqandfurious.filter_fastq_paired over two 1 GiB files in DIR (page cache)
                                                   against two filter_fastq runs, one after the other, in the same process:
                                                   quality_cutoff=(20, 20), min_len=30, content=ContentRules(max_n=0,
                                                   max_expected_errors=1.0); RUNS times each behind a warm-up, alternating.
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import fastqandfurious_amd
from fastqandfurious_amd import hip
from fastqandfurious_amd.sharded import SyntheticShard

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1 << 30)
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--e2e", metavar="DIR")
ap.add_argument("--runs", type=int, default=5)
args = ap.parse_args()

ctx = hip.Context(0)


def spread(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


if args.e2e:
    from fastqandfurious_amd import fastqandfurious as F
    sh = SyntheticShard(ctx, "single", args.size, 0, 1, torch.device("cuda:0"))
    nbytes = sh.ext_scanned_bytes
    names = ["bench_pairs_in1.fq", "bench_pairs_in2.fq", "bench_pairs_out1.fq", "bench_pairs_out2.fq"]
    src1, src2, dst1, dst2 = (os.path.join(args.e2e, x) for x in names)
    data = sh.ext[:nbytes].cpu().numpy()
    data.tofile(src1)
    data.tofile(src2)
    del sh, data
    kw = dict(quality_cutoff=(20, 20), min_len=30)
    result = {"bytes_per_file": nbytes, "runs": args.runs, "paired_s": [], "two_single_s": []}

    real, seen = hip.PairStream, {}

    def counted(*a, **k):                                    # (the walk's number of rounds: hip.PairStream.rounds)
        seen["last"] = real(*a, **k)
        return seen["last"]
    hip.PairStream = counted
    try:
        for run in range(args.runs + 1):                     # (the first run of each is a warm-up and is not kept)
            rules = F.ContentRules(max_n=0, max_expected_errors=1.0)
            t0 = time.perf_counter()
            with open(src1, "rb") as f1, open(src2, "rb") as f2, open(dst1, "wb") as o1, open(dst2, "wb") as o2:
                res = F.filter_fastq_paired(f1, f2, o1, o2, 1 << 24, content=rules, **kw)
            t1 = time.perf_counter()
            singles = []
            for src, dst in ((src1, dst1), (src2, dst2)):
                with open(src, "rb") as fh, open(dst, "wb") as fo:
                    singles.append(list(F.filter_fastq(fh, fo, 1 << 24, content=rules, **kw)))
            t2 = time.perf_counter()
            result["paired_result"] = [res.pairs_in, res.pairs_out, res.bases_removed, res.bytes_out1, res.bytes_out2, res.dropped]
            result["single_results"] = singles
            result["rounds"] = seen["last"].rounds
            if run:
                result["paired_s"].append(t1 - t0)
                result["two_single_s"].append(t2 - t1)
        p, s = spread(result["paired_s"]), spread(result["two_single_s"])
        result.update(paired=p, two_single=s, ratio=p["median"] / s["median"], GB_per_s_in_paired=2 * nbytes / p["median"] / 1e9,
                      GB_per_s_in_two_single=2 * nbytes / s["median"] / 1e9)
    finally:
        hip.PairStream = real
        for p in (src1, src2, dst1, dst2):
            if os.path.exists(p):
                os.unlink(p)
    print(json.dumps(result))
    sys.exit(0)

stream = torch.cuda.ExternalStream(ctx.stream())
ALL_RULES = hip.ContentRulesStruct(33, 5, 20, 15, 40, 30, 10 * 10 ** 6)          # every rule on (tools/bench_filter.py's)


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
    return {"ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "spread_ms": max(ts) - min(ts)}


mates = []
for _mate in (0, 1):
    sh = SyntheticShard(ctx, "single", args.size, 0, 1, torch.device("cuda:0"))
    table = torch.empty((sh.max_records, 6), dtype=torch.int64, device="cuda")
    rc, res = ctx.scan_device(sh.ext.data_ptr(), sh.ext_scanned_bytes, table.data_ptr(), sh.max_records)
    mates.append((sh, table, int(res.n_records)))
n = mates[0][2]
assert n == mates[1][2]
outs = [torch.empty_like(m[1]) for m in mates]
idx = torch.empty((n,), dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
views = [hip.table_view(sh.ext.data_ptr(), sh.ext_scanned_bytes, table.data_ptr()) for sh, table, _ in mates]
last = {}


def pairs():
    last["pairs"] = ctx.table_select_pairs(views[0], views[1], n, outs[0].data_ptr(), outs[1].data_ptr(), ALL_RULES, ALL_RULES, 30, None,
                                           "any", idx.data_ptr())


def two_reads():
    last["reads"] = [ctx.table_select_reads(sh.ext.data_ptr(), sh.ext_scanned_bytes, table.data_ptr(), n, out.data_ptr(), ALL_RULES, 30, None,
                                            idx.data_ptr()) for (sh, table, _), out in zip(mates, outs)]


def names():
    last["names"] = ctx.table_pair_names(views[0], views[1], n)


def render_sizing():
    sh, table, _ = mates[0]
    last["sizing"] = ctx.table_render_fastq(sh.ext.data_ptr(), sh.ext_scanned_bytes, table.data_ptr(), n, None, 0)


calls = (("select_pairs_all_rules", pairs), ("two_select_reads_all_rules", two_reads), ("pair_names", names), ("render_sizing", render_sizing))
if args.trace:
    for _name, call in calls:
        for _ in range(5):
            call()
    ctx.sync()
    print(json.dumps({"rows": n}))
    sys.exit(0)
r = {"rows_per_mate": n, "bytes_per_mate": mates[0][0].ext_scanned_bytes, "reps": args.reps}
for name, call in calls:
    r[name] = timed(call, args.reps)
k, h1, h2, pc = last["pairs"]
assert h1 == last["reads"][0][1] and h2 == last["reads"][1][1] and pc[0] + pc[1] == n and k == pc[0]
assert last["names"] == (n, 0, 0, -1)
r["select_pairs_all_rules"].update(hist1=h1, hist2=h2, pairs=pc)
r["pairs_minus_two_reads_ms"] = r["select_pairs_all_rules"]["ms"] - r["two_select_reads_all_rules"]["ms"]
r["pairs_within_the_two_calls_spread"] = r["pairs_minus_two_reads_ms"] <= r["two_select_reads_all_rules"]["spread_ms"]
r["names_over_render_sizing"] = r["pair_names"]["ms"] / r["render_sizing"]["ms"]
print(json.dumps(r))

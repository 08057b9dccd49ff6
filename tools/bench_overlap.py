"""Time of the overlap pass on two generated 1 GiB-class tables of 150-base mates, beside -- in the same process,
on the same tables -- what a pair costs today to lose its adapters:
    ffq_table_pair_overlap (min_overlap 30, max_diff 5, diff_permille 200, trim, histogram)
                                              against   two calls of ffq_table_trim_adapter, one per mate (13-base adapter,
                                                        err_permille 100, min_overlap 3: the arguments of DESIGN.md 4c)
hipEvent times on the context's stream around each call; median, minimum and maximum of REPS calls.

The pairs (pair_block): a fragment of seeded length is read 150 bases from either end, mate 2 as the reverse complement; where
the fragment is shorter than the read the adapters' bytes follow it; every base is changed with probability --err.  --short is
the share of pairs whose fragment is shorter than the read (35..149 bases; the others: 300..500, no overlap) -- early stopping
makes the time depend on it.  Records have one fixed size, so the tables are written down, not scanned; a block of 2^20 pairs
is generated and laid out three times (to different addresses: nothing is served from a cache that a whole file would miss).

    python tools/bench_overlap.py [--short 0.5] [--err 0.01] [--reps 25]
    python tools/bench_overlap.py --trace          five calls of each and nothing else, to run under rocprofv3 --kernel-trace
    python tools/bench_overlap.py --e2e DIR [--runs 5] [--plain-only]
                                                   fastqandfurious.filter_fastq_paired over two such files in DIR (page cache),
                                                   with overlap=OverlapRules() against the same call without it: quality_cutoff=
                                                   (20, 20), min_len=30, content=ContentRules(max_n=0, max_expected_errors=1.0)
                                                   (DESIGN.md 4h's); RUNS times each behind a warm-up, alternating.
                                                   --plain-only: the call without overlap alone (for a comparison of two trees)
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--short", type=float, default=0.5)
ap.add_argument("--err", type=float, default=0.01)
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--copies", type=int, default=3)
ap.add_argument("--block", type=int, default=1 << 20)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--e2e", metavar="DIR")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--plain-only", action="store_true")
args = ap.parse_args()

from pairgen import READ, ADAPTER1, ADAPTER2, HEAD, REC, pair_block


def spread(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


if args.e2e:
    from fastqandfurious_amd import fastqandfurious as F
    names = ["bench_overlap_in1.fq", "bench_overlap_in2.fq", "bench_overlap_out1.fq", "bench_overlap_out2.fq"]
    src1, src2, dst1, dst2 = (os.path.join(args.e2e, x) for x in names)
    b1, b2, share = pair_block(args.block, args.short, args.err, 1)
    for src, b in ((src1, b1), (src2, b2)):
        with open(src, "wb") as fh:
            for _ in range(args.copies):
                b.tofile(fh)
    nbytes = os.path.getsize(src1)
    del b1, b2
    kw = dict(quality_cutoff=(20, 20), min_len=30)
    result = {"bytes_per_file": nbytes, "runs": args.runs, "short_share": share, "err": args.err, "overlap_s": [], "plain_s": []}
    try:
        for run in range(args.runs + 1):                         # (the first run of each is a warm-up and is not kept)
            rules = F.ContentRules(max_n=0, max_expected_errors=1.0)
            t0 = time.perf_counter()
            if not args.plain_only:
                rep = F.OverlapReport()
                with open(src1, "rb") as f1, open(src2, "rb") as f2, open(dst1, "wb") as o1, open(dst2, "wb") as o2:
                    res = F.filter_fastq_paired(f1, f2, o1, o2, 1 << 24, content=rules, overlap=F.OverlapRules(), overlap_report=rep, **kw)
                result["overlap_result"] = [res.pairs_in, res.pairs_out, res.bases_removed, res.bytes_out1, res.bytes_out2, res.dropped]
                result["overlap_report"] = [rep.pairs_analysed, rep.pairs_overlapped, rep.pairs_trimmed, rep.bases_removed, rep.insert_peak]
            t1 = time.perf_counter()
            with open(src1, "rb") as f1, open(src2, "rb") as f2, open(dst1, "wb") as o1, open(dst2, "wb") as o2:
                res = F.filter_fastq_paired(f1, f2, o1, o2, 1 << 24, content=rules, **kw)
            t2 = time.perf_counter()
            result["plain_result"] = [res.pairs_in, res.pairs_out, res.bases_removed, res.bytes_out1, res.bytes_out2, res.dropped]
            if run:
                result["overlap_s"].append(t1 - t0)
                result["plain_s"].append(t2 - t1)
        result["plain"] = spread(result["plain_s"])
        result["GB_per_s_in_plain"] = 2 * nbytes / result["plain"]["median"] / 1e9
        if not args.plain_only:
            result["overlap"] = spread(result["overlap_s"])
            result["ratio"] = result["overlap"]["median"] / result["plain"]["median"]
            result["GB_per_s_in_overlap"] = 2 * nbytes / result["overlap"]["median"] / 1e9
    finally:
        for p in (src1, src2, dst1, dst2):
            if os.path.exists(p):
                os.unlink(p)
    print(json.dumps(result))
    sys.exit(0)

import torch
import fastqandfurious_amd
from fastqandfurious_amd import hip

ctx = hip.Context(0)
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
    return {"ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "spread_ms": max(ts) - min(ts)}


b1, b2, share = pair_block(args.block, args.short, args.err, 1)
n = args.block * args.copies
bufs = [torch.from_numpy(b).cuda().repeat(args.copies, 1).contiguous() for b in (b1, b2)]
del b1, b2
at = torch.arange(n, dtype=torch.int64, device="cuda") * REC
table = torch.stack([at, at + HEAD - 1, at + HEAD, at + HEAD + READ, at + HEAD + READ + 3, at + REC - 1], dim=1).contiguous()
outs = [torch.empty_like(table) for _ in (0, 1)]
hist = torch.zeros(hip.OVERLAP_HIST_WORDS + 1, dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
nbytes = n * REC
views = [hip.table_view(b.data_ptr(), nbytes, table.data_ptr(), False, 0) for b in bufs]
RULES = hip.OverlapRulesStruct(30, 5, 200, 1)
last = {}


def overlap():
    last["overlap"] = ctx.table_pair_overlap(views[0], views[1], n, RULES, outs[0].data_ptr(), outs[1].data_ptr(), None, hist.data_ptr(), False)


def two_adapters():
    last["adapters"] = [ctx.table_trim_adapter(b.data_ptr(), nbytes, table.data_ptr(), n, ad[:13], 100, 3, out.data_ptr(), sentinel=False, add=0)
                        for b, ad, out in zip(bufs, (ADAPTER1, ADAPTER2), outs)]


calls = (("pair_overlap", overlap), ("two_trim_adapter", two_adapters))
if args.trace:
    for _name, call in calls:
        for _ in range(5):
            call()
    ctx.sync()
    print(json.dumps({"pairs": n}))
    sys.exit(0)
r = {"pairs": n, "bytes_per_mate": nbytes, "reps": args.reps, "short_share": share, "err": args.err}
for name, call in calls:
    r[name] = timed(call, args.reps)
r["pair_overlap"]["counts"] = last["overlap"]
r["two_trim_adapter"]["stats"] = last["adapters"]
assert last["overlap"][0] == n and last["overlap"][5] == 0
r["overlap_over_two_adapter_calls"] = r["pair_overlap"]["ms"] / r["two_trim_adapter"]["ms"]
print(json.dumps(r))

"""Time of the merge pass on the two generated tables of tools/bench_overlap.py (3.1 M pairs of 150-base mates,
about half the fragments shorter than the reads), beside -- in the same process, on the same tables -- what rendering the same
pairs costs today:
    ffq_table_pair_merge (insert sizes of ffq_table_pair_overlap with trim 1, on the rows it left)
                                              against   two calls of ffq_table_render_fastq, one per mate, on the same rows
hipEvent times on the context's stream around each call; median, minimum and maximum of REPS calls.  The overlap pass runs
once, in front, and is not timed.  Qualities are seeded bytes in 'I' - 20 .. 'I', so that both mates win positions.

    python tools/bench_merge.py [--short 0.5] [--err 0.01] [--reps 25]
    python tools/bench_merge.py --trace            five calls of each and nothing else, to run under rocprofv3 --kernel-trace
    python tools/bench_merge.py --e2e DIR [--runs 5]
                                                   fastqandfurious.filter_fastq_paired over two such files in DIR (page cache),
                                                   overlap=OverlapRules(), quality_cutoff=(20, 20), min_len=30, with
                                                   merged_out against the same call without it; RUNS times each behind a
                                                   warm-up, alternating.
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pairgen import READ, HEAD, REC, pair_block

ap = argparse.ArgumentParser()
ap.add_argument("--short", type=float, default=0.5)
ap.add_argument("--err", type=float, default=0.01)
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--copies", type=int, default=3)
ap.add_argument("--block", type=int, default=1 << 20)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--e2e", metavar="DIR")
ap.add_argument("--runs", type=int, default=5)
args = ap.parse_args()

QUAL = (ord("I") - 20, ord("I") + 1)


def spread(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


if args.e2e:
    from fastqandfurious_amd import fastqandfurious as F
    names = ["bench_merge_in1.fq", "bench_merge_in2.fq", "bench_merge_out1.fq", "bench_merge_out2.fq", "bench_merge_merged.fq"]
    src1, src2, dst1, dst2, dstm = (os.path.join(args.e2e, x) for x in names)
    b1, b2, share = pair_block(args.block, args.short, args.err, 1, QUAL)
    for src, b in ((src1, b1), (src2, b2)):
        with open(src, "wb") as fh:
            for _ in range(args.copies):
                b.tofile(fh)
    nbytes = os.path.getsize(src1)
    del b1, b2
    kw = dict(quality_cutoff=(20, 20), min_len=30)
    result = {"bytes_per_file": nbytes, "runs": args.runs, "short_share": share, "err": args.err, "merge_s": [], "plain_s": []}
    try:
        for run in range(args.runs + 1):                         # (the first run of each is a warm-up and is not kept)
            t0 = time.perf_counter()
            rep = F.MergeReport()
            with open(src1, "rb") as f1, open(src2, "rb") as f2, open(dst1, "wb") as o1, open(dst2, "wb") as o2, open(dstm, "wb") as om:
                res = F.filter_fastq_paired(f1, f2, o1, o2, 1 << 24, overlap=F.OverlapRules(), merged_out=om, merge_report=rep, **kw)
            result["merge_result"] = [res.pairs_in, res.pairs_out, res.bases_removed, res.bytes_out1, res.bytes_out2, res.dropped]
            result["merge_report"] = [rep.pairs_merged, rep.bases_merged, rep.bytes_merged, rep.overlap_positions, rep.taken_from_mate2]
            t1 = time.perf_counter()
            with open(src1, "rb") as f1, open(src2, "rb") as f2, open(dst1, "wb") as o1, open(dst2, "wb") as o2:
                res = F.filter_fastq_paired(f1, f2, o1, o2, 1 << 24, overlap=F.OverlapRules(), **kw)
            t2 = time.perf_counter()
            result["plain_result"] = [res.pairs_in, res.pairs_out, res.bases_removed, res.bytes_out1, res.bytes_out2, res.dropped]
            if run:
                result["merge_s"].append(t1 - t0)
                result["plain_s"].append(t2 - t1)
        result["plain"] = spread(result["plain_s"])
        result["merge"] = spread(result["merge_s"])
        result["ratio"] = result["merge"]["median"] / result["plain"]["median"]
        result["GB_per_s_in_plain"] = 2 * nbytes / result["plain"]["median"] / 1e9
        result["GB_per_s_in_merge"] = 2 * nbytes / result["merge"]["median"] / 1e9
    finally:
        for p in (src1, src2, dst1, dst2, dstm):
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


b1, b2, share = pair_block(args.block, args.short, args.err, 1, QUAL)
n = args.block * args.copies
bufs = [torch.from_numpy(b).cuda().repeat(args.copies, 1).contiguous() for b in (b1, b2)]
del b1, b2
at = torch.arange(n, dtype=torch.int64, device="cuda") * REC
table = torch.stack([at, at + HEAD - 1, at + HEAD, at + HEAD + READ, at + HEAD + READ + 3, at + REC - 1], dim=1).contiguous()
rows = [torch.empty_like(table) for _ in (0, 1)]
rest = [torch.empty_like(table) for _ in (0, 1)]
insert = torch.empty(n, dtype=torch.int32, device="cuda")
nbytes = n * REC
text = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
views = [hip.table_view(b.data_ptr(), nbytes, table.data_ptr(), False, 0) for b in bufs]
# the rows as the overlap pass leaves them, and every pair's insert size: once, not timed
overlap_counts = ctx.table_pair_overlap(views[0], views[1], n, hip.OverlapRulesStruct(30, 5, 200, 1), rows[0].data_ptr(), rows[1].data_ptr(),
                                        d_insert=insert.data_ptr())
cut = [hip.table_view(b.data_ptr(), nbytes, r.data_ptr(), False, 0) for b, r in zip(bufs, rows)]
last = {}


def merge():
    last["merge"] = ctx.table_pair_merge(cut[0], cut[1], n, insert.data_ptr(), text.data_ptr(), nbytes + 64, rest[0].data_ptr(), rest[1].data_ptr())


def two_renders():
    last["renders"] = [ctx.table_render_fastq(b.data_ptr(), nbytes, r.data_ptr(), n, text.data_ptr(), nbytes + 64, sentinel=False, add=0)
                       for b, r in zip(bufs, rows)]


calls = (("pair_merge", merge), ("two_render_fastq", two_renders))
if args.trace:
    for _name, call in calls:
        for _ in range(5):
            call()
    ctx.sync()
    print(json.dumps({"pairs": n}))
    sys.exit(0)
r = {"pairs": n, "bytes_per_mate": nbytes, "reps": args.reps, "short_share": share, "err": args.err, "overlap_counts": overlap_counts}
for name, call in calls:
    r[name] = timed(call, args.reps)
rc, n_rest, counts = last["merge"]
assert rc == 0 and counts[0] + counts[1] == n and counts[0] == overlap_counts[1] and n_rest == counts[1]
r["pair_merge"]["counts"] = counts
r["two_render_fastq"]["stats"] = [list(s) for _rc, s in last["renders"]]
r["bytes_merged_over_bytes_rendered"] = counts[2] / sum(s[0] for _rc, s in last["renders"])
r["merge_over_two_render_calls"] = r["pair_merge"]["ms"] / r["two_render_fastq"]["ms"]
print(json.dumps(r))

"""Time of the correction pass on the two generated tables of tools/bench_overlap.py (3.1 M pairs of 150-base
mates, about half the fragments shorter than the reads and so with an overlap, every base wrong with probability --err), beside
-- in the same process, on the same tables -- the overlap pass that finds the insert sizes it works by:
    ffq_table_pair_correct  (insert sizes of ffq_table_pair_overlap with trim 1, on the rows it left)
                                              against   ffq_table_pair_overlap on the scanned rows
hipEvent times on the context's stream around each call; median, minimum and maximum of REPS calls.  The pass edits the bytes
and is idempotent, so it is timed twice: "first" with both buffers restored from a copy in front of every call (not timed) --
the call that stores --, and "again" on the corrected buffers, where nothing is left to store.  Qualities are seeded bytes over
Q2..Q40, so that a mismatch meets sure against poor on either side, sure against sure, and everything between.

    python tools/bench_correct.py [--short 0.5] [--err 0.01] [--reps 25]
    python tools/bench_correct.py --trace          five calls of each and nothing else, to run under rocprofv3 --kernel-trace
"""
import argparse, json, os, statistics, sys
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
args = ap.parse_args()

QUAL = (33 + 2, 33 + 41)

import torch
import fastqandfurious_amd
from fastqandfurious_amd import hip

ctx = hip.Context(0)
stream = torch.cuda.ExternalStream(ctx.stream())


def timed(call, reps, before=None):
    call()
    ctx.sync()
    ts = []
    for _ in range(reps):
        if before is not None:
            before()
            torch.cuda.synchronize()
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
pristine = [b.clone() for b in bufs]
at = torch.arange(n, dtype=torch.int64, device="cuda") * REC
table = torch.stack([at, at + HEAD - 1, at + HEAD, at + HEAD + READ, at + HEAD + READ + 3, at + REC - 1], dim=1).contiguous()
rows = [torch.empty_like(table) for _ in (0, 1)]
insert = torch.empty(n, dtype=torch.int32, device="cuda")
nbytes = n * REC
torch.cuda.synchronize()
views = [hip.table_view(b.data_ptr(), nbytes, table.data_ptr(), False, 0) for b in bufs]
cut = [hip.table_view(b.data_ptr(), nbytes, r.data_ptr(), False, 0) for b, r in zip(bufs, rows)]
RULES = hip.CorrectRulesStruct(30, 14, 33)
last = {}


def overlap():
    last["overlap"] = ctx.table_pair_overlap(views[0], views[1], n, hip.OverlapRulesStruct(30, 5, 200, 1), rows[0].data_ptr(), rows[1].data_ptr(),
                                             d_insert=insert.data_ptr())


def correct():
    last["correct"] = ctx.table_pair_correct(cut[0], cut[1], n, insert.data_ptr(), RULES)


def restore():
    for b, p in zip(bufs, pristine):
        b.copy_(p)


overlap()
if args.trace:
    for call in (overlap, correct):
        for _ in range(5):
            call()
    ctx.sync()
    print(json.dumps({"pairs": n}))
    sys.exit(0)
r = {"pairs": n, "bytes_per_mate": nbytes, "reps": args.reps, "short_share": share, "err": args.err}
r["pair_overlap"] = timed(overlap, args.reps)
r["pair_overlap"]["counts"] = last["overlap"]
r["pair_correct_first"] = timed(correct, args.reps, before=restore)
counts, matrix = last["correct"]
assert counts[0] + counts[5] == n and counts[0] == last["overlap"][1] and int(matrix.sum()) == counts[2] + counts[3]
r["pair_correct_first"]["counts"] = counts
r["pair_correct_first"]["matrix"] = matrix.tolist()
r["pair_correct_again"] = timed(correct, args.reps)
again = last["correct"][0]
assert again[1:4] == [0, 0, 0] and again[4] == counts[4] - counts[2] - counts[3]
r["pair_correct_again"]["counts"] = again
r["mismatches_per_pair_looked_at"] = counts[4] / max(counts[0], 1)
r["corrected_share_of_mismatches"] = (counts[2] + counts[3]) / max(counts[4], 1)
r["correct_first_over_overlap"] = r["pair_correct_first"]["ms"] / r["pair_overlap"]["ms"]
r["correct_again_over_overlap"] = r["pair_correct_again"]["ms"] / r["pair_overlap"]["ms"]
print(json.dumps(r))

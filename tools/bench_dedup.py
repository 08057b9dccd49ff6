"""Time of duplicate removal (ffq_table_seq_keys, ffq_dedup_select) on the table of the 1 GiB S-single buffer (150-base reads)
with duplicates injected by copying records over others -- 0 %, 20 % and 80 % of the records; a synthetic file has none of its
own.  hipEvent times on the context's stream around each call (a call with a host wait inside has its second event recorded
when that wait has returned); median, minimum and maximum of REPS calls.  Per share of duplicates:
  seq_keys            the key pass, in GB/s of SEQUENCE bytes (rows * 150); beside it, in the same process on the same table, the
                      passes that read the same bytes: ffq_table_trim_adapter, and ffq_table_select_reads with max_n alone
                      (k_filter_rows: both lines of every row)
  set_cold            ffq_dedup_select of all rows into a set created with expected_keys = 0: it grows once, from the minimum
  set_presized        ... into a set created for that many keys: no growth, every distinct key claims a slot
  set_warm            the same call again: every row is a duplicate of an earlier one, no growth, no claim
  rehash              two halves into a set that has to grow in front of the second, against two halves into a presized one:
                      what the growth (allocate, clear, rehash of the first half's keys) costs
  random_16B          the yardstick of the set passes: torch's index_select of rows random 16-byte elements of a table of the
                      set's size (one random access per row; insert + resolve make two and an atomic)
    python tools/bench_dedup.py [--size 1073741824] [--reps 9]
    python tools/bench_dedup.py --trace            three calls of each at 20 % and nothing else, to run under rocprofv3 --kernel-trace
    python tools/bench_dedup.py --e2e DIR [--runs 5] [--dups 20]
                                                   fastqandfurious.filter_fastq(quality_cutoff=(20, 20), min_len=30) over the buffer as a
                                                   file in DIR (page cache), with and without dedup=DedupRules(), alternating in one
                                                   process, RUNS each behind a warm-up of either
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import fastqandfurious_amd
from fastqandfurious_amd import hip
from fastqandfurious_amd.sharded import SyntheticShard

REC = 322                   # bytes of a record of the S-single buffer

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1 << 30)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--e2e", metavar="DIR")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--dups", type=int, default=20)
args = ap.parse_args()

ctx = hip.Context(0)


def with_duplicates(sh, percent, seed=1):
    """`percent` of the buffer's records overwritten by a copy of the sequence and quality lines of a record that is NOT
    overwritten: exactly that share of the records are then duplicates of an earlier or later one"""
    assert sh.tail == 0
    n = sh.ext_scanned_bytes // REC
    if percent == 0:
        return n
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    recs = sh.ext[:n * REC].view(n, REC)
    perm = torch.randperm(n, device="cuda", generator=g)
    dst, keep = perm[:n * percent // 100], perm[n * percent // 100:]
    src = keep[torch.randint(0, keep.numel(), (dst.numel(),), device="cuda", generator=g)]
    body = recs[src, 18:].clone()                   # (behind the 18 bytes of the header: the sequence, the '+' line, the quality)
    recs[dst, 18:] = body
    torch.cuda.synchronize()
    return n


if args.e2e:
    from fastqandfurious_amd import fastqandfurious as F
    sh = SyntheticShard(ctx, "single", args.size, 0, 1, torch.device("cuda:0"))
    with_duplicates(sh, args.dups)
    nbytes = sh.ext_scanned_bytes
    src, dst = os.path.join(args.e2e, "bench_dedup_in.fq"), os.path.join(args.e2e, "bench_dedup_out.fq")
    sh.ext[:nbytes].cpu().numpy().tofile(src)
    del sh
    result = {"bytes": nbytes, "runs": args.runs, "dups_percent": args.dups, "plain_s": [], "dedup_s": []}
    try:
        for run in range(args.runs + 1):                     # (the first run of either is a warm-up and is not kept)
            for which in (("plain", "dedup") if run % 2 == 0 else ("dedup", "plain")):
                rep = F.DedupReport() if which == "dedup" else None
                t0 = time.perf_counter()
                with open(src, "rb") as fh, open(dst, "wb") as fo:
                    res = F.filter_fastq(fh, fo, 1 << 24, quality_cutoff=(20, 20), min_len=30, dedup=F.DedupRules() if rep else None,
                                         dedup_report=rep)
                dt = time.perf_counter() - t0
                assert result.setdefault(which + "_result", list(res)) == list(res)
                if rep is not None:
                    result["report"] = dict(rep.__dict__, duplication_rate=rep.duplication_rate)
                if run:
                    result[which + "_s"].append(dt)
        for which in ("plain", "dedup"):
            s = result[which + "_s"]
            result[which] = dict(median_s=statistics.median(s), min_s=min(s), max_s=max(s), GB_per_s_in=nbytes / statistics.median(s) / 1e9)
        result["dedup_over_plain"] = result["dedup"]["median_s"] / result["plain"]["median_s"]
    finally:
        for p in (src, dst):
            if os.path.exists(p):
                os.unlink(p)
    print(json.dumps(result))
    sys.exit(0)

stream = torch.cuda.ExternalStream(ctx.stream())
MAX_N = hip.ContentRulesStruct(33, 0, 0, 15, -1, 0, -1)
ADAPTER = b"AGATCGGAAGAGC"


def timed(call, reps, setup=None):
    ts = []
    for r in range(reps + 1):                                # (the first is a warm-up)
        if setup is not None:
            setup()
        ctx.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        if r:
            ts.append(e0.elapsed_time(e1))
    return {"ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


results = []
for percent in ([20] if args.trace else [0, 20, 80]):
    sh = SyntheticShard(ctx, "single", args.size, 0, 1, torch.device("cuda:0"))
    with_duplicates(sh, percent)
    table = torch.empty((sh.max_records, 6), dtype=torch.int64, device="cuda")
    rc, res = ctx.scan_device(sh.ext.data_ptr(), sh.ext_scanned_bytes, table.data_ptr(), sh.max_records)
    n = int(res.n_records)
    out = torch.empty_like(table)
    idx = torch.empty((sh.max_records,), dtype=torch.int64, device="cuda")
    keys = torch.zeros((sh.max_records,), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    buf, nb = sh.ext.data_ptr(), sh.ext_scanned_bytes
    last, sets = {}, {}

    def seq_keys():
        last["keys"] = ctx.table_seq_keys(buf, nb, table.data_ptr(), n, keys.data_ptr())

    def adapter():
        ctx.table_trim_adapter(buf, nb, table.data_ptr(), n, ADAPTER, d_out=out.data_ptr())

    def max_n():
        ctx.table_select_reads(buf, nb, table.data_ptr(), n, out.data_ptr(), MAX_N, None, None, idx.data_ptr())

    def fresh(name, expected):
        def setup():
            if name in sets:
                sets[name].close()
            sets[name] = hip.Dedup(ctx, expected)
        return setup

    def select(name, lo=0, count=None, tables=True):
        def call():
            m = n - lo if count is None else count
            last[name] = sets[name].select(keys.data_ptr() + 8 * lo, m, d_table1=table.data_ptr() + 48 * lo if tables else None,
                                           d_out1=out.data_ptr() if tables else None, d_idx=idx.data_ptr() if tables else None)
        return call

    def halves(name):
        def call():
            select(name, 0, n // 2)()
            select(name, n // 2)()
        return call

    seq_keys()
    if args.trace:
        for call in (seq_keys, adapter, max_n):
            for _ in range(3):
                call()
        for _ in range(3):
            fresh("t", 0)()
            select("t")()
            select("t")()
        ctx.sync()
        print(json.dumps({"rows": n}))
        sys.exit(0)
    r = {"dups_percent": percent, "rows": n, "bytes": nb, "reps": args.reps}
    for name, call in (("seq_keys", seq_keys), ("trim_adapter", adapter), ("select_reads_max_n", max_n)):
        r[name] = timed(call, args.reps)
    r["seq_keys"]["GB_per_s_of_sequence"] = n * 150 / r["seq_keys"]["ms"] / 1e6
    r["seq_keys"]["x_trim_adapter"] = r["seq_keys"]["ms"] / r["trim_adapter"]["ms"]
    r["seq_keys"]["x_select_reads_max_n"] = r["seq_keys"]["ms"] / r["select_reads_max_n"]["ms"]
    r["keyed"] = list(last["keys"])
    r["set_cold"] = timed(select("cold"), args.reps, fresh("cold", 0))
    r["set_presized"] = timed(select("pre"), args.reps, fresh("pre", n))
    r["counts"] = last["pre"][1]
    r["set_warm"] = timed(select("pre"), args.reps)
    r["set_warm_keys_only"] = timed(select("pre", tables=False), args.reps)
    r["halves_growing"] = timed(halves("grow"), args.reps, fresh("grow", n // 4))
    r["halves_presized"] = timed(halves("pre2"), args.reps, fresh("pre2", n))
    r["rehash"] = {"ms": r["halves_growing"]["ms"] - r["halves_presized"]["ms"], "rehashes": last["grow"][1][5]}
    for name in ("set_cold", "set_presized", "set_warm", "set_warm_keys_only"):
        r[name]["M_rows_per_s"] = n / r[name]["ms"] / 1e3
    for s in sets.values():
        s.close()
    slots = r["counts"][4]
    tab = torch.zeros((slots, 2), dtype=torch.int64, device="cuda")
    where = torch.randint(0, slots, (n,), device="cuda")
    got = torch.empty((n, 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        r["random_16B"] = timed(lambda: torch.index_select(tab, 0, where, out=got), args.reps)
    r["random_16B"].update(slots=slots, M_rows_per_s=n / r["random_16B"]["ms"] / 1e3)
    results.append(r)
    print(json.dumps(r), flush=True)
    del sh, table, out, idx, keys, tab, where, got
    torch.cuda.empty_cache()

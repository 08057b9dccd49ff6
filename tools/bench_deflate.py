"""Time and size of writing FASTQ text as BGZF members on the device (ffq_deflate_bgzf), on two texts of --bytes each: the
S-single buffer (its rendered text is the buffer itself) and the Illumina-like records of tests/deflate_expect.py, tiled.

  deflate    ffq_deflate_bgzf alone, device to device
  way back   what a fill costs behind the filter, per text: render + deflate + copy of the MEMBERS to pinned memory, beside
             the uncompressed way: render + copy of the TEXT
  sizes      against zlib level 1 and level 6 on the same blocks (the first --zlib-bytes of the text: zlib is slow)
One process, medians of --reps rounds, wall clock around the blocking calls (each has one host wait).

    python tools/bench_deflate.py [--bytes N] [--reps 7] [--zlib-bytes N]
    python tools/bench_deflate.py --e2e DIR    filter_fastq(compress="bgzf") over the S-single buffer as a file in DIR beside
                                               filter_fastq into gzip.open(compresslevel=1), which takes minutes per GiB
"""
import argparse, gzip, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import fastqandfurious_amd
from fastqandfurious_amd import hip, synth
import deflate_expect as E

ap = argparse.ArgumentParser()
ap.add_argument("--bytes", type=int, default=1 << 30)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--zlib-bytes", type=int, default=32 << 20)
ap.add_argument("--e2e", metavar="DIR")
args = ap.parse_args()
ctx = hip.Context(0)
B = hip.BGZF_BLOCK_BYTES


def timed(fn, reps=args.reps):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


if args.e2e:
    from fastqandfurious_amd import fastqandfurious as F
    src, dst = os.path.join(args.e2e, "bench_deflate_in.fq"), os.path.join(args.e2e, "bench_deflate_out.fq.gz")
    n_rec = synth.single_records_for(args.bytes)
    synth.single(0, n_rec).tofile(src)
    result = {"bytes": n_rec * synth.RECORD_BYTES}
    kw = dict(quality_cutoff=(20, 20), min_len=30)
    try:
        for name in ("bgzf_on_device", "plain_text", "gzip_open_level_1"):
            t0 = time.perf_counter()
            with open(src, "rb") as fh:
                if name == "bgzf_on_device":
                    rep = F.CompressReport()
                    with open(dst, "wb") as fo:
                        res = F.filter_fastq(fh, fo, 1 << 24, compress="bgzf", compress_report=rep, **kw)
                    result["ratio"] = rep.ratio
                elif name == "plain_text":
                    with open(dst, "wb") as fo:
                        res = F.filter_fastq(fh, fo, 1 << 24, **kw)
                else:
                    with gzip.open(dst, "wb", compresslevel=1) as fo:
                        res = F.filter_fastq(fh, fo, 1 << 24, **kw)
            dt = time.perf_counter() - t0
            result[name] = {"s": dt, "GB_per_s_in": result["bytes"] / dt / 1e9, "file_bytes": os.path.getsize(dst), "text_bytes": res.bytes_out}
    finally:
        for p in (src, dst):
            if os.path.exists(p):
                os.unlink(p)
    print(json.dumps(result))
    sys.exit(0)


def texts():
    n_rec = synth.single_records_for(args.bytes)
    d = torch.empty(n_rec * synth.RECORD_BYTES, dtype=torch.uint8, device="cuda")
    ctx.synth_single(d.data_ptr(), 0, n_rec)
    yield "synth.single", d
    del d
    tile = np.frombuffer(E.illumina_like(20000), dtype=np.uint8)
    # (tiles of 7 MB: a repeat is far outside every block, so tiling changes nothing a member can see)
    reps = max(1, args.bytes // tile.size)
    yield "illumina-like", torch.from_numpy(tile).cuda().repeat(reps)


result = {}
for name, text in texts():
    n = text.numel()
    cap = hip.deflate_bgzf_bound(n)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    pinned = torch.empty(n + 64, dtype=torch.uint8).pin_memory()
    rc, stats = ctx.deflate_bgzf(text.data_ptr(), n, out.data_ptr(), cap)
    assert rc == hip.OK
    r = result[name] = {"bytes": n, "bgzf_bytes": stats[1], "ratio": n / stats[1], "members": stats[2], "members_stored": stats[3]}
    t = timed(lambda: ctx.deflate_bgzf(text.data_ptr(), n, out.data_ptr(), cap))
    r["deflate_ms"], r["deflate_GB_per_s"] = t * 1e3, n / t / 1e9
    # the way back of a fill: the table of the text, rendered, then one of the two ways
    max_rec = n // 100 + 16
    table = torch.empty((max_rec, 6), dtype=torch.int64, device="cuda")
    rc, res = ctx.scan_device(text.data_ptr(), n, table.data_ptr(), max_rec, sentinel=False)
    assert rc == hip.OK
    rows = int(res.n_records)
    ren = torch.empty(n + 64, dtype=torch.uint8, device="cuda")

    def render():
        rc, st = ctx.table_render_fastq(text.data_ptr(), n, table.data_ptr(), rows, ren.data_ptr(), n + 1, sentinel=False)
        assert rc == hip.OK
        return st[0]

    def back_text():
        nb = render()
        pinned[:nb].copy_(ren[:nb], non_blocking=True)

    def back_members():
        nb = render()
        rc, st = ctx.deflate_bgzf(ren.data_ptr(), nb, out.data_ptr(), cap)
        pinned[:st[1]].copy_(out[:st[1]], non_blocking=True)

    r["render_ms"] = timed(render) * 1e3
    r["way_back_text_ms"] = timed(back_text) * 1e3
    r["way_back_members_ms"] = timed(back_members) * 1e3
    r["way_back_members_over_text"] = r["way_back_members_ms"] / r["way_back_text_ms"]
    # sizes against zlib, per block, on the head of the text
    head = text[:min(n, args.zlib_bytes) // B * B or n].cpu().numpy().tobytes()
    rc, st = ctx.deflate_bgzf(text.data_ptr(), len(head), out.data_ptr(), cap)
    r["head_bytes"], r["head_bgzf"] = len(head), st[1]
    for level in (1, 6):
        z = E.zlib_level_bytes(head, B, level)
        r["head_zlib_level_%d" % level] = z
        r["size_over_zlib_level_%d" % level] = st[1] / z
    print(json.dumps({name: r}), flush=True)
    del out, pinned, ren, table, text
print(json.dumps(result))

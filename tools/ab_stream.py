"""Same-box A/B of the stream front end: A = another commit's library (LIB_A: what tools/ab_build.sh <ref> built), B = the
tree's.  Decompressed GB/s of hip.FileStream at 16 MiB over a 1 GiB S-single file in /dev/shm (plain; decoding), over
the first 256 MiB of it as .gz (one member, level 1) and as BGZF, and of filter_fastq (trim (20, 20), min_len 30, rendered)
over the 1 GiB file; every process takes the best of its runs, the driver prints min / median / max per side.
   python tools/ab_stream.py LIB_A LOG  driver: makes the files once, then alternates A / B children, REPS times each;
                                        writes every child's line and the summary to LOG (JSON lines)
   python tools/ab_stream.py gen DIR    child: the files
   python tools/ab_stream.py run DIR    child: one set of figures as a JSON line
"""
import json, os, statistics, subprocess, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
REPS = int(os.environ.get("AB_STREAM_REPS", "4"))          # processes a side
N_PLAIN, N_GZ = 1 << 30, 256 << 20


def gen(d):
    import gzip
    import torch
    from fastqandfurious_amd import hip, bgzf
    ctx = hip.Context(0)
    n = N_PLAIN // 322
    buf = torch.empty(n * 322 + 64, dtype=torch.uint8, device="cuda")
    ctx.synth_single(buf.data_ptr(), 0, n, 42)
    host = buf[:n * 322].cpu().numpy()
    host.tofile(os.path.join(d, "p.fq"))
    part = host[:(N_GZ // 322) * 322].tobytes()
    with gzip.open(os.path.join(d, "p.fq.gz"), "wb", compresslevel=1) as fh:
        fh.write(part)
    with open(os.path.join(d, "p.fq.bgz"), "wb") as fh:
        fh.write(bgzf.compress(part, level=1))
    print(json.dumps({"plain": host.size, "gz_in": len(part)}))


def run(d):
    from fastqandfurious_amd import hip, fastqandfurious as F
    ctx = hip.Context(0)
    out = {"lib": "parent" if os.environ.get("FFQ_HIP_LIB") else "tree"}

    def stream(path, nbytes, reps=3, **kw):
        best = None
        for _ in range(reps):
            fd = os.open(path, os.O_RDONLY)
            t0 = time.perf_counter()
            st = hip.FileStream(ctx, fd, 1 << 24, **kw)
            n = sum(rows.shape[0] for rows, _f, _o, _e, _x in st)
            st.close()
            os.close(fd)
            el = time.perf_counter() - t0
            best = el if best is None else min(best, el)
        assert n > 0
        return round(nbytes / best / 1e9, 3)

    plain = os.path.join(d, "p.fq")
    nb = os.path.getsize(plain)
    ngz = (N_GZ // 322) * 322
    stream(plain, nb, reps=1)                      # warm-up: pinned slots, page cache
    out["plain_gb_s"] = stream(plain, nb)
    out["decode_gb_s"] = stream(plain, nb, decode=True)
    out["gzip_gb_s"] = stream(plain + ".gz", ngz, gzip=True)
    out["bgzf_gb_s"] = stream(plain + ".bgz", ngz, gzip=True)
    best = None
    for _ in range(2):
        t0 = time.perf_counter()
        with open(plain, "rb") as fh, open(os.path.join(d, "out.fq"), "wb") as fo:
            res = F.filter_fastq(fh, fo, 1 << 24, quality_cutoff=(20, 20), min_len=30)
        el = time.perf_counter() - t0
        best = el if best is None else min(best, el)
    out["filter_fastq_gb_s"] = round(nb / best / 1e9, 3)
    out["filter_fastq_records_out"] = int(res.records_out)
    print(json.dumps(out))


def main(lib_a, log_path):
    import tempfile
    d = tempfile.mkdtemp(prefix="ffq_ab_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    log = open(log_path, "w")
    me = os.path.abspath(__file__)
    try:
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, me, "gen", d], capture_output=True, text=True)
        print("gen", r.returncode, r.stdout.strip()[-200:], r.stderr.strip()[-300:], flush=True)
        if r.returncode != 0:
            return r.returncode
        got = {"A": [], "B": []}
        for rep in range(REPS):
            for side in (("A", "B") if rep % 2 == 0 else ("B", "A")):          # (who goes first alternates too)
                env = dict(os.environ)
                env.pop("FFQ_HIP_LIB", None)
                if side == "A":
                    env["FFQ_HIP_LIB"] = os.path.abspath(lib_a)
                r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, me, "run", d], capture_output=True, text=True, env=env)
                if r.returncode != 0:          # nothing more on the GPU behind a failure
                    print("run", side, rep, "rc", r.returncode, r.stderr.strip()[-600:], flush=True)
                    return r.returncode
                res = json.loads(r.stdout.strip().splitlines()[-1])
                got[side].append(res)
                log.write(json.dumps({"side": "parent" if side == "A" else "new", "run": rep + 1, "result": res}) + "\n")
                log.flush()
                print(side, rep + 1, res, flush=True)
        for k in ("plain_gb_s", "decode_gb_s", "gzip_gb_s", "bgzf_gb_s", "filter_fastq_gb_s"):
            a, b = [x[k] for x in got["A"]], [x[k] for x in got["B"]]
            med = statistics.median(b)
            line = {"figure": k, "parent_min": min(a), "parent_median": statistics.median(a), "parent_max": max(a), "new_min": min(b),
                    "new_median": med, "new_max": max(b), "new_median_inside_parent_range": min(a) <= med <= max(a)}
            log.write(json.dumps(line) + "\n")
            print(line, flush=True)
        return 0
    finally:
        log.close()
        subprocess.run(["rm", "-rf", d])


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "gen":
        gen(sys.argv[2])
    elif len(sys.argv) > 2 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 3 and os.path.isfile(sys.argv[1]):
        sys.exit(main(sys.argv[1], sys.argv[2]))
    else:
        sys.exit(__doc__)

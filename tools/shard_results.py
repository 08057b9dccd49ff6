"""Every rank's ffq_shard_result over the GPU_CASES matrix of tests/test_sharded.py, one line per rank: what a change of
the shard step's host code must leave byte for byte as it is (run it in two trees, compare the two prints).

    python tools/shard_results.py > shard_results.txt

Drivers: the device step over a resident buffer (pipelined and serial), the file-backed step (ffq_shard_load_fd) and the
slabs (ffq_shard_scan_fd_slabs, 1 MiB slabs), plus the three error streams under each.  k logical ranks as threads of this
process on ONE GPU (hip.ShardWorld: the in-process transport), a fresh context per rank and case, fixed seeds.  Times are
not printed."""
import os
import sys
import threading

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from test_sharded import GPU_CASES, bounds_for, make_stream      # noqa: E402

FIELDS = ("n_rows", "row_lo", "row_hi", "exit_pos", "first_pos", "record_base", "total_records", "rounds", "regathers", "tail",
          "head", "handoff_bytes", "halo_source", "n_slabs", "err_state", "err_byte")
ERROR_CASES = [(kind, world, {}) for kind in ("truncated", "cut-header", "invalid") for world in (2, 8)]


def run_ranks(world, fn):
    from fastqandfurious_amd import hip
    sw = hip.ShardWorld(world)
    lines = [None] * world

    def work(rank):
        ctx = None
        try:
            ctx = hip.Context(0)
            rc, res = fn(rank, ctx, sw)
            lines[rank] = "rc %d " % rc + " ".join("%s %d" % (f, int(getattr(res, f))) for f in FIELDS)
        except BaseException as e:      # noqa: BLE001
            lines[rank] = "raised %s: %s" % (type(e).__name__, e)
            sw.abort()
        finally:
            if ctx is not None:
                ctx.close()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    sw.close()
    return lines


def resident(stream_t, bounds, serial, kw):
    from fastqandfurious_amd import sharded
    world, origin = len(bounds) - 1, bounds[0]

    def work(rank, ctx, sw):
        sc = sharded.NativeShardScanner(ctx, bounds, rank, world, local_world=sw, serial=serial, **kw)
        try:
            lo, hi = bounds[rank], bounds[rank + 1]
            tail, head = sc.halo()
            ext = torch.zeros(tail + (hi - lo) + head + 64, dtype=torch.uint8, device="cuda")
            ext[tail:tail + hi - lo] = stream_t[lo - origin:hi - origin]
            table = torch.empty((stream_t.numel() // 40 + 64, 6), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            sc.sh.step_submit(ext.data_ptr(), table.data_ptr(), table.shape[0])
            return sc.sh.step_wait()
        finally:
            sc.close()
    return run_ranks(world, work)


def from_file(path, world, slab_bytes, kw):
    from fastqandfurious_amd import sharded

    def work(rank, ctx, sw):
        sh = sharded.FileShard(ctx, path, rank, world, comm=sw, slab_bytes=slab_bytes, **kw)
        try:
            sh.load()
            sh._alloc(sh.n_view // 40 + 1024, False)
            ctx.reserve(min(sh.n_view, sh.slab_bytes or sh.n_view) + 64)
            if sh.slab_bytes:
                return sh.sh.scan_fd_slabs(sh.fd, sh.slab_bytes, sh.d_table, sh.table_cap)
            sh.sh.step_submit(sh.d_ext, sh.d_table, sh.table_cap)
            return sh.sh.step_wait()
        finally:
            sh.close()
    return run_ranks(world, work)


def main():
    d = "/dev/shm" if os.path.isdir("/dev/shm") else "/tmp"
    path = os.path.join(d, "ffq_shard_results.%d.fq" % os.getpid())
    streams = {}
    try:
        for kind, world, kw in GPU_CASES + ERROR_CASES:
            if kind not in streams:
                streams[kind] = make_stream(kind)
            stream = streams[kind]
            t = torch.from_numpy(stream.copy()).cuda()
            with open(path, "wb") as fh:
                fh.write(stream.tobytes())
            runs = [("step", lambda: resident(t, bounds_for(stream.size, world, 5 * (1 << 32) + 123457, 48), False, kw)),
                    ("step-serial", lambda: resident(t, bounds_for(stream.size, world), True, kw)),
                    ("file", lambda: from_file(path, world, None, kw)),
                    ("slabs", lambda: from_file(path, world, 1 << 20, kw))]
            for name, run in runs:
                for rank, line in enumerate(run()):
                    print("%s world %d %s %s rank %d: %s" % (kind, world, " ".join("%s %d" % i for i in sorted(kw.items())) or "-", name, rank, line))
                sys.stdout.flush()
    finally:
        if os.path.exists(path):
            os.unlink(path)


if __name__ == "__main__":
    main()

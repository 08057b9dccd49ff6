// ffq_shard_host.h -- one step of the byte-range shards over HOST memory with caller-supplied transport (and, for tests,
// scan): the same protocol functions AND the same loop as the device step (ffq_shard_proto.h: sh_settle), driven
// synchronously.  Who calls it:
//   * the CPU test-suite: ranks are processes of a gloo group (world 2 / 3) or threads, the exchange / gather callbacks go
//     through torch.distributed, the scan callback is the test's own engine -- so the protocol the product runs is the one the
//     multi-process CPU tests exercise (there used to be a second, Python statement of it);
//   * a functional dry run of bench.py's N > 1 path on ONE GPU (FFQ_BENCH_DRY_MULTI: RCCL refuses two ranks per device):
//     scan == NULL means ffq_scan_host on the caller's context, the transport is gloo.
// It is NOT a CPU fallback of anything: without a scan callback it needs a context (a gfx950 device) like every other
// compute entry point.  Included at the end of ffq_hip.hip, behind ffq_shard.h (whose shard_fail_verdict / shard_fill_result
// it ends with); tests/test_tsan.py runs it under ThreadSanitizer (k ranks as threads, a -fsanitize=thread build of the
// library's host code).
#pragma once
#include "ffq_shard_proto.h"

#include <cstdlib>
#include <cstring>
#include <string>

extern "C" void ffq_shard_host_free(void *p) { free(p); }

namespace ffq {

// the rank of one host step: its view, its own block, and sh_settle's hooks over the caller's callbacks
struct ShHostRank {
    const ffq_shard_host_ops *ops;
    ffq_ctx *ctx;
    int rank, world;
    const std::vector<int64_t> &B;
    int64_t head_bytes;
    int64_t *h_table, table_cap;
    ffq_shard_result *out;
    ShView v;
    uint8_t *ext, *grown = nullptr;      // (grown: a view with more look-ahead than the caller's buffer has room for)
    int64_t handoff_bytes = 0;
    int64_t w[SH_BLOCK] = {0};           // my own block: the words and my rows
    std::vector<int64_t> all;
    ShOwnFailure mine;

    // one collective exchange: this rank provides its own bytes out of `src` (its range starts at src + src_tail) and receives
    // what the plan sends it into dst (stream offset dst_start at index 0)
    int serve(const std::vector<ShPiece> &plan, uint8_t *src, int64_t src_tail, uint8_t *dst, int64_t dst_start)
    {
        std::vector<ffq_shard_piece> ps(plan.size());
        for (size_t i = 0; i < plan.size(); i++) {
            const ShPiece &p = plan[i];
            ps[i].src = p.src; ps[i].dst = p.dst; ps[i].a = p.a; ps[i].b = p.b; ps[i].ptr = nullptr;
            if (p.src == rank) { ps[i].ptr = src + src_tail + (p.a - v.lo); handoff_bytes += p.b - p.a; }
            if (p.dst == rank) { ps[i].ptr = dst + (p.a - dst_start); handoff_bytes += p.b - p.a; }
        }
        const int r = ops->exchange(ops->user, ps.data(), (int)ps.size());
        return r ? fail(r < 0 ? r : FFQ_E_INTERNAL, "ffq_shard_host_step: the exchange callback failed (%d)", r) : FFQ_OK;
    }
    // a scan of the current view from stream offset st (< 0: the view's beginning) and its words
    int local(int64_t st)
    {
        sh_owns_no_rows(w);
        if (v.n_bytes == 0) { sh_words_empty(v, head_bytes, w); return FFQ_OK; }
        const int64_t offset = st < 0 ? 0 : std::max(st, v.start) - v.add;
        ffq_scan_result &res = out->scan;
        memset(&res, 0, sizeof res);
        int r;
        if (!ops->scan) r = ffq_scan_host(ctx, ext, v.n_bytes, v.sentinel, offset, v.eof, v.add, 0, 0, h_table, table_cap, nullptr, 0, nullptr, &res);
        else r = ops->scan(ops->user, ext, v.n_bytes, v.sentinel, offset, v.eof, v.add, h_table, table_cap, &res);
        if (r && r != FFQ_E_TABLE_FULL) return r < 0 ? r : fail(FFQ_E_INTERNAL, "ffq_shard_host_step: the scan callback failed (%d)", r);
        const int64_t n = res.n_records;
        if (r == FFQ_E_TABLE_FULL || n > table_cap) {
            const int64_t tf[SH_WORDS] = {SH_UNKNOWN, SH_UNKNOWN, 0, 0, v.head, SH_ERR_TABLE_FULL, n, 0};
            memcpy(w, tf, sizeof tf);
            return FFQ_OK;
        }
        auto lower = [&](int64_t value) {
            int64_t a = 0, b = n;
            while (a < b) { const int64_t m = (a + b) >> 1; if (h_table[m * 6] < value) a = m + 1; else b = m; }
            return a;
        };
        ShScanFacts f;
        f.n = n; f.i0 = lower(sh_lo_bound(v)); f.i1 = lower(sh_hi_bound(v));
        f.p_i0 = f.i0 < n ? h_table[f.i0 * 6] : -1;
        f.p_i1 = f.i1 < n ? h_table[f.i1 * 6] : -1;
        f.q1 = f.i1 > 0 ? h_table[(f.i1 - 1) * 6 + 5] : -1;
        f.end_state = res.end_state; f.last_status = res.last_status; f.last_pos0 = res.last_pos[0]; f.end_offset = res.end_offset;
        sh_words_from(v, f, offset, head_bytes, w);
        w[SH_ROW_LO] = f.i0; w[SH_ROW_HI] = f.i1; w[SH_ROWS] = n;
        return FFQ_OK;
    }

    // ---- sh_settle's hooks: everything is synchronous, so "publish" only sets the words the next gather sends
    int gather(const int64_t **A)
    {
        const int r = ops->allgather(ops->user, w, all.data());
        *A = all.data();
        return r ? fail(r < 0 ? r : FFQ_E_INTERNAL, "ffq_shard_host_step: the gather callback failed (%d)", r) : FFQ_OK;
    }
    const ShView &view() const { return v; }
    int local_failure() const { return mine.code; }
    void look(const ShRound &, const int64_t *, int, int) {}
    int not_ready(int64_t) { return SH_REFUSED; }      // (no scan of this step leaves anything for later)
    int grow(const ShRound &d, const int64_t *A)
    {
        std::vector<ShPiece> plan;
        sh_grow_plan(A, B, d.grow, plan);
        uint8_t *dst = ext, *old = nullptr;
        int64_t dst_start = v.start;
        ShView nv = v;
        if (d.i_grow) {
            // a view with more look-ahead (the caller's buffer has room for its own halo only)
            nv = sh_make_view(v.lo, v.hi, v.total, v.origin, v.tail, A[(size_t)rank * SH_WORDS + 3]);
            uint8_t *g = static_cast<uint8_t *>(malloc((size_t)nv.n_bytes + 64));
            if (!g) return fail(FFQ_E_NOMEM, "ffq_shard_host_step: no memory for a view of %lld bytes", (long long)nv.n_bytes);
            memcpy(g, ext, (size_t)v.n_bytes);
            old = grown;                    // (still the source of what this rank provides in this round)
            grown = g; dst = g; dst_start = nv.start;
        }
        const int rc = serve(plan, ext, v.tail, dst, dst_start);
        free(old);
        if (rc) return rc;
        if (d.i_grow) { ext = grown; v = nv; }
        return FFQ_OK;
    }
    // A failure of THIS rank's scan (the callback's, ffq_scan_host's) must not leave the peers waiting in the next gather for a
    // rank that has gone home: its words say "failed" -- sh_decide makes that INTERNAL on every rank -- and it returns its
    // own error once everybody has seen them.
    int rescan(int64_t st)
    {
        const int rc = local(st);
        if (rc) sh_fail_locally(mine, rc, v, w);
        return FFQ_OK;
    }
    int publish(const int64_t *words)
    {
        if (words) { memcpy(w, words, SH_WORDS * 8); sh_owns_no_rows(w); }
        return FFQ_OK;                      // (else: my words stand; the others' rounds need them again)
    }
};

}  // namespace ffq

extern "C" int ffq_shard_host_step(const ffq_shard_host_ops *ops, ffq_ctx *ctx, int rank, int world, const int64_t *bounds,
                                   int64_t tail_bytes, int64_t head_bytes, uint8_t *h_ext, int64_t *h_table, int64_t table_cap,
                                   ffq_shard_result *out)
{
    using namespace ffq;
    if (!ops || !bounds || !out || !ops->allgather || (world > 1 && !ops->exchange)) return fail(FFQ_E_ARG, "ffq_shard_host_step: NULL argument");
    if (world < 1 || rank < 0 || rank >= world) return fail(FFQ_E_ARG, "ffq_shard_host_step: rank %d of %d", rank, world);
    if (tail_bytes < 1 || head_bytes < 1) return fail(FFQ_E_ARG, "ffq_shard_host_step: tail_bytes and head_bytes must be at least 1");
    for (int r = 0; r < world; r++)
        if (bounds[r] > bounds[r + 1]) return fail(FFQ_E_ARG, "ffq_shard_host_step: bounds must not decrease");
    if (!ops->scan && !ctx) return fail(FFQ_E_ARG, "ffq_shard_host_step: neither a scan callback nor a context");
    memset(out, 0, sizeof *out);
    const std::vector<int64_t> B(bounds, bounds + world + 1);
    int64_t tail, head;
    sh_halo_sizes(B, rank, tail_bytes, head_bytes, &tail, &head);
    const ShView v = sh_make_view(B[rank], B[rank + 1], B[world], B[0], tail, head);
    if (v.n_bytes > 0 && (!h_ext || !h_table)) return fail(FFQ_E_ARG, "ffq_shard_host_step: NULL buffer");
    ShHostRank R{ops, ctx, rank, world, B, head_bytes, h_table, table_cap, out, v, h_ext};
    R.all.resize((size_t)world * SH_WORDS);
    if (world > 1) {
        std::vector<ShPiece> plan;
        sh_halo_plan(B, tail_bytes, head_bytes, plan);
        const int rc = R.serve(plan, h_ext, tail, h_ext, v.start);
        if (rc) return rc;
    }
    R.rescan(-1);
    const ShVerdict verdict = sh_settle(R, world, rank, B);
    if (!verdict.ok()) { free(R.grown); return shard_fail_verdict(verdict, R.mine, out); }
    shard_fill_result(out, R.w, R.all.data(), world, rank, verdict);
    out->handoff_bytes = R.handoff_bytes;
    out->d_ext = R.ext; out->tail = R.v.tail; out->head = R.v.head;       // (ext != h_ext: a grown view; the caller frees it, ffq_shard_host_free)
    return FFQ_OK;
}

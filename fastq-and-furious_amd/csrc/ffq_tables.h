// ffq_tables.h -- host section of ffq_hip.hip: the TABLE CALLS.  A table call works on an offset table that a scan left on the
// device -- six int64 per row, 16-byte aligned -- and, where it looks into the reads, on the buffer that table indexes: it
// answers a question about the rows (lower bound, cut, names, statistics, keys), edits them (the trims, the overlap), keeps some
// and drops the rest (the selects, the dedup set), or writes them out (gather, render, merge).  The scans above know nothing of
// them; the stream front ends (ffq_stream.h, below) chain them.
//
//   * ONE HOST WAIT PER CALL.  A call enqueues everything it does on the context's stream, copies its counters to pinned
//     memory behind that, and waits once (call_blk_end, or the copy of a scratch word).
//   * GROW BEFORE ENQUEUE.  Growing a scratch buffer waits for the stream (grow_dev), so everything a call needs is grown
//     before its first kernel is enqueued: compact_reserve and compact_enqueue are two functions for that reason.
//   * SCRATCH BELONGS TO THE CONTEXT, not to a pass: the list of long rows, the verdict bytes, the counts and bases of the
//     compaction, the counter block.  Calls on a context follow one another, so one of each serves all of them -- and a call is
//     refused while a scan is pending on the context (no_pending).
//
// The kernels are in the headers the sections name.  Error texts are part of what tests see.

// ---- what the table calls check and set up alike ------------------------------------------------
static unsigned rows_grid(int64_t n_rows, int per_wg, int cap) { return (unsigned)std::min<int64_t>((n_rows + per_wg - 1) / per_wg, cap); }

// every pointer a multiple of `align` (a power of two; NULL passes)
static bool aligned(std::initializer_list<const void *> ps, uintptr_t align)
{
    uintptr_t all = 0;
    for (const void *q : ps) all |= reinterpret_cast<uintptr_t>(q);
    return (all & (align - 1)) == 0;
}

// a table call reads and writes what a pending scan's front may still be writing: refused
static int no_pending(const ffq_ctx *c, const char *who)
{
    return c->pend.active ? fail(FFQ_E_ARG, "%s: a scan is pending on this context", who) : FFQ_OK;
}

static bool view_ok(const ffq_table_view *m, int64_t n_rows)
{
    return m && m->n_bytes >= 0 && (n_rows == 0 || m->d_table) && aligned({m->d_table}, 16);
}

// the CSR offsets of no rows (d_off, where the caller wants them): one zero
static int no_rows_offsets(ffq_ctx *c, int64_t *d_off)
{
    if (!d_off) return FFQ_OK;
    HIPCHK(hipMemsetAsync(d_off, 0, sizeof(int64_t), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FFQ_OK;
}

// a mate's buffer and table as the pair kernels take them
static PairSide pair_side(const ffq_table_view *m) { return PairSide{m->d_buf, m->n_bytes, m->sentinel ? 1 : 0, m->add, m->d_table}; }

// a buffer behind either view that has bytes; to_what: the call's words for what it reads them for
static int pair_bufs(const char *who, const ffq_table_view *m1, const ffq_table_view *m2, const char *to_what)
{
    if ((m1->n_bytes > 0 && !m1->d_buf) || (m2->n_bytes > 0 && !m2->d_buf)) return fail(FFQ_E_ARG, "%s: no buffer to %s", who, to_what);
    return FFQ_OK;
}

// What the calls on two tables of mates check and set up alike, in the order a call with two bad arguments is answered in:
// the context, args_ok (the caller's own pointers) and the two views; own() -- the checks that are the call's alone --; a buffer
// behind the views (to_what NULL: the call does not read the mates' bytes, or looks for the buffers itself, in own() or later);
// no scan pending; the device.
template <class Own>
static int pairs_begin(ffq_ctx *c, const char *who, bool args_ok, const ffq_table_view *m1, const ffq_table_view *m2, int64_t n_pairs,
                       const char *to_what, Own own)
{
    if (!c || !args_ok || n_pairs < 0 || !view_ok(m1, n_pairs) || !view_ok(m2, n_pairs)) return fail(FFQ_E_ARG, "%s: bad argument", who);
    int rc = own();
    if (!rc && to_what) rc = pair_bufs(who, m1, m2, to_what);
    if (!rc) rc = no_pending(c, who);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    return FFQ_OK;
}

// The counters of a call, one block per context: calls on a context follow one another, so one block serves all of them.  B is
// the call's block type, at the head of the context's words.  begin: cleared on the stream, the device's copy handed back;
// end: copied to the pinned half and waited for -- the call's one host wait -- and that half handed back.
template <class B>
static B *call_blk_as(uint64_t *words)
{
    static_assert(sizeof(B) <= CALL_BLK_WORDS * sizeof(uint64_t) && alignof(B) <= alignof(uint64_t), "CALL_BLK_WORDS");
    return reinterpret_cast<B *>(words);
}

template <class B>
static int call_blk_begin(ffq_ctx *c, B **d_blk)
{
    *d_blk = call_blk_as<B>(c->blk.d.p);
    HIPCHK(hipMemsetAsync(c->blk.d, 0, sizeof(B), c->stream));
    return FFQ_OK;
}

template <class B>
static int call_blk_end(ffq_ctx *c, const B **h_blk)
{
    *h_blk = call_blk_as<B>(c->blk.h.p);
    HIPCHK(hipMemcpyAsync(c->blk.h, c->blk.d, sizeof(B), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return FFQ_OK;
}

// ---- the compaction of csrc/ffq_compact.h, enqueued: count, scan, scatter -----------------------
// (two steps, because everything is grown before anything is enqueued: growing waits for the stream)
static int compact_reserve(ffq_ctx *c, int64_t n)
{
    const int64_t nblk = (n + 255) / 256;
    int rc = grow_dev(c, c->sel_cnt, nblk);
    if (!rc) rc = grow_dev(c, c->sel_base, nblk);
    return rc;
}

template <class Keep, int NT, bool ORD>
static void compact_launch(ffq_ctx *c, hipStream_t st, Keep keep, int64_t n, const int64_t *t1, const int64_t *t2, const int64_t *ord,
                           int64_t *out1, int64_t *out2, int64_t *idx)
{
    hipLaunchKernelGGL((k_compact_scatter<Keep, NT, ORD>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keep, n,
                       (const long long *)c->sel_base, t1, t2, ord, out1, out2, idx);
}

// behind a count kernel that filled c->sel_cnt: the scan and the scatter, the instantiation for the tables (a NULL one is not
// copied) and `ord` there are.  The number of kept rows is left in c->d_word[0].
template <class Keep>
static int compact_scatter(ffq_ctx *c, hipStream_t st, Keep keep, int64_t n, const int64_t *t1, const int64_t *t2, const int64_t *ord,
                           int64_t *out1, int64_t *out2, int64_t *idx)
{
    const int64_t nblk = (n + 255) / 256;
    const int rc = launch_scan(c, st, (const unsigned int *)c->sel_cnt, nblk, c->sel_base, ScanToWord{(long long *)c->d_word.p});
    if (rc) return rc;
    if (!t1) { t1 = t2; out1 = out2; t2 = nullptr; }       // (one table: it is the first)
    auto *launch = !t1 ? (ord ? compact_launch<Keep, 0, true> : compact_launch<Keep, 0, false>)
                 : !t2 ? (ord ? compact_launch<Keep, 1, true> : compact_launch<Keep, 1, false>)
                       : (ord ? compact_launch<Keep, 2, true> : compact_launch<Keep, 2, false>);
    launch(c, st, keep, n, t1, t2, ord, out1, out2, idx);
    return FFQ_OK;
}

template <class Keep>
static int compact_enqueue(ffq_ctx *c, hipStream_t st, Keep keep, int64_t n, const int64_t *t1, const int64_t *t2, const int64_t *ord,
                           int64_t *out1, int64_t *out2, int64_t *idx)
{
    hipLaunchKernelGGL((k_compact_count<Keep>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keep, n, c->sel_cnt.p);
    return compact_scatter(c, st, keep, n, t1, t2, ord, out1, out2, idx);
}

extern "C" int ffq_entrypos(ffq_ctx *c, const uint8_t *h_buf, int64_t len, int64_t offset, int64_t *pos,
                            int *status)
{
    mark_other(c);
    if (!c || !pos || !status) return fail(FFQ_E_ARG, "ffq_entrypos: NULL argument");
    int64_t row[6];
    ffq_scan_result r;
    int rc = ffq_scan_host(c, h_buf, len, 0, offset, 0, 0, 0, 0, row, 1, nullptr, 0, nullptr, &r);
    if (rc != FFQ_OK && rc != FFQ_E_TABLE_FULL) return rc;
    if (r.n_records >= 1) {
        for (int i = 0; i < 6; i++) pos[i] = row[i];
        *status = FFQ_COMPLETE;
    } else {
        for (int i = 0; i < 6; i++) pos[i] = r.last_pos[i];
        *status = r.last_status;
    }
    g_err.clear();
    return FFQ_OK;
}

extern "C" int ffq_table_lower_bound(ffq_ctx *c, const int64_t *d_table, int64_t n_rows, int col,
                                     int64_t value, int64_t *idx)
{
    mark_other(c);
    if (!c || !idx || n_rows < 0 || col < 0 || col > 5 || (n_rows > 0 && !d_table))
        return fail(FFQ_E_ARG, "ffq_table_lower_bound: bad argument");
    HIPCHK(hipSetDevice(c->device));
    int64_t *slot = c->h_word, *dslot = c->d_word;
    hipLaunchKernelGGL(k_table_lower_bound, dim3(1), dim3(64), 0, c->stream, d_table, n_rows, col, value, dslot);
    HIPCHK(hipMemcpyAsync(slot, dslot, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    *idx = *slot;
    return FFQ_OK;
}

extern "C" int ffq_table_cut(ffq_ctx *c, const int64_t *d_table, int64_t n_rows, int64_t lo, int64_t hi,
                             int64_t out[6])
{
    mark_other(c);
    if (!c || !out || n_rows < 0 || (n_rows > 0 && !d_table)) return fail(FFQ_E_ARG, "ffq_table_cut: bad argument");
    HIPCHK(hipSetDevice(c->device));
    hipLaunchKernelGGL(k_table_cut, dim3(1), dim3(64), 0, c->stream, d_table, n_rows, lo, hi, c->d_cut);
    HIPCHK(hipMemcpyAsync(c->h_cut, c->d_cut, 6 * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < 6; i++) out[i] = c->h_cut[i];
    return FFQ_OK;
}

static int table_select(ffq_ctx *c, const int64_t *d_table, int64_t n_rows, int64_t min_len, int64_t max_len, int64_t *d_out,
                        int64_t *d_idx, int64_t *n_out);

extern "C" int ffq_table_select_seqlen(ffq_ctx *c, const int64_t *d_table, int64_t n_rows, int64_t min_len,
                                       int64_t max_len, int64_t *d_out, int64_t *n_out)
{
    return table_select(c, d_table, n_rows, min_len, max_len, d_out, nullptr, n_out);
}

extern "C" int ffq_table_select_seqlen_idx(ffq_ctx *c, const int64_t *d_table, int64_t n_rows, int64_t min_len,
                                           int64_t max_len, int64_t *d_out, int64_t *d_idx, int64_t *n_out)
{
    return table_select(c, d_table, n_rows, min_len, max_len, d_out, d_idx, n_out);
}

// (d_idx, optional: the ordinal of every kept row -- the stream front end's push-down, ffq_stream_set_filter)
static int table_select(ffq_ctx *c, const int64_t *d_table, int64_t n_rows, int64_t min_len, int64_t max_len, int64_t *d_out,
                        int64_t *d_idx, int64_t *n_out)
{
    mark_other(c);
    if (!c || !n_out || n_rows < 0 || (n_rows > 0 && (!d_table || !d_out)))
        return fail(FFQ_E_ARG, "ffq_table_select_seqlen: bad argument");
    if (d_table == d_out && n_rows > 0) return fail(FFQ_E_ARG, "ffq_table_select_seqlen: d_out must not be d_table");
    if (!aligned({d_table, d_out}, 16)) return fail(FFQ_E_ARG, "ffq_table_select_seqlen: tables must be 16-byte aligned");
    HIPCHK(hipSetDevice(c->device));
    *n_out = 0;
    if (n_rows == 0) return FFQ_OK;
    int rc = compact_reserve(c, n_rows);
    if (rc) return rc;
    hipStream_t st = c->stream;
    if ((rc = compact_enqueue(c, st, KeepLen{d_table, min_len, max_len}, n_rows, d_table, nullptr, nullptr, d_out, nullptr, d_idx))) return rc;
    HIPCHK(hipMemcpyAsync(c->h_word, c->d_word, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    *n_out = c->h_word[0];
    return FFQ_OK;
}

// ---- column selection ----------------------------------------------------------------------
extern "C" int ffq_table_gather_column(ffq_ctx *c, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                                       const int64_t *d_table, int64_t n_rows, int col_begin, int begin_shift,
                                       int col_end, int value_add, int8_t *d_out, int64_t out_cap, int64_t *d_off,
                                       int64_t *n_out_bytes)
{
    mark_other(c);
    if (!c || !n_out_bytes || n_rows < 0 || n_bytes < 0 || out_cap < 0 || !d_off || (n_rows > 0 && !d_table))
        return fail(FFQ_E_ARG, "ffq_table_gather_column: bad argument");
    if (out_cap > 0 && (!d_out || (n_bytes > 0 && !d_buf)))
        return fail(FFQ_E_ARG, "ffq_table_gather_column: no output, or no buffer, to copy %lld bytes", (long long)out_cap);
    if (col_begin < 0 || col_begin > 5 || col_end < 0 || col_end > 5)
        return fail(FFQ_E_ARG, "ffq_table_gather_column: columns are 0..5");
    if (int rc = no_pending(c, "ffq_table_gather_column")) return rc;
    HIPCHK(hipSetDevice(c->device));
    *n_out_bytes = 0;
    hipStream_t st = c->stream;
    if (n_rows == 0) return no_rows_offsets(c, d_off);
    const int64_t nblk = (n_rows + 255) / 256;
    int rc = grow_dev(c, c->col_sum, nblk);
    // the copy kernel's scratch: a start per row, the directory of the output stream
    const int64_t nqb = (out_cap + DQ_BLK - 1) / DQ_BLK + 1;
    if (!rc) rc = reserve_qdir(c, nqb);
    if (!rc) rc = reserve_p4s(c, n_rows);
    if (rc) return rc;
    hipLaunchKernelGGL(k_col_sum, dim3((unsigned)nblk), dim3(256), 0, st, d_table, n_rows, col_begin, begin_shift, col_end,
                       n_bytes, sentinel ? 1 : 0, add, c->col_sum);
    if ((rc = launch_scan(c, st, (const long long *)c->col_sum, nblk, c->col_sum, ScanToRes{c->col_res, n_rows}))) return rc;
    hipLaunchKernelGGL(k_col_offsets, dim3((unsigned)nblk), dim3(256), 0, st, d_table, n_rows, col_begin, begin_shift,
                       col_end, n_bytes, sentinel ? 1 : 0, add, (const long long *)c->col_sum, (const DevRes *)c->col_res, d_off,
                       c->p4s, c->qdir, c->qdir.cap);
    if (out_cap > 0)
        hipLaunchKernelGGL(k_decode_stream, dim3((unsigned)nqb), dim3(256), 0, st, d_buf, n_bytes, sentinel ? 1 : 0,
                           (const int64_t *)c->p4s, (const int64_t *)d_off, (const int64_t *)c->qdir,
                           (const DevRes *)c->col_res, n_rows, add, value_add, d_out, out_cap);
    HIPCHK(hipMemcpyAsync(c->h_word, &c->col_res->n_qual_bytes, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    *n_out_bytes = c->h_word[0];
    if (*n_out_bytes > out_cap)
        return fail(FFQ_E_TABLE_FULL, "output holds %lld bytes, the column has %lld", (long long)out_cap,
                    (long long)*n_out_bytes);
    return FFQ_OK;
}

// ---- the table passes on csrc/ffq_rows.h: quality trim, adapter trim, poly tails, ends, statistics (ffq_trim.h, ffq_adapter.h, ffq_poly.h, ffq_ends.h, ffq_stats.h) ----
// Workgroups of a pass's launches, each capped: they stride over what there is.  The short rows' launch has WG / ROWS_G rows
// per workgroup and step; the long rows' launches have a wave per row, and as the list's length is known on the device only,
// they are sized by the table.
constexpr int EDIT_GRID_SHORT = 2048, EDIT_GRID_LONG = 1024;                       // the three trims
constexpr int STATS_GRID_SHORT = 512, STATS_GRID_CHECK = 512, STATS_GRID_COUNT = 128;   // (two workgroups per CU: their LDS); x tiles

// What the passes check and set up alike.  args_ok: the caller's own pointers; d_dst: what the pass writes on the device.  With
// rows, the long list is grown (before anything is enqueued: growing waits for the stream) and the call's counters are cleared:
// *blk.  The list and the counters are the context's, not a pass's: calls on a context follow one another.
static int rows_begin(ffq_ctx *c, const char *who, bool args_ok, const uint8_t *d_buf, int64_t n_bytes, const int64_t *d_table,
                      int64_t n_rows, const void *d_dst, RowsBlock **blk)
{
    if (!c || !args_ok || n_rows < 0 || n_bytes < 0 || (n_bytes > 0 && !d_buf) || (n_rows > 0 && (!d_table || !d_dst)))
        return fail(FFQ_E_ARG, "%s: bad argument", who);
    if (!aligned({d_table, d_dst}, 16)) return fail(FFQ_E_ARG, "%s: the table and what is written must be 16-byte aligned", who);
    if (int rc = no_pending(c, who)) return rc;
    HIPCHK(hipSetDevice(c->device));
    if (n_rows == 0) return FFQ_OK;
    const int rc = grow_dev(c, c->rows_list, n_rows);
    if (rc) return rc;
    return call_blk_begin(c, blk);
}

// the counters of an editing pass back: the call's one host wait
static int rows_end(ffq_ctx *c, int64_t stats[3])
{
    const RowsBlock *h = nullptr;
    const int rc = call_blk_end(c, &h);
    if (rc) return rc;
    stats[0] = (int64_t)h->changed; stats[1] = (int64_t)h->removed; stats[2] = (int64_t)h->skipped;
    return FFQ_OK;
}

// A row-editing pass from its call to its counters: the frame of the four trims.  arg_rc: what the pass's own check of its
// parameters said; launch(st, s, blk): its two launches, the short rows' and the long rows', on the context's stream.
template <class Launch>
static int rows_edit(ffq_ctx *c, const char *who, int arg_rc, const uint8_t *d_buf, int64_t n_bytes, int sentinel, const int64_t *d_table,
                     int64_t n_rows, int64_t *d_out, int64_t stats[3], Launch launch)
{
    mark_other(c);
    RowsBlock *blk = nullptr;
    int rc = arg_rc;
    if (!rc) rc = rows_begin(c, who, stats != nullptr, d_buf, n_bytes, d_table, n_rows, d_out, &blk);
    if (rc) return rc;
    stats[0] = stats[1] = stats[2] = 0;
    if (n_rows == 0) return FFQ_OK;
    launch(c->stream, sentinel ? 1 : 0, blk);
    return rows_end(c, stats);
}

// parameters of a quality trim and of a statistics call, checked: for the table calls and for the stream's setters
static int trim_arg(const char *who, int qual_base, int cutoff_front, int cutoff_back)
{
    if (cutoff_front < 0 || cutoff_front > 127 || cutoff_back < 0 || cutoff_back > 127) return fail(FFQ_E_ARG, "%s: cutoffs are 0..127", who);
    if (qual_base < 0 || qual_base > 255) return fail(FFQ_E_ARG, "%s: qual_base is 0..255", who);
    return FFQ_OK;
}

static int stats_arg(const char *who, int qual_base, int max_cycles)
{
    if (max_cycles < 1 || max_cycles > FFQ_STATS_MAX_CYCLES) return fail(FFQ_E_ARG, "%s: max_cycles is 1..%d", who, FFQ_STATS_MAX_CYCLES);
    if (qual_base < 0 || qual_base > 255) return fail(FFQ_E_ARG, "%s: qual_base is 0..255", who);
    return FFQ_OK;
}

extern "C" int ffq_table_trim_quality(ffq_ctx *c, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                                      const int64_t *d_table, int64_t n_rows, int qual_base, int cutoff_front,
                                      int cutoff_back, int64_t *d_out, int64_t stats[3])
{
    static const char *const who = "ffq_table_trim_quality";
    return rows_edit(c, who, trim_arg(who, qual_base, cutoff_front, cutoff_back), d_buf, n_bytes, sentinel, d_table, n_rows, d_out, stats,
                     [&](hipStream_t st, int s, RowsBlock *blk) {
        hipLaunchKernelGGL(k_trim_rows, dim3(rows_grid(n_rows, TRIM_WG / ROWS_G, EDIT_GRID_SHORT)), dim3(TRIM_WG), 0, st, d_buf, n_bytes, s,
                           add, d_table, n_rows, qual_base, cutoff_front, cutoff_back, d_out, c->rows_list, blk);
        hipLaunchKernelGGL(k_trim_long, dim3(rows_grid(n_rows, TRIM_WG / 64, EDIT_GRID_LONG)), dim3(TRIM_WG), 0, st, d_buf, n_bytes, s,
                           add, d_table, qual_base, cutoff_front, cutoff_back, d_out, (const int64_t *)c->rows_list, blk);
    });
}

// parameters of an adapter call, checked; the adapter's bytes and its wildcard mask as the kernels take them
static int adapter_arg(const char *who, const uint8_t *adapter, int adapter_len, int err_permille, int min_overlap, AdapterArg *ad)
{
    if (!adapter || adapter_len < 1 || adapter_len > ADAPTER_MAX) return fail(FFQ_E_ARG, "%s: the adapter has 1..%d bytes", who, ADAPTER_MAX);
    if (min_overlap < 1 || min_overlap > adapter_len) return fail(FFQ_E_ARG, "%s: min_overlap is 1..adapter_len", who);
    if (err_permille < 0 || err_permille > 1000) return fail(FFQ_E_ARG, "%s: err_permille is 0..1000", who);
    if (ad) {
        memset(ad, 0, sizeof *ad);
        for (int j = 0; j < adapter_len; j++) {
            ad->a[j >> 2] |= (uint32_t)adapter[j] << (8 * (j & 3));
            if (adapter[j] != (uint8_t)'N') ad->k[j >> 2] |= 0xFFu << (8 * (j & 3));
        }
    }
    return FFQ_OK;
}

extern "C" int ffq_table_trim_adapter(ffq_ctx *c, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                                      const int64_t *d_table, int64_t n_rows, const uint8_t *adapter, int adapter_len,
                                      int err_permille, int min_overlap, int64_t *d_out, int64_t stats[3])
{
    static const char *const who = "ffq_table_trim_adapter";
    AdapterArg ad;
    return rows_edit(c, who, adapter_arg(who, adapter, adapter_len, err_permille, min_overlap, &ad), d_buf, n_bytes, sentinel, d_table, n_rows,
                     d_out, stats, [&](hipStream_t st, int s, RowsBlock *blk) {
        hipLaunchKernelGGL(k_adapter_rows, dim3(rows_grid(n_rows, ADAPTER_WG / ROWS_G, EDIT_GRID_SHORT)), dim3(ADAPTER_WG), 0, st, d_buf,
                           n_bytes, s, add, d_table, n_rows, ad, adapter_len, err_permille, min_overlap, d_out, c->rows_list, blk);
        hipLaunchKernelGGL(k_adapter_long, dim3(rows_grid(n_rows, ADAPTER_WG / 64, EDIT_GRID_LONG)), dim3(ADAPTER_WG), 0, st, d_buf,
                           n_bytes, s, add, d_table, ad, adapter_len, err_permille, min_overlap, d_out, (const int64_t *)c->rows_list, blk);
    });
}

// parameters of a poly-tail call, checked: for the table call and for ffq_stream_set_poly
static_assert(POLY_ANY == FFQ_POLY_ANY, "include/ffq.h");
static int poly_arg(const char *who, int base, int min_len)
{
    if (base != FFQ_POLY_ANY && (base < 0 || base > 3)) return fail(FFQ_E_ARG, "%s: base is 0..3 (A, C, G, T) or FFQ_POLY_ANY", who);
    if (min_len < POLY_MIN_LEN_LO || min_len > POLY_MIN_LEN_HI) return fail(FFQ_E_ARG, "%s: min_len is %d..%d", who, POLY_MIN_LEN_LO, POLY_MIN_LEN_HI);
    return FFQ_OK;
}

extern "C" int ffq_table_trim_poly(ffq_ctx *c, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                                   const int64_t *d_table, int64_t n_rows, int base, int min_len, int64_t *d_out, int64_t stats[3])
{
    static const char *const who = "ffq_table_trim_poly";
    return rows_edit(c, who, poly_arg(who, base, min_len), d_buf, n_bytes, sentinel, d_table, n_rows, d_out, stats,
                     [&](hipStream_t st, int s, RowsBlock *blk) {
        hipLaunchKernelGGL(k_poly_rows, dim3(rows_grid(n_rows, POLY_WG / ROWS_G, EDIT_GRID_SHORT)), dim3(POLY_WG), 0, st, d_buf, n_bytes, s,
                           add, d_table, n_rows, base, min_len, d_out, c->rows_list, blk);
        hipLaunchKernelGGL(k_poly_long, dim3(rows_grid(n_rows, POLY_WG / 64, EDIT_GRID_LONG)), dim3(POLY_WG), 0, st, d_buf, n_bytes, s,
                           add, d_table, base, min_len, d_out, (const int64_t *)c->rows_list, blk);
    });
}

// the rules of an ends call, checked, as the kernels take them: for the table call and for ffq_stream_set_ends
static_assert(ENDS_WINDOW_MAX == 64 && ENDS_QUALITY_LO == 1 && ENDS_QUALITY_HI == 93, "include/ffq.h");
static int ends_arg(const char *who, const ffq_ends_rules *r, EndsRules *R)
{
    if (!r) return fail(FFQ_E_ARG, "%s: NULL rules", who);
    if (r->trim_front < 0 || r->trim_tail < 0 || r->keep_len < 0) return fail(FFQ_E_ARG, "%s: trim_front, trim_tail and keep_len are >= 0", who);
    if (r->qual_base < 0 || r->qual_base > 255) return fail(FFQ_E_ARG, "%s: qual_base is 0..255", who);
    const EndsStage st[3] = {{r->front_window, r->front_quality}, {r->right_window, r->right_quality}, {r->tail_window, r->tail_quality}};
    for (const EndsStage &e : st) {
        if (e.window < 0 || e.window > ENDS_WINDOW_MAX) return fail(FFQ_E_ARG, "%s: a window is 0..%d", who, ENDS_WINDOW_MAX);
        if (e.window > 0 && (e.quality < ENDS_QUALITY_LO || e.quality > ENDS_QUALITY_HI))
            return fail(FFQ_E_ARG, "%s: the quality of a window is %d..%d", who, ENDS_QUALITY_LO, ENDS_QUALITY_HI);
    }
    if (!r->trim_front && !r->trim_tail && !r->keep_len && !st[0].window && !st[1].window && !st[2].window)
        return fail(FFQ_E_ARG, "%s: every rule is off", who);
    if (R) *R = EndsRules{r->trim_front, r->trim_tail, r->keep_len, r->qual_base, st[0], st[1], st[2]};
    return FFQ_OK;
}

extern "C" int ffq_table_trim_ends(ffq_ctx *c, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                                   const int64_t *d_table, int64_t n_rows, const ffq_ends_rules *rules, int64_t *d_out, int64_t stats[3])
{
    static const char *const who = "ffq_table_trim_ends";
    EndsRules R;
    return rows_edit(c, who, ends_arg(who, rules, &R), d_buf, n_bytes, sentinel, d_table, n_rows, d_out, stats,
                     [&](hipStream_t st, int s, RowsBlock *blk) {
        hipLaunchKernelGGL(k_ends_rows, dim3(rows_grid(n_rows, ENDS_WG / ROWS_G, EDIT_GRID_SHORT)), dim3(ENDS_WG), 0, st, d_buf, n_bytes, s,
                           add, d_table, n_rows, R, d_out, c->rows_list, blk);
        hipLaunchKernelGGL(k_ends_long, dim3(rows_grid(n_rows, ENDS_WG / 64, EDIT_GRID_LONG)), dim3(ENDS_WG), 0, st, d_buf, n_bytes, s,
                           add, d_table, R, d_out, (const int64_t *)c->rows_list, blk);
    });
}

static_assert(STATS_QBINS == FFQ_STATS_QBINS && STATS_GCBINS == FFQ_STATS_GCBINS && STATS_HEAD == FFQ_STATS_HEAD &&
              STATS_MAX_CYCLES == FFQ_STATS_MAX_CYCLES && stats_words(150) == FFQ_STATS_WORDS(150), "include/ffq.h");

extern "C" int ffq_table_stats(ffq_ctx *c, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                               const int64_t *d_table, int64_t n_rows, int qual_base, int max_cycles, int accumulate,
                               uint64_t *d_stats, int64_t head[FFQ_STATS_HEAD])
{
    mark_other(c);
    int rc = stats_arg("ffq_table_stats", qual_base, max_cycles);
    RowsBlock *blk = nullptr;
    if (!rc) rc = rows_begin(c, "ffq_table_stats", d_stats != nullptr, d_buf, n_bytes, d_table, n_rows, d_stats, &blk);
    if (rc) return rc;
    hipStream_t st = c->stream;
    stats_u64 *out = reinterpret_cast<stats_u64 *>(d_stats);
    if (!accumulate) HIPCHK(hipMemsetAsync(d_stats, 0, (size_t)stats_words(max_cycles) * 8, st));
    if (n_rows > 0) {
        // every workgroup of the short rows' launch flushes a whole tile at its end; the rows it left are checked and counted
        // per read first, then per cycle tile
        hipLaunchKernelGGL(k_stats_rows, dim3(rows_grid(n_rows, STATS_WG / STATS_G, STATS_GRID_SHORT)), dim3(STATS_WG), 0, st, d_buf,
                           n_bytes, sentinel ? 1 : 0, add, d_table, n_rows, qual_base, max_cycles, out, c->rows_list, blk);
        hipLaunchKernelGGL(k_stats_long_check, dim3(rows_grid(n_rows, STATS_WG / 64, STATS_GRID_CHECK)), dim3(STATS_WG), 0, st, d_buf,
                           n_bytes, sentinel ? 1 : 0, add, d_table, qual_base, max_cycles, out, c->rows_list,
                           (const RowsBlock *)blk);
        const int n_tiles = (max_cycles + STATS_TILE - 1) / STATS_TILE;
        hipLaunchKernelGGL(k_stats_long_count, dim3(rows_grid(n_rows, STATS_WG / 64, STATS_GRID_COUNT), (unsigned)n_tiles),
                           dim3(STATS_WG), 0, st, d_buf, n_bytes, sentinel ? 1 : 0, add, d_table, qual_base, max_cycles, out,
                           (const int64_t *)c->rows_list, (const RowsBlock *)blk);
    }
    HIPCHK(hipGetLastError());
    if (head) {
        HIPCHK(hipMemcpyAsync(c->h_stats, d_stats, STATS_HEAD * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int i = 0; i < STATS_HEAD; i++) head[i] = (int64_t)c->h_stats[i];
    }
    return FFQ_OK;
}

// ---- rows kept or dropped for what is in the read (csrc/ffq_filter.h) ---------------------------
static_assert(FILTER_COUNTS == FFQ_FILTER_COUNTS, "include/ffq.h");
static const uint32_t g_ee_micro[STATS_QBINS] = {FFQ_EE_MICRO_VALUES};
extern "C" const uint32_t *ffq_ee_micro_table(void) { return g_ee_micro; }

// content rules checked (NULL: every rule off); *on: one of rules 2 to 6 is switched on; R: as the kernels take them
static int content_arg(const char *who, const ffq_content_rules *r, bool *on, FilterRules *R)
{
    *on = false;
    if (!r) return FFQ_OK;
    if (r->qual_base < 0 || r->qual_base > 255) return fail(FFQ_E_ARG, "%s: qual_base is 0..255", who);
    if (r->max_n < -1) return fail(FFQ_E_ARG, "%s: max_n is -1 (off) or a count", who);
    if (r->min_mean_qual < 0 || r->min_mean_qual > 95) return fail(FFQ_E_ARG, "%s: min_mean_qual is 0 (off) or 1..95", who);
    if (r->qualified_qual < 0 || r->qualified_qual > 95) return fail(FFQ_E_ARG, "%s: qualified_qual is 0..95", who);
    if (r->max_unqualified_pct < -1 || r->max_unqualified_pct > 100) return fail(FFQ_E_ARG, "%s: max_unqualified_pct is -1 (off) or 0..100", who);
    if (r->min_complexity_pct < 0 || r->min_complexity_pct > 100) return fail(FFQ_E_ARG, "%s: min_complexity_pct is 0 (off) or 1..100", who);
    if (r->max_ee_micro < -1) return fail(FFQ_E_ARG, "%s: max_ee_micro is -1 (off) or a number of millionths", who);
    *on = r->max_n >= 0 || r->min_mean_qual > 0 || r->max_unqualified_pct >= 0 || r->max_ee_micro >= 0 || r->min_complexity_pct > 0;
    if (R) *R = FilterRules{r->qual_base, r->max_n, r->min_mean_qual, r->qualified_qual, r->max_unqualified_pct, r->min_complexity_pct,
                            (long long)r->max_ee_micro};
    return FFQ_OK;
}

constexpr int FILTER_GRID_SHORT = 2048, FILTER_GRID_LONG = 1024;

extern "C" int ffq_table_select_reads(ffq_ctx *c, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                                      const int64_t *d_table, int64_t n_rows, int64_t min_len, int64_t max_len,
                                      const ffq_content_rules *rules, int64_t *d_out, int64_t *d_idx, int64_t *n_out,
                                      int64_t counts[FFQ_FILTER_COUNTS])
{
    static const char *const who = "ffq_table_select_reads";
    mark_other(c);
    bool on = false;
    FilterRules R = {};
    int rc = content_arg(who, rules, &on, &R);
    if (rc) return rc;
    if (!c || !n_out || !counts || n_rows < 0 || n_bytes < 0 || (n_rows > 0 && (!d_table || !d_out)))
        return fail(FFQ_E_ARG, "%s: bad argument", who);
    if ((rc = no_pending(c, who))) return rc;
    for (int i = 0; i < FFQ_FILTER_COUNTS; i++) counts[i] = 0;
    if (!on) {
        // no content rule: the length filter as it is -- nothing reads the buffer, nothing new is launched
        rc = table_select(c, d_table, n_rows, min_len, max_len, d_out, d_idx, n_out);
        if (!rc) { counts[0] = *n_out; counts[1] = n_rows - *n_out; }
        return rc;
    }
    if (n_bytes > 0 && !d_buf) return fail(FFQ_E_ARG, "%s: no buffer to judge the rows by", who);
    if (d_table == d_out && n_rows > 0) return fail(FFQ_E_ARG, "%s: d_out must not be d_table", who);
    if (!aligned({d_table, d_out}, 16)) return fail(FFQ_E_ARG, "%s: tables must be 16-byte aligned", who);
    HIPCHK(hipSetDevice(c->device));
    *n_out = 0;
    if (n_rows == 0) return FFQ_OK;
    // (everything is grown before anything is enqueued: growing waits for the stream)
    rc = grow_dev(c, c->rows_list, n_rows);
    if (!rc) rc = grow_dev(c, c->filter_verdict, n_rows);
    if (!rc) rc = compact_reserve(c, n_rows);
    if (rc) return rc;
    hipStream_t st = c->stream;
    const int s = sentinel ? 1 : 0;
    FilterBlock *blk = nullptr;
    if ((rc = call_blk_begin(c, &blk))) return rc;
    hipLaunchKernelGGL(k_filter_rows, dim3(rows_grid(n_rows, FILTER_WG / FILTER_G, FILTER_GRID_SHORT)), dim3(FILTER_WG), 0, st, d_buf,
                       n_bytes, s, add, d_table, n_rows, min_len, max_len, R, c->filter_verdict.p, c->rows_list.p, blk);
    hipLaunchKernelGGL(k_filter_long, dim3(rows_grid(n_rows, FILTER_WG / 64, FILTER_GRID_LONG)), dim3(FILTER_WG), 0, st, d_buf,
                       n_bytes, s, add, d_table, R, c->filter_verdict.p, (const int64_t *)c->rows_list, blk);
    if ((rc = compact_enqueue(c, st, KeepVerdict{c->filter_verdict.p}, n_rows, d_table, nullptr, nullptr, d_out, nullptr, d_idx))) return rc;
    const FilterBlock *h = nullptr;
    if ((rc = call_blk_end(c, &h))) return rc;
    for (int i = 0; i < FFQ_FILTER_COUNTS; i++) counts[i] = (int64_t)h->cnt[i];
    *n_out = counts[0];
    return FFQ_OK;
}

// ---- two tables whose rows are mates (csrc/ffq_pair.h) ------------------------------------------
static_assert(PAIR_ANY == FFQ_PAIR_ANY && PAIR_BOTH == FFQ_PAIR_BOTH && PAIR_FIRST == FFQ_PAIR_FIRST, "include/ffq.h");

constexpr int PAIR_GRID_COUNT = 1024;

// the counters of a pairs call: a block per judged mate (each its own count of long rows) and the pair counts
struct PairCallBlock { FilterBlock mate[2]; PairBlock pairs; };

extern "C" int ffq_table_select_pairs(ffq_ctx *c, const ffq_table_view *m1, const ffq_table_view *m2, int64_t n_pairs,
                                      const int64_t len_bounds[4], const ffq_content_rules *rules1, const ffq_content_rules *rules2,
                                      int pair_filter, int64_t *d_out1, int64_t *d_out2, int64_t *d_idx, int64_t *n_out,
                                      int64_t hist1[FFQ_FILTER_COUNTS], int64_t hist2[FFQ_FILTER_COUNTS], int64_t pairs[5])
{
    static const char *const who = "ffq_table_select_pairs";
    mark_other(c);
    bool on[2] = {false, false};
    FilterRules R[2] = {};
    int rc = content_arg(who, rules1, &on[0], &R[0]);
    if (!rc) rc = content_arg(who, rules2, &on[1], &R[1]);
    if (rc) return rc;
    if (pair_filter != FFQ_PAIR_ANY && pair_filter != FFQ_PAIR_BOTH && pair_filter != FFQ_PAIR_FIRST)
        return fail(FFQ_E_ARG, "%s: pair_filter is FFQ_PAIR_ANY, FFQ_PAIR_BOTH or FFQ_PAIR_FIRST", who);
    // (which mates' buffers are read depends on the rules: looked for below)
    rc = pairs_begin(c, who, len_bounds && n_out && hist1 && hist2 && pairs && (n_pairs <= 0 || (d_out1 && d_out2)), m1, m2, n_pairs, nullptr, [&] {
        return aligned({d_out1, d_out2}, 16) ? FFQ_OK : fail(FFQ_E_ARG, "%s: tables must be 16-byte aligned", who);
    });
    if (rc) return rc;
    const ffq_table_view *m[2] = {m1, m2};
    int64_t *hist[2] = {hist1, hist2};
    const int n_judged = pair_filter == FFQ_PAIR_FIRST ? 1 : 2;
    for (int k = 0; k < n_judged; k++)
        if (on[k] && m[k]->n_bytes > 0 && !m[k]->d_buf) return fail(FFQ_E_ARG, "%s: no buffer to judge the rows of mate %d by", who, k + 1);
    if (n_pairs > 0 && (d_out1 == m1->d_table || d_out2 == m2->d_table || d_out1 == d_out2 || d_out1 == m2->d_table || d_out2 == m1->d_table))
        return fail(FFQ_E_ARG, "%s: d_out1 and d_out2 must not be one of the tables, or each other", who);
    for (int i = 0; i < FFQ_FILTER_COUNTS; i++) hist1[i] = hist2[i] = 0;
    for (int i = 0; i < PAIR_COUNTS; i++) pairs[i] = 0;
    *n_out = 0;
    if (n_pairs == 0) return FFQ_OK;
    const int64_t nblk = (n_pairs + 255) / 256;
    // (everything is grown before anything is enqueued: growing waits for the stream)
    rc = grow_dev(c, c->rows_list, n_pairs);
    if (!rc) rc = grow_dev(c, c->filter_verdict, n_pairs);
    if (!rc && n_judged == 2) rc = grow_dev(c, c->filter_verdict2, n_pairs);
    if (!rc) rc = compact_reserve(c, n_pairs);
    if (rc) return rc;
    hipStream_t st = c->stream;
    uint8_t *verdict[2] = {c->filter_verdict.p, n_judged == 2 ? c->filter_verdict2.p : nullptr};
    PairCallBlock *blk = nullptr;
    if ((rc = call_blk_begin(c, &blk))) return rc;
    // the judging, once per mate: the list of long rows is the call's, every mate has counters of its own
    for (int k = 0; k < n_judged; k++) {
        const ffq_table_view *v = m[k];
        const int s = v->sentinel ? 1 : 0;
        const int64_t lo = len_bounds[2 * k], hi = len_bounds[2 * k + 1];
        if (on[k]) {
            hipLaunchKernelGGL(k_filter_rows, dim3(rows_grid(n_pairs, FILTER_WG / FILTER_G, FILTER_GRID_SHORT)), dim3(FILTER_WG), 0, st,
                               v->d_buf, v->n_bytes, s, v->add, v->d_table, n_pairs, lo, hi, R[k], verdict[k], c->rows_list.p, &blk->mate[k]);
            hipLaunchKernelGGL(k_filter_long, dim3(rows_grid(n_pairs, FILTER_WG / 64, FILTER_GRID_LONG)), dim3(FILTER_WG), 0, st,
                               v->d_buf, v->n_bytes, s, v->add, v->d_table, R[k], verdict[k], (const int64_t *)c->rows_list, &blk->mate[k]);
        } else {
            hipLaunchKernelGGL(k_pair_len, dim3(rows_grid(n_pairs, 256, FILTER_GRID_SHORT)), dim3(256), 0, st, v->d_table, n_pairs, lo, hi,
                               verdict[k], &blk->mate[k]);
        }
    }
    const KeepPair keep = {verdict[0], verdict[1], pair_filter};
    hipLaunchKernelGGL(k_pair_count, dim3((unsigned)std::min<int64_t>(nblk, PAIR_GRID_COUNT)), dim3(256), 0, st, keep, n_pairs, nblk,
                       c->sel_cnt.p, &blk->pairs);
    if ((rc = compact_scatter(c, st, keep, n_pairs, m1->d_table, m2->d_table, nullptr, d_out1, d_out2, d_idx))) return rc;
    const PairCallBlock *h = nullptr;
    if ((rc = call_blk_end(c, &h))) return rc;
    for (int k = 0; k < n_judged; k++)
        for (int i = 0; i < FFQ_FILTER_COUNTS; i++) hist[k][i] = (int64_t)h->mate[k].cnt[i];
    for (int i = 0; i < PAIR_COUNTS; i++) pairs[i] = (int64_t)h->pairs.cnt[i];
    *n_out = pairs[0];
    return FFQ_OK;
}

extern "C" int ffq_table_pair_names(ffq_ctx *c, const ffq_table_view *m1, const ffq_table_view *m2, int64_t n_pairs, int64_t out[4])
{
    static const char *const who = "ffq_table_pair_names";
    mark_other(c);
    if (int rc = pairs_begin(c, who, out != nullptr, m1, m2, n_pairs, "read the headers from", [] { return FFQ_OK; })) return rc;
    out[0] = out[1] = out[2] = 0; out[3] = -1;
    if (n_pairs == 0) return FFQ_OK;
    hipStream_t st = c->stream;
    // (the block begins as the host says, not cleared: `first` is a minimum)
    *call_blk_as<PairNamesBlock>(c->blk.h.p) = PairNamesBlock{0, 0, 0, (unsigned long long)n_pairs};
    HIPCHK(hipMemcpyAsync(c->blk.d, c->blk.h, sizeof(PairNamesBlock), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pair_names, dim3(rows_grid(n_pairs, PAIR_NAMES_WG / ROWS_G, EDIT_GRID_SHORT)), dim3(PAIR_NAMES_WG), 0, st,
                       pair_side(m1), pair_side(m2), n_pairs, call_blk_as<PairNamesBlock>(c->blk.d.p));
    const PairNamesBlock *h = nullptr;
    if (int rc = call_blk_end(c, &h)) return rc;
    out[0] = (int64_t)h->equal; out[1] = (int64_t)h->different; out[2] = (int64_t)h->not_compared;
    out[3] = h->different ? (int64_t)h->first : -1;
    return FFQ_OK;
}

// ---- the overlap of the mates of a pair (csrc/ffq_overlap.h) -------------------------------------
static_assert(OVL_MAX_LEN == FFQ_OVERLAP_MAX_LEN && OVERLAP_HIST == FFQ_OVERLAP_HIST_WORDS && OVERLAP_COUNTS == FFQ_OVERLAP_COUNTS,
              "include/ffq.h");

// the rules of an overlap call, checked: for the table call and for ffq_pair_set_overlap
static int overlap_arg(const char *who, const ffq_overlap_rules *r)
{
    if (!r) return fail(FFQ_E_ARG, "%s: no rules", who);
    if (r->min_overlap < 1 || r->min_overlap > FFQ_OVERLAP_MAX_LEN) return fail(FFQ_E_ARG, "%s: min_overlap is 1..%d", who, FFQ_OVERLAP_MAX_LEN);
    if (r->max_diff < 0 || r->max_diff > FFQ_OVERLAP_MAX_LEN) return fail(FFQ_E_ARG, "%s: max_diff is 0..%d", who, FFQ_OVERLAP_MAX_LEN);
    if (r->diff_permille < 0 || r->diff_permille > 1000) return fail(FFQ_E_ARG, "%s: diff_permille is 0..1000", who);
    if (r->trim != 0 && r->trim != 1) return fail(FFQ_E_ARG, "%s: trim is 0 or 1", who);
    return FFQ_OK;
}

extern "C" int ffq_table_pair_overlap(ffq_ctx *c, const ffq_table_view *m1, const ffq_table_view *m2, int64_t n_pairs,
                                      const ffq_overlap_rules *rules, int64_t *d_out1, int64_t *d_out2, int32_t *d_insert,
                                      uint64_t *d_hist, int accumulate, int64_t counts[FFQ_OVERLAP_COUNTS])
{
    static const char *const who = "ffq_table_pair_overlap";
    mark_other(c);
    int rc = overlap_arg(who, rules);
    if (rc) return rc;
    rc = pairs_begin(c, who, counts && (n_pairs <= 0 || (d_out1 && d_out2)), m1, m2, n_pairs, "read the sequences from", [&]() -> int {
        if (!aligned({d_out1, d_out2}, 16)) return fail(FFQ_E_ARG, "%s: tables must be 16-byte aligned", who);
        if (!aligned({d_hist}, 8) || !aligned({d_insert}, 4)) return fail(FFQ_E_ARG, "%s: d_hist must be 8-byte aligned, d_insert 4-byte aligned", who);
        return FFQ_OK;
    });
    if (rc) return rc;
    for (int i = 0; i < OVERLAP_COUNTS; i++) counts[i] = 0;
    hipStream_t st = c->stream;
    if (d_hist && !accumulate) HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)OVERLAP_HIST * 8, st));
    if (n_pairs == 0) {
        HIPCHK(hipStreamSynchronize(st));
        return FFQ_OK;
    }
    OverlapBlock *blk = nullptr;
    if ((rc = call_blk_begin(c, &blk))) return rc;
    const OverlapRules R = {rules->min_overlap, rules->max_diff, rules->diff_permille, rules->trim};
    hipLaunchKernelGGL(k_pair_overlap, dim3(rows_grid(n_pairs, OVERLAP_WG / ROWS_G, EDIT_GRID_SHORT)), dim3(OVERLAP_WG), 0, st, pair_side(m1),
                       pair_side(m2), n_pairs, R, d_out1, d_out2, d_insert, reinterpret_cast<unsigned long long *>(d_hist), blk);
    const OverlapBlock *h = nullptr;
    if ((rc = call_blk_end(c, &h))) return rc;
    for (int i = 0; i < OVERLAP_COUNTS; i++) counts[i] = (int64_t)h->cnt[i];
    return FFQ_OK;
}

// ---- FASTQ text from (buffer, table) (csrc/ffq_render.h) ---------------------------------------
extern "C" int ffq_table_render_fastq(ffq_ctx *c, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                                      const int64_t *d_table, int64_t n_rows, uint8_t *d_out, int64_t out_cap,
                                      int64_t *d_off, int64_t stats[3])
{
    mark_other(c);
    if (!c || !stats || n_rows < 0 || n_bytes < 0 || out_cap < 0 || (n_bytes > 0 && !d_buf) || (n_rows > 0 && !d_table) ||
        (out_cap > 0 && !d_out))
        return fail(FFQ_E_ARG, "ffq_table_render_fastq: bad argument");
    if (!aligned({d_table}, 16) || !aligned({d_off}, 8))
        return fail(FFQ_E_ARG, "ffq_table_render_fastq: the table must be 16-byte aligned, the offsets 8-byte");
    if (int rc = no_pending(c, "ffq_table_render_fastq")) return rc;
    HIPCHK(hipSetDevice(c->device));
    stats[0] = stats[1] = stats[2] = 0;
    hipStream_t st = c->stream;
    if (n_rows == 0) return no_rows_offsets(c, d_off);
    const int64_t nblk = (n_rows + RENDER_WG - 1) / RENDER_WG;
    int rc = grow_dev(c, c->col_sum, nblk);
    if (!rc) rc = grow_dev(c, c->render_list, 2 * n_rows);
    if (rc) return rc;
    const int s = sentinel ? 1 : 0;
    RenderBlock *blk = nullptr;
    if ((rc = call_blk_begin(c, &blk))) return rc;
    hipLaunchKernelGGL(k_render_sum, dim3((unsigned)std::min<int64_t>(nblk, 2048)), dim3(RENDER_WG), 0, st, n_bytes, s, add,
                       d_table, n_rows, nblk, c->col_sum, blk);
    if ((rc = launch_scan(c, st, (const long long *)c->col_sum, nblk, c->col_sum, ScanToRes{c->col_res, n_rows}))) return rc;
    hipLaunchKernelGGL(k_render_rows, dim3((unsigned)nblk), dim3(RENDER_WG), 0, st, d_buf, n_bytes, s, add, d_table, n_rows,
                       (const long long *)c->col_sum, (const DevRes *)c->col_res, d_out, out_cap, d_off, c->render_list,
                       blk);
    // the rows it left (above RENDER_LONG output bytes; their number is known on the device only): a wave each
    const int64_t nblk_long = std::min<int64_t>((n_rows + 3) / 4, 1024);
    hipLaunchKernelGGL(k_render_long, dim3((unsigned)nblk_long), dim3(RENDER_WG), 0, st, d_buf, n_bytes, s, add, d_table, n_rows,
                       d_out, (const int64_t *)c->render_list, (const RenderBlock *)blk);
    const RenderBlock *h = nullptr;
    if ((rc = call_blk_end(c, &h))) return rc;
    stats[0] = (int64_t)h->total; stats[1] = (int64_t)h->rendered;
    stats[2] = n_rows - stats[1];
    if (stats[0] > out_cap)
        return fail(FFQ_E_TABLE_FULL, "output holds %lld bytes, the rendered rows have %lld", (long long)out_cap,
                    (long long)stats[0]);
    return FFQ_OK;
}

// ---- UMIs: off the reads, into the names (csrc/ffq_umi.h, built as csrc/ffq_umi.hip and launched through ffq_umi_launch.h) ----
typedef ffq_umi::Arg UmiArg;
typedef ffq_umi::RenderCounts UmiRenderBlock;
static_assert(ffq_umi::RENDER_WG == RENDER_WG, "ffq_umi_launch.h");
static_assert(UMI_READ1 == FFQ_UMI_READ1 && UMI_READ2 == FFQ_UMI_READ2 && UMI_PER_READ == FFQ_UMI_PER_READ &&
              UMI_PREFIX_MAX == sizeof(((ffq_umi_rules *)nullptr)->prefix), "include/ffq.h");

static int umi_take_arg(const char *who, int len, int skip)
{
    if (len < 1 || len > UMI_LEN_MAX) return fail(FFQ_E_ARG, "%s: umi_len is 1..%d", who, UMI_LEN_MAX);
    if (skip < 0 || skip > UMI_SKIP_MAX) return fail(FFQ_E_ARG, "%s: umi_skip is 0..%d", who, UMI_SKIP_MAX);
    return FFQ_OK;
}

// the rules of a UMI call, checked, as the kernels take them (A may be NULL): for the table call and for the setters
static int umi_arg(const char *who, const ffq_umi_rules *r, UmiArg *A)
{
    if (!r) return fail(FFQ_E_ARG, "%s: NULL rules", who);
    if (r->loc != FFQ_UMI_READ1 && r->loc != FFQ_UMI_READ2 && r->loc != FFQ_UMI_PER_READ)
        return fail(FFQ_E_ARG, "%s: loc is FFQ_UMI_READ1, FFQ_UMI_READ2 or FFQ_UMI_PER_READ", who);
    if (int rc = umi_take_arg(who, r->len, r->skip)) return rc;
    if (r->delim < 0x21 || r->delim > 0x7E) return fail(FFQ_E_ARG, "%s: delim is a printable byte, 0x21..0x7E", who);
    if (r->prefix_len > UMI_PREFIX_MAX) return fail(FFQ_E_ARG, "%s: prefix_len is 0..%d", who, UMI_PREFIX_MAX);
    for (int j = 0; j < r->prefix_len; j++)
        if (const uint8_t b = r->prefix[j]; !((b >= '0' && b <= '9') || (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z'))) return fail(FFQ_E_ARG, "%s: the prefix is bytes of [A-Za-z0-9]", who);
    if (A) {
        memset(A, 0, sizeof *A);
        A->loc = r->loc; A->len = r->len; A->prefix_len = r->prefix_len;
        uint8_t lit[sizeof A->lit] = {0};
        static_assert(sizeof lit >= UMI_LIT_MAX, "UmiArg::lit");
        umi_literal(lit, r->delim, r->prefix, r->prefix_len);
        for (size_t j = 0; j < sizeof lit; j++) A->lit[j >> 2] |= (uint32_t)lit[j] << (8 * (j & 3));
    }
    return FFQ_OK;
}

extern "C" int ffq_table_take_umi(ffq_ctx *c, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                                  const int64_t *d_table, int64_t n_rows, int umi_len, int umi_skip, int64_t *d_out, int64_t stats[3])
{
    static const char *const who = "ffq_table_take_umi";
    return rows_edit(c, who, umi_take_arg(who, umi_len, umi_skip), d_buf, n_bytes, sentinel, d_table, n_rows, d_out, stats,
                     [&](hipStream_t st, int s, RowsBlock *blk) {
        ffq_umi::launch_take(st, rows_grid(n_rows, ffq_umi::TAKE_WG / ROWS_G, EDIT_GRID_SHORT), rows_grid(n_rows, ffq_umi::TAKE_WG / 64, EDIT_GRID_LONG),
                             d_buf, n_bytes, s, add, d_table, n_rows, umi_len, umi_skip, d_out, c->rows_list, blk);
    });
}

// Workgroups of the tagged render's capped launches (the rows' launch has a workgroup per block of 256 rows, uncapped)
constexpr int UMI_GRID_SUM = 2048, UMI_GRID_LONG = 1024;

extern "C" int ffq_table_render_fastq_umi(ffq_ctx *c, const ffq_table_view *rows, int64_t n_rows, const ffq_table_view *src1,
                                          const ffq_table_view *src2, const ffq_umi_rules *rules, uint8_t *d_out, int64_t out_cap,
                                          int64_t *d_off, int64_t stats[4])
{
    static const char *const who = "ffq_table_render_fastq_umi";
    mark_other(c);
    if (!c || !stats || n_rows < 0 || out_cap < 0 || !view_ok(rows, n_rows) || (out_cap > 0 && !d_out))
        return fail(FFQ_E_ARG, "%s: bad argument", who);
    UmiArg A;
    if (int rc = umi_arg(who, rules, &A)) return rc;
    const bool need1 = A.loc != UMI_READ2, need2 = A.loc != UMI_READ1;
    if ((need1 && !view_ok(src1, n_rows)) || (need2 && !view_ok(src2, n_rows)))
        return fail(FFQ_E_ARG, "%s: the location needs a source table that is not there", who);
    if (!need1) src1 = rows;                                // (a side the location does not name is never looked at)
    if (!need2) src2 = rows;
    for (const ffq_table_view *m : {rows, src1, src2})
        if (m->n_bytes > 0 && !m->d_buf) return fail(FFQ_E_ARG, "%s: no buffer to read the rows from", who);
    if (!aligned({d_off}, 8)) return fail(FFQ_E_ARG, "%s: the tables must be 16-byte aligned, the offsets 8-byte", who);
    if (int rc = no_pending(c, who)) return rc;
    HIPCHK(hipSetDevice(c->device));
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    hipStream_t st = c->stream;
    if (n_rows == 0) return no_rows_offsets(c, d_off);
    const int64_t nblk = (n_rows + RENDER_WG - 1) / RENDER_WG;
    int rc = grow_dev(c, c->col_sum, nblk);
    if (!rc) rc = grow_dev(c, c->render_list, 2 * n_rows);
    if (rc) return rc;
    UmiRenderBlock *blk = nullptr;
    if ((rc = call_blk_begin(c, &blk))) return rc;
    const auto side = [](const ffq_table_view *m) { return ffq_umi::Side{m->d_buf, m->n_bytes, m->sentinel ? 1 : 0, m->add, m->d_table}; };
    const ffq_umi::Side S0 = side(rows), S1 = side(src1), S2 = side(src2);
    ffq_umi::launch_render_sum(st, (unsigned)std::min<int64_t>(nblk, UMI_GRID_SUM), S0, S1, S2, A, n_rows, nblk, c->col_sum, blk);
    if ((rc = launch_scan(c, st, (const long long *)c->col_sum, nblk, c->col_sum, ScanToRes{c->col_res, n_rows}))) return rc;
    ffq_umi::launch_render_rows(st, (unsigned)nblk, (unsigned)std::min<int64_t>((n_rows + 3) / 4, UMI_GRID_LONG), S0, S1, S2, A, n_rows,
                                (const long long *)c->col_sum, (const DevRes *)c->col_res, d_out, out_cap, d_off, c->render_list, blk);
    const UmiRenderBlock *h = nullptr;
    if ((rc = call_blk_end(c, &h))) return rc;
    stats[0] = (int64_t)h->total; stats[1] = (int64_t)h->rendered;
    stats[2] = n_rows - stats[1];
    stats[3] = (int64_t)h->tagged;
    if (stats[0] > out_cap)
        return fail(FFQ_E_TABLE_FULL, "output holds %lld bytes, the rendered rows have %lld", (long long)out_cap, (long long)stats[0]);
    return FFQ_OK;
}

// ---- BGZF members from device bytes (csrc/ffq_deflate.h) --------------------------------------
static_assert(DFL_BLOCK == FFQ_BGZF_BLOCK_BYTES && DFL_SEG == FFQ_DEFLATE_SEG_BYTES && DFL_ROUND == FFQ_DEFLATE_ROUND_POSITIONS &&
              DEFLATE_GRID == FFQ_DEFLATE_GRID_BLOCKS && DEFLATE_COUNTS == FFQ_DEFLATE_COUNTS, "include/ffq.h");

static int64_t deflate_blocks(int64_t n_bytes) { return (n_bytes + DFL_BLOCK - 1) / DFL_BLOCK; }

extern "C" int64_t ffq_deflate_bgzf_bound(int64_t n_bytes) { return n_bytes <= 0 ? 0 : n_bytes + DFL_OVERHEAD * deflate_blocks(n_bytes); }

extern "C" void ffq_bgzf_eof_block(uint8_t out[28]) { if (out) dfl_eof_member(out); }

// everything a deflate of n_bytes needs, grown (before anything is enqueued: growing waits for the stream)
static int deflate_reserve(ffq_ctx *c, int64_t n_bytes)
{
    const int64_t n_blocks = deflate_blocks(n_bytes);
    int rc = grow_dev(c, c->deflate_slots, std::min<int64_t>(n_blocks, DEFLATE_GRID) * DFL_BLOCK);
    if (!rc) rc = grow_dev(c, c->deflate_members, n_blocks * DFL_SLOT);
    if (!rc) rc = grow_dev(c, c->col_sum, n_blocks);
    return rc;
}

// the three launches, behind whatever the stream holds; the counters in *blk (cleared by the caller), the total there too
static int deflate_enqueue(ffq_ctx *c, hipStream_t st, const uint8_t *d_src, int64_t n_bytes, uint8_t *d_out, int64_t out_cap,
                           int64_t *d_member_off, DeflateBlock *blk)
{
    const int64_t n_blocks = deflate_blocks(n_bytes);
    hipLaunchKernelGGL(k_deflate_members, dim3((unsigned)std::min<int64_t>(n_blocks, DEFLATE_GRID)), dim3(DFL_LANES), 0, st, d_src, n_bytes,
                       n_blocks, c->deflate_slots.p, c->deflate_members.p, c->col_sum.p, blk);
    if (int rc = launch_scan(c, st, (const long long *)c->col_sum, n_blocks, c->col_sum, ScanToRes{c->col_res, n_blocks})) return rc;
    hipLaunchKernelGGL(k_deflate_pack, dim3((unsigned)std::min<int64_t>(n_blocks, 4096)), dim3(256), 0, st, (const uint8_t *)c->deflate_members.p,
                       (const long long *)c->col_sum.p, n_blocks, (const DevRes *)c->col_res.p, d_out, out_cap, d_member_off, blk);
    return FFQ_OK;
}

extern "C" int ffq_deflate_bgzf(ffq_ctx *c, const uint8_t *d_src, int64_t n_bytes, uint8_t *d_out, int64_t out_cap, int64_t *d_member_off,
                                int64_t stats[FFQ_DEFLATE_COUNTS])
{
    static const char *const who = "ffq_deflate_bgzf";
    mark_other(c);
    if (!c || !stats || n_bytes < 0 || out_cap < 0 || (n_bytes > 0 && !d_src) || (out_cap > 0 && !d_out))
        return fail(FFQ_E_ARG, "%s: bad argument", who);
    if (!aligned({d_member_off}, 8)) return fail(FFQ_E_ARG, "%s: d_member_off must be 8-byte aligned", who);
    int rc = no_pending(c, who);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    for (int i = 0; i < FFQ_DEFLATE_COUNTS; i++) stats[i] = 0;
    if (n_bytes == 0) return no_rows_offsets(c, d_member_off);
    if ((rc = deflate_reserve(c, n_bytes))) return rc;
    hipStream_t st = c->stream;
    DeflateBlock *blk = nullptr;
    if ((rc = call_blk_begin(c, &blk))) return rc;
    if ((rc = deflate_enqueue(c, st, d_src, n_bytes, d_out, out_cap, d_member_off, blk))) return rc;
    const DeflateBlock *h = nullptr;
    if ((rc = call_blk_end(c, &h))) return rc;
    stats[0] = n_bytes; stats[1] = (int64_t)h->total; stats[2] = deflate_blocks(n_bytes); stats[3] = (int64_t)h->stored;
    if (stats[1] > out_cap)
        return fail(FFQ_E_TABLE_FULL, "output holds %lld bytes, the members have %lld", (long long)out_cap, (long long)stats[1]);
    return FFQ_OK;
}

// ---- the mates of a pair merged into one read (csrc/ffq_merge.h) ------------------------------
static_assert(MRG_MAX_LEN == FFQ_OVERLAP_MAX_LEN && MERGE_COUNTS == FFQ_MERGE_COUNTS, "include/ffq.h");

extern "C" int ffq_table_pair_merge(ffq_ctx *c, const ffq_table_view *m1, const ffq_table_view *m2, int64_t n_pairs,
                                    const int32_t *d_insert, const int64_t *d_ord, uint8_t *d_text, int64_t text_cap, int64_t *d_off,
                                    int64_t *d_rest1, int64_t *d_rest2, int64_t *d_rest_ord, int64_t *n_rest,
                                    int64_t counts[FFQ_MERGE_COUNTS])
{
    static const char *const who = "ffq_table_pair_merge";
    mark_other(c);
    // (the rest tables are told from the mates' behind the look for the buffers: that look is in own())
    int rc = pairs_begin(c, who, counts && n_rest && text_cap >= 0 && (text_cap == 0 || d_text) && (n_pairs <= 0 || (d_rest1 && d_rest2)), m1, m2,
                         n_pairs, nullptr, [&]() -> int {
        if (n_pairs > 0 && !d_insert) return fail(FFQ_E_ARG, "%s: no insert sizes (d_insert)", who);
        if (!aligned({d_rest1, d_rest2}, 16)) return fail(FFQ_E_ARG, "%s: tables must be 16-byte aligned", who);
        if (!aligned({d_off, d_ord, d_rest_ord}, 8) || !aligned({d_insert}, 4))
            return fail(FFQ_E_ARG, "%s: d_off, d_ord and d_rest_ord must be 8-byte aligned, d_insert 4-byte aligned", who);
        if (int e = pair_bufs(who, m1, m2, "read the mates from")) return e;
        if (n_pairs > 0 && (d_rest1 == m1->d_table || d_rest1 == m2->d_table || d_rest2 == m1->d_table || d_rest2 == m2->d_table || d_rest1 == d_rest2))
            return fail(FFQ_E_ARG, "%s: d_rest1 and d_rest2 must not be one of the tables, or each other", who);
        return FFQ_OK;
    });
    if (rc) return rc;
    for (int i = 0; i < MERGE_COUNTS; i++) counts[i] = 0;
    *n_rest = 0;
    hipStream_t st = c->stream;
    if (n_pairs == 0) return no_rows_offsets(c, d_off);
    const int64_t nblk = (n_pairs + MERGE_WG - 1) / MERGE_WG;
    // (everything is grown before anything is enqueued: growing waits for the stream)
    rc = grow_dev(c, c->col_sum, nblk);
    if (!rc) rc = grow_dev(c, c->sel_cnt, nblk);
    if (!rc) rc = grow_dev(c, c->sel_base, nblk);
    if (rc) return rc;
    const PairSide A = pair_side(m1), B = pair_side(m2);
    MergeBlock *blk = nullptr;
    if ((rc = call_blk_begin(c, &blk))) return rc;
    hipLaunchKernelGGL(k_merge_sum, dim3((unsigned)std::min<int64_t>(nblk, 2048)), dim3(MERGE_WG), 0, st, A, B, n_pairs, nblk, d_insert, d_ord,
                       c->col_sum.p, c->sel_cnt.p, blk);
    if ((rc = launch_scan(c, st, (const long long *)c->col_sum, nblk, c->col_sum, ScanToRes{c->col_res, n_pairs}))) return rc;
    if ((rc = launch_scan(c, st, (const unsigned int *)c->sel_cnt, nblk, c->sel_base, ScanToWord{(long long *)c->d_word.p}))) return rc;
    hipLaunchKernelGGL(k_merge_rows, dim3((unsigned)nblk), dim3(MERGE_WG), 0, st, A, B, n_pairs, d_insert, d_ord, (const long long *)c->col_sum,
                       (const DevRes *)c->col_res, (const long long *)c->sel_base, d_text, text_cap, d_off, d_rest1, d_rest2, d_rest_ord,
                       blk);
    const MergeBlock *h = nullptr;
    if ((rc = call_blk_end(c, &h))) return rc;
    for (int i = 0; i < MERGE_COUNTS; i++) counts[i] = (int64_t)h->cnt[i];
    counts[1] = n_pairs - counts[0];
    *n_rest = counts[1];
    if (counts[2] > text_cap)
        return fail(FFQ_E_TABLE_FULL, "text holds %lld bytes, the merged reads have %lld", (long long)text_cap, (long long)counts[2]);
    return FFQ_OK;
}

// ---- bases corrected inside the mates' overlap (csrc/ffq_correct.h) ---------------------------
static_assert(CORRECT_COUNTS == FFQ_CORRECT_COUNTS && CORRECT_MATRIX == FFQ_CORRECT_MATRIX_WORDS, "include/ffq.h");

// the rules of a correction call, checked: for the table call and for ffq_pair_set_correct
static int correct_arg(const char *who, const ffq_correct_rules *r)
{
    if (!r) return fail(FFQ_E_ARG, "%s: no rules", who);
    if (r->bad_quality < 0 || r->bad_quality >= r->good_quality) return fail(FFQ_E_ARG, "%s: 0 <= bad_quality < good_quality", who);
    if (r->qual_base < 0 || r->qual_base > 255 || r->good_quality > 255 - r->qual_base)
        return fail(FFQ_E_ARG, "%s: qual_base is 0..255 and qual_base + good_quality at most 255", who);
    return FFQ_OK;
}

// THE ONE PLACE where a view's bytes become writable.  A ffq_table_view says `const uint8_t *d_buf` because every other table
// pass only reads the bytes and edits rows; the correction is the one pass that edits the bytes themselves, and its caller
// hands it device memory of its own (the stream: its fill's slot) knowing that.
static uint8_t *correct_writable(const ffq_table_view *m) { return const_cast<uint8_t *>(m->d_buf); }

extern "C" int ffq_table_pair_correct(ffq_ctx *c, const ffq_table_view *m1, const ffq_table_view *m2, int64_t n_pairs,
                                      const int32_t *d_insert, const ffq_correct_rules *rules, int64_t counts[FFQ_CORRECT_COUNTS],
                                      int64_t matrix[FFQ_CORRECT_MATRIX_WORDS])
{
    static const char *const who = "ffq_table_pair_correct";
    mark_other(c);
    int rc = correct_arg(who, rules);
    if (rc) return rc;
    rc = pairs_begin(c, who, counts != nullptr, m1, m2, n_pairs, "correct the mates in", [&]() -> int {
        if (n_pairs > 0 && !d_insert) return fail(FFQ_E_ARG, "%s: no insert sizes (d_insert)", who);
        if (!aligned({d_insert}, 4)) return fail(FFQ_E_ARG, "%s: d_insert must be 4-byte aligned", who);
        return FFQ_OK;
    });
    if (rc) return rc;
    for (int i = 0; i < CORRECT_COUNTS; i++) counts[i] = 0;
    if (matrix) for (int i = 0; i < CORRECT_MATRIX; i++) matrix[i] = 0;
    if (n_pairs == 0) return FFQ_OK;
    hipStream_t st = c->stream;
    CorrectBlock *blk = nullptr;
    if ((rc = call_blk_begin(c, &blk))) return rc;
    const CorrectRules R = {(uint32_t)(rules->qual_base + rules->good_quality), (uint32_t)(rules->qual_base + rules->bad_quality)};
    hipLaunchKernelGGL(k_pair_correct, dim3(rows_grid(n_pairs, CORRECT_WG / ROWS_G, EDIT_GRID_SHORT)), dim3(CORRECT_WG), 0, st, pair_side(m1),
                       pair_side(m2), correct_writable(m1), correct_writable(m2), n_pairs, d_insert, R, matrix ? 1 : 0, blk);
    const CorrectBlock *h = nullptr;
    if ((rc = call_blk_end(c, &h))) return rc;
    for (int i = 0; i < CORRECT_COUNTS; i++) counts[i] = (int64_t)h->cnt[i];
    if (matrix) for (int i = 0; i < CORRECT_MATRIX; i++) matrix[i] = (int64_t)h->matrix[i];
    return FFQ_OK;
}

// ---- duplicate reads and pairs (csrc/ffq_dedup.h) -----------------------------------------------
static_assert(DEDUP_KEY_NONE == FFQ_KEY_NONE && DEDUP_COUNTS == FFQ_DEDUP_COUNTS, "include/ffq.h");

constexpr int SEQKEY_GRID_SHORT = 2048, SEQKEY_GRID_LONG = 1024, DEDUP_GRID_TABLE = 4096, DEDUP_GRID_ROWS = 2048;

extern "C" uint64_t ffq_seq_key_host(const uint8_t *seq, int64_t n) { return (seq || n <= 0) ? dedup_seq_key(seq, n < 0 ? 0 : n) : FFQ_KEY_NONE; }
extern "C" uint64_t ffq_pair_key_host(uint64_t k1, uint64_t k2) { return dedup_pair_key(k1, k2); }

extern "C" int ffq_table_seq_keys(ffq_ctx *c, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                                  const int64_t *d_table, int64_t n_rows, uint64_t *d_keys, int64_t counts[2])
{
    static const char *const who = "ffq_table_seq_keys";
    mark_other(c);
    if (!c || !counts || n_rows < 0 || n_bytes < 0 || (n_bytes > 0 && !d_buf) || (n_rows > 0 && (!d_table || !d_keys)))
        return fail(FFQ_E_ARG, "%s: bad argument", who);
    if (!aligned({d_table}, 16) || !aligned({d_keys}, 8))
        return fail(FFQ_E_ARG, "%s: the table must be 16-byte aligned, the keys 8-byte aligned", who);
    int rc = no_pending(c, who);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    counts[0] = counts[1] = 0;
    if (n_rows == 0) return FFQ_OK;
    if ((rc = grow_dev(c, c->rows_list, n_rows))) return rc;      // (before anything is enqueued: growing waits for the stream)
    hipStream_t st = c->stream;
    const int s = sentinel ? 1 : 0;
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(d_keys);
    RowsBlock *blk = nullptr;
    if ((rc = call_blk_begin(c, &blk))) return rc;
    hipLaunchKernelGGL(k_seqkey_rows, dim3(rows_grid(n_rows, SEQKEY_WG / SEQKEY_G, SEQKEY_GRID_SHORT)), dim3(SEQKEY_WG), 0, st, d_buf,
                       n_bytes, s, add, d_table, n_rows, keys, c->rows_list.p, blk);
    hipLaunchKernelGGL(k_seqkey_long, dim3(rows_grid(n_rows, SEQKEY_WG / 64, SEQKEY_GRID_LONG)), dim3(SEQKEY_WG), 0, st, d_buf,
                       n_bytes, s, add, d_table, keys, (const int64_t *)c->rows_list, blk);
    int64_t stats[3];
    if ((rc = rows_end(c, stats))) return rc;
    counts[0] = stats[0]; counts[1] = stats[2];
    return FFQ_OK;
}

// The set: the table in use (tab[cur]) and the one it grew out of, which the next growth reuses -- the old and the new table
// are alive together while one is rehashed into the other.  The host knows, without asking the device, how many keys the
// table holds (`distinct`, from the last call's one wait) and how many rows were ever submitted (the next global ordinal).
struct ffq_dedup {
    ffq_ctx *c = nullptr;
    DevBuf<DedupSlot> tab[2];
    int cur = 0;
    int64_t slots = 0, distinct = 0, submitted = 0, rehashes = 0, max_bytes = 0;
    DevBuf<DedupBlock> d_blk;
    PinBuf<DedupBlock> h_blk;
};

static unsigned dedup_table_grid(int64_t slots) { return (unsigned)std::min<int64_t>((slots + 255) / 256, DEDUP_GRID_TABLE); }

extern "C" void ffq_dedup_destroy(ffq_dedup *d)
{
    if (!d) return;
    if (d->c && d->c->stream && hipSetDevice(d->c->device) == hipSuccess) (void)hipStreamSynchronize(d->c->stream);
    delete d;                    // (the buffers free themselves)
}

extern "C" int ffq_dedup_create(ffq_ctx *c, int64_t expected_keys, int64_t max_bytes, ffq_dedup **out)
{
    static const char *const who = "ffq_dedup_create";
    mark_other(c);
    if (!c || !out || expected_keys < 0 || max_bytes < 0 || expected_keys > ((int64_t)1 << 56))
        return fail(FFQ_E_ARG, "%s: bad argument", who);
    *out = nullptr;
    HIPCHK(hipSetDevice(c->device));
    const int64_t slots = dedup_slots_for(0, expected_keys, 0);
    if (max_bytes > 0 && slots * (int64_t)sizeof(DedupSlot) > max_bytes)
        return fail(FFQ_E_NOMEM, "%s: a set for %lld keys needs %lld bytes (%lld slots), max_bytes is %lld", who, (long long)expected_keys,
                    (long long)(slots * (int64_t)sizeof(DedupSlot)), (long long)slots, (long long)max_bytes);
    ffq_dedup *d = new (std::nothrow) ffq_dedup();
    if (!d) return fail(FFQ_E_NOMEM, "out of host memory");
    d->c = c; d->max_bytes = max_bytes;
    hipError_t e = d->tab[0].grow(slots);
    if (e == hipSuccess) e = d->d_blk.grow(1);
    if (e == hipSuccess) e = d->h_blk.grow(1);
    if (e != hipSuccess) {
        delete d;
        return fail(FFQ_E_NOMEM, "%s: no memory for %lld slots: %s", who, (long long)slots, hipGetErrorString(e));
    }
    d->slots = slots;
    hipLaunchKernelGGL(k_dedup_clear, dim3(dedup_table_grid(slots)), dim3(256), 0, c->stream, d->tab[0].p, slots);
    const hipError_t e2 = hipGetLastError();
    if (e2 != hipSuccess) {
        ffq_dedup_destroy(d);
        return fail(FFQ_E_HIP, "%s: %s", who, hipGetErrorString(e2));
    }
    *out = d;
    return FFQ_OK;
}

extern "C" int ffq_dedup_select(ffq_dedup *d, const uint64_t *d_keys1, const uint64_t *d_keys2, const int64_t *d_ord, int64_t n,
                                const int64_t *d_table1, const int64_t *d_table2, int64_t *d_out1, int64_t *d_out2, int64_t *d_idx,
                                int64_t *n_out, int drop, int64_t counts[FFQ_DEDUP_COUNTS])
{
    static const char *const who = "ffq_dedup_select";
    if (!d) return fail(FFQ_E_ARG, "%s: NULL set", who);
    ffq_ctx *c = d->c;
    mark_other(c);
    if (!n_out || !counts || n < 0 || (n > 0 && !d_keys1)) return fail(FFQ_E_ARG, "%s: bad argument", who);
    if (d_table2 && !d_keys2) return fail(FFQ_E_ARG, "%s: a second table without a second mate's keys", who);
    if ((d_table1 && !d_out1) || (d_table2 && !d_out2)) return fail(FFQ_E_ARG, "%s: a table without a place for its kept rows", who);
    if (!aligned({d_table1, d_table2, d_out1, d_out2}, 16)) return fail(FFQ_E_ARG, "%s: tables must be 16-byte aligned", who);
    if (!aligned({d_keys1, d_keys2, d_ord, d_idx}, 8)) return fail(FFQ_E_ARG, "%s: keys and ordinals must be 8-byte aligned", who);
    if (n > 0 && ((d_table1 && (d_out1 == d_table1 || d_out1 == d_table2)) || (d_table2 && (d_out2 == d_table2 || d_out2 == d_table1)) ||
                  (d_out1 && d_out1 == d_out2)))
        return fail(FFQ_E_ARG, "%s: d_out1 and d_out2 must not be one of the tables, or each other", who);
    int rc = no_pending(c, who);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    *n_out = 0;
    counts[0] = counts[1] = counts[2] = 0;
    counts[3] = d->distinct; counts[4] = d->slots; counts[5] = d->rehashes;
    if (n == 0) return FFQ_OK;
    // growth, decided here: a call of n rows adds at most n keys
    const int64_t want = dedup_slots_for(d->slots, d->distinct, n);
    if (want != d->slots && d->max_bytes > 0 && want * (int64_t)sizeof(DedupSlot) > d->max_bytes)
        return fail(FFQ_E_NOMEM, "%s: %lld keys and %lld more rows need %lld bytes (%lld slots), max_bytes is %lld", who,
                    (long long)d->distinct, (long long)n, (long long)(want * (int64_t)sizeof(DedupSlot)), (long long)want,
                    (long long)d->max_bytes);
    const int64_t nblk = (n + 255) / 256;
    // (everything is grown before anything is enqueued: growing waits for the stream)
    rc = grow_dev(c, c->filter_verdict, n);
    if (!rc) rc = compact_reserve(c, n);
    if (rc) return rc;
    hipStream_t st = c->stream;
    HIPCHK(hipMemsetAsync(d->d_blk, 0, sizeof(DedupBlock), st));
    if (want != d->slots) {
        DevBuf<DedupSlot> &nu = d->tab[d->cur ^ 1];
        CTX_SYNC(c);                                        // (the table before last goes away)
        const hipError_t e = nu.grow(want);
        if (e != hipSuccess)
            return fail(FFQ_E_NOMEM, "%s: no memory for %lld slots: %s", who, (long long)want, hipGetErrorString(e));
        hipLaunchKernelGGL(k_dedup_clear, dim3(dedup_table_grid(want)), dim3(256), 0, st, nu.p, want);
        hipLaunchKernelGGL(k_dedup_rehash, dim3(dedup_table_grid(d->slots)), dim3(256), 0, st, (const DedupSlot *)d->tab[d->cur].p, d->slots,
                           nu.p, want, d->d_blk.p);
        d->cur ^= 1; d->slots = want; d->rehashes++;
    }
    DedupSlot *tab = d->tab[d->cur].p;
    const unsigned long long *k1 = reinterpret_cast<const unsigned long long *>(d_keys1);
    const unsigned long long *k2 = reinterpret_cast<const unsigned long long *>(d_keys2);
    const unsigned long long g0 = (unsigned long long)d->submitted;
    uint8_t *verdict = c->filter_verdict.p;
    const unsigned rows_wgs = (unsigned)std::min<int64_t>(nblk, DEDUP_GRID_ROWS);
    hipLaunchKernelGGL(k_dedup_insert, dim3(rows_wgs), dim3(DEDUP_WG), 0, st, tab, d->slots, k1, k2, d_ord, n, g0, d->d_blk.p);
    hipLaunchKernelGGL(k_dedup_resolve, dim3(rows_wgs), dim3(DEDUP_WG), 0, st, tab, d->slots, k1, k2, d_ord, n, g0, drop ? 1 : 0, verdict,
                       d->d_blk.p);
    if ((d_table1 || d_table2 || d_idx) && (rc = compact_enqueue(c, st, KeepVerdict{verdict}, n, d_table1, d_table2, d_ord, d_out1, d_out2, d_idx)))
        return rc;
    HIPCHK(hipMemcpyAsync(d->h_blk, d->d_blk, sizeof(DedupBlock), hipMemcpyDeviceToHost, st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    const DedupBlock &b = *d->h_blk.p;
    d->submitted += n;
    d->distinct += (int64_t)b.added;
    if (b.err)
        return fail(FFQ_E_INTERNAL, "%s: a probe visited all %lld slots (stage mask %llu): the table is damaged", who, (long long)d->slots,
                    b.err);
    counts[0] = (int64_t)b.kept; counts[1] = (int64_t)b.dups; counts[2] = (int64_t)b.nokey;
    counts[3] = d->distinct; counts[4] = d->slots; counts[5] = d->rehashes;
    *n_out = drop ? counts[0] : n;
    return FFQ_OK;
}

// ffq_stream.h -- the stream front end of the path, natively (host code of libffq_hip.so):
//   /root/reference/src/fastqandfurious.py:30-36    read(fh, fbufsize): one read, eof := short read
//   /root/reference/src/fastqandfurious.py:241-279  the refill loop of readfastq_iter: sentinel once,
//                                                   buf = buf[offset:] + next chunk, globaloffset
// over a file descriptor, as a three-stage pipeline:
//
//   feeder thread   chunk k+2: pread by a pool of helper threads into pinned slot memory, then
//                   hipMemcpyAsync of the chunk to the slot's device buffer on a COPY stream
//   copy stream     chunk k+1 on its way over PCIe
//   caller thread   fill k: the carried tail buf[offset:] of fill k-1 is put in front of chunk k
//                   (host memcpy + a small H2D on the scan stream), the scan waits for the
//                   chunk's copy event, rows come back into pinned memory
//
// so the file read, the H2D copy and the scan + D2H of three consecutive chunks overlap (the
// first version overlapped only the read).  A slot is [room | fbufsize] on both sides: the
// chunk always lands at offset `room`, the carry ends there, and the fill is the contiguous
// range [room - carry, room + got).  The scan is given the 16-byte aligned address below the
// fill's first byte and starts its search at the fill's first byte (`offset`), so no byte is
// moved to align anything.  Each call of ffq_stream_next hands back the rows (absolute stream
// offsets, what entryfunc_abspos yields, :186-195) of one buffer fill and the fill's bytes for
// slicing; both stay valid until the next call.
//
// Three kinds of source feed the same slots:
//   a descriptor        the feeder thread: pread in parallel slices (regular files), or read()
//                       behind poll() (pipes: interruptible, and a chunk is handed over short when
//                       nothing more has arrived for a while -- a short chunk is not the end)
//   a gzip descriptor   the feeder thread inflates (GzReader, ffq_gzread.h; concatenated members) straight into
//                       the pinned slot: decompression is the feeder stage, no interpreter involved
//                       (reference: FORMAT_OPENERS / automagic_open, fastqandfurious.py:282-334)
//   pushed chunks       no feeder thread: the host writes every chunk into the slot's pinned memory
//                       itself (ffq_stream_push_buffer / ffq_stream_push) -- any Python file-like
//                       object (BytesIO, bz2, lzma ...) read with readinto(), no bytes copy
#pragma once
#include "ffq_gzread.h"
#include "ffq_pairwalk.h"

#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>

#ifndef FFQ_STREAM_SLOTS
#define FFQ_STREAM_SLOTS 3
#endif
#ifndef FFQ_STREAM_AHEAD
#define FFQ_STREAM_AHEAD 2
#endif
constexpr int STREAM_SLOTS = FFQ_STREAM_SLOTS;

struct StreamSlot {
    Mirror<uint8_t> buf;         // pinned h and device d, the same layout: [room | fbufsize (+16)]
    hipEvent_t copied[2] = {nullptr, nullptr};   // the chunk's H2D copy is through (one half per copy stream)
    int64_t got = 0;             // bytes of the chunk (at offset room)
    bool eof = false;            // the source is exhausted behind this chunk
    int64_t end_pos = 0;         // position of the source behind this chunk (ffq_stream_tell)
    ChunkRead cr;                // its slices while they are being read
};

// everything a stream allocates; parked in the context when a stream closes so that the next
// stream of the same chunk size starts without the pinned allocations (milliseconds each)
struct StreamBufs {
    int64_t fbufsize = 0, room = 0;
    StreamSlot slot[STREAM_SLOTS];
    hipStream_t cs[2] = {nullptr, nullptr};      // copy streams of the chunks: a chunk goes over in two halves, one
                                                 // per stream (two DMA engines: one did 41-45 GB/s of the link's ~55)
    bool one_copy_stream = false;                // ... unless much goes BACK as well (stream_copy_chunk)
    // device + pinned pairs (ffq_mem.h), grown by stream_grow
    Mirror<int64_t> tab;         // the fill's rows: 6 words each (stream_tab_rows)
    Mirror<int8_t> qual;
    Mirror<int64_t> qoff;
    // push-down (ffq_stream_set_filter): the kept rows and their ordinals, the gathered column
    DevBuf<int64_t> sel;
    Mirror<int64_t> idx;
    Mirror<int8_t> col;
    Mirror<int64_t> coff;
    // rendering (ffq_stream_set_render): the fill's FASTQ text
    Mirror<uint8_t> ren;
    // ... and, compressed (ffq_stream_set_compress), its BGZF members: what is copied back in the text's place
    Mirror<uint8_t> bgz;
    ReadPool *pool = nullptr;    // the context's helper threads (not owned)
};

static void streambufs_free(StreamBufs *b)
{
    if (!b) return;
    for (auto &s : b->slot) for (auto &e : s.copied) if (e) (void)hipEventDestroy(e);
    for (auto &st : b->cs) if (st) (void)hipStreamDestroy(st);
    delete b;                    // (the buffers free themselves)
}

// called by ffq_ctx_destroy
static void stream_cache_drop(ffq_ctx *c)
{
    streambufs_free(static_cast<StreamBufs *>(c->stream_cache));
    c->stream_cache = nullptr;
}

static int streambufs_alloc_slots(ffq_ctx *c, StreamBufs *b, int64_t room)
{
    NearGpu near(c);                   // (the pinned slots on the GPU's node: ffq_hip.hip)
    for (auto &s : b->slot)
        if (s.buf.grow(room + b->fbufsize + 16) != hipSuccess)
            return fail(FFQ_E_NOMEM, "ffq_stream: no memory for %lld-byte chunks with a %lld-byte carry",
                        (long long)b->fbufsize, (long long)room);
    b->room = room;
    return FFQ_OK;
}

// the H2D copy of a slot's chunk: two halves, two streams, two events
static hipError_t stream_copy_chunk(StreamBufs *b, StreamSlot &sl, int64_t got)
{
    // (one stream for a stream that DECODES: two copy streams in and the copies back on a third share the copy engines --
    // 42.9 GB/s in + 28.7 back against 54.7 + 36.6 with one stream in, tools/link_duplex.py; the stream front end with the
    // decode 34-36 -> 43-45 GB/s, without it 54 -> 47-50, so a plain stream keeps its two)
    const bool one = b->one_copy_stream;
    const int64_t half = one ? got : ((got / 2) + 4095) & ~(int64_t)4095;
    hipError_t e = hipSuccess;
    for (int h = 0; h < 2 && e == hipSuccess; h++) {
        const int64_t a = h ? std::min(half, got) : 0, z = h ? got : std::min(half, got);
        hipStream_t st = b->cs[one ? 0 : h];
        if (z > a) e = hipMemcpyAsync(sl.buf.d + b->room + a, sl.buf.h + b->room + a, (size_t)(z - a), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(sl.copied[h], st);
    }
    return e;
}

constexpr int SRC_FD = 0, SRC_GZIP = 1, SRC_PUSH = 2;

// a length bound that bounds nothing: what a stream without a length filter is selected by
constexpr int64_t LEN_UNBOUNDED = (int64_t)1 << 62;

// What the dedup stage of a chain owns, in a stream (one table) and in a pair (two): the set, the rows and the ordinals that
// remain behind it, the counts summed over the fills or rounds.
struct DedupStage {
    bool on = false;
    int drop = 1;
    ffq_dedup *set = nullptr;
    DevBuf<int64_t> rows[2], idx;
    int64_t total[FFQ_DEDUP_COUNTS] = {0, 0, 0, 0, 0, 0};
};

struct ffq_stream {
    ffq_ctx *c = nullptr;
    StreamBufs *b = nullptr;
    int fd = -1, src = SRC_FD;
    bool seekable = false;
    bool sliced = false;                // the source is read in slices queued ahead: a plain descriptor that can seek
    std::unique_ptr<GzReader> gz;       // SRC_GZIP: the inflating source (feeder thread only)
    Interrupt irq = {nullptr, nullptr}; // what the feeder's blocking reads ask: stream_asked
    int64_t handed_pos = 0;             // position of the source behind the last chunk handed out
    uint32_t flags = 0;                 // FFQ_F_DECODE_QUAL: qualities decoded per fill
    int qual_add = -33;
    // ---- feeder <-> caller (under m) ----
    std::thread feeder;
    std::mutex m;
    std::condition_variable cv;
    int64_t produced = 0;               // chunks [0, produced) are read and their copy is enqueued
    int64_t released = 0;               // chunks [0, released) are consumed: their slots may be refilled
    int64_t file_pos = 0;               // next byte to read
    bool stop = false, feeder_done = false, pause_req = false, paused = false;
    int feeder_rc = FFQ_OK;
    std::string feeder_msg;
    // ---- caller only ----
    int64_t cur = -1;                   // chunk of the fill handed out last
    int64_t fill_start = 0, fill_len = 0;   // that fill is slot.h[fill_start, fill_start + fill_len)
    int64_t carry_from = 0;             // fill-relative offset the next fill starts with (buf[offset:], :277)
    bool done = false, failed = false;
    bool paired = false;                // a pair walks this stream (ffq_pair_open): ffq_stream_next is refused
    int64_t globaloffset = -1;          // readfastq_iter :242
    int64_t last_nq = 0;
    int last_path = -1;                 // ffq_scan_result.path of the last fill's scan
    // statistics of every fill's table, summed over the fills on the device (ffq_stream_set_stats): the IN block, the OUT block
    struct { int which = 0, base = 33, cycles = 0; DevBuf<uint64_t> d; } stats;
    // fixed trims and sliding-window cutting of every fill's table, in front of every other trim (ffq_stream_set_ends)
    struct { bool on = false; ffq_ends_rules rules = {}; int64_t last[3] = {0, 0, 0}; } ends;
    // quality trimming of every fill's table, in front of the filter (ffq_stream_set_trim)
    struct { bool on = false; int base = 33, front = 0, back = 0; int64_t last[3] = {0, 0, 0}; } trim;
    // 3' adapter trimming of every fill's table, behind the quality trim and in front of the filter (ffq_stream_set_adapter)
    struct { bool on = false; uint8_t bytes[64] = {0}; int len = 0, err = 0, overlap = 0; int64_t last[3] = {0, 0, 0}; } adapter;
    // poly-tail trimming of every fill's table: poly-G in front of the adapter trim, poly-X behind it (ffq_stream_set_poly; 0: off)
    struct { int g = 0, x = 0; int64_t last_g[3] = {0, 0, 0}, last_x[3] = {0, 0, 0}; } poly;
    // UMIs (ffq_stream_set_umi, ffq_pair_set_umi): on: the render puts the tag into the names; take: this stream's reads begin with
    // one, which every fill's table loses in front of the trims; the take's counts and the tagged rows of the last fill or round
    struct { bool on = false, take = false; ffq_umi_rules rules = {}; int64_t last[3] = {0, 0, 0}, tagged = 0; } umi;
    // push-down: rows by sequence length, one component of the kept rows (ffq_stream_set_filter)
    struct { bool on = false; int64_t min = 0, max = 0; int col = 0, add = 0; int64_t scanned = 0, col_bytes = 0; } filter;
    // content rules of the filter (ffq_stream_set_content) and the eight counts of the last fill's select (with or without them)
    struct { bool on = false; ffq_content_rules rules = {}; int64_t last[FFQ_FILTER_COUNTS] = {0, 0, 0, 0, 0, 0, 0, 0}; } content;
    // FASTQ text of every fill's table, behind the trim and the filter (ffq_stream_set_render)
    struct { bool on = false; int64_t last[3] = {0, 0, 0}; } render;
    // ... written as BGZF members on the device, which go back in its place (ffq_stream_set_compress)
    struct { bool on = false; int64_t last[FFQ_DEFLATE_COUNTS] = {0, 0, 0, 0}; } compress;
    // duplicate removal (ffq_stream_set_dedup): the stream's own set, the keys of the fill's rows as scanned, the rows and
    // ordinals that remain behind it, and the counts summed over the fills.  keys_on alone: a pair takes the keys (ffq_pair_set_dedup)
    struct : DedupStage {
        bool keys_on = false;
        DevBuf<uint64_t> keys;
        int64_t keyed[2] = {0, 0};
    } dedup;
    // FFQ_STREAM_PROF=1: where the time of a stream goes (printed when it closes)
    bool prof = false;
    double t_read = 0, t_slot = 0, t_feed = 0, t_scan = 0, t_rows = 0, t_copy = 0;
};

// has the caller asked the feeder to stop -- or_park: or to park (stream_grow_room)?
static bool stream_asked(void *owner, bool or_park)
{
    ffq_stream *s = static_cast<ffq_stream *>(owner);
    std::lock_guard<std::mutex> lk(s->m);
    return s->stop || (or_park && s->pause_req);
}

static inline double stream_now()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- the feeder thread ------------------------------------------------------------------------------------------------
// It completes chunks in order: once chunk p is in its slot, its H2D copy goes onto the copy stream and the caller may take
// it.  Of a sliced source it queues the slices of chunk e as soon as slot e % STREAM_SLOTS is free, up to FFQ_STREAM_AHEAD
// chunks in front of p; any other source is read when its chunk's turn comes (e == p between chunks).  Each turn of its
// loop is three steps: feeder_wait, feeder_queue (as often as feeder_wait says), feeder_complete.
struct Feeder {
    ffq_stream *s;
    StreamBufs *b;
    int64_t pos0;                // the file offset of chunk 0
    int64_t p = 0, e = 0;        // chunk to complete next; chunks [0, e) have their slices queued
};

enum FeedNext { FEED_STOP, FEED_QUEUE, FEED_READ };

// Step 1: wait for a free slot, a park request or a stop (under s->m); what to do next.
static FeedNext feeder_wait(Feeder &f)
{
    ffq_stream *s = f.s;
    std::unique_lock<std::mutex> lk(s->m);
    for (;;) {
        if (s->stop) return FEED_STOP;
        if (s->pause_req && f.e == f.p) {          // the caller reallocates the slots: park here (nothing in flight)
            s->paused = true;
            s->cv.notify_all();
            s->cv.wait(lk);
            continue;
        }
        s->paused = false;
        if (f.e > f.p || (s->sliced ? f.e : f.p) - s->released < STREAM_SLOTS) break;   // a read to wait for, or a free slot
        s->cv.wait(lk);
    }
    const bool ahead = s->sliced && !s->pause_req && f.e - s->released < STREAM_SLOTS && f.e - f.p < FFQ_STREAM_AHEAD;
    return ahead ? FEED_QUEUE : FEED_READ;
}

// Step 2 (a sliced source): queue the slices of chunk e.
static void feeder_queue(Feeder &f)
{
    StreamSlot &sq = f.b->slot[f.e % STREAM_SLOTS];
    f.b->pool->enqueue(f.s->fd, sq.buf.h + f.b->room, f.b->fbufsize, f.pos0 + f.e * f.b->fbufsize, &sq.cr);
    f.e++;
}

// the slices of chunks [from, e) are in flight: nothing may be freed or reallocated under them
static void feeder_drain(Feeder &f, int64_t from)
{
    for (int64_t k = from; k < f.e; k++) f.b->pool->wait(&f.b->slot[k % STREAM_SLOTS].cr);
}

// Chunk p of each kind of source into its slot.  Returns the bytes; -1: error; -2 (a pipe): asked to stop / park with
// nothing read.  *eof: the source ends behind them.
static int64_t feed_slices(Feeder &f, StreamSlot &sl, bool *eof)
{
    f.b->pool->wait(&sl.cr);
    const int64_t got = sl.cr.total();
    *eof = got < f.b->fbufsize;
    return got;
}
static int64_t feed_gzip(Feeder &f, StreamSlot &sl, bool *eof) { return f.s->gz->read(sl.buf.h + f.b->room, f.b->fbufsize, eof); }
static int64_t feed_pipe(Feeder &f, StreamSlot &sl, bool *eof) { return stream_fd_read(f.s->fd, &f.s->irq, sl.buf.h + f.b->room, f.b->fbufsize, eof); }

// Step 3: read chunk p from its source, enqueue its copy, publish it.  false: the feeder is through (the end, or an error).
static bool feeder_complete(Feeder &f, double tw0)
{
    ffq_stream *s = f.s;
    StreamBufs *b = f.b;
    StreamSlot &sl = b->slot[f.p % STREAM_SLOTS];
    const double tr0 = s->prof ? stream_now() : 0;
    bool src_eof = false;
    const int64_t got = (s->sliced ? feed_slices : s->src == SRC_GZIP ? feed_gzip : feed_pipe)(f, sl, &src_eof);
    if (got == -2) return true;                    // back to feeder_wait, for the same chunk
    if (!s->sliced) f.e = f.p + 1;
    if (s->prof) { const double t = stream_now(); s->t_slot += tr0 - tw0; s->t_read += t - tr0; }
    int rc = FFQ_OK;
    std::string msg;
    if (got < 0) {
        rc = FFQ_E_ARG;
        msg = s->src == SRC_GZIP ? std::string("ffq_stream: gzip: ") + s->gz->msg() : std::string("ffq_stream: read failed: ") + strerror(errno);
    } else {
        sl.got = got;
        sl.eof = src_eof;
        const hipError_t er = stream_copy_chunk(b, sl, got);
        if (er != hipSuccess) { rc = FFQ_E_HIP; msg = std::string("ffq_stream: chunk copy failed: ") + hipGetErrorString(er); }
    }
    if (rc || sl.eof) feeder_drain(f, f.p + 1);    // reads past the end
    {
        std::lock_guard<std::mutex> lk(s->m);
        if (rc) { s->feeder_rc = rc; s->feeder_msg = msg; s->feeder_done = true; }
        else {
            s->file_pos = s->src == SRC_GZIP ? s->gz->file_pos() : s->file_pos + got;
            sl.end_pos = s->file_pos;
            s->produced = f.p + 1;
            if (sl.eof) s->feeder_done = true;
        }
    }
    s->cv.notify_all();
    f.p++;
    return !(rc || sl.eof);
}

static void stream_feeder(ffq_stream *s)
{
    (void)hipSetDevice(s->c->device);
    Feeder f{s, s->b, s->file_pos};
    for (;;) {
        const double tw0 = s->prof ? stream_now() : 0;
        FeedNext next;
        while ((next = feeder_wait(f)) == FEED_QUEUE) feeder_queue(f);
        if (next == FEED_STOP) {
            feeder_drain(f, f.p);                  // reads in flight
            std::lock_guard<std::mutex> lk(s->m);
            s->feeder_done = true;
            s->cv.notify_all();
            return;
        }
        if (!feeder_complete(f, tw0)) return;
    }
}

static void stream_stop_feeder(ffq_stream *s)
{
    if (!s->feeder.joinable()) return;
    { std::lock_guard<std::mutex> lk(s->m); s->stop = true; }
    s->cv.notify_all();
    s->feeder.join();
}

static void stream_free(ffq_stream *s)
{
    if (!s) return;
    stream_stop_feeder(s);
    if (s->prof)
        fprintf(stderr, "[ffq stream] %lld fills: reader %.3f ms reading, %.3f ms waiting for a slot; caller %.3f ms waiting "
                        "for the reader, %.3f ms carry + scan (of which %.3f ms waiting for the chunk's copy), %.3f ms rows back\n",
                (long long)(s->cur + 1), s->t_read * 1e3, s->t_slot * 1e3, s->t_feed * 1e3, s->t_scan * 1e3, s->t_copy * 1e3,
                s->t_rows * 1e3);
    ffq_dedup_destroy(s->dedup.set);         // (waits for the scan stream)
    if (s->b) {
        for (auto &st : s->b->cs) if (st) (void)hipStreamSynchronize(st);
        if (s->c->stream) (void)hipStreamSynchronize(s->c->stream);
        // park the buffers in the context for the next stream
        if (!s->c->stream_cache) s->c->stream_cache = s->b;
        else streambufs_free(s->b);
    }
    delete s;
}

// One of the stream's buffers (a device + pinned pair, or the device-only rows of the push-down) grown to `n` elements, or
// FFQ_E_NOMEM with the text `what` ("ffq_stream: no memory for %lld ...") about `said`.  What is large enough stays.
template <class B>
static int stream_grow(B &buf, int64_t n, const char *what, int64_t said)
{
    if (buf.grow(n) == hipSuccess) return FFQ_OK;
    return fail(FFQ_E_NOMEM, what, (long long)said);
}

static int64_t stream_tab_rows(const StreamBufs *b) { return b->tab.d.cap / 6; }

static int stream_alloc_tab(ffq_stream *s, int64_t rows)
{
    StreamBufs *b = s->b;
    NearGpu near(s->c);
    int rc = stream_grow(b->tab, rows * 6, "ffq_stream: no memory for %lld rows", rows);
    if (!rc && (s->flags & FFQ_F_DECODE_QUAL))
        rc = stream_grow(b->qoff, stream_tab_rows(b) + 1, "ffq_stream: no memory for %lld quality offsets", stream_tab_rows(b));
    return rc;
}

// device / pinned buffers of the push-down for a fill of up to `rows` rows (and `bytes` of column)
static int stream_alloc_sel(ffq_stream *s, int64_t rows, int64_t bytes)
{
    StreamBufs *b = s->b;
    int rc = stream_grow(b->sel, rows * 6, "ffq_stream: no memory for %lld selected rows", rows);
    if (!rc) rc = stream_grow(b->idx, rows, "ffq_stream: no memory for %lld selected rows", rows);
    if (!rc && s->filter.col) rc = stream_grow(b->coff, rows + 1, "ffq_stream: no memory for %lld column offsets", rows);
    if (!rc && s->filter.col) rc = stream_grow(b->col, bytes, "ffq_stream: no memory for %lld column bytes", bytes);
    return rc;
}

// One fill: chunk k in its slot behind the carry, slot bytes [start, start + len), and the ONE view of it that the scan and
// every table pass are given: from the 16-byte aligned address below the fill's first byte (mis bytes below it); a row
// (a stream offset) minus `add` is a coordinate of that view.
struct Fill {
    StreamSlot *sl;
    int64_t start, len, mis;
    bool eof;                    // the source ends behind this fill
    const uint8_t *d_buf;        // sl->buf.d + start - mis
    int64_t n, add;              // len + mis; the view's first byte as a stream offset
};

// the table the chain is at: the scan's rows at first, the kept rows behind the select
struct Table { const int64_t *d_rows; int64_t n; };

// The rows the fill hands out (trimmed and filtered, if the stream does that) as FASTQ text, on the device, and its copy
// back enqueued.  BOUND: the rows of a fill are records of the fill that do not overlap, and a scanned record never
// renders longer than it was -- "@header\n", "sequence\n" and "quality\n" are copied, the '+' line becomes the bare "+\n"
// (it had at least that), a trim only takes bytes away -- except a record whose quality ends with the buffer, without a newline, which gains one
// byte: a fill of `len` bytes renders to at most len + 1.  A stream that compresses (ffq_stream_set_compress) deflates the
// text where it lies, behind the render, and only the members go back.
// THE TAGGED ROUTE (s->umi.on) has another bound: a row gains its insert -- a mate that gives no bases still gains a tag, so "never
// longer than it was" no longer holds --, at most 3 + prefix_len + 2 * len bytes (delim, prefix and '_', two tags and the '_'
// between them): len + 1 + rows * that.  src: the views whose row i may carry the tag of read 1 / read 2, in step with t's rows;
// NULL: the rendered table itself carries it (a single stream).
static int stream_render(ffq_stream *s, const Fill &f, const Table &t, const ffq_table_view *src)
{
    StreamBufs *b = s->b;
    int64_t *last = s->render.last;
    last[0] = last[1] = last[2] = 0;
    s->umi.tagged = 0;
    for (int64_t &x : s->compress.last) x = 0;
    if (t.n <= 0) return FFQ_OK;
    int rc = FFQ_OK;
    const int64_t cap = f.n + 1 + (s->umi.on ? t.n * (3 + s->umi.rules.prefix_len + 2 * (int64_t)s->umi.rules.len) : 0);
    if (cap + 63 > b->ren.d.cap) {
        NearGpu near(s->c);
        rc = stream_grow(b->ren, cap + 63, "ffq_stream: no memory for %lld rendered bytes", cap + 63);
    }
    const int64_t bgz_cap = ffq_deflate_bgzf_bound(cap);
    if (!rc && s->compress.on && bgz_cap > b->bgz.d.cap) {
        NearGpu near(s->c);
        rc = stream_grow(b->bgz, bgz_cap, "ffq_stream: no memory for %lld compressed bytes", bgz_cap);
    }
    if (!rc && s->umi.on) {
        const ffq_table_view own = {f.d_buf, f.n, 0, f.add, t.d_rows};
        int64_t st[4] = {0, 0, 0, 0};
        rc = ffq_table_render_fastq_umi(s->c, &own, t.n, src ? &src[0] : &own, src ? &src[1] : &own, &s->umi.rules, b->ren.d, cap, nullptr, st);
        last[0] = st[0]; last[1] = st[1]; last[2] = st[2];
        s->umi.tagged = st[3];
    } else if (!rc)
        rc = ffq_table_render_fastq(s->c, f.d_buf, f.n, 0, f.add, t.d_rows, t.n, b->ren.d, f.n + 1, nullptr, last);
    if (rc == FFQ_E_TABLE_FULL)
        return fail(FFQ_E_INTERNAL, "ffq_stream: a fill of %lld bytes rendered to %lld", (long long)f.n, (long long)last[0]);
    if (rc) return rc;
    if (s->compress.on) {
        int64_t *z = s->compress.last;
        rc = ffq_deflate_bgzf(s->c, b->ren.d, last[0], b->bgz.d, b->bgz.d.cap, nullptr, z);
        if (rc == FFQ_E_TABLE_FULL)
            return fail(FFQ_E_INTERNAL, "ffq_stream: %lld rendered bytes deflated to %lld", (long long)last[0], (long long)z[1]);
        if (rc) return rc;
        if (z[1] > 0) HIPCHK(hipMemcpyAsync(b->bgz.h, b->bgz.d, (size_t)z[1], hipMemcpyDeviceToHost, s->c->stream));
        return FFQ_OK;
    }
    if (last[0] > 0) HIPCHK(hipMemcpyAsync(b->ren.h, b->ren.d, (size_t)last[0], hipMemcpyDeviceToHost, s->c->stream));
    return FFQ_OK;
}

// A carry that does not fit in front of a chunk (a record longer than `room`): every slot is
// reallocated with more room.  The feeder is parked first; chunks it has read ahead are moved
// and their copy is enqueued again.  Called at the START of ffq_stream_next, before any pointer
// of the new fill is handed out -- the previous fill's pointers expire with this call anyway.
static int stream_grow_room(ffq_stream *s, int64_t need)
{
    StreamBufs *b = s->b;
    if (s->src != SRC_PUSH) {
        std::unique_lock<std::mutex> lk(s->m);
        s->pause_req = true;
        s->cv.notify_all();
        s->cv.wait(lk, [&] { return s->paused || s->feeder_done; });
    }
    int rc = FFQ_OK;
    hipError_t e = hipStreamSynchronize(b->cs[0]);
    if (e == hipSuccess) e = hipStreamSynchronize(b->cs[1]);
    if (e != hipSuccess) rc = fail(FFQ_E_HIP, "ffq_stream: %s", hipGetErrorString(e));
    const int64_t room = (std::max<int64_t>(2 * b->room, need + 4096) + 4095) & ~(int64_t)4095;
    {
        // the slots' memory moves into `old` and is freed where that ends: both copy streams are through with it (above)
        Mirror<uint8_t> old[STREAM_SLOTS];
        for (int i = 0; i < STREAM_SLOTS; i++) old[i] = std::move(b->slot[i].buf);
        const int64_t old_room = b->room;
        if (!rc) rc = streambufs_alloc_slots(s->c, b, room);
        if (!rc) {
            // chunks [released, produced) are alive: the one being carried from (cur, all of its fill)
            // and the ones read ahead (their chunk bytes)
            for (int64_t k = std::max<int64_t>(s->released, 0); k < s->produced && !rc; k++) {
                StreamSlot &n = b->slot[k % STREAM_SLOTS];
                const uint8_t *oh = old[k % STREAM_SLOTS].h;
                if (k == s->cur) {
                    memcpy(n.buf.h + room - (old_room - s->fill_start), oh + s->fill_start, (size_t)s->fill_len);
                    s->fill_start = room - (old_room - s->fill_start);
                } else {
                    memcpy(n.buf.h + room, oh + old_room, (size_t)n.got);
                    e = stream_copy_chunk(b, n, n.got);
                    if (e != hipSuccess) rc = fail(FFQ_E_HIP, "ffq_stream: %s", hipGetErrorString(e));
                }
            }
        }
    }
    {
        std::lock_guard<std::mutex> lk(s->m);
        s->pause_req = false;
    }
    s->cv.notify_all();
    return rc;
}

static int stream_open_impl(ffq_ctx *c, int src, int fd, int64_t fbufsize, uint32_t flags, int qual_add, int64_t start,
                            ffq_stream **out)
{
    if (!c || !out || (src != SRC_PUSH && fd < 0) || fbufsize <= 0) return fail(FFQ_E_ARG, "ffq_stream_open: bad argument");
    *out = nullptr;
    HIPCHK(hipSetDevice(c->device));
    ffq_stream *s = new (std::nothrow) ffq_stream();
    if (!s) return fail(FFQ_E_NOMEM, "out of host memory");
    s->c = c; s->fd = fd; s->src = src; s->irq = Interrupt{stream_asked, s};
    // (FFQ_F_SINGLE_PASS: the fill's qualities come SEGMENTED -- ffq_stream_quals -- from the pass that builds the index)
    s->flags = flags & (FFQ_F_DECODE_QUAL | ((flags & FFQ_F_DECODE_QUAL) ? FFQ_F_SINGLE_PASS : 0u)); s->qual_add = qual_add;
    s->prof = getenv("FFQ_STREAM_PROF") != nullptr;
    if (src == SRC_PUSH) s->feeder_done = true;          // there is no reader thread: chunks are pushed
    else {
        // where to read from: `start` (pread; the descriptor's own position is left alone), or the
        // descriptor's current position if start < 0; a descriptor that cannot seek is read in order
        const off_t at = lseek(fd, 0, SEEK_CUR);
        s->seekable = at != (off_t)-1;
        s->sliced = s->seekable && src == SRC_FD;
        s->file_pos = s->seekable ? (start >= 0 ? start : (int64_t)at) : 0;
        s->handed_pos = s->file_pos;
    }
    if (src == SRC_GZIP) {
        s->gz.reset(new (std::nothrow) GzReader(fd, s->file_pos, s->seekable, 0, &s->irq));
        if (!s->gz || !s->gz->ok()) { delete s; return fail(FFQ_E_NOMEM, "ffq_stream_open: zlib could not be initialised"); }
    }
    StreamBufs *b = static_cast<StreamBufs *>(c->stream_cache);
    c->stream_cache = nullptr;
    if (b && b->fbufsize != fbufsize) { streambufs_free(b); b = nullptr; }
    int rc = FFQ_OK;
    if (!b) {
        b = new (std::nothrow) StreamBufs();
        if (!b) { delete s; return fail(FFQ_E_NOMEM, "out of host memory"); }
        b->fbufsize = fbufsize;
        hipError_t e = hipSuccess;
        for (auto &st : b->cs)
            if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        for (auto &sl : b->slot)
            for (auto &ev : sl.copied)
                if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) rc = fail(FFQ_E_HIP, "ffq_stream_open: %s", hipGetErrorString(e));
        if (!rc) rc = streambufs_alloc_slots(c, b, 1 << 20);
    }
    if (!rc && !(b->pool = ctx_pool(c))) rc = fail(FFQ_E_NOMEM, "out of host memory");
    const char *e1 = getenv("FFQ_STREAM_ONE_COPY_STREAM");                 // (measurements: 0 / 1 whatever the stream does)
    b->one_copy_stream = e1 ? atoi(e1) != 0 : (flags & FFQ_F_DECODE_QUAL) != 0;
    s->b = b;
    if (!rc) rc = stream_alloc_tab(s, fbufsize / 64 + 1024);
    if (rc) { stream_free(s); return rc; }
    if (src != SRC_PUSH) s->feeder = std::thread(stream_feeder, s);
    *out = s;
    return FFQ_OK;
}

extern "C" int ffq_stream_open2(ffq_ctx *c, int fd, int64_t fbufsize, uint32_t flags, int qual_add, int64_t start,
                                ffq_stream **out)
{
    return stream_open_impl(c, SRC_FD, fd, fbufsize, flags, qual_add, start, out);
}

extern "C" int ffq_stream_open(ffq_ctx *c, int fd, int64_t fbufsize, ffq_stream **out)
{
    return stream_open_impl(c, SRC_FD, fd, fbufsize, 0, 0, -1, out);
}

extern "C" int ffq_stream_open_gzip(ffq_ctx *c, int fd, int64_t fbufsize, uint32_t flags, int qual_add, int64_t start,
                                    ffq_stream **out)
{
    return stream_open_impl(c, SRC_GZIP, fd, fbufsize, flags, qual_add, start, out);
}

// The gzip reader on its own: the file behind fd (from its current position; a pipe works), inflated into
// host memory chunk by chunk as the stream's reader thread does it.  Returns the bytes written, or FFQ_E_*.
extern "C" int64_t ffq_gunzip_fd(int fd, uint8_t *h_dst, int64_t cap, int64_t chunk, int threads, int64_t *n_parallel_members)
{
    if (fd < 0 || (!h_dst && cap > 0) || cap < 0 || chunk <= 0) return fail(FFQ_E_ARG, "ffq_gunzip_fd: bad argument");
    const off_t at = lseek(fd, 0, SEEK_CUR);
    GzReader gz(fd, at != (off_t)-1 ? (int64_t)at : 0, at != (off_t)-1, threads, nullptr);
    if (!gz.ok()) return fail(FFQ_E_NOMEM, "ffq_gunzip_fd: zlib could not be initialised");
    int64_t rc = FFQ_OK, got = 0;
    bool eof = false;
    uint8_t one[1];
    while (!eof) {
        const bool full = got == cap;
        const int64_t r = gz.read(full ? one : h_dst + got, full ? 1 : std::min(chunk, cap - got), &eof);
        if (r < 0) { rc = fail(FFQ_E_ARG, "ffq_gunzip_fd: gzip: %s", gz.msg()); break; }
        if (full && r > 0) { rc = fail(FFQ_E_TABLE_FULL, "ffq_gunzip_fd: the file inflates to more than %lld bytes", (long long)cap); break; }
        got += full ? 0 : r;
    }
    if (n_parallel_members) *n_parallel_members = gz.parallel_members();
    return rc ? rc : got;
}

extern "C" void ffq_gunzip_stats(int64_t out[5])
{
    pgz::Stats &st = pgz::stats();
    out[0] = st.batches.load(); out[1] = st.chunks.load(); out[2] = st.rejected.load(); out[3] = st.giveups.load(); out[4] = st.members.load();
}

extern "C" int ffq_stream_open_push(ffq_ctx *c, int64_t fbufsize, uint32_t flags, int qual_add, ffq_stream **out)
{
    return stream_open_impl(c, SRC_PUSH, -1, fbufsize, flags, qual_add, -1, out);
}

// push mode: where the next chunk's bytes go (pinned memory, fbufsize bytes of room) ...
extern "C" int ffq_stream_push_buffer(ffq_stream *s, uint8_t **dst, int64_t *cap)
{
    if (!s || !dst || !cap || s->src != SRC_PUSH) return fail(FFQ_E_ARG, "ffq_stream_push_buffer: not a push stream");
    if (s->failed || s->done) return fail(FFQ_E_ARG, "ffq_stream_push_buffer: the stream has %s", s->failed ? "failed" : "ended");
    if (s->produced - s->released >= STREAM_SLOTS) return fail(FFQ_E_ARG, "ffq_stream_push_buffer: every slot holds an unconsumed chunk");
    *dst = s->b->slot[s->produced % STREAM_SLOTS].buf.h + s->b->room;
    *cap = s->b->fbufsize;
    return FFQ_OK;
}

// ... and: n bytes are there now; eof: nothing follows.  The chunk's copy to the device is enqueued.
extern "C" int ffq_stream_push(ffq_stream *s, int64_t n, int eof)
{
    if (!s || s->src != SRC_PUSH) return fail(FFQ_E_ARG, "ffq_stream_push: not a push stream");
    if (n < 0 || n > s->b->fbufsize) return fail(FFQ_E_ARG, "ffq_stream_push: %lld bytes do not fit a chunk of %lld", (long long)n, (long long)s->b->fbufsize);
    if (s->failed || s->done) return fail(FFQ_E_ARG, "ffq_stream_push: the stream has %s", s->failed ? "failed" : "ended");
    if (s->produced - s->released >= STREAM_SLOTS) return fail(FFQ_E_ARG, "ffq_stream_push: every slot holds an unconsumed chunk");
    HIPCHK(hipSetDevice(s->c->device));
    StreamSlot &sl = s->b->slot[s->produced % STREAM_SLOTS];
    sl.got = n; sl.eof = eof != 0;
    s->file_pos += n;
    sl.end_pos = s->file_pos;
    const hipError_t e = stream_copy_chunk(s->b, sl, n);
    if (e != hipSuccess) { s->failed = true; return fail(FFQ_E_HIP, "ffq_stream_push: chunk copy failed: %s", hipGetErrorString(e)); }
    s->produced++;
    return FFQ_OK;
}

extern "C" void ffq_stream_close(ffq_stream *s) { stream_free(s); }

extern "C" int64_t ffq_stream_tell(ffq_stream *s)
{
    if (!s) return -1;
    // behind the last chunk HANDED OUT (the reader runs up to two chunks ahead of that): where the
    // reference's loop would have left the file after the same fills
    return s->handed_pos;
}

// ffq_scan_result.path of the last fill's scan (6: index and decoded qualities in one pass)
extern "C" int ffq_stream_path(ffq_stream *s) { return s ? s->last_path : -1; }

// decoded qualities of the fill ffq_stream_next has just returned (streams opened with
// FFQ_F_DECODE_QUAL): int8 bytes + offsets (n_rows + 1), pinned, valid until the next call.  Record i's bytes are
// h_qual[h_qoff[i] : h_qoff[i] + pos5(i) - pos4(i)] -- packed back to back (then h_qoff[i + 1] is where they end), or,
// for a stream opened with FFQ_F_SINGLE_PASS whose fill the single pass took, with gaps between the index tiles'
// segments (include/ffq.h, FFQ_F_SINGLE_PASS); h_qoff[n_rows] = *n_qual_bytes = where the last record's bytes end.
extern "C" int ffq_stream_quals(ffq_stream *s, const int8_t **h_qual, const int64_t **h_qoff, int64_t *n_qual_bytes)
{
    if (!s || !h_qual || !h_qoff || !n_qual_bytes) return fail(FFQ_E_ARG, "ffq_stream_quals: NULL argument");
    if (!(s->flags & FFQ_F_DECODE_QUAL)) return fail(FFQ_E_ARG, "ffq_stream_quals: the stream was opened without FFQ_F_DECODE_QUAL");
    *h_qual = s->b->qual.h; *h_qoff = s->b->qoff.h; *n_qual_bytes = s->last_nq;
    return FFQ_OK;
}

// What the setters below share: a stage that cannot serve a stream that decodes says why (`decode_why`, behind the text
// all three begin with), and every stage but the filter is set before the first fill.
static const char *const DECODE_GATHERS = "; a filtered stream gathers the kept records' (column = FFQ_COL_QUALITY, value_add)";
static const char *const DECODE_UNTRIMMED = " beside the scan, untrimmed; a filtered stream gathers the trimmed ones "
                                            "(ffq_stream_set_filter: column = FFQ_COL_QUALITY, value_add)";
static const char *const DECODE_TEXT = "; FASTQ text holds them as they are";

static int stream_settable(ffq_stream *s, const char *who, const char *decode_why, bool fresh)
{
    if (decode_why && (s->flags & FFQ_F_DECODE_QUAL))
        return fail(FFQ_E_ARG, "%s: the stream decodes every record's qualities (FFQ_F_DECODE_QUAL)%s", who, decode_why);
    if (fresh && s->cur >= 0) return fail(FFQ_E_ARG, "%s: the stream has handed out a fill already", who);
    return FFQ_OK;
}

// Push-down into the stream (the reference's user guide, doc/user-guide.rst:153-180: an entryfunc that looks at the read's
// length and builds one component of the entries it keeps): from the next fill on, ffq_stream_next hands back only the rows
// with min_seq_len <= pos3 - pos2 <= max_seq_len, in order, and -- column != 0 -- that component of every kept row as a
// packed stream (+ value_add: -33 on the quality is the Phred decode of the kept records only).
extern "C" int ffq_stream_set_filter(ffq_stream *s, int64_t min_seq_len, int64_t max_seq_len, int column, int value_add)
{
    if (!s) return fail(FFQ_E_ARG, "ffq_stream_set_filter: NULL stream");
    if (column < 0 || column > 3) return fail(FFQ_E_ARG, "ffq_stream_set_filter: column is FFQ_COL_NONE / _HEADER / _SEQUENCE / _QUALITY");
    const int rc = stream_settable(s, "ffq_stream_set_filter", DECODE_GATHERS, false);
    if (rc) return rc;
    if (s->render.on && column) return fail(FFQ_E_ARG, "ffq_stream_set_filter: a stream that renders FASTQ (ffq_stream_set_render) gathers no column");
    s->filter.on = true;
    s->filter.min = min_seq_len; s->filter.max = max_seq_len; s->filter.col = column; s->filter.add = value_add;
    return FFQ_OK;
}

// a stream without a filter gets one with unbounded length and no column: every stage behind the select finds its rows and
// ordinals where a filter leaves them
static void stream_filter_default(ffq_stream *s)
{
    if (s->filter.on) return;
    s->filter.on = true;
    s->filter.min = -LEN_UNBOUNDED; s->filter.max = LEN_UNBOUNDED; s->filter.col = 0; s->filter.add = 0;
}

// Content rules in the stream: the select of every fill judges the rows by ffq_table_select_reads -- as the trims left them,
// which is cutadapt's order -- instead of by their length alone.  Before the first fill.  A stream without a filter gets one
// with unbounded length and no column; ffq_stream_set_filter, before or behind this call, sets the bounds and the column
// and leaves the rules alone, as this call leaves those.
extern "C" int ffq_stream_set_content(ffq_stream *s, const ffq_content_rules *rules)
{
    if (!s || !rules) return fail(FFQ_E_ARG, "ffq_stream_set_content: NULL argument");
    bool on = false;
    int rc = content_arg("ffq_stream_set_content", rules, &on, nullptr);
    if (!rc) rc = stream_settable(s, "ffq_stream_set_content", DECODE_GATHERS, true);
    if (rc) return rc;
    stream_filter_default(s);
    s->content.on = true;
    s->content.rules = *rules;
    return FFQ_OK;
}

// the eight counts (FFQ_FILTER_COUNTS) of the select of the fill ffq_stream_next has just returned
extern "C" int ffq_stream_filter_counts(ffq_stream *s, int64_t counts[FFQ_FILTER_COUNTS])
{
    if (!s || !counts) return fail(FFQ_E_ARG, "ffq_stream_filter_counts: NULL argument");
    if (!s->filter.on) return fail(FFQ_E_ARG, "ffq_stream_filter_counts: the stream has no filter (ffq_stream_set_filter, ffq_stream_set_content)");
    for (int i = 0; i < FFQ_FILTER_COUNTS; i++) counts[i] = s->content.last[i];
    return FFQ_OK;
}

// Duplicate removal in the stream (include/ffq.h states the rule): the stream owns one set for its whole life.  Every fill's
// rows get their keys in FRONT of the trims, as scanned (ffq_table_seq_keys), and the rows the select kept are entered into
// the set right BEHIND it (ffq_dedup_select with the select's ordinals): a read never loses to a copy the filters dropped.
// drop == 0: counted only, every row stays.  A stream without a filter gets one with unbounded length and no column, as
// ffq_stream_set_content arranges it.  Before the first fill; not with FFQ_F_DECODE_QUAL.
extern "C" int ffq_stream_set_dedup(ffq_stream *s, int drop, int64_t expected_keys, int64_t max_bytes)
{
    if (!s) return fail(FFQ_E_ARG, "ffq_stream_set_dedup: NULL stream");
    int rc = stream_settable(s, "ffq_stream_set_dedup", DECODE_GATHERS, true);
    if (rc) return rc;
    if (s->paired) return fail(FFQ_E_ARG, "ffq_stream_set_dedup: the stream belongs to a pair (ffq_pair_set_dedup)");
    ffq_dedup *set = nullptr;
    rc = ffq_dedup_create(s->c, expected_keys, max_bytes, &set);
    if (rc) return rc;
    ffq_dedup_destroy(s->dedup.set);
    s->dedup.set = set;
    stream_filter_default(s);
    s->dedup.on = s->dedup.keys_on = true;
    s->dedup.drop = drop ? 1 : 0;
    return FFQ_OK;
}

// The six counts (FFQ_DEDUP_COUNTS) over EVERY fill up to the one ffq_stream_next has just returned: [0] to [2] summed,
// [3] to [5] the set as it stands.
extern "C" int ffq_stream_dedup_counts(ffq_stream *s, int64_t counts[FFQ_DEDUP_COUNTS])
{
    if (!s || !counts) return fail(FFQ_E_ARG, "ffq_stream_dedup_counts: NULL argument");
    if (!s->dedup.on) return fail(FFQ_E_ARG, "ffq_stream_dedup_counts: the stream does not look for duplicates (ffq_stream_set_dedup)");
    for (int i = 0; i < FFQ_DEDUP_COUNTS; i++) counts[i] = s->dedup.total[i];
    return FFQ_OK;
}

// what a round or a fill adds to the running counts
static void dedup_tally(int64_t total[FFQ_DEDUP_COUNTS], const int64_t c[FFQ_DEDUP_COUNTS])
{
    for (int i = 0; i < 3; i++) total[i] += c[i];
    for (int i = 3; i < FFQ_DEDUP_COUNTS; i++) total[i] = c[i];
}

// a device buffer of the dedup stage grown to n elements: the stream is waited for first (the old block goes away)
template <class B>
static int dedup_room(ffq_ctx *c, B &buf, int64_t n, const char *who, const char *what)
{
    if (buf.cap >= n) return FFQ_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (buf.grow(std::max<int64_t>(n, 1 << 12)) == hipSuccess) return FFQ_OK;
    return fail(FFQ_E_NOMEM, "%s: no memory for %lld %s", who, (long long)n, what);
}

// The dedup stage of a chain, over the one table of a stream's fill or the two of a round of a pair (rows[1] and keys[1] NULL
// for one): the *n rows the select kept entered into the stage's set by their keys and the select's ordinals *d_ord, the
// counts tallied.  Dropping, there is room for the rows and ordinals that remain, and rows[], *d_ord and *n are switched to
// them; counting only, nothing is copied and the chain goes on with the select's rows.  who: "ffq_stream" or "ffq_pair".
static int chain_dedup(ffq_ctx *c, const char *who, DedupStage &d, const uint64_t *const keys[2], const int64_t *rows[2], const int64_t **d_ord,
                       int64_t *n)
{
    const bool drop = d.drop != 0;
    int64_t cnt[FFQ_DEDUP_COUNTS], left = 0;
    int rc = FFQ_OK;
    for (int k = 0; k < 2 && !rc && drop; k++)
        if (rows[k]) rc = dedup_room(c, d.rows[k], 6 * *n, who, "rows behind the dedup");
    if (!rc && drop) rc = dedup_room(c, d.idx, *n, who, "ordinals behind the dedup");
    if (!rc) rc = ffq_dedup_select(d.set, keys[0], keys[1], *d_ord, *n, drop ? rows[0] : nullptr, drop ? rows[1] : nullptr,
                                   drop ? d.rows[0].p : nullptr, drop ? d.rows[1].p : nullptr, drop ? d.idx.p : nullptr, &left, drop ? 1 : 0, cnt);
    if (rc) return rc;
    dedup_tally(d.total, cnt);
    if (drop) {
        for (int k = 0; k < 2; k++)
            if (rows[k]) rows[k] = d.rows[k].p;
        *d_ord = d.idx.p; *n = left;
    }
    return FFQ_OK;
}

// Quality trimming in the stream: from the next fill on, every fill's table is trimmed in place on the device
// (ffq_table_trim_quality) right behind the scan -- in front of the filter, the column gather and the rows' copy back, so
// that all of them see the trimmed rows.  Refill and carry go by the scan's end offset, not by the table.
extern "C" int ffq_stream_set_trim(ffq_stream *s, int qual_base, int cutoff_front, int cutoff_back)
{
    if (!s) return fail(FFQ_E_ARG, "ffq_stream_set_trim: NULL stream");
    int rc = trim_arg("ffq_stream_set_trim", qual_base, cutoff_front, cutoff_back);
    if (!rc) rc = stream_settable(s, "ffq_stream_set_trim", DECODE_UNTRIMMED, true);
    if (rc) return rc;
    s->trim.on = true;
    s->trim.base = qual_base; s->trim.front = cutoff_front; s->trim.back = cutoff_back;
    return FFQ_OK;
}

// {rows changed, bases removed, rows skipped} of the fill ffq_stream_next has just returned
extern "C" int ffq_stream_trimmed(ffq_stream *s, int64_t stats[3])
{
    if (!s || !stats) return fail(FFQ_E_ARG, "ffq_stream_trimmed: NULL argument");
    if (!s->trim.on) return fail(FFQ_E_ARG, "ffq_stream_trimmed: the stream does not trim (ffq_stream_set_trim)");
    for (int i = 0; i < 3; i++) stats[i] = s->trim.last[i];
    return FFQ_OK;
}

// 3' adapter trimming in the stream: every fill's table is adapter-trimmed in place on the device (ffq_table_trim_adapter)
// right behind the quality trim (cutadapt's own order: -q first, -a on the row as that trim left it) -- in front of the
// filter, the column gather, the render and the rows' copy back.  The other rules are ffq_stream_set_trim's.
extern "C" int ffq_stream_set_adapter(ffq_stream *s, const uint8_t *adapter, int adapter_len, int err_permille, int min_overlap)
{
    if (!s) return fail(FFQ_E_ARG, "ffq_stream_set_adapter: NULL stream");
    int rc = adapter_arg("ffq_stream_set_adapter", adapter, adapter_len, err_permille, min_overlap, nullptr);
    if (!rc) rc = stream_settable(s, "ffq_stream_set_adapter", DECODE_UNTRIMMED, true);
    if (rc) return rc;
    s->adapter.on = true;
    memcpy(s->adapter.bytes, adapter, (size_t)adapter_len);
    s->adapter.len = adapter_len; s->adapter.err = err_permille; s->adapter.overlap = min_overlap;
    return FFQ_OK;
}

// {rows changed, bases removed, rows skipped} by the adapter step of the fill ffq_stream_next has just returned
extern "C" int ffq_stream_adapter_trimmed(ffq_stream *s, int64_t stats[3])
{
    if (!s || !stats) return fail(FFQ_E_ARG, "ffq_stream_adapter_trimmed: NULL argument");
    if (!s->adapter.on) return fail(FFQ_E_ARG, "ffq_stream_adapter_trimmed: the stream trims no adapter (ffq_stream_set_adapter)");
    for (int i = 0; i < 3; i++) stats[i] = s->adapter.last[i];
    return FFQ_OK;
}

// Fixed trims and sliding-window cutting in the stream: every fill's table goes through ffq_table_trim_ends in place on the
// device, behind the statistics IN and in front of the quality trim and every trim behind that (fastp's order).  Per mate, in
// front of a pair's overlap.  The other rules are ffq_stream_set_trim's.
extern "C" int ffq_stream_set_ends(ffq_stream *s, const ffq_ends_rules *rules)
{
    if (!s) return fail(FFQ_E_ARG, "ffq_stream_set_ends: NULL stream");
    int rc = ends_arg("ffq_stream_set_ends", rules, nullptr);
    if (!rc) rc = stream_settable(s, "ffq_stream_set_ends", DECODE_UNTRIMMED, true);
    if (rc) return rc;
    s->ends.on = true;
    s->ends.rules = *rules;
    return FFQ_OK;
}

// {rows changed, bases removed, rows skipped} by the ends step of the fill ffq_stream_next has just returned
extern "C" int ffq_stream_ends_trimmed(ffq_stream *s, int64_t stats[3])
{
    if (!s || !stats) return fail(FFQ_E_ARG, "ffq_stream_ends_trimmed: NULL argument");
    if (!s->ends.on) return fail(FFQ_E_ARG, "ffq_stream_ends_trimmed: the stream trims no ends (ffq_stream_set_ends)");
    for (int i = 0; i < 3; i++) stats[i] = s->ends.last[i];
    return FFQ_OK;
}

// Poly-tail trimming in the stream: every fill's table goes through ffq_table_trim_poly in place on the device -- poly-G behind
// the quality trim and in front of the adapter trim (the G tail behind an adapter spoils the adapter match), poly-X behind the
// adapter trim.  Per mate, in front of a pair's overlap (fastp runs poly-X behind its overlap trim: a departure).  The other
// rules are ffq_stream_set_trim's.
extern "C" int ffq_stream_set_poly(ffq_stream *s, int poly_g_min_len, int poly_x_min_len)
{
    if (!s) return fail(FFQ_E_ARG, "ffq_stream_set_poly: NULL stream");
    if (!poly_g_min_len && !poly_x_min_len) return fail(FFQ_E_ARG, "ffq_stream_set_poly: both steps are off");
    int rc = poly_g_min_len ? poly_arg("ffq_stream_set_poly", 2, poly_g_min_len) : FFQ_OK;
    if (!rc && poly_x_min_len) rc = poly_arg("ffq_stream_set_poly", FFQ_POLY_ANY, poly_x_min_len);
    if (!rc) rc = stream_settable(s, "ffq_stream_set_poly", DECODE_UNTRIMMED, true);
    if (rc) return rc;
    s->poly.g = poly_g_min_len; s->poly.x = poly_x_min_len;
    return FFQ_OK;
}

// {rows changed, bases removed, rows skipped} by either poly step of the fill ffq_stream_next has just returned
extern "C" int ffq_stream_poly_trimmed(ffq_stream *s, int64_t stats_g[3], int64_t stats_x[3])
{
    if (!s || !stats_g || !stats_x) return fail(FFQ_E_ARG, "ffq_stream_poly_trimmed: NULL argument");
    if (!s->poly.g && !s->poly.x) return fail(FFQ_E_ARG, "ffq_stream_poly_trimmed: the stream trims no poly tails (ffq_stream_set_poly)");
    for (int i = 0; i < 3; i++) { stats_g[i] = s->poly.last_g[i]; stats_x[i] = s->poly.last_x[i]; }
    return FFQ_OK;
}

// UMIs in the stream: every fill's table goes through ffq_table_take_umi in place on the device, in front of every trim, and the
// render puts the tag into the names (ffq_table_render_fastq_umi, the rendered rows their own source).  A single stream has
// read 1 only.  The other rules are ffq_stream_set_trim's.
extern "C" int ffq_stream_set_umi(ffq_stream *s, const ffq_umi_rules *rules)
{
    if (!s) return fail(FFQ_E_ARG, "ffq_stream_set_umi: NULL stream");
    int rc = umi_arg("ffq_stream_set_umi", rules, nullptr);
    if (!rc && rules->loc != FFQ_UMI_READ1) rc = fail(FFQ_E_ARG, "ffq_stream_set_umi: a single stream has read 1 only (loc is FFQ_UMI_READ1)");
    if (!rc && s->paired) rc = fail(FFQ_E_ARG, "ffq_stream_set_umi: a pair walks this stream (ffq_pair_set_umi)");
    if (!rc) rc = stream_settable(s, "ffq_stream_set_umi", DECODE_UNTRIMMED, true);
    if (rc) return rc;
    s->umi.on = s->umi.take = true;
    s->umi.rules = *rules;
    return FFQ_OK;
}

// {rows taken, bases removed, rows skipped, rows tagged in the output} of the fill ffq_stream_next has just returned
extern "C" int ffq_stream_umi_counts(ffq_stream *s, int64_t counts[4])
{
    if (!s || !counts) return fail(FFQ_E_ARG, "ffq_stream_umi_counts: NULL argument");
    if (!s->umi.on) return fail(FFQ_E_ARG, "ffq_stream_umi_counts: the stream takes no UMIs (ffq_stream_set_umi)");
    for (int i = 0; i < 3; i++) counts[i] = s->umi.last[i];
    counts[3] = s->umi.tagged;
    return FFQ_OK;
}

// Statistics in the stream: every fill's table is counted on the device (ffq_table_stats, accumulating, no host wait) --
// FFQ_STATS_IN right behind the scan, FFQ_STATS_OUT on the table that is rendered and copied back -- into two blocks of
// FFQ_STATS_WORDS(max_cycles) words the stream owns.
extern "C" int ffq_stream_set_stats(ffq_stream *s, int which, int qual_base, int max_cycles)
{
    if (!s) return fail(FFQ_E_ARG, "ffq_stream_set_stats: NULL stream");
    if (which < 1 || which > (FFQ_STATS_IN | FFQ_STATS_OUT)) return fail(FFQ_E_ARG, "ffq_stream_set_stats: which is FFQ_STATS_IN, FFQ_STATS_OUT or both");
    int rc = stats_arg("ffq_stream_set_stats", qual_base, max_cycles);
    if (!rc) rc = stream_settable(s, "ffq_stream_set_stats", nullptr, true);
    if (rc) return rc;
    ffq_ctx *c = s->c;
    HIPCHK(hipSetDevice(c->device));
    // (an even number of words per block: the OUT block is 16-byte aligned as well)
    const int64_t words = (FFQ_STATS_WORDS(max_cycles) + 1) & ~(int64_t)1;
    if (s->stats.d.cap < 2 * words) {
        HIPCHK(hipStreamSynchronize(c->stream));
        rc = stream_grow(s->stats.d, 2 * words, "ffq_stream: no memory for %lld words of statistics", 2 * words);
        if (rc) return rc;
    }
    HIPCHK(hipMemsetAsync(s->stats.d.p, 0, (size_t)(2 * words) * 8, c->stream));
    s->stats.which = which; s->stats.base = qual_base; s->stats.cycles = max_cycles;
    return FFQ_OK;
}

static uint64_t *stream_stats_block(ffq_stream *s, int which)
{
    const int64_t words = (FFQ_STATS_WORDS(s->stats.cycles) + 1) & ~(int64_t)1;
    return s->stats.d.p + (which == FFQ_STATS_OUT ? words : 0);
}

// the running totals of one of the blocks, over every fill handed out so far; one host wait
extern "C" int ffq_stream_stats(ffq_stream *s, int which, uint64_t *h_out, int64_t cap_words)
{
    if (!s || !h_out) return fail(FFQ_E_ARG, "ffq_stream_stats: NULL argument");
    if ((which != FFQ_STATS_IN && which != FFQ_STATS_OUT) || !(s->stats.which & which))
        return fail(FFQ_E_ARG, "ffq_stream_stats: the stream does not count that (ffq_stream_set_stats)");
    const int64_t words = FFQ_STATS_WORDS(s->stats.cycles);
    if (cap_words < words) return fail(FFQ_E_ARG, "ffq_stream_stats: the totals have %lld words, the output holds %lld", (long long)words,
                                       (long long)cap_words);
    ffq_ctx *c = s->c;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(h_out, stream_stats_block(s, which), (size_t)words * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FFQ_OK;
}

// Rendering in the stream: from the first fill on, the rows ffq_stream_next hands out -- trimmed (ffq_stream_set_trim) and
// filtered (ffq_stream_set_filter, without a column) first, if the stream does that -- are rendered as FASTQ text on the
// device (ffq_table_render_fastq) and the text is copied back to pinned memory beside the rows.
extern "C" int ffq_stream_set_render(ffq_stream *s)
{
    if (!s) return fail(FFQ_E_ARG, "ffq_stream_set_render: NULL stream");
    int rc = stream_settable(s, "ffq_stream_set_render", DECODE_TEXT, false);
    if (rc) return rc;
    if (s->filter.on && s->filter.col) return fail(FFQ_E_ARG, "ffq_stream_set_render: the stream's filter gathers a column (ffq_stream_set_filter: "
                                                               "column != FFQ_COL_NONE); a stream that renders FASTQ gathers none");
    rc = stream_settable(s, "ffq_stream_set_render", nullptr, true);
    if (rc) return rc;
    s->render.on = true;
    return FFQ_OK;
}

// FASTQ text of the fill ffq_stream_next has just returned and {bytes rendered, rows rendered, rows skipped}; pinned
// memory, valid until the next call.
extern "C" int ffq_stream_rendered(ffq_stream *s, const uint8_t **h_fastq, int64_t *n_fastq_bytes, int64_t stats[3])
{
    if (!s || !h_fastq || !n_fastq_bytes) return fail(FFQ_E_ARG, "ffq_stream_rendered: NULL argument");
    if (!s->render.on) return fail(FFQ_E_ARG, "ffq_stream_rendered: the stream does not render (ffq_stream_set_render)");
    *h_fastq = s->compress.on ? nullptr : s->b->ren.h.p;      // (compressed: the text never leaves the device)
    *n_fastq_bytes = s->render.last[0];
    if (stats) for (int i = 0; i < 3; i++) stats[i] = s->render.last[i];
    return FFQ_OK;
}

// Compression in a stream that renders (before the first ffq_stream_next): every fill's text is written as BGZF members on
// the device (ffq_deflate_bgzf) behind the render, and the members are copied back instead of the text.
extern "C" int ffq_stream_set_compress(ffq_stream *s, int mode)
{
    if (!s) return fail(FFQ_E_ARG, "ffq_stream_set_compress: NULL stream");
    if (mode != FFQ_COMPRESS_NONE && mode != FFQ_COMPRESS_BGZF) return fail(FFQ_E_ARG, "ffq_stream_set_compress: mode is FFQ_COMPRESS_NONE or FFQ_COMPRESS_BGZF");
    if (!s->render.on) return fail(FFQ_E_ARG, "ffq_stream_set_compress: the stream does not render (ffq_stream_set_render first)");
    const int rc = stream_settable(s, "ffq_stream_set_compress", nullptr, true);
    if (rc) return rc;
    s->compress.on = mode == FFQ_COMPRESS_BGZF;
    return FFQ_OK;
}

// the BGZF members of the fill ffq_stream_next has just returned and {bytes in, bytes out, members, members stored}; pinned
// memory, valid until the next call
extern "C" int ffq_stream_compressed(ffq_stream *s, const uint8_t **h_bgzf, int64_t *n_bytes, int64_t stats[FFQ_DEFLATE_COUNTS])
{
    if (!s || !h_bgzf || !n_bytes) return fail(FFQ_E_ARG, "ffq_stream_compressed: NULL argument");
    if (!s->compress.on) return fail(FFQ_E_ARG, "ffq_stream_compressed: the stream does not compress (ffq_stream_set_compress)");
    *h_bgzf = s->b->bgz.h; *n_bytes = s->compress.last[1];
    if (stats) for (int i = 0; i < FFQ_DEFLATE_COUNTS; i++) stats[i] = s->compress.last[i];
    return FFQ_OK;
}

// What the filter did with the fill ffq_stream_next has just returned: h_index[i] = ordinal, among the n_scanned records of
// the fill, of kept row i (the caller that owes its own caller one item per record puts the kept ones back by it); the
// gathered column: bytes of kept row i = h_col[h_coloff[i] : h_coloff[i + 1]].  Pinned memory, valid until the next call.
extern "C" int ffq_stream_selected(ffq_stream *s, const int64_t **h_index, int64_t *n_scanned, const int8_t **h_col,
                                   const int64_t **h_coloff, int64_t *n_col_bytes)
{
    if (!s || !h_index || !n_scanned) return fail(FFQ_E_ARG, "ffq_stream_selected: NULL argument");
    if (!s->filter.on) return fail(FFQ_E_ARG, "ffq_stream_selected: the stream has no filter (ffq_stream_set_filter)");
    *h_index = s->b->idx.h; *n_scanned = s->filter.scanned;
    if (h_col) *h_col = s->filter.col ? s->b->col.h : nullptr;
    if (h_coloff) *h_coloff = s->filter.col ? s->b->coff.h : nullptr;
    if (n_col_bytes) *n_col_bytes = s->filter.col_bytes;
    return FFQ_OK;
}

// ---- chunk k: wait for the feeder -------------------------------------------------------
static int stream_wait_chunk(ffq_stream *s, int64_t k)
{
    std::unique_lock<std::mutex> lk(s->m);
    s->cv.wait(lk, [&] { return s->produced > k || s->feeder_done; });
    if (s->produced > k) return FFQ_OK;
    if (s->feeder_rc) return fail(s->feeder_rc, "%s", s->feeder_msg.c_str());
    if (s->src == SRC_PUSH) { s->failed = false; return fail(FFQ_E_ARG, "ffq_stream_next: no chunk has been pushed"); }
    return fail(FFQ_E_INTERNAL, "ffq_stream: the reader stopped early");
}

// ---- take chunk k: buf = buf[offset:] + chunk (:277); the first fill: b'\n' + chunk (:245) -----------------
// The carry goes in front of the chunk (the slots grow if it needs more room); the scan stream gets its copy and the two waits.
static int stream_take(ffq_stream *s, int64_t k, Fill *f)
{
    ffq_ctx *c = s->c;
    StreamBufs *b = s->b;
    const int64_t carry = k == 0 ? 1 : s->fill_len - s->carry_from;
    if (carry > b->room) {
        int rc = stream_grow_room(s, carry);
        if (rc) return rc;
    }
    StreamSlot &sl = b->slot[k % STREAM_SLOTS];
    const int64_t room = b->room;
    if (k == 0) sl.buf.h[room - 1] = (uint8_t)'\n';
    else {
        const StreamSlot &pv = b->slot[s->cur % STREAM_SLOTS];
        memcpy(sl.buf.h + room - carry, pv.buf.h + s->fill_start + s->carry_from, (size_t)carry);
        // the previous fill's slot goes back to the feeder (the caller's pointers into it expired with this call)
        { std::lock_guard<std::mutex> lk(s->m); s->released = k; }
        s->cv.notify_all();
    }
    const int64_t start = room - carry, len = carry + sl.got, mis = start & 15;
    *f = Fill{&sl, start, len, mis, sl.eof, sl.buf.d + start - mis, len + mis, s->globaloffset - mis};
    mark_other(c);          // (a copy and two event waits go onto the scan stream in front of the scan)
    HIPCHK(hipMemcpyAsync(sl.buf.d + start, sl.buf.h + start, (size_t)carry, hipMemcpyHostToDevice, c->stream));
    if (s->prof) {          // (profiling only: the wait for the chunk's copy on its own)
        const double t = stream_now();
        HIPCHK(hipEventSynchronize(sl.copied[0]));
        HIPCHK(hipEventSynchronize(sl.copied[1]));
        s->t_copy += stream_now() - t;
    }
    HIPCHK(hipStreamWaitEvent(c->stream, sl.copied[0], 0));
    HIPCHK(hipStreamWaitEvent(c->stream, sl.copied[1], 0));
    return FFQ_OK;
}

// ---- scan: from the aligned address below the fill, searching from the fill's first byte ----
static int stream_scan(ffq_stream *s, const Fill &f, ffq_scan_result *res)
{
    StreamBufs *b = s->b;
    const bool decode = (s->flags & FFQ_F_DECODE_QUAL) != 0;
    if (decode) {
        // qualities are at most half of the bytes; the segmented layout of the single pass owns FFQ_SEG_STRIDE bytes per tile
        int64_t need = f.len / 2 + 64;
        if (s->flags & FFQ_F_SINGLE_PASS) need = std::max<int64_t>(need, ((f.n + 16383) >> 14) * (int64_t)FFQ_SEG_STRIDE);
        int rc = stream_grow(b->qual, need, "ffq_stream: no memory for %lld decoded bytes", need);
        if (rc) return rc;
    }
    memset(res, 0, sizeof *res);
    for (int attempt = 0;; attempt++) {
        int rc = ffq_scan_device(s->c, f.d_buf, f.n, 0, f.mis, f.eof ? 1 : 0, f.add, s->flags, s->qual_add, b->tab.d, stream_tab_rows(b),
                                 decode ? b->qual.d.p : nullptr, decode ? b->qual.d.cap : 0, decode ? b->qoff.d : nullptr, res);
        if (rc != FFQ_E_TABLE_FULL || attempt == 1) return rc;
        rc = stream_alloc_tab(s, res->n_records + 1024);
        if (rc) return rc;
    }
}

// ---- the two ends of a mate's chain (a fill of a single stream, either mate of a round of a pair).  front: [keys], [stats IN],
// [UMI take], [ends], [quality trim], [poly-G], [adapter], [poly-X] on the `n` scanned rows at `rows`, which the trims edit in place
static int chain_front(ffq_stream *s, const Fill &f, int64_t *rows, int64_t n)
{
    int rc = FFQ_OK;
    if (s->dedup.keys_on && n > 0) {   // (the keys of the rows as scanned: a trim moves a row's end and the table forgets the old one)
        rc = dedup_room(s->c, s->dedup.keys, n, "ffq_stream", "keys");
        if (!rc) rc = ffq_table_seq_keys(s->c, f.d_buf, f.n, 0, f.add, rows, n, s->dedup.keys.p, s->dedup.keyed);
    }
    if (!rc && (s->stats.which & FFQ_STATS_IN))
        rc = ffq_table_stats(s->c, f.d_buf, f.n, 0, f.add, rows, n, s->stats.base, s->stats.cycles, 1, stream_stats_block(s, FFQ_STATS_IN), nullptr);
    if (!rc && s->umi.take)         // (behind the keys and the statistics IN, which see the read as read; every trim sees it without its UMI)
        rc = ffq_table_take_umi(s->c, f.d_buf, f.n, 0, f.add, rows, n, s->umi.rules.len, s->umi.rules.skip, rows, s->umi.last);
    if (!rc && s->ends.on)          // (in front of every other trim: fastp's order)
        rc = ffq_table_trim_ends(s->c, f.d_buf, f.n, 0, f.add, rows, n, &s->ends.rules, rows, s->ends.last);
    if (!rc && s->trim.on)
        rc = ffq_table_trim_quality(s->c, f.d_buf, f.n, 0, f.add, rows, n, s->trim.base, s->trim.front, s->trim.back, rows, s->trim.last);
    if (!rc && s->poly.g)           // (in front of the adapter: the G tail behind an adapter spoils its match)
        rc = ffq_table_trim_poly(s->c, f.d_buf, f.n, 0, f.add, rows, n, 2, s->poly.g, rows, s->poly.last_g);
    if (!rc && s->adapter.on)       // (as the trims in front left them)
        rc = ffq_table_trim_adapter(s->c, f.d_buf, f.n, 0, f.add, rows, n, s->adapter.bytes, s->adapter.len, s->adapter.err, s->adapter.overlap, rows, s->adapter.last);
    if (!rc && s->poly.x)
        rc = ffq_table_trim_poly(s->c, f.d_buf, f.n, 0, f.add, rows, n, FFQ_POLY_ANY, s->poly.x, rows, s->poly.last_x);
    return rc;
}

// back: [stats OUT], [render + text D2H], rows D2H into the stream's tab.h, of the table that is handed out.  umi_src: of a pair
// whose names get a UMI, both mates' views of their kept rows (stream_render's src): the tag may be the other mate's, which is
// handed in here -- a mate's chain does not reach across
static int chain_back(ffq_stream *s, const Fill &f, const Table &t, const ffq_table_view *umi_src = nullptr)
{
    int rc = FFQ_OK;
    if (s->stats.which & FFQ_STATS_OUT)
        rc = ffq_table_stats(s->c, f.d_buf, f.n, 0, f.add, t.d_rows, t.n, s->stats.base, s->stats.cycles, 1, stream_stats_block(s, FFQ_STATS_OUT), nullptr);
    if (!rc && s->render.on) rc = stream_render(s, f, t, umi_src);
    if (rc) return rc;
    if (t.n > 0) HIPCHK(hipMemcpyAsync(s->b->tab.h, t.d_rows, (size_t)t.n * 48, hipMemcpyDeviceToHost, s->c->stream));
    return FFQ_OK;
}

// ---- the table chain of a fill: every stage the stream has switched on, over the fill's view, on the table the chain is
// at.  With a filter the select REPLACES that table by the kept rows (on the DEVICE, before anything is copied back: a
// dropped record costs the host nothing, doc/user-guide.rst:153-180); what follows is written once, for either table.
// This is the one place that states the order of a fill's work on the scan stream, in every configuration:
//     carry H2D, wait copied[0], wait copied[1], scan, front (the keys of the dedup first, on the rows as scanned; then
//     [stats IN], [UMI take], [ends], [quality trim], [poly-G], [adapter], [poly-X]), [select:
//     by length, or -- content rules -- by length and content (ffq_table_select_reads), on the rows as the trims left them],
//     [dedup: the kept rows entered into the stream's set by their keys and the select's ordinals, the first copies kept
//     (ffq_dedup_select) -- what follows is on the rows that remain], back, [idx D2H], [gather, col D2H, coff D2H],
//     [qual D2H, qoff D2H], synchronise
// and of a round of a pair (pair_chain): [names check], mate 1: front, room for its kept rows (stream_alloc_sel), mate 2: the
// same, room for the ordinals, [room for the merge], [the mates' overlap], [bases corrected inside it], the pair select, [the pair dedup: both tables
// compacted in step by the pairs' keys], [the merge of the kept pairs: then what follows is on the rest tables and the rest
// ordinals], mate 1: back, mate 2: back, ordinals D2H, [merged text D2H], synchronise
// No rows are copied back from an empty table; a fill without records allocates and launches nothing of the push-down,
// but statistics OUT and the render are still called (n = 0).  *n_out: the rows handed out.
// The UMI take stands behind the keys and the statistics IN and in front of every trim: keys and "before" statistics see the read
// as read -- two reads with the same sequence and different UMIs are no duplicates --, every trim, the overlap, the correction and
// the "after" statistics see it without its UMI.  A pair's names check compares the headers as read; both mates' renders put the
// same insert into their names.
static int stream_chain(ffq_stream *s, const Fill &f, const ffq_scan_result &res, int64_t *n_out)
{
    ffq_ctx *c = s->c;
    StreamBufs *b = s->b;
    Table t = {b->tab.d, res.n_records};
    s->filter.scanned = res.n_records; s->filter.col_bytes = 0;
    int rc = chain_front(s, f, b->tab.d, res.n_records);
    if (!rc && s->filter.on) {
        if (res.n_records > 0) rc = stream_alloc_sel(s, res.n_records, f.len + 64);
        t = Table{b->sel, 0};
        for (int i = 0; i < FFQ_FILTER_COUNTS; i++) s->content.last[i] = 0;
        if (!rc && res.n_records > 0) {
            if (s->content.on)
                rc = ffq_table_select_reads(c, f.d_buf, f.n, 0, f.add, b->tab.d, res.n_records, s->filter.min, s->filter.max,
                                            &s->content.rules, b->sel, b->idx.d, &t.n, s->content.last);
            else {
                rc = table_select(c, b->tab.d, res.n_records, s->filter.min, s->filter.max, b->sel, b->idx.d, &t.n);
                s->content.last[0] = t.n; s->content.last[1] = res.n_records - t.n;
            }
        }
    }
    const int64_t *d_idx = b->idx.d;
    if (!rc && s->dedup.on && t.n > 0) {
        const uint64_t *const keys[2] = {s->dedup.keys.p, nullptr};
        const int64_t *rows[2] = {t.d_rows, nullptr};
        rc = chain_dedup(c, "ffq_stream", s->dedup, keys, rows, &d_idx, &t.n);
        t.d_rows = rows[0];
    }
    if (!rc) rc = chain_back(s, f, t);
    if (rc) return rc;
    if (s->filter.on && t.n > 0) HIPCHK(hipMemcpyAsync(b->idx.h, d_idx, (size_t)t.n * 8, hipMemcpyDeviceToHost, c->stream));
    if (s->filter.on && s->filter.col && res.n_records > 0) {
        static const int COLS[4][3] = {{0, 0, 0}, {0, 1, 1}, {2, 0, 3}, {4, 0, 5}};       // header: buf[pos0 + 1 : pos1] (:161-171)
        const int *col = COLS[s->filter.col];
        int64_t nb = 0;
        rc = ffq_table_gather_column(c, f.d_buf, f.n, 0, f.add, t.d_rows, t.n, col[0], col[1], col[2], s->filter.add, b->col.d, b->col.d.cap,
                                     b->coff.d, &nb);
        if (rc) return rc;
        s->filter.col_bytes = nb;
        if (nb > 0) HIPCHK(hipMemcpyAsync(b->col.h, b->col.d, (size_t)nb, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(b->coff.h, b->coff.d, (size_t)(t.n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    }
    *n_out = t.n;
    return FFQ_OK;
}

// ---- the two pieces of a fill that ffq_stream_next and the pair walk (ffq_pair_next) share ---------------------------------
// advance: the stream's next chunk waited for, taken behind the carry and scanned -- the fill and the scan's result
static int stream_advance(ffq_stream *s, Fill *f, ffq_scan_result *res)
{
    const int64_t k = s->cur + 1;
    const double tp0 = s->prof ? stream_now() : 0;
    int rc = stream_wait_chunk(s, k);
    const double tp1 = s->prof ? stream_now() : 0;
    if (!rc) rc = stream_take(s, k, f);
    if (!rc) rc = stream_scan(s, *f, res);
    if (s->prof) { s->t_feed += tp1 - tp0; s->t_scan += stream_now() - tp1; }
    return rc;
}

// finish: the fill is handed out -- the stream remembers it, ends (*err_offset: the byte an error state names, else -1) or
// sets up the refill: buf = buf[offset:] + next chunk (:277), globaloffset += offset (:275)
static void stream_finish(ffq_stream *s, const Fill &f, const ffq_scan_result &res, int64_t *err_offset)
{
    s->cur += 1;
    s->handed_pos = f.sl->end_pos;
    s->fill_start = f.start; s->fill_len = f.len;
    const int64_t ds = res.end_offset - f.mis;             // the iterator's `offset` at exit, fill-relative
    *err_offset = -1;
    if (res.end_state != FFQ_END_REFILL) {
        if (res.end_state != FFQ_END_OK) *err_offset = s->globaloffset + ds;
        s->done = true;
        stream_stop_feeder(s);
        return;
    }
    s->carry_from = ds;
    s->globaloffset += ds;
}

extern "C" int ffq_stream_next(ffq_stream *s, const int64_t **h_rows, int64_t *n_rows, int *end_state,
                               int64_t *err_offset, const uint8_t **h_bytes, int64_t *n_bytes,
                               int64_t *bytes_offset)
{
    if (!s || !h_rows || !n_rows || !end_state) return fail(FFQ_E_ARG, "ffq_stream_next: NULL argument");
    if (s->paired) return fail(FFQ_E_ARG, "ffq_stream_next: the stream belongs to a pair (ffq_pair_open): ffq_pair_next walks it");
    ffq_ctx *c = s->c;
    StreamBufs *b = s->b;
    HIPCHK(hipSetDevice(c->device));
    *h_rows = b->tab.h; *n_rows = 0; *end_state = FFQ_END_OK;
    if (err_offset) *err_offset = -1;
    if (h_bytes) *h_bytes = nullptr;
    if (n_bytes) *n_bytes = 0;
    if (bytes_offset) *bytes_offset = 0;
    if (s->failed) return fail(FFQ_E_ARG, "ffq_stream_next: the stream has failed");
    if (s->done) return FFQ_OK;
    s->failed = true;                    // until this call gets through: an error leaves no half-advanced state behind

    Fill f;
    ffq_scan_result res;
    int64_t n_out = 0;
    int rc = stream_advance(s, &f, &res);
    const double tp2 = s->prof ? stream_now() : 0;
    if (!rc) rc = stream_chain(s, f, res, &n_out);
    if (rc) return rc;
    // ---- the decoded qualities' copies, the one wait of the fill, and what the caller is told ----
    s->last_path = res.path;
    s->last_nq = 0;
    if (s->flags & FFQ_F_DECODE_QUAL) {
        s->last_nq = res.n_qual_bytes;
        if (res.n_qual_bytes > 0)
            HIPCHK(hipMemcpyAsync(b->qual.h, b->qual.d, (size_t)res.n_qual_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(b->qoff.h, b->qoff.d, (size_t)(res.n_records + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    if (s->prof) s->t_rows += stream_now() - tp2;

    *h_rows = b->tab.h;
    *n_rows = n_out;
    if (h_bytes) *h_bytes = f.sl->buf.h + f.start;
    if (n_bytes) *n_bytes = f.len;
    // byte i of this fill is stream offset globaloffset + i (the sentinel of the first fill is -1)
    if (bytes_offset) *bytes_offset = s->globaloffset;
    *end_state = res.end_state;
    int64_t err = -1;
    stream_finish(s, f, res, &err);
    if (err_offset) *err_offset = err;
    s->failed = false;
    return FFQ_OK;
}

// ---- two streams whose records are mates: ffq_pair (include/ffq.h; the bookkeeping is csrc/ffq_pairwalk.h) ------------------
static_assert(WALK_END_OK == FFQ_END_OK && WALK_END_REFILL == FFQ_END_REFILL && WALK_END_ERR_PAIR_COUNT == FFQ_END_ERR_PAIR_COUNT &&
              WALK_END_ERR_PAIR_NAMES == FFQ_END_ERR_PAIR_NAMES, "include/ffq.h");

struct PairMate {
    ffq_stream *s = nullptr;
    Fill f = {};                 // the fill its window lies in
    bool have = false;
    int64_t bytes_offset = 0;    // byte i of that fill is stream offset bytes_offset + i
};

struct ffq_pair {
    ffq_ctx *c = nullptr;
    PairMate m[2];
    PairWalk w;
    int mode = FFQ_PAIR_ANY;
    bool check_names = true, failed = false;
    Mirror<int64_t> idx;         // the ordinals, among the round's pairs, of the kept ones
    int64_t last_pairs[5] = {0, 0, 0, 0, 0};
    int64_t last_out = 0;
    bool started = false;        // ffq_pair_next has been called: the setters are refused
    // the mates' overlap analysed, and cut by, in every round (ffq_pair_set_overlap): the insert sizes summed over the rounds
    // on the device, the six counts of the last round
    struct { bool on = false; ffq_overlap_rules rules = {}; DevBuf<uint64_t> hist; int64_t last[FFQ_OVERLAP_COUNTS] = {0, 0, 0, 0, 0, 0}; } overlap;
    // the kept pairs merged where the rule allows it (ffq_pair_set_merge): the round's insert sizes, the rows and ordinals of the
    // kept pairs that are not merged (what the round hands out then), the merged text and the six counts of the last round
    struct {
        bool on = false;
        DevBuf<int32_t> insert;
        DevBuf<int64_t> rest[2];
        Mirror<int64_t> ord;
        Mirror<uint8_t> text;
        int64_t last[FFQ_MERGE_COUNTS] = {0, 0, 0, 0, 0, 0};
        // the merged text as BGZF members (ffq_pair_set_compress), which go back in its place
        bool compress = false;
        Mirror<uint8_t> bgz;
        int64_t zlast[FFQ_DEFLATE_COUNTS] = {0, 0, 0, 0};
    } merge;
    // duplicate pairs dropped behind the pair select (ffq_pair_set_dedup): the pair's own set, the rows of both mates and the
    // ordinals that remain, the counts summed over the rounds
    DedupStage dedup;
    // bases corrected inside the overlap, in both fills' device bytes (ffq_pair_set_correct): between the overlap and the pair
    // select, by the round's insert sizes (merge.insert, which is then allocated without merging too); the six counts of the last
    // round, the matrix summed over the rounds
    struct {
        bool on = false;
        ffq_correct_rules rules = {};
        int64_t last[FFQ_CORRECT_COUNTS] = {0, 0, 0, 0, 0, 0};
        int64_t matrix[FFQ_CORRECT_MATRIX_WORDS] = {0};
    } correct;
};

extern "C" int ffq_pair_open(ffq_stream *mate1, ffq_stream *mate2, int pair_filter, int check_names, ffq_pair **out)
{
    if (!mate1 || !mate2 || !out || mate1 == mate2) return fail(FFQ_E_ARG, "ffq_pair_open: two streams and a place for the pair");
    *out = nullptr;
    if (pair_filter != FFQ_PAIR_ANY && pair_filter != FFQ_PAIR_BOTH && pair_filter != FFQ_PAIR_FIRST)
        return fail(FFQ_E_ARG, "ffq_pair_open: pair_filter is FFQ_PAIR_ANY, FFQ_PAIR_BOTH or FFQ_PAIR_FIRST");
    if (mate1->c != mate2->c) return fail(FFQ_E_ARG, "ffq_pair_open: the two streams are on different contexts");
    ffq_stream *st[2] = {mate1, mate2};
    for (int k = 0; k < 2; k++) {
        ffq_stream *s = st[k];
        if (s->paired) return fail(FFQ_E_ARG, "ffq_pair_open: mate %d belongs to a pair already", k + 1);
        if (s->cur >= 0 || s->done || s->failed) return fail(FFQ_E_ARG, "ffq_pair_open: mate %d is not a fresh stream", k + 1);
        if (s->flags & FFQ_F_DECODE_QUAL) return fail(FFQ_E_ARG, "ffq_pair_open: mate %d decodes every record's qualities (FFQ_F_DECODE_QUAL)", k + 1);
        if (s->filter.on && s->filter.col) return fail(FFQ_E_ARG, "ffq_pair_open: mate %d's filter gathers a column", k + 1);
        if (s->dedup.on) return fail(FFQ_E_ARG, "ffq_pair_open: mate %d has a dedup of its own (ffq_stream_set_dedup); a pair's is ffq_pair_set_dedup", k + 1);
    }
    ffq_pair *p = new (std::nothrow) ffq_pair();
    if (!p) return fail(FFQ_E_NOMEM, "out of host memory");
    p->c = mate1->c; p->mode = pair_filter; p->check_names = check_names != 0;
    for (int k = 0; k < 2; k++) { p->m[k].s = st[k]; st[k]->paired = true; }
    *out = p;
    return FFQ_OK;
}

extern "C" void ffq_pair_close(ffq_pair *p)
{
    if (!p) return;
    if (p->c && p->c->stream) (void)hipStreamSynchronize(p->c->stream);      // (the index buffer goes away)
    ffq_dedup_destroy(p->dedup.set);
    delete p;
}

extern "C" int ffq_pair_set_overlap(ffq_pair *p, const ffq_overlap_rules *rules)
{
    if (!p) return fail(FFQ_E_ARG, "ffq_pair_set_overlap: NULL pair");
    if (p->started) return fail(FFQ_E_ARG, "ffq_pair_set_overlap: the walk has begun (call it before the first ffq_pair_next)");
    if (!rules) { p->overlap.on = p->merge.on = p->correct.on = false; return FFQ_OK; }       // (no insert sizes: nothing to merge or correct by)
    int rc = overlap_arg("ffq_pair_set_overlap", rules);
    if (rc) return rc;
    ffq_ctx *c = p->c;
    HIPCHK(hipSetDevice(c->device));
    if (p->overlap.hist.cap < FFQ_OVERLAP_HIST_WORDS) {
        HIPCHK(hipStreamSynchronize(c->stream));
        rc = stream_grow(p->overlap.hist, (int64_t)FFQ_OVERLAP_HIST_WORDS, "ffq_pair: no memory for %lld words of insert sizes",
                         (int64_t)FFQ_OVERLAP_HIST_WORDS);
        if (rc) return rc;
    }
    HIPCHK(hipMemsetAsync(p->overlap.hist.p, 0, (size_t)FFQ_OVERLAP_HIST_WORDS * 8, c->stream));
    p->overlap.rules = *rules;
    p->overlap.on = true;
    return FFQ_OK;
}

// the last round's six counts, and the insert sizes of every round so far; one host wait
extern "C" int ffq_pair_overlap(ffq_pair *p, int64_t counts[FFQ_OVERLAP_COUNTS], uint64_t *h_hist, int64_t cap_words)
{
    if (!p || !counts) return fail(FFQ_E_ARG, "ffq_pair_overlap: NULL argument");
    if (!p->overlap.on) return fail(FFQ_E_ARG, "ffq_pair_overlap: the pair does not analyse overlaps (ffq_pair_set_overlap)");
    for (int i = 0; i < FFQ_OVERLAP_COUNTS; i++) counts[i] = p->overlap.last[i];
    if (!h_hist) return FFQ_OK;
    if (cap_words < FFQ_OVERLAP_HIST_WORDS)
        return fail(FFQ_E_ARG, "ffq_pair_overlap: the insert sizes have %d words, the output holds %lld", FFQ_OVERLAP_HIST_WORDS, (long long)cap_words);
    ffq_ctx *c = p->c;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(h_hist, p->overlap.hist.p, (size_t)FFQ_OVERLAP_HIST_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FFQ_OK;
}

extern "C" int ffq_pair_set_merge(ffq_pair *p, int on)
{
    if (!p) return fail(FFQ_E_ARG, "ffq_pair_set_merge: NULL pair");
    if (p->started) return fail(FFQ_E_ARG, "ffq_pair_set_merge: the walk has begun (call it before the first ffq_pair_next)");
    if (on && !p->overlap.on) return fail(FFQ_E_ARG, "ffq_pair_set_merge: the pair does not analyse overlaps (ffq_pair_set_overlap first)");
    if (on && p->m[0].s->umi.on) return fail(FFQ_E_ARG, "ffq_pair_set_merge: the pair puts UMIs into the names (ffq_pair_set_umi); a merged read's header is not tagged");
    p->merge.on = on != 0;
    return FFQ_OK;
}

// the last round's merged text and its six counts
extern "C" int ffq_pair_merged(ffq_pair *p, const uint8_t **h_text, int64_t *n_bytes, int64_t counts[FFQ_MERGE_COUNTS])
{
    if (!p || !h_text || !n_bytes) return fail(FFQ_E_ARG, "ffq_pair_merged: NULL argument");
    if (!p->merge.on) return fail(FFQ_E_ARG, "ffq_pair_merged: the pair does not merge (ffq_pair_set_merge)");
    *h_text = p->merge.compress ? nullptr : p->merge.text.h.p;      // (compressed: the text never leaves the device)
    *n_bytes = p->merge.last[2];
    if (counts) for (int i = 0; i < FFQ_MERGE_COUNTS; i++) counts[i] = p->merge.last[i];
    return FFQ_OK;
}

// the merged text of every round as BGZF members (ffq_stream_set_compress's way; the mates' own text is their streams' business)
extern "C" int ffq_pair_set_compress(ffq_pair *p, int mode)
{
    if (!p) return fail(FFQ_E_ARG, "ffq_pair_set_compress: NULL pair");
    if (mode != FFQ_COMPRESS_NONE && mode != FFQ_COMPRESS_BGZF) return fail(FFQ_E_ARG, "ffq_pair_set_compress: mode is FFQ_COMPRESS_NONE or FFQ_COMPRESS_BGZF");
    if (p->started) return fail(FFQ_E_ARG, "ffq_pair_set_compress: the walk has begun (call it before the first ffq_pair_next)");
    if (!p->merge.on) return fail(FFQ_E_ARG, "ffq_pair_set_compress: the pair does not merge (ffq_pair_set_merge first)");
    p->merge.compress = mode == FFQ_COMPRESS_BGZF;
    return FFQ_OK;
}

// the last round's merged text as BGZF members and {bytes in, bytes out, members, members stored}
extern "C" int ffq_pair_merged_bgzf(ffq_pair *p, const uint8_t **h_bgzf, int64_t *n_bytes, int64_t stats[FFQ_DEFLATE_COUNTS])
{
    if (!p || !h_bgzf || !n_bytes) return fail(FFQ_E_ARG, "ffq_pair_merged_bgzf: NULL argument");
    if (!p->merge.compress) return fail(FFQ_E_ARG, "ffq_pair_merged_bgzf: the pair does not compress its merged reads (ffq_pair_set_compress)");
    *h_bgzf = p->merge.bgz.h; *n_bytes = p->merge.zlast[1];
    if (stats) for (int i = 0; i < FFQ_DEFLATE_COUNTS; i++) stats[i] = p->merge.zlast[i];
    return FFQ_OK;
}

// Bases corrected inside the mates' overlap in every round (include/ffq.h, ffq_table_pair_correct), by the round's insert sizes.
extern "C" int ffq_pair_set_correct(ffq_pair *p, const ffq_correct_rules *rules)
{
    if (!p) return fail(FFQ_E_ARG, "ffq_pair_set_correct: NULL pair");
    if (p->started) return fail(FFQ_E_ARG, "ffq_pair_set_correct: the walk has begun (call it before the first ffq_pair_next)");
    if (!rules) { p->correct.on = false; return FFQ_OK; }
    if (!p->overlap.on) return fail(FFQ_E_ARG, "ffq_pair_set_correct: the pair does not analyse overlaps (ffq_pair_set_overlap first)");
    const int rc = correct_arg("ffq_pair_set_correct", rules);
    if (rc) return rc;
    p->correct.rules = *rules;
    p->correct.on = true;
    for (int64_t &x : p->correct.matrix) x = 0;
    return FFQ_OK;
}

// the last round's six counts, and the corrections of every round so far by kind
extern "C" int ffq_pair_corrected(ffq_pair *p, int64_t counts[FFQ_CORRECT_COUNTS], int64_t matrix[FFQ_CORRECT_MATRIX_WORDS])
{
    if (!p) return fail(FFQ_E_ARG, "ffq_pair_corrected: NULL pair");
    if (!p->correct.on) return fail(FFQ_E_ARG, "ffq_pair_corrected: the pair does not correct (ffq_pair_set_correct)");
    if (counts) for (int i = 0; i < FFQ_CORRECT_COUNTS; i++) counts[i] = p->correct.last[i];
    if (matrix) for (int i = 0; i < FFQ_CORRECT_MATRIX_WORDS; i++) matrix[i] = p->correct.matrix[i];
    return FFQ_OK;
}

// Duplicate PAIRS dropped (include/ffq.h: the pair key): the pair owns the set; both mates' fronts compute their keys over the
// round's window, and the kept pairs of the pair select are entered by their pair keys, in front of the merge.
extern "C" int ffq_pair_set_dedup(ffq_pair *p, int drop, int64_t expected_keys, int64_t max_bytes)
{
    if (!p) return fail(FFQ_E_ARG, "ffq_pair_set_dedup: NULL pair");
    if (p->started) return fail(FFQ_E_ARG, "ffq_pair_set_dedup: the walk has begun (call it before the first ffq_pair_next)");
    for (int k = 0; k < 2; k++)
        if (p->m[k].s->dedup.on) return fail(FFQ_E_ARG, "ffq_pair_set_dedup: mate %d has a dedup of its own (ffq_stream_set_dedup)", k + 1);
    ffq_dedup *set = nullptr;
    const int rc = ffq_dedup_create(p->c, expected_keys, max_bytes, &set);
    if (rc) return rc;
    ffq_dedup_destroy(p->dedup.set);
    p->dedup.set = set;
    p->dedup.on = true;
    p->dedup.drop = drop ? 1 : 0;
    for (int k = 0; k < 2; k++) p->m[k].s->dedup.keys_on = true;
    return FFQ_OK;
}

// the six counts over every round so far (ffq_stream_dedup_counts' way), in pairs
extern "C" int ffq_pair_dedup_counts(ffq_pair *p, int64_t counts[FFQ_DEDUP_COUNTS])
{
    if (!p || !counts) return fail(FFQ_E_ARG, "ffq_pair_dedup_counts: NULL argument");
    if (!p->dedup.on) return fail(FFQ_E_ARG, "ffq_pair_dedup_counts: the pair does not look for duplicates (ffq_pair_set_dedup)");
    for (int i = 0; i < FFQ_DEDUP_COUNTS; i++) counts[i] = p->dedup.total[i];
    return FFQ_OK;
}

// UMIs of a pair (include/ffq.h): the take runs in the front of the mate or mates the location names, and BOTH mates' renders
// put the same insert into their names, each from the kept rows of the mate that carries the tag.  Not with merging: the merged
// read's header is written by ffq_merge.h.
extern "C" int ffq_pair_set_umi(ffq_pair *p, const ffq_umi_rules *rules)
{
    if (!p) return fail(FFQ_E_ARG, "ffq_pair_set_umi: NULL pair");
    if (p->started) return fail(FFQ_E_ARG, "ffq_pair_set_umi: the walk has begun (call it before the first ffq_pair_next)");
    int rc = umi_arg("ffq_pair_set_umi", rules, nullptr);
    if (!rc && p->merge.on) rc = fail(FFQ_E_ARG, "ffq_pair_set_umi: the pair merges (ffq_pair_set_merge); a merged read's header is not tagged");
    for (int k = 0; k < 2 && !rc; k++) rc = stream_settable(p->m[k].s, "ffq_pair_set_umi", DECODE_UNTRIMMED, true);
    if (rc) return rc;
    for (int k = 0; k < 2; k++) {
        ffq_stream *s = p->m[k].s;
        s->umi.on = true;
        s->umi.take = rules->loc == FFQ_UMI_PER_READ || rules->loc == (k == 0 ? FFQ_UMI_READ1 : FFQ_UMI_READ2);
        s->umi.rules = *rules;
    }
    return FFQ_OK;
}

// ffq_stream_umi_counts of both mates for the round ffq_pair_next has just returned (a mate the location does not name takes nothing)
extern "C" int ffq_pair_umi_counts(ffq_pair *p, int64_t counts1[4], int64_t counts2[4])
{
    if (!p || !counts1 || !counts2) return fail(FFQ_E_ARG, "ffq_pair_umi_counts: NULL argument");
    if (!p->m[0].s->umi.on) return fail(FFQ_E_ARG, "ffq_pair_umi_counts: the pair takes no UMIs (ffq_pair_set_umi)");
    int rc = ffq_stream_umi_counts(p->m[0].s, counts1);
    if (!rc) rc = ffq_stream_umi_counts(p->m[1].s, counts2);
    return rc;
}

extern "C" int ffq_pair_wants(ffq_pair *p) { return p && !p->failed ? walk_wants(p->w) : 0; }

// what the per-stream accessors report for a round: zero until the round's chain says otherwise
static void pair_clear_last(ffq_stream *s)
{
    for (int i = 0; i < 3; i++) s->ends.last[i] = s->trim.last[i] = s->adapter.last[i] = s->poly.last_g[i] = s->poly.last_x[i] = s->render.last[i] = 0;
    for (int64_t &x : s->compress.last) x = 0;
    for (int i = 0; i < 3; i++) s->umi.last[i] = 0;
    s->umi.tagged = 0;
    for (int i = 0; i < FFQ_FILTER_COUNTS; i++) s->content.last[i] = 0;
    s->filter.scanned = 0; s->filter.col_bytes = 0;
}

// The end of a merging round's chain, behind the pair select (and the pair dedup): the `kept` pairs of both tables `rows` merged
// by the insert sizes of their ordinals `d_ord`, the two ends of the mates' chains on the rest tables, the rest ordinals and the merged text copied back.
static int pair_chain_merge(ffq_pair *p, const int64_t *const rows[2], const int64_t *d_ord, int64_t kept, int64_t *n_out)
{
    ffq_ctx *c = p->c;
    ffq_table_view v[2];
    for (int k = 0; k < 2; k++) v[k] = ffq_table_view{p->m[k].f.d_buf, p->m[k].f.n, 0, p->m[k].f.add, rows[k]};
    int64_t n_rest = 0;
    int rc = ffq_table_pair_merge(c, &v[0], &v[1], kept, p->merge.insert.p, d_ord, p->merge.text.d, p->merge.text.d.cap, nullptr,
                                  p->merge.rest[0].p, p->merge.rest[1].p, p->merge.ord.d, &n_rest, p->merge.last);
    if (rc == FFQ_E_TABLE_FULL)
        return fail(FFQ_E_INTERNAL, "ffq_pair: fills of %lld and %lld bytes merged to %lld", (long long)v[0].n_bytes, (long long)v[1].n_bytes,
                    (long long)p->merge.last[2]);
    for (int k = 0; k < 2 && !rc; k++) rc = chain_back(p->m[k].s, p->m[k].f, Table{p->merge.rest[k].p, n_rest});
    if (rc) return rc;
    if (n_rest > 0) HIPCHK(hipMemcpyAsync(p->merge.ord.h, p->merge.ord.d, (size_t)n_rest * 8, hipMemcpyDeviceToHost, c->stream));
    if (p->merge.compress) {
        int64_t *z = p->merge.zlast;
        rc = ffq_deflate_bgzf(c, p->merge.text.d, p->merge.last[2], p->merge.bgz.d, p->merge.bgz.d.cap, nullptr, z);
        if (rc == FFQ_E_TABLE_FULL)
            return fail(FFQ_E_INTERNAL, "ffq_pair: %lld merged bytes deflated to %lld", (long long)p->merge.last[2], (long long)z[1]);
        if (rc) return rc;
        if (z[1] > 0) HIPCHK(hipMemcpyAsync(p->merge.bgz.h, p->merge.bgz.d, (size_t)z[1], hipMemcpyDeviceToHost, c->stream));
    } else if (p->merge.last[2] > 0) {
        HIPCHK(hipMemcpyAsync(p->merge.text.h, p->merge.text.d, (size_t)p->merge.last[2], hipMemcpyDeviceToHost, c->stream));
    }
    *n_out = n_rest;
    return FFQ_OK;
}

// The table chain of a round over the slices [lo, lo + m) of both mates' fills, in the order stated above stream_chain (the overlap
// edits both slices in place, the pair select writes each stream's own `sel`).  *differ: the names check found a different pair
// (its ordinal in the round), nothing else was done.
static int pair_chain(ffq_pair *p, int64_t m, int64_t *n_out, int64_t *differ)
{
    ffq_ctx *c = p->c;
    ffq_table_view v[2];
    for (int k = 0; k < 2; k++) {
        const PairMate &pm = p->m[k];
        v[k] = ffq_table_view{pm.f.d_buf, pm.f.n, 0, pm.f.add, pm.s->b->tab.d.p + 6 * p->w.m[k].lo};
    }
    *n_out = 0; *differ = -1;
    int rc = FFQ_OK;
    if (p->check_names) {
        int64_t names[4];
        rc = ffq_table_pair_names(c, &v[0], &v[1], m, names);
        if (rc) return rc;
        if (names[1] > 0) { *differ = names[3]; return FFQ_OK; }
    }
    int64_t bounds[4];              // (a stream without a filter counts as unbounded and ruleless)
    const ffq_content_rules *rules[2];
    for (int k = 0; k < 2 && !rc; k++) {
        ffq_stream *s = p->m[k].s;
        rc = chain_front(s, p->m[k].f, const_cast<int64_t *>(v[k].d_table), m);
        if (!rc) rc = stream_alloc_sel(s, m, 0);
        bounds[2 * k] = s->filter.on ? s->filter.min : -LEN_UNBOUNDED;
        bounds[2 * k + 1] = s->filter.on ? s->filter.max : LEN_UNBOUNDED;
        rules[k] = s->content.on ? &s->content.rules : nullptr;
        s->filter.scanned = m;
    }
    if (!rc && p->idx.d.cap < m) {
        HIPCHK(hipStreamSynchronize(c->stream));
        rc = stream_grow(p->idx, m, "ffq_pair: no memory for %lld selected pairs", m);
    }
    int32_t *d_insert = nullptr;
    if (!rc && p->correct.on) {
        // (the correction needs the insert sizes even where nothing is merged)
        if (p->merge.insert.cap < m) {
            HIPCHK(hipStreamSynchronize(c->stream));
            rc = stream_grow(p->merge.insert, m, "ffq_pair: no memory for %lld insert sizes", m);
        }
        d_insert = p->merge.insert.p;
    }
    if (!rc && p->merge.on) {
        // (the merged text of a pair is shorter than its two records together: header + 2 (n1 + n2 - 1) + 6 bytes)
        const int64_t text_cap = p->m[0].f.n + p->m[1].f.n + 64;
        if (p->merge.insert.cap < m || p->merge.rest[0].cap < 6 * m || p->merge.rest[1].cap < 6 * m || p->merge.ord.d.cap < m ||
            p->merge.text.d.cap < text_cap || (p->merge.compress && p->merge.bgz.d.cap < ffq_deflate_bgzf_bound(text_cap))) {
            HIPCHK(hipStreamSynchronize(c->stream));
            rc = stream_grow(p->merge.insert, m, "ffq_pair: no memory for %lld insert sizes", m);
            for (int k = 0; k < 2 && !rc; k++) rc = stream_grow(p->merge.rest[k], 6 * m, "ffq_pair: no memory for %lld unmerged rows", m);
            if (!rc) rc = stream_grow(p->merge.ord, m, "ffq_pair: no memory for %lld unmerged pairs", m);
            if (!rc) rc = stream_grow(p->merge.text, text_cap, "ffq_pair: no memory for %lld merged bytes", text_cap);
            if (!rc && p->merge.compress)
                rc = stream_grow(p->merge.bgz, ffq_deflate_bgzf_bound(text_cap), "ffq_pair: no memory for %lld compressed bytes", ffq_deflate_bgzf_bound(text_cap));
        }
        d_insert = p->merge.insert.p;
    }
    if (!rc && p->overlap.on)
        rc = ffq_table_pair_overlap(c, &v[0], &v[1], m, &p->overlap.rules, const_cast<int64_t *>(v[0].d_table), const_cast<int64_t *>(v[1].d_table),
                                    d_insert, p->overlap.hist.p, 1, p->overlap.last);
    if (!rc && p->correct.on) {
        // (both fills' device bytes are edited: the filter, statistics OUT, the render and the merge behind this see the corrected
        // bytes; statistics IN and the dedup keys were taken by chain_front, and the pinned host copy stays as read)
        int64_t mat[FFQ_CORRECT_MATRIX_WORDS];
        rc = ffq_table_pair_correct(c, &v[0], &v[1], m, d_insert, &p->correct.rules, p->correct.last, mat);
        for (int i = 0; i < FFQ_CORRECT_MATRIX_WORDS && !rc; i++) p->correct.matrix[i] += mat[i];
    }
    int64_t kept = 0;
    if (!rc) rc = ffq_table_select_pairs(c, &v[0], &v[1], m, bounds, rules[0], rules[1], p->mode, p->m[0].s->b->sel, p->m[1].s->b->sel,
                                         p->idx.d, &kept, p->m[0].s->content.last, p->m[1].s->content.last, p->last_pairs);
    const int64_t *rows[2] = {p->m[0].s->b->sel.p, p->m[1].s->b->sel.p}, *d_ord = p->idx.d;
    if (!rc && p->dedup.on && kept > 0) {
        const uint64_t *const keys[2] = {p->m[0].s->dedup.keys.p, p->m[1].s->dedup.keys.p};
        rc = chain_dedup(c, "ffq_pair", p->dedup, keys, rows, &d_ord, &kept);
    }
    if (!rc && p->merge.on) return pair_chain_merge(p, rows, d_ord, kept, n_out);
    if (p->m[0].s->umi.on) {
        // (a pair with UMIs: either mate's render is handed both mates' kept rows, which are in step)
        ffq_table_view uv[2];
        for (int k = 0; k < 2; k++) uv[k] = ffq_table_view{p->m[k].f.d_buf, p->m[k].f.n, 0, p->m[k].f.add, rows[k]};
        for (int k = 0; k < 2 && !rc; k++) rc = chain_back(p->m[k].s, p->m[k].f, Table{rows[k], kept}, uv);
    } else
        for (int k = 0; k < 2 && !rc; k++) rc = chain_back(p->m[k].s, p->m[k].f, Table{rows[k], kept});
    if (rc) return rc;
    if (kept > 0) HIPCHK(hipMemcpyAsync(p->idx.h, d_ord, (size_t)kept * 8, hipMemcpyDeviceToHost, c->stream));
    *n_out = kept;
    return FFQ_OK;
}

extern "C" int ffq_pair_next(ffq_pair *p, int64_t *n_pairs_in, int64_t *n_pairs_out, int *end_state, int *err_mate, int64_t *err_offset)
{
    if (!p || !n_pairs_in || !n_pairs_out || !end_state) return fail(FFQ_E_ARG, "ffq_pair_next: NULL argument");
    ffq_ctx *c = p->c;
    HIPCHK(hipSetDevice(c->device));
    *n_pairs_in = *n_pairs_out = 0; *end_state = FFQ_END_OK;
    if (err_mate) *err_mate = 0;
    if (err_offset) *err_offset = -1;
    if (p->failed) return fail(FFQ_E_ARG, "ffq_pair_next: the pair has failed");
    for (int i = 0; i < 5; i++) p->last_pairs[i] = 0;
    for (int i = 0; i < FFQ_OVERLAP_COUNTS; i++) p->overlap.last[i] = 0;
    for (int i = 0; i < FFQ_MERGE_COUNTS; i++) p->merge.last[i] = 0;
    for (int64_t &x : p->merge.zlast) x = 0;
    for (int64_t &x : p->correct.last) x = 0;
    p->last_out = 0;
    p->started = true;
    for (int k = 0; k < 2; k++) pair_clear_last(p->m[k].s);
    if (p->w.done) return FFQ_OK;
    p->failed = true;                    // until this call gets through
    for (int k = 0; k < 2; k++) p->m[k].s->failed = true;

    // every mate whose window is empty takes its stream's next fill: the stream's own wait, take and scan -- the slot of the
    // fill it had is released by that take, not before
    walk_begin(p->w);
    const int wants = walk_wants(p->w);
    for (int k = 0; k < 2; k++) {
        if (!(wants & (1 << k))) continue;
        PairMate &pm = p->m[k];
        ffq_scan_result res;
        int rc = stream_advance(pm.s, &pm.f, &res);
        if (rc) return rc;
        pm.have = true;
        pm.bytes_offset = pm.s->globaloffset;
        pm.s->last_path = res.path;
        int64_t err = -1;
        stream_finish(pm.s, pm.f, res, &err);
        walk_filled(p->w, k, res.n_records, res.end_state, err);
    }
    const int64_t m = walk_take(p->w);
    if (!walk_check(p->w, m)) return fail(FFQ_E_INTERNAL, "ffq_pair_next: a round without pairs and without a new fill");
    int64_t n_out = 0, differ = -1;
    if (m > 0) {
        const int rc = pair_chain(p, m, &n_out, &differ);
        if (rc) return rc;
    }
    WalkRound r;
    if (differ >= 0) {
        // the round hands out nothing: what its stages reported so far is taken back
        // ... and the two records that are not mates go back, one row each, for the caller's message
        for (int k = 0; k < 2; k++) {
            ffq_stream *s = p->m[k].s;
            pair_clear_last(s);
            HIPCHK(hipMemcpyAsync(s->b->tab.h, s->b->tab.d.p + 6 * (p->w.m[k].lo + differ), 48, hipMemcpyDeviceToHost, c->stream));
        }
        r = walk_names_differ(p->w, differ);
    } else {
        r = walk_moved(p->w, m);
        if (r.end_state == FFQ_END_ERR_PAIR_COUNT) {
            // pos0 of the longer mate's first unpaired record
            const PairMate &pm = p->m[r.err_mate - 1];
            HIPCHK(hipMemcpyAsync(c->h_word, pm.s->b->tab.d.p + 6 * r.err_row, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            r.err_offset = c->h_word[0];
        }
        *n_pairs_in = m;
        *n_pairs_out = n_out;
        p->last_out = n_out;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    *end_state = r.end_state;
    if (err_mate) *err_mate = r.err_mate;
    if (err_offset) *err_offset = r.err_offset;
    if (p->w.done)
        for (int k = 0; k < 2; k++) { p->m[k].s->done = true; stream_stop_feeder(p->m[k].s); }
    p->failed = false;
    for (int k = 0; k < 2; k++) p->m[k].s->failed = false;
    return FFQ_OK;
}

// a mate's share of the round ffq_pair_next has just returned: the kept rows, and the fill they point into
extern "C" int ffq_pair_rows(ffq_pair *p, int mate, const int64_t **h_rows, const uint8_t **h_bytes, int64_t *n_bytes, int64_t *bytes_offset)
{
    if (!p || (mate != 1 && mate != 2) || !h_rows) return fail(FFQ_E_ARG, "ffq_pair_rows: a pair, mate 1 or 2, and a place for the rows");
    const PairMate &pm = p->m[mate - 1];
    *h_rows = pm.s->b->tab.h;
    if (h_bytes) *h_bytes = pm.have ? pm.f.sl->buf.h + pm.f.start : nullptr;
    if (n_bytes) *n_bytes = pm.have ? pm.f.len : 0;
    if (bytes_offset) *bytes_offset = pm.bytes_offset;
    return FFQ_OK;
}

extern "C" int ffq_pair_selected(ffq_pair *p, const int64_t **h_index, int64_t pairs[5])
{
    if (!p || !h_index) return fail(FFQ_E_ARG, "ffq_pair_selected: NULL argument");
    *h_index = p->merge.on ? p->merge.ord.h : p->idx.h;
    if (pairs) for (int i = 0; i < 5; i++) pairs[i] = p->last_pairs[i];
    return FFQ_OK;
}

// ffq_hip.hip -- C ABI of libffq_hip.so (see include/ffq.h).
// Host side of the MI355X FASTQ buffer-scan path: context, scratch sizing,
// kernel sequencing on one HIP stream, pinned staging for host buffers.
// No CPU fallback: every compute entry point needs a live gfx950 device.
#include "../../include/ffq.h"
#ifdef FFQ_PROBES
#include "../../include/ffq_probe.h"
#endif
#include "ffq_kernels.h"
#include "ffq_fasta.h"
#include "ffq_rows.h"
#include "ffq_trim.h"
#include "ffq_adapter.h"
#include "ffq_poly.h"
#include "ffq_ends.h"
#include "ffq_stats.h"
#include "ffq_filter.h"
#include "ffq_compact.h"
#include "ffq_pair.h"
#include "ffq_overlap.h"
#include "ffq_render.h"
#include "ffq_umiwalk.h"
#include "ffq_umi_launch.h"
#include "ffq_merge.h"
#include "ffq_correct.h"
#include "ffq_dedup.h"
#include "ffq_deflate.h"
#include "ffq_pool.h"
#include "ffq_mem.h"
#include "ffq_scanwalk.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <cctype>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

using namespace ffq;

static thread_local std::string g_err;

static int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(expr)                                                                     \
    do {                                                                                 \
        hipError_t e__ = (expr);                                                         \
        if (e__ != hipSuccess)                                                           \
            return fail(FFQ_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                        __FILE__, __LINE__);                                             \
    } while (0)

struct ScanArgs {
    const uint8_t *d_buf; int64_t n_bytes; int s; int64_t offset; int eof; int64_t add; uint32_t flags;
    int qual_add; int64_t *d_table; int64_t table_cap; int8_t *d_qual; int64_t qual_cap; int64_t *d_qoff;
};

// A scan between ffq_scan_submit and ffq_scan_wait: what the ladder decides on (ScanWalk, ffq_scanwalk.h) and what the
// launches need beside it.
struct ScanState : ScanWalk {
    bool active = false;
    ScanArgs a{};
    unsigned long long poll_seq = 0;   // FFQ_F_POLL_RESULT: the front ends in a publisher that writes this number; no end event
};

static_assert(WALK_ERR_POOL == ERR_POOL && WALK_ERR_INTERNAL == ERR_INTERNAL && WALK_ERR_DSTAGE == ERR_DSTAGE &&
              WALK_FZ_BAD_SHAPE == (int32_t)FZ_BAD_SHAPE && WALK_FZ_BAD_INDEX == (int32_t)FZ_BAD_INDEX && WALK_TILE == TILE &&
              WALK_SEG_STRIDE == SG_STRIDE && WALK_POOL_MIN == (unsigned long long)POOL_NB * TILE &&
              WALK_PATH_IN_PLACE == FFQ_PATH_IN_PLACE && WALK_E_INTERNAL == FFQ_E_INTERNAL,
              "ffq_scanwalk.h disagrees with ffq_dev.h, ffq_fused.h or include/ffq.h");

// What the library knows about the tail of a scan stream (kept in the context that owns the stream; contexts that share it
// point there).  FFQ_F_NO_TIMING lets a front start its index kernel without a barrier in front -- beside the previous scan's
// last, one-workgroup kernel -- and the library does that only when IT can vouch for the order not mattering: the last thing
// enqueued on the stream is the front of another scan (nothing else -- no copy, no wait for an event, no other kernel -- has gone
// onto the stream since, and the stream's handle was never given out), and none of that scan's outputs overlaps the bytes this
// one reads.
struct StreamTail {
    bool is_scan = false;                // the last operation enqueued on the stream is the end of a scan front
    bool exposed = false;                // ffq_ctx_stream() handed the stream out: others may enqueue on it unseen
    const void *out_p[3] = {nullptr, nullptr, nullptr};      // that scan's outputs (table, qualities, quality offsets)
    size_t out_n[3] = {0, 0, 0};
};

// The memory behind the kernel argument structs ChainBufs (ffq_chain.h) and RankBufs (ffq_ranked.h).  Those are plain
// structs of raw pointers that go to the kernels by value; these own what they point to.
struct ChainMem {
    DevBuf<int64_t> y, exit, qb, rloc, qloc, part, force;
    DevBuf<uint32_t> cnt, flags, lines, dlist, ilist;
    DevBuf<GroupTerm> term;
    DevBuf<int32_t> mins;
    DevBuf<StageRec> stage, dstage;
};
struct RankMem {
    DevBuf<long long> tbase;
    DevBuf<H> cand;
    DevBuf<RankRec> rec;
    DevBuf<uint32_t> succ, S[2], C[2], D, root;
};

// words of a context's counter block: what the largest table call needs (ffq_tables.h asserts it per block type)
constexpr int CALL_BLK_WORDS = 32;

struct ffq_ctx {
    ScanState pend;                      // the scan enqueued by ffq_scan_submit, if any
    ffq_ctx *owner = nullptr;            // the context whose stream this one uses (itself unless created shared)
    StreamTail tail;                     // (in the owner)
    bool owns_streams = true;            // false: streams borrowed from another context
    double watchdog_s = 0;               // > 0: the waits INSIDE a scan (its marks, the stream in front of a scratch that grows) poll and give
                                         //   up after this long with FFQ_E_TIMEOUT -- set by a shard step around its scan (ffq_shard.h): a scan
                                         //   stream that waits for a hand-off, or carries a gather, whose peer never comes must not hold the host
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    InputMemory mem;                     // what the recent scans found the input to be
    // Scratch, grow-only.  Every buffer is a member that frees itself (ffq_mem.h); the kernel argument structs `rk` and
    // `cb` are raw-pointer VIEWS of the members of RankMem / ChainMem, rebuilt by the functions that regrow those.
    RankMem rm;                          // list ranking (ffq_ranked.h): rm.tbase.cap tiles, rm.cand.cap candidates
    RankBufs rk = {};
    // single-pass index + decode (ffq_fused.h): per-tile phases, verdict
    DevBuf<uint8_t> fz_qphase;
    DevBuf<uint32_t> fz_bad;
    bool decode_timed = false;           // ev[6] marks the start of the decode kernel of the pending front
    int64_t cap_tiles = 0;               // what ent .. sbqbase and the per-group buffers of `cm` are sized for (reserve_tiles)
    DevBuf<uint16_t> ent;
    DevBuf<uint32_t> cnt;
    DevBuf<unsigned long long> ovf;
    DevBuf<uint16_t> pool;
    ChainMem cm;                         // cm.stage.cap: StageRec entries; cm.dstage.cap / DCHUNK: chunks of the walked groups' stage
    ChainBufs cb = {};
    DevBuf<long long> sbbase;
    DevBuf<TileQ> tileq;                 // fast path + decode: records / quality bytes per tile
    DevBuf<unsigned int> sbq;            //   quality bytes per 64 tiles
    DevBuf<long long> sbqbase;           //   their exclusive scan
    DevBuf<Fast4Hdr> hdr4;
    DevBuf<TermInfo4> tinfo4;
    DevBuf<Ctl> ctl;
    DevBuf<LineIndex> d_L;               // device copy of the LineIndex (out-of-line device functions)
    PinBuf<LineIndex> h_L;               // pinned source of that copy
    DevBuf<DevRes> dres;
    DevBuf<int64_t> qdir;                // directory of the decoded-quality stream (qdir_mark)
    DevBuf<int64_t> p4s;                 // pos4 of every record, compact: what the decode reads instead of the 48-byte rows
    DevBuf<uint32_t> qrel;               // tile-relative quality offsets of the fast path (p4s.cap entries)
    // pinned mirrors
    PinBuf<Ctl, hipHostMallocMapped> h_ctl;        // host-mapped pinned: written by the publishing kernel (Pub)
    PinBuf<DevRes, hipHostMallocMapped> h_res;
    Ctl *hm_ctl = nullptr;              // device addresses of the two
    DevRes *hm_res = nullptr;
    PinBuf<unsigned long long, hipHostMallocMapped> h_seq;    // completion word of FFQ_F_POLL_RESULT (host-mapped)
    unsigned long long *hm_seq = nullptr;                     //   and its device address
    unsigned long long seq = 0;         // last number handed out
    unsigned long long pub_seq = 0;     // what the publisher being enqueued writes (0: nothing)
    bool ctl_clean = false;             // the control block is zero (creation, or a publisher ran last)
    bool ctl_was_clean = false;         //   ... as it was when the front being enqueued began (no memset in front of it)
    DevBuf<int64_t> d_word;             // 2 scratch words for the small table queries
    PinBuf<int64_t> h_word;             //   and their pinned mirror
    DevBuf<int64_t> d_cut;              // ffq_table_cut: 6 words
    PinBuf<int64_t> h_cut;
    Mirror<uint64_t> blk;               // the table calls: a call's counters and their pinned mirror, CALL_BLK_WORDS words
                                        //   (ffq_tables.h: call_blk_begin / call_blk_end)
    DevBuf<int64_t> rows_list;          // the table passes of ffq_rows.h: rows left to the wave-per-row launch
    PinBuf<uint64_t> h_stats;           // ffq_table_stats: the head words handed back
    DevBuf<uint8_t> filter_verdict;     // ffq_table_select_reads: a verdict byte per row
    DevBuf<uint8_t> filter_verdict2;    //   ... and per row of the second mate (ffq_table_select_pairs)
    DevBuf<int64_t> render_list;        // ffq_table_render_fastq: (row, place in the output) of the rows left to the wave-per-row launch
    DevBuf<uint32_t> deflate_slots;     // ffq_deflate_bgzf: candidates, then tokens, DFL_BLOCK words per workgroup of its capped grid
    DevBuf<uint8_t> deflate_members;    //   ... and a DFL_SLOT bytes slot per block, where its member is built
    DevBuf<FaHdr> fa_hdr;               // FASTA scan: starts, the last start
    // staging for the host-buffer entry points
    DevBuf<uint8_t> stage_d;
    PinBuf<uint8_t> stage_h;
    DevBuf<int64_t> tab_d;
    DevBuf<int8_t> qual_d;
    DevBuf<int64_t> qoff_d;
    DevBuf<unsigned int> sel_cnt;       // row selection: kept rows per workgroup, their scan
    DevBuf<long long> sel_base;
    DevBuf<long long> col_sum;          // column selection: bytes per block of rows, their scan
    DevBuf<long long> scan_bs;          // block sums of the two-level scan (launch_scan)
    DevBuf<DevRes> col_res;             //   its result block (row count, total bytes)
    // ffq_scan_host: pageable memory goes through three pinned staging slots, copied in by the
    // helper threads and out over two copy streams (and back the same way)
    hipEvent_t stage_ev[3][2] = {};
    hipStream_t stage_cs[2] = {nullptr, nullptr};
    ChunkRead stage_cr[3];
    ReadPool *helpers = nullptr;   // helper threads (ffq_pool.h), started on first use
    cpu_set_t near_cpus;           // the CPUs next to the GPU (ctx_near), near_ok: known
    int near_ok = -1;
    void *stream_cache = nullptr;  // buffers of the last closed ffq_stream (ffq_stream.h), reused by the next one
};

extern "C" int ffq_abi_version(void) { return FFQ_ABI_VERSION; }
// hash of the sources this binary was compiled from (csrc/*, include/*.h), baked in by build.py
#ifndef FFQ_BUILD_ID
#define FFQ_BUILD_ID "unknown"
#endif
#ifdef FFQ_PROBES
static const char g_build_tag[] = "FFQ_BUILD_ID=" FFQ_BUILD_ID "+probes";      // (build.py reads the tag out of the file)
#else
static const char g_build_tag[] = "FFQ_BUILD_ID=" FFQ_BUILD_ID;
#endif
extern "C" const char *ffq_build_id(void) { return g_build_tag + 13; }
extern "C" const char *ffq_last_error(void) { return g_err.c_str(); }

extern "C" int ffq_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int ctx_create_impl(int device, ffq_ctx *share, ffq_ctx **out);
extern "C" void ffq_ctx_destroy(ffq_ctx *c);
static void stream_cache_drop(ffq_ctx *c);

extern "C" int ffq_ctx_create(int device, ffq_ctx **out) { return ctx_create_impl(device, nullptr, out); }

static int ctx_create_impl(int device, ffq_ctx *share, ffq_ctx **out)
{
    if (!out) return fail(FFQ_E_ARG, "ffq_ctx_create: out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(FFQ_E_NODEVICE, "no HIP device visible: the FASTQ scan path needs an MI355X (gfx950); there is no CPU fallback");
    if (device < 0 || device >= n) return fail(FFQ_E_ARG, "device %d out of range (0..%d)", device, n - 1);
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(FFQ_E_NODEVICE, "device %d is %s; libffq_hip is built for gfx950 only", device, prop.gcnArchName);
    HIPCHK(hipSetDevice(device));
    ffq_ctx *c = new (std::nothrow) ffq_ctx();
    if (!c) return fail(FFQ_E_NOMEM, "out of host memory");
    c->device = device;
    hipError_t e = hipSuccess;
    c->owner = share ? share->owner : c;
    if (share) {
        // same streams as `share`: scans of the two contexts execute in submission order
        c->stream = share->stream; c->owns_streams = false;
    } else {
        e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    }
    // timing marks need no system-scope release (an L2 write-back per record); only ev[3] / ev[2],
    // which the host waits on before it reads the published result block, keep the default
    for (int i = 0; i < 7 && e == hipSuccess; i++)
        e = (i == 2 || i == 3) ? hipEventCreate(&c->ev[i])
                               : hipEventCreateWithFlags(&c->ev[i], hipEventDisableSystemFence);
    if (e == hipSuccess) e = c->ctl.grow(1);
    if (e == hipSuccess) e = c->dres.grow(1);
    if (e == hipSuccess) e = c->col_res.grow(1);
    if (e == hipSuccess) e = c->d_L.grow(1);
    if (e == hipSuccess) e = c->d_word.grow(2);
    if (e == hipSuccess) e = c->h_word.grow(2);
    if (e == hipSuccess) e = c->d_cut.grow(6);
    if (e == hipSuccess) e = c->blk.grow(CALL_BLK_WORDS);
    if (e == hipSuccess) e = c->h_stats.grow(STATS_HEAD);
    if (e == hipSuccess) e = c->fa_hdr.grow(1);
    if (e == hipSuccess) e = c->h_cut.grow(6);
    if (e == hipSuccess) e = c->h_L.grow(1);
    if (e == hipSuccess) e = c->h_ctl.grow(1);
    if (e == hipSuccess) e = c->h_res.grow(1);
    if (e == hipSuccess) e = c->h_seq.grow(8);
    if (e == hipSuccess) { *c->h_seq = 0; e = hipHostGetDevicePointer((void **)&c->hm_seq, c->h_seq, 0); }
    if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&c->hm_ctl, c->h_ctl, 0);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&c->hm_res, c->h_res, 0);
    if (e != hipSuccess) {
        ffq_ctx_destroy(c);
        return fail(FFQ_E_HIP, "context setup failed: %s", hipGetErrorString(e));
    }
    *out = c;
    return FFQ_OK;
}

// c->cb as the buffers of c->cm are now.  The functions that regrow those (reserve_tiles, reserve_stage, reserve_dstage)
// hold one of these: whichever way they return, the view is rebuilt -- no kernel gets a pointer to a block that was freed.
struct ChainView {
    ffq_ctx *c;
    ~ChainView()
    {
        ChainMem &m = c->cm;
        ChainBufs &b = c->cb;
        b = ChainBufs{};
        b.y = m.y; b.exit = m.exit; b.cnt = m.cnt; b.flags = m.flags; b.lines = m.lines; b.qb = m.qb; b.term = m.term;
        b.stage = m.stage; b.dstage = m.dstage; b.dchunks = (int32_t)(m.dstage.cap / DCHUNK);
        b.dlist = m.dlist; b.ilist = m.ilist; b.rloc = m.rloc; b.qloc = m.qloc; b.part = m.part; b.mins = m.mins;
        b.force = m.force;
    }
};

// everything sized by the tile count but the line index itself
static void free_chain(ffq_ctx *c)
{
    ChainMem &m = c->cm;
    m.y.reset(); m.exit.reset(); m.cnt.reset(); m.flags.reset(); m.lines.reset(); m.qb.reset(); m.term.reset(); m.stage.reset();
    m.rloc.reset(); m.qloc.reset(); m.part.reset(); m.mins.reset(); m.force.reset(); m.dlist.reset(); m.ilist.reset();
    // (the walked groups' stage, m.dstage, does not depend on the tile count: it stays)
    c->sbbase.reset(); c->tinfo4.reset(); c->tileq.reset(); c->sbq.reset(); c->sbqbase.reset();
}

extern "C" int ffq_ctx_create_shared(ffq_ctx *parent, ffq_ctx **out)
{
    if (!parent || !out) return fail(FFQ_E_ARG, "ffq_ctx_create_shared: NULL argument");
    return ctx_create_impl(parent->device, parent, out);
}

extern "C" void ffq_ctx_destroy(ffq_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    stream_cache_drop(c);
    for (auto &r : c->stage_ev) for (auto &e : r) if (e) (void)hipEventDestroy(e);
    for (auto &st : c->stage_cs) if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    delete c->helpers;
    for (int i = 0; i < 7; i++) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    if (c->stream && c->owns_streams) (void)hipStreamDestroy(c->stream);
    delete c;                            // (the buffers are members: they free themselves here)
}

// something other than a scan front goes onto the context's stream (every entry point that enqueues there says so)
static inline void mark_other(ffq_ctx *c) { if (c && c->owner) c->owner->tail.is_scan = false; }

// The waits of the scan path, with the context's watchdog (ffq_ctx::watchdog_s; 0: the plain blocking calls).  A scan is
// through in milliseconds: the first two are spun, the rest slept in 100 us pieces.
static int ctx_wait(ffq_ctx *c, hipEvent_t ev, hipStream_t st)
{
    if (c->watchdog_s <= 0) {
        if (ev) HIPCHK(hipEventSynchronize(ev)); else HIPCHK(hipStreamSynchronize(st));
        return FFQ_OK;
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t spins = 1;; spins++) {
        const hipError_t e = ev ? hipEventQuery(ev) : hipStreamQuery(st);
        if (e == hipSuccess) return FFQ_OK;
        if (e != hipErrorNotReady) return fail(FFQ_E_HIP, "%s failed: %s", ev ? "hipEventQuery" : "hipStreamQuery", hipGetErrorString(e));
        if ((spins & 31) == 0) {
            const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (dt > c->watchdog_s) return fail(FFQ_E_TIMEOUT, "scan: the stream made no progress within %.1f s", dt);
            if (dt > 2e-3) usleep(100);
        }
        __builtin_ia32_pause();
    }
}
#define CTX_WAIT_EVENT(c, ev) do { const int rc__ = ctx_wait((c), (ev), nullptr); if (rc__) return rc__; } while (0)
#define CTX_SYNC(c) do { const int rc__ = ctx_wait((c), nullptr, (c)->stream); if (rc__) return rc__; } while (0)

extern "C" void *ffq_ctx_stream(ffq_ctx *c)
{
    if (!c) return nullptr;
    c->owner->tail.exposed = true;       // (whoever holds the handle may enqueue on the stream without the library seeing it)
    c->owner->tail.is_scan = false;
    return (void *)c->stream;
}

// The CPUs next to the context's GPU (sysfs: /sys/bus/pci/devices/<bdf>/local_cpulist), looked up once.
// FFQ_POOL_AFFINITY=0: nothing is bound.
static bool ctx_near(ffq_ctx *c)
{
    if (c->near_ok < 0) {
        char bdf[32] = {0};
        const char *a = getenv("FFQ_POOL_AFFINITY");
        bool ok = !(a && atoi(a) == 0) && hipDeviceGetPCIBusId(bdf, (int)sizeof bdf - 1, c->device) == hipSuccess;
        for (char *p = bdf; *p; p++) *p = (char)tolower((unsigned char)*p);      // (sysfs spells the address in lower case)
        ok = ok && ReadPool::local_cpus(bdf, &c->near_cpus);
        c->near_ok = ok ? 1 : 0;
        if (getenv("FFQ_POOL_DEBUG")) fprintf(stderr, "[ffq pool] device %d at %s: %s (%d CPUs)\n", c->device, bdf, ok ? "helpers and staging memory next to the GPU" : "not bound", ok ? CPU_COUNT(&c->near_cpus) : 0);
    }
    return c->near_ok == 1;
}

// The calling thread next to the GPU for as long as this lives: pinned staging memory is allocated (and touched) from there,
// so that its pages lie on the GPU's node whatever the runtime's own policy is (on the two-socket boxes here the loader ran
// at 46 instead of 52 GB/s in one process of six with the helpers bound but the slots allocated from wherever the caller ran).
struct NearGpu {
    cpu_set_t saved;
    bool bound = false;
    explicit NearGpu(ffq_ctx *c)
    {
        if (!ctx_near(c) || sched_getaffinity(0, sizeof saved, &saved) != 0) return;
        bound = sched_setaffinity(0, sizeof c->near_cpus, &c->near_cpus) == 0;
    }
    ~NearGpu() { if (bound) (void)sched_setaffinity(0, sizeof saved, &saved); }
    NearGpu(const NearGpu &) = delete;
    NearGpu &operator=(const NearGpu &) = delete;
};

static ReadPool *ctx_pool(ffq_ctx *c)
{
    if (!c->helpers) {
        c->helpers = new (std::nothrow) ReadPool();
        if (c->helpers) {
            const unsigned hw = std::thread::hardware_concurrency();
            const char *e = getenv("FFQ_POOL_THREADS");              // (measurements; default: up to 16)
            const unsigned want = (e && atoi(e) > 0) ? (unsigned)std::min(atoi(e), 64) : 16u;
            // the helpers run on the CPUs next to the GPU (FFQ_POOL_AFFINITY=0: wherever the scheduler puts them)
            const bool bind = ctx_near(c);
            c->helpers->start((int)std::min<unsigned>(want, hw > 2 ? hw - 2 : 1), bind ? &c->near_cpus : nullptr);
        }
    }
    return c->helpers;
}

static int64_t tiles_for(int64_t n) { return (n + TILE - 1) >> TILE_SHIFT; }
static int64_t groups_for(int64_t ntiles) { return (ntiles + OWN_T - 1) / OWN_T; }
constexpr int PER_FAST = 6, EMAX_FAST = 2048, WPB_FAST = 2;   // k_chain_wave, usual line/record density
constexpr int PER_DENSE = 15, EMAX_DENSE = NTW * SLOT + 8, WPB_DENSE = 1;   // short records / short lines
constexpr int NMAX_FAST = PER_FAST * 64, NMAX_DENSE = PER_DENSE * 64;
constexpr int WPB_LITE = 2;                                    // k_chain_lite (ffq_lite.h): groups per workgroup

static int reserve_tiles(ffq_ctx *c, int64_t ntiles)
{
    if (ntiles <= c->cap_tiles) return FFQ_OK;
    CTX_SYNC(c);
    ChainView refill{c};
    ChainMem &m = c->cm;
    c->ent.reset(); c->cnt.reset(); c->ovf.reset();
    free_chain(c);
    c->cap_tiles = 0;
    const int64_t ng = groups_for(ntiles);
    const int64_t nblk = (ng + RES_BLOCK - 1) / RES_BLOCK;
    HIPCHK(c->ent.grow(ntiles * SLOT));
    HIPCHK(c->cnt.grow(ntiles));
    HIPCHK(c->ovf.grow(ntiles));
    HIPCHK(m.y.grow(ng));
    HIPCHK(m.exit.grow(ng));
    HIPCHK(m.cnt.grow(ng));
    HIPCHK(m.flags.grow(2 * ng + 8));      // (flags | sbase | dhead | dcnt: one fill per scan, chain_bufs)
    HIPCHK(m.dlist.grow(ng));
    HIPCHK(m.ilist.grow(ng));
    HIPCHK(m.lines.grow(ng));
    HIPCHK(m.qb.grow(ng));
    HIPCHK(m.term.grow(ng));
    HIPCHK(m.rloc.grow(ng));
    HIPCHK(m.qloc.grow(ng));
    HIPCHK(m.part.grow(nblk * 4));
    HIPCHK(m.mins.grow(4));
    HIPCHK(m.force.grow(ng));
    {
        const int64_t nsb = (ntiles + SB_TILES - 1) / SB_TILES;
        HIPCHK(c->sbbase.grow(nsb));
        HIPCHK(c->tinfo4.grow(ntiles));
        HIPCHK(c->tileq.grow(ntiles));
        HIPCHK(c->sbq.grow(nsb));
        HIPCHK(c->sbqbase.grow(nsb));
        HIPCHK(c->hdr4.grow(1));
    }
    c->cap_tiles = ntiles;
    return FFQ_OK;
}

// the walked groups' stage (k_dense_walk): `chunks` chunks of DCHUNK records
static int reserve_dstage(ffq_ctx *c, int64_t chunks)
{
    if (chunks * DCHUNK <= c->cm.dstage.cap) return FFQ_OK;
    CTX_SYNC(c);
    ChainView refill{c};
    const hipError_t e = c->cm.dstage.grow(chunks * DCHUNK);
    if (e != hipSuccess) return fail(FFQ_E_NOMEM, "hipMalloc(walked groups' stage, %lld chunks) failed: %s", (long long)chunks, hipGetErrorString(e));
    return FFQ_OK;
}

static int reserve_stage(ffq_ctx *c, int64_t ng, int nmax)
{
    const int64_t need = ng * nmax;
    if (need <= c->cm.stage.cap) return FFQ_OK;
    CTX_SYNC(c);
    ChainView refill{c};
    const hipError_t e = c->cm.stage.grow(need);
    if (e != hipSuccess) return fail(FFQ_E_NOMEM, "hipMalloc(stage) failed: %s", hipGetErrorString(e));
    return FFQ_OK;
}

// blocks of the decoded-quality stream for this scan (upper bound: half of the bytes are
// qualities at most, and no more than the caller's buffer holds)
static int64_t qdir_blocks(int64_t n_bytes, int64_t qual_cap)
{
    return (std::min<int64_t>(qual_cap, n_bytes / 2 + 16) + DQ_BLK - 1) / DQ_BLK + 1;
}

static int reserve_qdir(ffq_ctx *c, int64_t blocks)
{
    if (blocks <= c->qdir.cap) return FFQ_OK;
    CTX_SYNC(c);
    const hipError_t e = c->qdir.grow(blocks);
    if (e != hipSuccess) return fail(FFQ_E_NOMEM, "hipMalloc(qdir) failed: %s", hipGetErrorString(e));
    return FFQ_OK;
}

// one int64 per possible record of this scan (a record starts with "\n@" and has three more
// newlines: no more than a quarter of the bytes), capped by the caller's table
static int64_t p4s_need(int64_t n_bytes, int64_t table_cap) { return std::min<int64_t>(table_cap, n_bytes / 4 + 2); }
static int reserve_p4s(ffq_ctx *c, int64_t entries)
{
    if (entries <= c->p4s.cap) return FFQ_OK;
    CTX_SYNC(c);
    c->p4s.reset(); c->qrel.reset();
    hipError_t e = c->p4s.grow(entries);
    if (e == hipSuccess) e = c->qrel.grow(entries);
    if (e != hipSuccess) {
        c->p4s.reset(); c->qrel.reset();          // (p4s.cap stands for both)
        return fail(FFQ_E_NOMEM, "hipMalloc(p4s) failed: %s", hipGetErrorString(e));
    }
    return FFQ_OK;
}

// the smallest pool: every region holds one full tile of newlines
constexpr unsigned long long POOL_MIN = (unsigned long long)POOL_NB * TILE;

static int reserve_pool(ffq_ctx *c, unsigned long long entries)
{
    if (entries <= (unsigned long long)c->pool.cap) return FFQ_OK;
    CTX_SYNC(c);
    HIPCHK(c->pool.grow((int64_t)entries));
    return FFQ_OK;
}

extern "C" void ffq_ctx_forget(ffq_ctx *c)
{
    if (c) forget(c->mem);
}

extern "C" int ffq_ctx_reserve(ffq_ctx *c, int64_t max_bytes)
{
    if (!c || max_bytes < 0) return fail(FFQ_E_ARG, "ffq_ctx_reserve: bad argument");
    HIPCHK(hipSetDevice(c->device));
    const int64_t nt = std::max<int64_t>(tiles_for(max_bytes), 1);
    int rc = reserve_tiles(c, nt);
    if (rc) return rc;
    rc = reserve_stage(c, groups_for(nt), NMAX_FAST);
    if (rc) return rc;
    return reserve_pool(c, POOL_MIN);
}

// ---- memory plumbing -----------------------------------------------------
extern "C" int ffq_dev_alloc(ffq_ctx *c, int64_t bytes, void **dptr)
{
    if (!c || !dptr || bytes < 0) return fail(FFQ_E_ARG, "ffq_dev_alloc: bad argument");
    HIPCHK(hipSetDevice(c->device));
    *dptr = nullptr;
    hipError_t e = hipMalloc(dptr, (size_t)std::max<int64_t>(bytes, 16));
    if (e != hipSuccess) return fail(FFQ_E_NOMEM, "hipMalloc(%lld) failed: %s", (long long)bytes, hipGetErrorString(e));
    return FFQ_OK;
}
extern "C" int ffq_dev_free(ffq_ctx *c, void *dptr)
{
    if (!c) return fail(FFQ_E_ARG, "ffq_dev_free: ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipFree(dptr));
    return FFQ_OK;
}
extern "C" int ffq_pinned_alloc(int64_t bytes, void **hptr)
{
    if (!hptr || bytes < 0) return fail(FFQ_E_ARG, "ffq_pinned_alloc: bad argument");
    *hptr = nullptr;
    hipError_t e = hipHostMalloc(hptr, (size_t)std::max<int64_t>(bytes, 16), hipHostMallocDefault);
    if (e != hipSuccess) return fail(FFQ_E_NOMEM, "hipHostMalloc(%lld) failed: %s", (long long)bytes, hipGetErrorString(e));
    return FFQ_OK;
}
extern "C" int ffq_pinned_free(void *hptr)
{
    HIPCHK(hipHostFree(hptr));
    return FFQ_OK;
}
extern "C" int ffq_copy_h2d(ffq_ctx *c, void *dptr, const void *hptr, int64_t bytes, int async)
{
    mark_other(c);
    if (!c || bytes < 0) return fail(FFQ_E_ARG, "ffq_copy_h2d: bad argument");
    HIPCHK(hipSetDevice(c->device));
    if (bytes) HIPCHK(hipMemcpyAsync(dptr, hptr, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    if (!async) HIPCHK(hipStreamSynchronize(c->stream));
    return FFQ_OK;
}
extern "C" int ffq_copy_d2h(ffq_ctx *c, void *hptr, const void *dptr, int64_t bytes, int async)
{
    mark_other(c);
    if (!c || bytes < 0) return fail(FFQ_E_ARG, "ffq_copy_d2h: bad argument");
    HIPCHK(hipSetDevice(c->device));
    if (bytes) HIPCHK(hipMemcpyAsync(hptr, dptr, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    if (!async) HIPCHK(hipStreamSynchronize(c->stream));
    return FFQ_OK;
}
extern "C" int ffq_sync(ffq_ctx *c)
{
    if (!c) return fail(FFQ_E_ARG, "ffq_sync: ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FFQ_OK;
}

// ---- the hot path ----------------------------------------------------------
static void fill_result(ffq_scan_result *res, const DevRes &r, int path, int retries)
{
    res->n_records = r.n_records;
    res->n_qual_bytes = r.n_qual_bytes;
    res->end_offset = r.end_offset;
    for (int i = 0; i < 6; i++) res->last_pos[i] = r.last_pos[i];
    res->last_status = r.last_status;
    res->end_state = r.end_state;
    res->path = path;
    res->retries = retries;
    res->n_lines = r.n_lines;
}

// ---- one scan = front (enqueue) + finish (sync, fallbacks) ---------------------------------
// ffq_scan_submit enqueues the front and returns; ffq_scan_wait finishes.  ffq_scan_device is
// submit + wait.  Two contexts that share their streams (ffq_ctx_create_shared) let a host
// keep the next batch's kernels queued behind the current one's: no idle GPU between steps.
static LineIndex make_index(ffq_ctx *c, const ScanArgs &a, int64_t ntiles)
{
    LineIndex L;
    L.d = a.d_buf; L.n = a.n_bytes; L.s = a.s; L.ntiles = (int32_t)ntiles; L.ready = (int32_t)ntiles; L.pad_ = 0;
    L.ent = c->ent; L.cnt = c->cnt; L.ovf = c->ovf; L.pool = c->pool; L.pool_cap = (unsigned long long)c->pool.cap;
    return L;
}

// The line-index launch: one workgroup per whole tile; the ragged last tile (if any) rides along
// as workgroup 0's second tile.  A buffer shorter than a tile is one workgroup.
static void launch_scan_lines(ffq_ctx *c, hipStream_t st, const uint8_t *d_buf, int64_t n_bytes, int64_t ntiles,
                              const LineIndex &L, uint32_t at_char, bool any_order = false,
                              int8_t *wout = nullptr, int wadd = 0)
{
    const int64_t nfull = n_bytes >> TILE_SHIFT;
    const int ragged = ntiles > nfull ? (int)nfull : -1;
    const unsigned long long pool_cap = (unsigned long long)c->pool.cap;
    int8_t *const no_out = nullptr;
    if (wout) {
        // the WIDE instantiation (ffq_kernels.h): the index AND every byte decoded in place, for the decode of records of any
        // layout in one pass (FFQ_F_DECODE_QUAL | FFQ_F_SINGLE_PASS on the general path)
        if (nfull > 0)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_lines<true, 8, true>), dim3((unsigned)nfull), dim3(256), 0, st, d_buf,
                               n_bytes, c->ent, c->cnt, c->ovf, c->pool, pool_cap, c->ctl, 0, L, c->d_L,
                               at_char, ragged, wout, (uint32_t)wadd);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_lines<false, 8, true>), dim3(1), dim3(256), 0, st, d_buf,
                               n_bytes, c->ent, c->cnt, c->ovf, c->pool, pool_cap, c->ctl, 0, L, c->d_L,
                               at_char, 0, wout, (uint32_t)wadd);
        return;
    }
    if (nfull > 0 && any_order)
        // No barrier in front of this dispatch: it may start while the kernel queued before it (the previous
        // scan's last, one-workgroup kernel -- another context's, on the same stream) is still running.  The
        // index kernel reads the caller's bytes and writes this context's own scratch, nothing the previous
        // scan touches; the kernels behind it are ordinary launches and wait for everything in front of them.
        hipExtLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_lines<true, 8>), dim3((unsigned)nfull), dim3(256), 0, st, nullptr, nullptr,
                              hipExtAnyOrderLaunch, d_buf, n_bytes, c->ent.p, c->cnt.p, c->ovf.p, c->pool.p, pool_cap, c->ctl.p, 0,
                              L, c->d_L.p, at_char, ragged, no_out, 0u);
    else if (nfull > 0)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_lines<true, 8>), dim3((unsigned)nfull), dim3(256), 0, st, d_buf,
                           n_bytes, c->ent, c->cnt, c->ovf, c->pool, pool_cap, c->ctl, 0, L, c->d_L,
                           at_char, ragged, no_out, 0u);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_lines<false, 8>), dim3(1), dim3(256), 0, st, d_buf,
                           n_bytes, c->ent, c->cnt, c->ovf, c->pool, pool_cap, c->ctl, 0, L, c->d_L,
                           at_char, 0, no_out, 0u);
}

// Phred decode of the finished table: the grid covers the largest possible quality stream;
// workgroups past the real end return at once
static void enqueue_decode(ffq_ctx *c, const ScanArgs &a, hipStream_t st, bool timed = false)
{
    if (timed) { (void)hipEventRecord(c->ev[6], st); c->decode_timed = true; }
    const int64_t nblk = qdir_blocks(a.n_bytes, a.qual_cap);
    hipLaunchKernelGGL(k_decode_stream, dim3((unsigned)nblk), dim3(256), 0, st, a.d_buf, a.n_bytes, a.s,
                       (const int64_t *)c->p4s, (const int64_t *)a.d_qoff, (const int64_t *)c->qdir,
                       (const DevRes *)c->dres, std::min<int64_t>(a.table_cap, c->p4s.cap), a.add, a.qual_add, a.d_qual,
                       a.qual_cap);
}

// ---- the single-pass index + decode front (ffq_fused.h) ---------------------------------------------
static LineIndex make_index(ffq_ctx *c, const ScanArgs &a, int64_t ntiles);

static_assert(SG_STRIDE == FFQ_SEG_STRIDE, "include/ffq.h and csrc/ffq_fused.h disagree on the segment stride");

static int enqueue_fused_index(ffq_ctx *c, const ScanArgs &a, int64_t ntiles, bool in_place)
{
    if (ntiles > c->fz_qphase.cap) {
        CTX_SYNC(c);
        if (c->fz_qphase.grow(ntiles) != hipSuccess) return fail(FFQ_E_NOMEM, "hipMalloc(fused scratch) failed");
    }
    if (c->fz_bad.grow(4) != hipSuccess) return fail(FFQ_E_NOMEM, "hipMalloc failed");
    hipStream_t sA = c->stream;
    HIPCHK(hipMemsetAsync(c->fz_bad, 0, 16, sA));
    SegArgs fa{};
    fa.d = a.d_buf; fa.n = a.n_bytes; fa.s = a.s; fa.ntiles = (int32_t)ntiles;
    fa.ent = c->ent; fa.cnt = c->cnt;
    fa.qphase = c->fz_qphase; fa.bad = c->fz_bad;
    fa.out = a.d_qual; fa.out_cap = a.qual_cap; fa.qadd = a.qual_add; fa.at_char = (uint32_t)'@';
    fa.Lval = make_index(c, a, ntiles); fa.d_L = c->d_L;      // (the device copy of the index descriptor, as k_scan_lines leaves it)
    HIPCHK(hipEventRecord(c->ev[0], sA));
    if (in_place) hipLaunchKernelGGL(k_scan_ident, dim3((unsigned)ntiles), dim3(256), 0, sA, fa);
    else hipLaunchKernelGGL(k_scan_seg, dim3((unsigned)ntiles), dim3(256), 0, sA, fa);
    HIPCHK(hipEventRecord(c->ev[1], sA));
    return FFQ_OK;
}

static Pub make_pub(ffq_ctx *c) { return Pub{c->ctl, c->hm_ctl, c->hm_res, c->pub_seq ? c->hm_seq : nullptr, c->pub_seq}; }
static Pub no_pub(ffq_ctx *c) { return Pub{c->ctl, nullptr, nullptr, nullptr, 0}; }

// FFQ_F_POLL_RESULT: wait for the publisher of a front by polling the host-mapped completion word
// (every event record on the stream is a few microseconds of idle GPU; a front that ends in a
// publisher needs none to say that it is through)
static int poll_seq(ffq_ctx *c, unsigned long long want)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t spins = 1;; spins++) {
        if (__atomic_load_n(c->h_seq.p, __ATOMIC_ACQUIRE) >= want) return FFQ_OK;
        if ((spins & 0x7FFF) == 0) {
            if (c->watchdog_s > 0) {
                const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                if (dt > c->watchdog_s) return fail(FFQ_E_TIMEOUT, "scan: the result block was not published within %.1f s", dt);
                if (dt > 2e-3) usleep(100);
            }
            const hipError_t e = hipStreamQuery(c->stream);
            if (e == hipSuccess) {           // the stream has drained: the publisher has run, or never will
                if (__atomic_load_n(c->h_seq.p, __ATOMIC_ACQUIRE) >= want) return FFQ_OK;
                return fail(FFQ_E_INTERNAL, "the result block was not published");
            }
            if (e != hipErrorNotReady) return fail(FFQ_E_HIP, "hipStreamQuery failed: %s", hipGetErrorString(e));
        }
        __builtin_ia32_pause();
    }
}

// verification + scan of the group counts, rows, result block (publishes) [-> decode]
static int enqueue_resolve(ffq_ctx *c, const ScanState &st, const ChainBufs &cb, bool timed, bool mins_set = false)
{
    const ScanArgs &a = st.a;
    const bool wide = st.wide;          // (the qualities are there already, in place: k_expand writes qoff[i] = pos4's buffer offset)
    int64_t *qoff = st.decode ? a.d_qoff : nullptr;
    hipStream_t sA = c->stream;
    const int ngroups = cb.ng;
    const int nblk = (ngroups + RES_BLOCK - 1) / RES_BLOCK;
    if (!mins_set) HIPCHK(hipMemsetAsync(cb.mins, 0x7F, 16, sA));       // (the list kernel of the lean path sets them itself)
    hipLaunchKernelGGL(k_resolve_a, dim3(nblk), dim3(RES_BLOCK), 0, sA, cb);
    hipLaunchKernelGGL(k_resolve_b, dim3(1), dim3(1024), 0, sA, cb, nblk, a.eof, a.offset, a.add, c->dres);
    hipLaunchKernelGGL(k_expand, dim3(ngroups), dim3(64), 0, sA, cb, (const DevRes *)c->dres, a.add, a.d_table,
                       a.table_cap, qoff, wide ? (int64_t *)nullptr : c->qdir, c->qdir.cap, (qoff && !wide) ? c->p4s : (int64_t *)nullptr,
                       (qoff && !wide) ? std::min<int64_t>(a.table_cap, c->p4s.cap) : (int64_t)0, a.s, wide ? 1 : 0);
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(64), 0, sA, c->dres, a.d_table, a.table_cap, a.add, a.offset, qoff,
                       make_pub(c), wide ? a.s : -1);
    c->ctl_clean = true;
    if (st.decode && !wide) enqueue_decode(c, a, sA, timed);
    return FFQ_OK;
}

// the chain scratch of a scan of `ngroups` groups: the walked groups' chunk numbers and the chunk counter lie right behind the
// group flags (one fill zeroes all three at the start of the chain stage; sbase: chunk + 1, 0 = none)
static ChainBufs chain_bufs(ffq_ctx *c, int ngroups, int nmax)
{
    ChainBufs cb = c->cb;
    cb.ng = ngroups;
    cb.nmax = nmax;
    cb.sbase = reinterpret_cast<int32_t *>(cb.flags + ngroups);
    cb.dhead = cb.flags + 2 * (size_t)ngroups;
    cb.dcnt = cb.dhead + 1;
    cb.icnt = cb.dhead + 2;
    return cb;
}

// FFQ_NO_FAST4 is read at every call (tests flip it while a process runs), the other three once
static Switches scan_switches()
{
    static const Switches once{false, getenv("FFQ_NO_WIDE") != nullptr, getenv("FFQ_NO_LITE") != nullptr, getenv("FFQ_NO_RANKED") != nullptr};
    Switches sw = once;
    sw.no_fast4 = getenv("FFQ_NO_FAST4") != nullptr;
    return sw;
}

// repair pass: the groups whose entry guess the verification rejected are re-run from their
// predecessor's exit (k_repair_mark), then everything is verified again
static int enqueue_repair(ffq_ctx *c, const ScanState &st, const LineIndex &L)
{
    const ScanArgs &a = st.a;
    const bool dense_cfg = st.dense_cfg;
    const int ngroups = st.ngroups;
    ChainBufs cb = chain_bufs(c, ngroups, dense_cfg ? NMAX_DENSE : NMAX_FAST);
    hipStream_t sA = c->stream;
    hipLaunchKernelGGL(k_repair_mark, dim3((unsigned)((ngroups + 255) / 256)), dim3(256), 0, sA, cb);
    if (!dense_cfg)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chain_wave<PER_FAST, EMAX_FAST, WPB_FAST, false>),
                           dim3((ngroups + WPB_FAST - 1) / WPB_FAST), dim3(WPB_FAST * 64), 0, sA, L,
                           (const LineIndex *)c->d_L, a.offset, a.eof, cb, 0, ngroups, 2);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chain_wave<PER_DENSE, EMAX_DENSE, WPB_DENSE, true>),
                           dim3((ngroups + WPB_DENSE - 1) / WPB_DENSE), dim3(WPB_DENSE * 64), 0, sA, L,
                           (const LineIndex *)c->d_L, a.offset, a.eof, cb, 0, ngroups, 2);
    // the groups that do not fit the kernel above (dense tiles) and whose entry is known: walked
    hipLaunchKernelGGL(k_dense_walk, dim3((unsigned)((ngroups + 3) / 4)), dim3(256), 0, sA, L, cb, a.offset, a.eof, 0, dense_cfg ? 1 : 0, c->ctl, 0);
    return enqueue_resolve(c, st, cb, false);
}

// general path: chain summaries -> resolve -> expand -> finalize (publishes) [-> decode]
static int enqueue_general(ffq_ctx *c, ScanState &st, const LineIndex &L, bool timed = false)
{
    const ScanArgs &a = st.a;
    const bool dense_cfg = st.dense_cfg;
    const int ngroups = st.ngroups;
    const int nmax = dense_cfg ? NMAX_DENSE : NMAX_FAST;
    int rc = reserve_stage(c, ngroups, nmax);
    if (rc) return rc;
    rc = reserve_dstage(c, 64);             // (8 MiB to start with; a scan that walks more groups asks for more: ERR_DSTAGE)
    if (rc) return rc;
    ChainBufs cb = chain_bufs(c, ngroups, nmax);
    hipStream_t sA = c->stream;
    HIPCHK(hipMemsetAsync(cb.flags, 0, (2 * (size_t)ngroups + 3) * 4, sA));      // flags, and: no group has a chunk of the walked groups' stage yet
    const bool lite = plan_lite(st, c->mem, scan_switches());
    if (lite) {
        // ordinary groups by the lean kernel; what it declines (flag bit 3) goes to k_chain_wave right behind.  The groups it
        // cannot take by their place -- the first one (sentinel, search offset), the last ones (the buffer's end) -- are
        // k_chain_wave's from the start: two small launches IN FRONT of the lean kernel's, which is dispatched without a barrier
        // so that their one-wave latency (30 us) runs under it (all three read the same finished line index and write different
        // groups' summaries)
        const int gl = lite_first_end_group(a.n_bytes, L.ntiles, ngroups);
        // (round 5: those groups go onto the lean kernel's list of declined groups and are run by the list kernel behind
        // it with whatever else was declined -- one launch of one-wave latency instead of three, and none in FRONT of the lean
        // kernel, where round 4's ordinary launch of the first group held the whole GPU for 29 us)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chain_lite<WPB_LITE>), dim3((ngroups + WPB_LITE - 1) / WPB_LITE), dim3(WPB_LITE * 64), 0, sA,
                           L, a.offset, cb, ngroups, gl);
    }
    if (lite)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chain_wave_list<PER_FAST, EMAX_FAST, WPB_FAST, false>),
                           dim3(std::min((ngroups + WPB_FAST - 1) / WPB_FAST, 4096)), dim3(WPB_FAST * 64), 0, sA, L,
                           (const LineIndex *)c->d_L, a.offset, a.eof, cb);
    else if (!dense_cfg)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chain_wave<PER_FAST, EMAX_FAST, WPB_FAST, false>),
                           dim3((ngroups + WPB_FAST - 1) / WPB_FAST), dim3(WPB_FAST * 64), 0, sA, L,
                           (const LineIndex *)c->d_L, a.offset, a.eof, cb, 0, ngroups, 0);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_chain_wave<PER_DENSE, EMAX_DENSE, WPB_DENSE, true>),
                           dim3((ngroups + WPB_DENSE - 1) / WPB_DENSE), dim3(WPB_DENSE * 64), 0, sA, L,
                           (const LineIndex *)c->d_L, a.offset, a.eof, cb, 0, ngroups, 0);
    // the groups the kernel above declined (dense tiles), each from a guessed entry
    hipLaunchKernelGGL(k_dense_walk, dim3((unsigned)std::min((ngroups + 3) / 4, 1024)), dim3(256), 0, sA, L, cb, a.offset, a.eof, 1,
                       dense_cfg ? 1 : 0, c->ctl, 1);
    return enqueue_resolve(c, st, cb, timed, lite);
}

// The row kernels' prologue: the newline counts of every superblock of SB_TILES tiles and their scan (k_sbscan) -- for a
// large buffer the per-superblock sums by many workgroups first (k_sum64), the scan kernel then only scans.
static void enqueue_sbscan(ffq_ctx *c, const LineIndex &L, int64_t ntiles, int nsb, int64_t offset)
{
    const unsigned int *presum = nullptr;
    if (nsb > 2048) {
        hipLaunchKernelGGL(k_sum64, dim3((unsigned)((nsb + 3) / 4)), dim3(256), 0, c->stream, (const uint32_t *)c->cnt, 1,
                           (int64_t)ntiles, c->sbq, nsb);
        presum = c->sbq;
    }
    hipLaunchKernelGGL(k_sbscan, dim3(1), dim3(1024), 0, c->stream, L, nsb, c->sbbase, offset, c->hdr4, presum);
}

// The end of every front: ev[3] behind its last kernel (its result block is in host memory), and the stream now ends in
// a scan front of `c` (StreamTail)
static int end_front(ffq_ctx *c, const ScanState &st)
{
    const ScanArgs &a = st.a;
    c->pub_seq = 0;                       // (publishers of later tiers, enqueued at the wait, signal with events)
    if (!st.poll_seq) HIPCHK(hipEventRecord(c->ev[3], c->stream));
    HIPCHK(hipGetLastError());
    StreamTail &tl = c->owner->tail;
    tl.is_scan = true;
    tl.out_p[0] = a.d_table; tl.out_n[0] = (size_t)a.table_cap * 48;
    tl.out_p[1] = st.decode ? a.d_qual : nullptr; tl.out_n[1] = st.decode ? (size_t)a.qual_cap : 0;
    tl.out_p[2] = st.decode ? a.d_qoff : nullptr; tl.out_n[2] = st.decode ? ((size_t)a.table_cap + 1) * 8 : 0;
    return FFQ_OK;
}

// The four-line rows of a front: k_sbscan -> k_rows4<...> -> k_finalize4.  `o` is what the row kernel writes for the decode
// beside the table (all null: the rows only) and the single pass's verdict word for k_finalize4.
struct Rows4Out {
    bool zero_tileq; uint32_t *qrel; int64_t *p4s; int64_t p4_cap;       // the fast path's own decode
    int64_t fz_stride; const uint8_t *fz_phase; int64_t *fz_qoff;       // the single pass: its layout, per-tile phases, offsets
    const uint32_t *fz_bad;
};
static int enqueue_rows4(ffq_ctx *c, const ScanState &st, const LineIndex &L, decltype(&k_rows4<0, false>) rows4, const Rows4Out &o,
                         const Pub &pub)
{
    const ScanArgs &a = st.a;
    hipStream_t sA = c->stream;
    enqueue_sbscan(c, L, st.ntiles, (int)((st.ntiles + SB_TILES - 1) / SB_TILES), a.offset);
    if (o.zero_tileq) HIPCHK(hipMemsetAsync(c->tileq, 0, (size_t)st.ntiles * sizeof(TileQ), sA));
    hipLaunchKernelGGL(rows4, dim3((unsigned)((st.ntiles + 3) / 4)), dim3(256), 0, sA, L, (const long long *)c->sbbase, a.eof, a.add,
                       c->hdr4, c->tinfo4, a.d_table, a.table_cap, o.qrel, c->tileq, o.p4s, o.p4_cap, o.fz_stride, o.fz_phase, o.fz_qoff);
    hipLaunchKernelGGL(k_finalize4, dim3(1), dim3(64), 0, sA, L, c->hdr4, (const TermInfo4 *)c->tinfo4, a.eof, a.offset, a.add,
                       (const int64_t *)a.d_table, a.table_cap, c->dres, pub, o.fz_bad);
    return FFQ_OK;
}

// front of a scan: everything on ONE in-order stream (the context's), no host synchronisation
// and no copy or fill between the kernels:
//     k_scan_lines -> (k_sbscan -> k_rows4 -> k_finalize4)  or  (general kernels) [-> decode]
// The ragged last tile of the buffer rides along in the index kernel's launch (workgroup 0's
// second tile).  The last result-writing kernel publishes the result block into host-mapped
// memory and zeroes the control block for the next scan; ev[3] follows the last kernel.  A
// second context on the same stream queues its front right behind: the GPU never idles.  Which front: plan_front
// (ffq_scanwalk.h); this function launches what the plan says.
static int enqueue_front(ffq_ctx *c, ScanState &st)
{
    const ScanArgs &a = st.a;
    const bool decode = st.decode;
    hipStream_t sA = c->stream;
    const int64_t ntiles = st.ntiles;
    const int nsb = (int)((ntiles + SB_TILES - 1) / SB_TILES);
    const FrontPlan p = plan_front(st, c->mem, CallFacts{a.offset, a.qual_cap, a.n_bytes, (reinterpret_cast<uintptr_t>(a.d_qual) & 15) == 0},
                                   scan_switches());
    const LineIndex L = make_index(c, a, ntiles);
    c->decode_timed = false;
    st.poll_seq = p.polled ? ++c->seq : 0;
    c->pub_seq = st.poll_seq;
    c->ctl_was_clean = c->ctl_clean;
    if (!c->ctl_clean) HIPCHK(hipMemsetAsync(c->ctl, 0, sizeof(Ctl), sA));    // first scan, or an abandoned front
    c->ctl_clean = false;
    const Rows4Out rows_only{false, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr};

    if (p.front == FRONT_FUSED) {
        // ---- four-line input with the decode: index AND decoded stream in one pass over the bytes ---------
        int rc = enqueue_fused_index(c, a, ntiles, p.in_place);
        if (rc) return rc;
        rc = enqueue_rows4(c, st, L, p.in_place ? k_rows4<2, false> : k_rows4<1, false>,
                           Rows4Out{false, nullptr, nullptr, a.table_cap, (int64_t)(p.in_place ? TILE : SG_STRIDE), c->fz_qphase, a.d_qoff, c->fz_bad},
                           no_pub(c));
        if (rc) return rc;
        hipLaunchKernelGGL(k_qtotal4, dim3(1), dim3(1), 0, sA, c->dres, (const int64_t *)a.d_table, a.table_cap,
                           a.d_qoff, make_pub(c));
        c->ctl_clean = true;
        return end_front(c, st);
    }

    // ---- line index --------------------------------------------------------------------
    // the index kernel without a barrier in front of it only where the library itself can vouch for it (StreamTail)
    bool any_order = p.untimed && c->ctl_was_clean;
    {
        const StreamTail &tl = c->owner->tail;
        if (!tl.is_scan || tl.exposed) any_order = false;
        const uintptr_t b0 = reinterpret_cast<uintptr_t>(a.d_buf), b1 = b0 + (size_t)a.n_bytes;
        for (int i = 0; i < 3 && any_order; i++) {
            const uintptr_t o0 = reinterpret_cast<uintptr_t>(tl.out_p[i]), o1 = o0 + tl.out_n[i];
            if (tl.out_p[i] && o0 < b1 && b0 < o1) any_order = false;
        }
    }
    if (!p.untimed) HIPCHK(hipEventRecord(c->ev[0], sA));
    if (p.run_index)             // (a later tier of the same scan: the index is there already)
        launch_scan_lines(c, sA, a.d_buf, a.n_bytes, ntiles, L, (uint32_t)'@', any_order && !p.wide,
                          p.wide ? a.d_qual : (int8_t *)nullptr, a.qual_add);
    if (!p.untimed) HIPCHK(hipEventRecord(c->ev[1], sA));

    if (p.front == FRONT_FAST4) {
        // ---- plain four-line records: rows straight from newline ordinals, then validated -----
        const Rows4Out with_decode{true, c->qrel, c->p4s, std::min<int64_t>(a.table_cap, c->p4s.cap), 0, nullptr, nullptr, nullptr};
        int rc = enqueue_rows4(c, st, L, p.dense4 ? k_rows4<false, true> : k_rows4<false, false>, decode ? with_decode : rows_only,
                               decode ? no_pub(c) : make_pub(c));
        if (rc) return rc;
        if (decode) {
            // quality offsets: superblock sums + scan, per-tile fix-up (+ stream directory), total
            // (publishes); then the decode itself.  All of it is skipped on the device if the
            // fast path is rejected.
            hipLaunchKernelGGL(k_sum64, dim3((unsigned)((nsb + 3) / 4)), dim3(256), 0, sA,
                               reinterpret_cast<const uint32_t *>(c->tileq.p) + 3, 4, (int64_t)ntiles, c->sbq, nsb);
            hipLaunchKernelGGL(k_qscan4, dim3(1), dim3(1024), 0, sA, (const unsigned int *)c->sbq, nsb, c->sbqbase);
            hipLaunchKernelGGL(k_qfix4, dim3((unsigned)((ntiles + 7) / 8)), dim3(256), 0, sA, (int)ntiles,
                               (const Fast4Hdr *)c->hdr4, (const TileQ *)c->tileq, (const long long *)c->sbqbase,
                               (const uint32_t *)c->qrel, a.d_qoff, std::min<int64_t>(a.table_cap, c->p4s.cap), c->qdir,
                               c->qdir.cap);
            hipLaunchKernelGGL(k_qtotal4, dim3(1), dim3(1), 0, sA, c->dres, (const int64_t *)a.d_table, a.table_cap,
                               a.d_qoff, make_pub(c));
            enqueue_decode(c, a, sA, true);
        }
        c->ctl_clean = true;
        return end_front(c, st);
    }
    if (p.probe4) {
        // has the input turned plain four-line again?  The fast path's kernels (rows into the caller's
        // table, which the general kernels then write again; no decode tail), their verdict left in
        // DevRes::fast4_hint for the publisher of the general path to carry out
        int rc = enqueue_rows4(c, st, L, p.dense4 ? k_rows4<false, true> : k_rows4<false, false>, rows_only, no_pub(c));
        if (rc) return rc;
    }
    if (p.front == FRONT_GENERAL) {
        int rc = enqueue_general(c, st, L, true);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(k_publish, dim3(1), dim3(1), 0, sA, c->dres, make_pub(c), 1);
        c->ctl_clean = true;
    }
    return end_front(c, st);
}

template <class T>
static int grow_dev(ffq_ctx *c, DevBuf<T> &b, int64_t need);

// Exclusive scan of the nv values v[] (u32 counts or int64; hipMalloc'ed) into out[] on stream st -- out may be v -- and the
// total where `total` puts it (ScanToWord, ScanToRes: ffq_scan.h).  One workgroup for short arrays, two levels for long ones;
// the middle level scans the blocks' sums in place and its total is the array's.
template <class T, class Total>
static int launch_scan(ffq_ctx *c, hipStream_t st, const T *v, int64_t nv, long long *out, Total total)
{
    if (nv <= scan_one_max<T>()) {
        hipLaunchKernelGGL((k_scan_one<T, Total>), dim3(1), dim3(SCAN_ONE_WG), 0, st, v, nv, out, total);
        return FFQ_OK;
    }
    const int64_t nb = (nv + SCAN_BLK - 1) / SCAN_BLK;
    int rc = grow_dev(c, c->scan_bs, nb);
    if (rc) return rc;
    hipLaunchKernelGGL(k_scan_blksum<T>, dim3((unsigned)nb), dim3(SCAN_BLK_WG), 0, st, v, nv, c->scan_bs);
    hipLaunchKernelGGL((k_scan_one<long long, Total>), dim3(1), dim3(SCAN_ONE_WG), 0, st, (const long long *)c->scan_bs, nb, c->scan_bs, total);
    hipLaunchKernelGGL(k_scan_blkapply<T>, dim3((unsigned)nb), dim3(SCAN_BLK_WG), 0, st, v, nv, (const long long *)c->scan_bs, out);
    return FFQ_OK;
}

// ---- the list-ranking tier (ffq_ranked.h): exact on any input, cost per "\n@" match ----------------
// Its scratch comes in two groups, one per tile and one per candidate.  Each has ONE function that grows its buffers and
// then rebuilds c->rk from c->rm, whichever way the growing went (RankBufs::nc is the caller's); false: no memory.
static void rank_view(ffq_ctx *c)
{
    RankMem &M = c->rm;
    c->rk = RankBufs{M.tbase, M.cand, M.rec, M.succ, {M.S[0], M.S[1]}, {M.C[0], M.C[1]}, M.D, M.root, 0};
}

static bool rank_reserve_tiles(ffq_ctx *c, int64_t ntiles)
{
    RankMem &M = c->rm;
    const bool ok = M.tbase.grow(ntiles) == hipSuccess && M.root.grow(4) == hipSuccess;
    rank_view(c);
    return ok;
}

static bool rank_reserve_cands(ffq_ctx *c, int64_t nc)
{
    RankMem &M = c->rm;
    if (nc <= M.cand.cap) return true;             // (M.cand.cap stands for the group)
    M.cand.reset(); M.rec.reset(); M.succ.reset(); M.D.reset();
    for (int i = 0; i < 2; i++) { M.S[i].reset(); M.C[i].reset(); }
    const int64_t n = nc + (nc >> 3) + 1024;
    bool ok = M.cand.grow(n) == hipSuccess && M.rec.grow(n) == hipSuccess && M.succ.grow(n) == hipSuccess && M.D.grow(n) == hipSuccess;
    for (int i = 0; i < 2 && ok; i++) ok = M.S[i].grow(n) == hipSuccess && M.C[i].grow(n) == hipSuccess;
    if (!ok) M.cand.reset();                       // (the next scan asks again)
    rank_view(c);
    return ok;
}

// The tier in two halves around its host wait.  ranked_count: the candidates ("\n@" matches) per tile, their scan, the total
// back on the host in *nc.  ranked_emit: the ranking over nc candidates and the rows, published.  Both return FFQ_OK, or
// RK_CANNOT if the tier cannot run here (no memory: the caller then takes the one-wave walker); ranked_verdict
// (ffq_scanwalk.h) judges nc between them.
static int ranked_count(ffq_ctx *c, const LineIndex &L, int64_t ntiles, int64_t *nc)
{
    hipStream_t sA = c->stream;
    RankBufs &R = c->rk;
    if (!rank_reserve_tiles(c, ntiles)) return RK_CANNOT;
    if (c->col_res.grow(1) != hipSuccess) return RK_CANNOT;
    hipLaunchKernelGGL(k_rk_count, dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, sA, L, R.tbase);
    if (launch_scan(c, sA, (const long long *)R.tbase, ntiles, R.tbase, ScanToRes{c->col_res, 0})) return RK_CANNOT;
    HIPCHK(hipMemcpyAsync(c->h_word, &c->col_res->n_qual_bytes, sizeof(int64_t), hipMemcpyDeviceToHost, sA));
    HIPCHK(hipGetLastError());
    CTX_SYNC(c);
    *nc = c->h_word[0];
    return FFQ_OK;
}

static int ranked_emit(ffq_ctx *c, const ScanArgs &a, const LineIndex &L, int64_t ntiles, int64_t nc)
{
    hipStream_t sA = c->stream;
    RankBufs &R = c->rk;
    if (!rank_reserve_cands(c, nc)) { (void)hipGetLastError(); return RK_CANNOT; }
    R.nc = nc;
    const unsigned gthr = (unsigned)std::max<int64_t>((nc + 255) / 256, 1);
    if (nc > 0) {
        hipLaunchKernelGGL(k_rk_list, dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, sA, L, R);
        hipLaunchKernelGGL(k_rk_succ, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, sA, L, R, a.eof);
    }
    hipLaunchKernelGGL(k_rk_root, dim3(1), dim3(1024), 0, sA, L, R, a.offset, c->dres);
    int rounds = 0;
    while (((int64_t)1 << rounds) <= nc) rounds++;
    int cur = 0;
    for (int k = 0; k < rounds; k++, cur ^= 1)
        hipLaunchKernelGGL(k_rk_round, dim3(gthr), dim3(256), 0, sA, nc, (const uint32_t *)R.S[cur], (const uint32_t *)R.C[cur],
                           R.S[cur ^ 1], R.C[cur ^ 1], R.D, k);
    hipLaunchKernelGGL(k_rk_emit, dim3(gthr), dim3(256), 0, sA, L, R, a.eof, a.offset, a.add, a.d_table, a.table_cap, c->dres);
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(64), 0, sA, c->dres, (const int64_t *)a.d_table, a.table_cap, a.add, a.offset,
                       (int64_t *)nullptr, make_pub(c), -1);
    c->ctl_clean = true;
    HIPCHK(hipGetLastError());
    return FFQ_OK;
}

// quality offsets of a finished table (n rows known to the host) + the decode: the column kernels
// with columns 4 / 5 (what the fast path and k_expand do on the way, for the tiers that do not)
static int enqueue_offsets_and_decode(ffq_ctx *c, const ScanArgs &a, int64_t n_rows)
{
    hipStream_t sA = c->stream;
    if (n_rows <= 0 || n_rows > a.table_cap) {
        if (n_rows == 0) HIPCHK(hipMemsetAsync(a.d_qoff, 0, sizeof(int64_t), sA));     // qoff[0] = 0
        return FFQ_OK;
    }
    const int64_t nblk = (n_rows + 255) / 256;
    int rc = grow_dev(c, c->col_sum, nblk);
    if (rc) return rc;
    hipLaunchKernelGGL(k_col_sum, dim3((unsigned)nblk), dim3(256), 0, sA, (const int64_t *)a.d_table, n_rows, 4, 0, 5,
                       a.n_bytes, a.s, a.add, c->col_sum);
    // (the scan's totals go into the scan's own result block: the decode kernel and the host read them there)
    if ((rc = launch_scan(c, sA, (const long long *)c->col_sum, nblk, c->col_sum, ScanToRes{c->dres, n_rows}))) return rc;
    hipLaunchKernelGGL(k_col_offsets, dim3((unsigned)nblk), dim3(256), 0, sA, (const int64_t *)a.d_table, n_rows, 4, 0, 5,
                       a.n_bytes, a.s, a.add, (const long long *)c->col_sum, (const DevRes *)c->dres, a.d_qoff, c->p4s, c->qdir,
                       c->qdir.cap);
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(1), 0, sA, c->dres, make_pub(c), 0);
    enqueue_decode(c, a, sA);
    return FFQ_OK;
}

// ... and for a scan whose index pass decoded everything in place (ScanState::wide): only the offsets, qoff[i] = the
// offset pos4 has in the buffer, from the finished table
static int enqueue_offsets_in_place(ffq_ctx *c, const ScanArgs &a, int64_t n_rows)
{
    (void)n_rows;
    hipLaunchKernelGGL(k_qoff_in_place, dim3(256), dim3(256), 0, c->stream, c->dres, (const int64_t *)a.d_table, a.table_cap, a.add, a.s,
                       a.d_qoff, make_pub(c));
    return FFQ_OK;
}

// A tier scan_finish enqueues behind the front: marked by ev[4] / ev[2], waited for, its time added to ms_chain / ms_total.
template <class Enqueue>
static int run_tier(ffq_ctx *c, ffq_scan_result *res, Enqueue enqueue)
{
    HIPCHK(hipEventRecord(c->ev[4], c->stream));
    const int rc = enqueue();
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->ev[2], c->stream));
    HIPCHK(hipGetLastError());
    CTX_WAIT_EVENT(c, c->ev[2]);
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[4], c->ev[2]));
    res->ms_chain += ms; res->ms_total += ms;
    return FFQ_OK;
}

// the list-ranking tier behind a front: *how = RK_* (ffq_scanwalk.h); where it ran, with the quality offsets and the decode
// it does not do on the way, its time added like a tier's
static int ranked_tier(ffq_ctx *c, const ScanState &st, const LineIndex &L, ffq_scan_result *res, bool only_if_sparse, int *how)
{
    const ScanArgs &a = st.a;
    hipStream_t sA = c->stream;
    HIPCHK(hipEventRecord(c->ev[4], sA));
    int64_t nc = 0;
    int rr = ranked_count(c, L, st.ntiles, &nc);
    if (rr == FFQ_OK) rr = ranked_verdict(nc, a.n_bytes, only_if_sparse);
    if (rr == RK_GO) rr = ranked_emit(c, a, L, st.ntiles, nc);
    if (rr < 0) return rr;
    *how = rr;
    if (rr != RK_GO) return FFQ_OK;
    HIPCHK(hipEventRecord(c->ev[2], sA));
    CTX_WAIT_EVENT(c, c->ev[2]);
    if (st.decode && !c->h_res->fallback) {
        int rc = st.wide ? enqueue_offsets_in_place(c, a, c->h_res->n_records) : enqueue_offsets_and_decode(c, a, c->h_res->n_records);
        if (rc) return rc;
        HIPCHK(hipEventRecord(c->ev[2], sA));
        HIPCHK(hipGetLastError());
        CTX_WAIT_EVENT(c, c->ev[2]);
    }
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[4], c->ev[2]));
    res->ms_chain += ms; res->ms_total += ms;
    return FFQ_OK;
}

// the one-wave walk: exact on anything, one wave for the whole buffer
static int enqueue_walk(ffq_ctx *c, const ScanState &st, const LineIndex &L)
{
    const ScanArgs &a = st.a;
    hipStream_t sA = c->stream;
    const bool decode = st.decode;
    int64_t *const sq = (decode && !st.wide) ? a.d_qoff : (int64_t *)nullptr;       // (wide: the offsets from the finished table, below)
    hipLaunchKernelGGL(k_chain_serial, dim3(1), dim3(64), 0, sA, L, a.offset, a.eof, a.add, a.d_table,
                       a.table_cap, sq, c->qdir, c->qdir.cap, sq ? c->p4s : (int64_t *)nullptr,
                       sq ? std::min<int64_t>(a.table_cap, c->p4s.cap) : (int64_t)0, c->dres);
    hipLaunchKernelGGL(k_finalize_serial, dim3(1), dim3(64), 0, sA, c->dres, a.table_cap, sq, (decode && st.wide) ? no_pub(c) : make_pub(c));
    c->ctl_clean = true;
    if (decode && st.wide) hipLaunchKernelGGL(k_qoff_in_place, dim3(256), dim3(256), 0, sA, c->dres, (const int64_t *)a.d_table, a.table_cap, a.add, a.s, a.d_qoff, make_pub(c));
    else if (decode) enqueue_decode(c, a, sA);
    return FFQ_OK;
}

// wait for THIS scan's front only: the stream may already hold the next scan of a context that shares it
static int wait_front(ffq_ctx *c, const ScanState &st)
{
    if (st.poll_seq) {
        int rc = poll_seq(c, st.poll_seq);
        if (rc) return rc;
        // (the GPU is past this mark; the wait only lets the runtime note it before the mark is read)
        if (!st.untimed) CTX_WAIT_EVENT(c, c->ev[1]);
    } else CTX_WAIT_EVENT(c, c->ev[3]);
    return FFQ_OK;
}

// the times of a front that stood, from its marks (`untimed`, `had_index`: as the front was enqueued)
static int time_front(ffq_ctx *c, const ScanState &st, ffq_scan_result *res, bool untimed, bool had_index)
{
    float ms = 0;
    if (!untimed) HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    if (!had_index) res->ms_index = ms;
    res->ms_decode = 0;
    if (!st.poll_seq) {                // (a polled front has no end mark: its tail is not timed)
        HIPCHK(hipEventElapsedTime(&ms, c->ev[1], c->ev[3])); res->ms_chain += ms;
        if (c->decode_timed) {
            // the decode kernel is the tail of the front: split it off the chain time
            HIPCHK(hipEventElapsedTime(&ms, c->ev[6], c->ev[3]));
            res->ms_decode = ms; res->ms_chain -= ms;
        }
        HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[3])); res->ms_total += ms;
    }
    return FFQ_OK;
}

static Report read_report(const ffq_ctx *c, int ranked)
{
    const Ctl &k = *c->h_ctl;
    const DevRes &d = *c->h_res;
    Report r;
    r.err = k.err; r.pool_head = k.pool_head;
    r.fallback = d.fallback; r.fast4_hint = d.fast4_hint; r.fused_bad = d.fused_bad; r.fast4_dense = d.fast4_dense;
    r.bad_group = d.bad_group; r.bad_irregular = d.bad_irregular; r.n_bad = d.n_bad; r.n_declined = d.n_declined;
    r.approx_records = d.approx_records;
    r.ranked = ranked;
    return r;
}

// The scan from its first front (enqueued by the submit) to its result: wait, read the report, ask next_step
// (ffq_scanwalk.h), run what it says.
static int scan_finish(ffq_ctx *c, ScanState &st, ffq_scan_result *res)
{
    const ScanArgs &a = st.a;
    int ranked = RK_GO;
    int rc = wait_front(c, st);
    while (!rc) {
        const LineIndex L = make_index(c, a, st.ntiles);
        const bool untimed = st.untimed, had_index = st.index_done;
        const Step s = next_step(st, c->mem, read_report(c, ranked), scan_switches());
        if (s.front_counts && (rc = time_front(c, st, res, untimed, had_index))) return rc;
        bool front = false;
        switch (s.kind) {
        case STEP_DONE:
            fill_result(res, *c->h_res, s.path, s.retries);
            if (res->n_records > a.table_cap)
                return fail(FFQ_E_TABLE_FULL, "table holds %lld rows, the buffer has %lld records", (long long)a.table_cap,
                            (long long)res->n_records);
            if (st.decode && res->n_qual_bytes > a.qual_cap)
                return fail(FFQ_E_TABLE_FULL, "quality buffer holds %lld bytes, %lld needed", (long long)a.qual_cap,
                            (long long)res->n_qual_bytes);
            return FFQ_OK;
        case STEP_FAIL: return fail(s.code, "%s", s.text);
        case STEP_FRONT: front = true; break;
        case STEP_GROW_POOL: rc = reserve_pool(c, s.n); front = true; break;
        case STEP_GROW_STAGE: {
            uint32_t asked = 0;
            HIPCHK(hipMemcpy(&asked, c->cb.flags + 2 * (size_t)st.ngroups, sizeof asked, hipMemcpyDeviceToHost));
            rc = reserve_dstage(c, stage_chunks(asked, c->cb.dchunks));
            front = true;
            break;
        }
        case STEP_GENERAL: rc = run_tier(c, res, [&] { return enqueue_general(c, st, L); }); break;
        case STEP_REPAIR: rc = run_tier(c, res, [&] { return enqueue_repair(c, st, L); }); break;
        case STEP_RANKED: rc = ranked_tier(c, st, L, res, s.only_if_sparse, &ranked); break;
        case STEP_WALK: rc = run_tier(c, res, [&] { return enqueue_walk(c, st, L); }); break;
        }
        if (front && !rc) rc = enqueue_front(c, st);
        if (front && !rc) rc = wait_front(c, st);
    }
    return rc;
}

// the scratch a scan of n_bytes needs (grow-only: a second call with the same sizes does nothing)
static int scan_reserve(ffq_ctx *c, int64_t n_bytes, uint32_t flags, int64_t table_cap, int64_t qual_cap)
{
    const int64_t ntiles = tiles_for(n_bytes);
    if (ntiles == 0 || ntiles > 0x7FFFFFF0) return FFQ_OK;          // (nothing to enqueue / refused by the submit)
    int rc = reserve_tiles(c, ntiles);
    if (!rc) rc = reserve_pool(c, POOL_MIN);
    if (!rc && (flags & FFQ_F_DECODE_QUAL)) rc = reserve_qdir(c, qdir_blocks(n_bytes, qual_cap));
    if (!rc && (flags & FFQ_F_DECODE_QUAL)) rc = reserve_p4s(c, p4s_need(n_bytes, table_cap));
    return rc;
}

extern "C" int ffq_scan_submit(ffq_ctx *c, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t offset,
                               int eof, int64_t add, uint32_t flags, int qual_add, int64_t *d_table,
                               int64_t table_cap, int8_t *d_qual, int64_t qual_cap, int64_t *d_qoff)
{
    if (!c) return fail(FFQ_E_ARG, "ffq_scan_submit: ctx is NULL");
    if (c->pend.active) return fail(FFQ_E_ARG, "ffq_scan_submit: a scan is already pending on this context");
    if (n_bytes < 0 || offset < 0 || table_cap < 0) return fail(FFQ_E_ARG, "ffq_scan: negative size");
    if (n_bytes > 0 && !d_buf) return fail(FFQ_E_ARG, "ffq_scan: d_buf is NULL");
    if ((reinterpret_cast<uintptr_t>(d_buf) & 15) != 0) return fail(FFQ_E_ARG, "ffq_scan: d_buf must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_table) & 15) != 0) return fail(FFQ_E_ARG, "ffq_scan: d_table must be 16-byte aligned");
    if (table_cap > 0 && !d_table) return fail(FFQ_E_ARG, "ffq_scan: d_table is NULL");
    const bool decode = (flags & FFQ_F_DECODE_QUAL) != 0;
    if (decode && (!d_qual || !d_qoff)) return fail(FFQ_E_ARG, "ffq_scan: FFQ_F_DECODE_QUAL needs d_qual and d_qoff");
    HIPCHK(hipSetDevice(c->device));
    ScanState &st = c->pend;
    st = ScanState{};
    st.a = ScanArgs{d_buf, n_bytes, sentinel ? 1 : 0, offset, eof, add, flags, qual_add, d_table, table_cap,
                    d_qual, qual_cap, d_qoff};
    st.serial = (flags & FFQ_F_FORCE_SERIAL) != 0;
    st.decode = decode;
    st.single_pass = (flags & FFQ_F_SINGLE_PASS) != 0;
    st.force_ranked = (flags & FFQ_F_FORCE_RANKED) != 0;
    st.force_general = (flags & FFQ_F_FORCE_GENERAL) != 0;
    st.poll_result = (flags & FFQ_F_POLL_RESULT) != 0;
    st.no_timing = (flags & FFQ_F_NO_TIMING) != 0;
    st.ntiles = tiles_for(n_bytes);
    st.active = true;
    if (st.ntiles == 0) return FFQ_OK;                   // nothing to enqueue: ffq_scan_wait fills the result
    if (st.ntiles > 0x7FFFFFF0) { st.active = false; return fail(FFQ_E_ARG, "buffer too large"); }
    int rc = scan_reserve(c, n_bytes, flags, table_cap, qual_cap);
    if (!rc) {
        st.ngroups = (int)groups_for(st.ntiles);
        rc = enqueue_front(c, st);
    }
    if (rc) st.active = false;
    return rc;
}

extern "C" int ffq_scan_wait(ffq_ctx *c, ffq_scan_result *res)
{
    if (!c || !res) return fail(FFQ_E_ARG, "ffq_scan_wait: ctx/res is NULL");
    if (!c->pend.active) return fail(FFQ_E_ARG, "ffq_scan_wait: no scan is pending on this context");
    memset(res, 0, sizeof *res);
    HIPCHK(hipSetDevice(c->device));
    ScanState &st = c->pend;
    st.active = false;
    if (st.ntiles == 0) {
        // empty data: with a sentinel the buffer is "\n", no "\n@" can match
        res->end_state = st.a.eof ? FFQ_END_OK : FFQ_END_REFILL;
        res->last_status = FFQ_POS_HEAD_BEG;
        res->end_offset = st.a.offset;
        for (int i = 0; i < 6; i++) res->last_pos[i] = -1;
        if (st.decode) {
            HIPCHK(hipMemsetAsync(st.a.d_qoff, 0, sizeof(int64_t), c->stream));
            CTX_SYNC(c);
        }
        return FFQ_OK;
    }
    return scan_finish(c, st, res);
}

extern "C" int ffq_scan_device(ffq_ctx *c, const uint8_t *d_buf, int64_t n_bytes, int sentinel,
                               int64_t offset, int eof, int64_t add, uint32_t flags, int qual_add,
                               int64_t *d_table, int64_t table_cap, int8_t *d_qual,
                               int64_t qual_cap, int64_t *d_qoff, ffq_scan_result *res)
{
    if (!c || !res) return fail(FFQ_E_ARG, "ffq_scan_device: ctx/res is NULL");
    int rc = ffq_scan_submit(c, d_buf, n_bytes, sentinel, offset, eof, add, flags, qual_add, d_table, table_cap,
                             d_qual, qual_cap, d_qoff);
    if (rc) return rc;
    return ffq_scan_wait(c, res);
}

// a buffer of the table utilities and the host-buffer entry points: at least 65536 elements, so that small calls of
// growing sizes do not each reallocate
template <class T>
static int grow_dev(ffq_ctx *c, DevBuf<T> &b, int64_t need)
{
    if (need <= b.cap) return FFQ_OK;
    CTX_SYNC(c);
    const hipError_t e = b.grow(std::max<int64_t>(need, 1 << 16));
    if (e != hipSuccess) return fail(FFQ_E_NOMEM, "hipMalloc failed: %s", hipGetErrorString(e));
    return FFQ_OK;
}

// ---- staging of the host-buffer entry points --------------------------------------------------
constexpr int64_t STAGE_CH = 8 << 20;

static int stage_setup(ffq_ctx *c, int64_t ch = STAGE_CH)
{
    if (c->stage_h.cap < 3 * ch) {
        NearGpu near(c);
        const hipError_t e = c->stage_h.grow(3 * ch);
        if (e != hipSuccess) return fail(FFQ_E_NOMEM, "hipHostMalloc failed: %s", hipGetErrorString(e));
    }
    for (auto &st : c->stage_cs)
        if (!st) HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (auto &r : c->stage_ev)
        for (auto &e : r)
            if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (!ctx_pool(c)) return fail(FFQ_E_NOMEM, "out of host memory");
    return FFQ_OK;
}

// device -> pageable host memory: chunks over the link into the pinned slots (after whatever the
// scan stream holds), out of them by the helper threads; the copy out of chunk k runs while chunk
// k+1 is on the link
static int stage_d2h(ffq_ctx *c, void *h_dst, const void *d_src, int64_t bytes)
{
    if (bytes <= 0) return FFQ_OK;
    int rc = stage_setup(c);
    if (rc) return rc;
    uint8_t *dst = static_cast<uint8_t *>(h_dst);
    const uint8_t *src = static_cast<const uint8_t *>(d_src);
    const int64_t nch = (bytes + STAGE_CH - 1) / STAGE_CH;
    bool busy[3] = {false, false, false};               // a host copy out of the slot is in flight
    for (int64_t k = 0; k <= nch; k++) {
        if (k < nch) {
            const int b = (int)(k % 3);
            if (busy[b]) { c->helpers->wait(&c->stage_cr[b]); busy[b] = false; }
            const int64_t at = k * STAGE_CH, m = std::min<int64_t>(STAGE_CH, bytes - at);
            HIPCHK(hipMemcpyAsync(c->stage_h + b * STAGE_CH, src + at, (size_t)m, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipEventRecord(c->stage_ev[b][0], c->stream));
        }
        if (k > 0) {
            const int b = (int)((k - 1) % 3);
            const int64_t at = (k - 1) * STAGE_CH, m = std::min<int64_t>(STAGE_CH, bytes - at);
            HIPCHK(hipEventSynchronize(c->stage_ev[b][0]));
            c->helpers->enqueue_copy(dst + at, c->stage_h + b * STAGE_CH, m, &c->stage_cr[b]);
            busy[b] = true;
        }
    }
    for (int b = 0; b < 3; b++)
        if (busy[b]) c->helpers->wait(&c->stage_cr[b]);
    return FFQ_OK;
}

// ---- a byte range of a file into device memory ----------------------------------------------------------------------
// (/root/reference/src/fastqandfurious.py:30-36 `read(fh, fbufsize)`, for a range that stays resident: a shard of a
// file, ffq_shard.h)  pread in slices by the helper threads into three pinned slots of 32 MiB, each slot over the link
// in two halves on the two copy streams while the next one is read; the context's stream waits for the last copies.
constexpr int64_t FSTAGE_CH = 32 << 20;

static int stage_fd2d(ffq_ctx *c, uint8_t *d_dst, int fd, int64_t pos, int64_t n, int64_t *got)
{
    *got = 0;
    if (n <= 0) return FFQ_OK;
    int rc = stage_setup(c, FSTAGE_CH);
    if (rc) return rc;
    mark_other(c);
    // the copies start behind whatever the scan stream holds (a scan in flight may still read d_dst)
    hipEvent_t front = nullptr;
    HIPCHK(hipEventCreateWithFlags(&front, hipEventDisableTiming));
    hipError_t e = hipEventRecord(front, c->stream);
    for (auto &st : c->stage_cs) if (e == hipSuccess) e = hipStreamWaitEvent(st, front, 0);
    (void)hipEventDestroy(front);
    if (e != hipSuccess) return fail(FFQ_E_HIP, "ffq_load_fd: %s", hipGetErrorString(e));
    bool used[3] = {false, false, false};
    const int64_t nch = (n + FSTAGE_CH - 1) / FSTAGE_CH;
    int64_t k_enq = 0, k = 0;
    static const int ablate = (PROBES && getenv("FFQ_LOAD_ABLATE")) ? atoi(getenv("FFQ_LOAD_ABLATE")) : 0;     // 1: no copies, 2: no reads, 4: one copy stream
    bool ended = false;
    for (; k < nch && !ended && !rc; k++) {
        for (; k_enq < nch && k_enq - k < 3; k_enq++) {
            const int b = (int)(k_enq % 3);
            if (used[b]) { (void)hipEventSynchronize(c->stage_ev[b][0]); (void)hipEventSynchronize(c->stage_ev[b][1]); }
            const int64_t at = k_enq * FSTAGE_CH;
            if (ablate & 2) { std::lock_guard<std::mutex> lk(c->helpers->m); ChunkRead &cr = c->stage_cr[b]; cr.nsl = 1; cr.left = 0; cr.got[0] = cr.want[0] = std::min<int64_t>(FSTAGE_CH, n - at); }
            else c->helpers->enqueue(fd, c->stage_h + b * FSTAGE_CH, std::min<int64_t>(FSTAGE_CH, n - at), pos + at, &c->stage_cr[b]);
        }
        const int b = (int)(k % 3);
        const int64_t at = k * FSTAGE_CH, want = std::min<int64_t>(FSTAGE_CH, n - at);
        c->helpers->wait(&c->stage_cr[b]);
        const int64_t m = c->stage_cr[b].total();
        if (m < 0) { rc = fail(FFQ_E_ARG, "ffq_load_fd: read failed at byte %lld: %s", (long long)(pos + at), strerror(errno)); break; }
        if (m < want) ended = true;                       // the file ends here
        const int64_t half = (ablate & 4) ? m : ((m / 2) + 4095) & ~(int64_t)4095;
        for (int h = 0; h < 2 && !rc; h++) {
            const int64_t a = h ? std::min(half, m) : 0, z = h ? m : std::min(half, m);
            if (z > a && !(ablate & 1)) e = hipMemcpyAsync(d_dst + at + a, c->stage_h + b * FSTAGE_CH + a, (size_t)(z - a), hipMemcpyHostToDevice, c->stage_cs[h]);
            if (e == hipSuccess) e = hipEventRecord(c->stage_ev[b][h], c->stage_cs[h]);
            if (e != hipSuccess) rc = fail(FFQ_E_HIP, "ffq_load_fd: chunk copy failed: %s", hipGetErrorString(e));
        }
        used[b] = true;
        *got += m;
    }
    // reads queued past the end of the file (or past an error) still write into the slots
    for (int64_t j = k; j < k_enq; j++) c->helpers->wait(&c->stage_cr[j % 3]);
    // the slots belong to the next caller when this returns: the copies out of them are waited for here (the bytes
    // are then in d_dst for whatever is enqueued next, on any stream)
    for (int b = 0; b < 3; b++)
        if (used[b])
            for (int h = 0; h < 2; h++)
                if ((e = hipEventSynchronize(c->stage_ev[b][h])) != hipSuccess && !rc) rc = fail(FFQ_E_HIP, "ffq_load_fd: %s", hipGetErrorString(e));
    return rc;
}

extern "C" int ffq_load_fd(ffq_ctx *c, int fd, int64_t pos, int64_t n_bytes, void *d_dst, int64_t *n_loaded)
{
    if (!c || fd < 0 || pos < 0 || n_bytes < 0 || (n_bytes > 0 && !d_dst)) return fail(FFQ_E_ARG, "ffq_load_fd: bad argument");
    HIPCHK(hipSetDevice(c->device));
    int64_t got = 0;
    const int rc = stage_fd2d(c, static_cast<uint8_t *>(d_dst), fd, pos, n_bytes, &got);
    if (n_loaded) *n_loaded = got;
    return rc;
}

extern "C" int ffq_scan_host(ffq_ctx *c, const uint8_t *h_buf, int64_t n_bytes, int sentinel,
                             int64_t offset, int eof, int64_t add, uint32_t flags, int qual_add,
                             int64_t *h_table, int64_t table_cap, int8_t *h_qual, int64_t qual_cap,
                             int64_t *h_qoff, ffq_scan_result *res)
{
    mark_other(c);
    if (!c || !res) return fail(FFQ_E_ARG, "ffq_scan_host: ctx/res is NULL");
    if (n_bytes < 0 || table_cap < 0 || qual_cap < 0) return fail(FFQ_E_ARG, "ffq_scan_host: negative size");
    if (n_bytes > 0 && !h_buf) return fail(FFQ_E_ARG, "ffq_scan_host: h_buf is NULL");
    const bool decode = (flags & FFQ_F_DECODE_QUAL) != 0;
    if (decode && (!h_qual || !h_qoff)) return fail(FFQ_E_ARG, "ffq_scan_host: FFQ_F_DECODE_QUAL needs h_qual and h_qoff");
    HIPCHK(hipSetDevice(c->device));
    int rc;
    if ((rc = grow_dev(c, c->stage_d, n_bytes + 16))) return rc;
    if ((rc = grow_dev(c, c->tab_d, std::max<int64_t>(table_cap, 1) * 6))) return rc;
    if (decode) {
        if ((rc = grow_dev(c, c->qual_d, std::max<int64_t>(qual_cap, 16)))) return rc;
        if ((rc = grow_dev(c, c->qoff_d, table_cap + 1))) return rc;
    }
    // pageable -> device: three pinned staging slots, filled by the helper threads (slices of a
    // chunk in parallel), emptied over two copy streams (half a chunk each): the host copy of chunk
    // k+1 runs while chunk k is on the link
    rc = stage_setup(c);
    if (rc) return rc;
    bool used[3] = {false, false, false};
    const int64_t nch = (n_bytes + STAGE_CH - 1) / STAGE_CH;
    for (int64_t k_enq = 0, k = 0; k < nch; k++) {
        // keep the helper threads fed: the host copies of up to three chunks are queued at a time
        // (a slot is free again once the link copy out of it, three chunks back, is through)
        for (; k_enq < nch && k_enq - k < 3; k_enq++) {
            const int b = (int)(k_enq % 3);
            if (used[b]) { HIPCHK(hipEventSynchronize(c->stage_ev[b][0])); HIPCHK(hipEventSynchronize(c->stage_ev[b][1])); }
            const int64_t at = k_enq * STAGE_CH;
            c->helpers->enqueue_copy(c->stage_h + b * STAGE_CH, h_buf + at, std::min<int64_t>(STAGE_CH, n_bytes - at), &c->stage_cr[b]);
        }
        const int b = (int)(k % 3);
        const int64_t at = k * STAGE_CH, m = std::min<int64_t>(STAGE_CH, n_bytes - at);
        c->helpers->wait(&c->stage_cr[b]);
        const int64_t half = ((m / 2) + 4095) & ~(int64_t)4095;
        for (int h = 0; h < 2; h++) {
            const int64_t a = h ? std::min(half, m) : 0, z = h ? m : std::min(half, m);
            if (z > a)
                HIPCHK(hipMemcpyAsync(c->stage_d + at + a, c->stage_h + b * STAGE_CH + a, (size_t)(z - a), hipMemcpyHostToDevice,
                                      c->stage_cs[h]));
            HIPCHK(hipEventRecord(c->stage_ev[b][h], c->stage_cs[h]));
        }
        used[b] = true;
    }
    // the scan stream waits for the copies (the last event of each copy stream covers the earlier ones)
    for (int b = 0; b < 3; b++)
        if (used[b]) { HIPCHK(hipStreamWaitEvent(c->stream, c->stage_ev[b][0], 0)); HIPCHK(hipStreamWaitEvent(c->stream, c->stage_ev[b][1], 0)); }

    rc = ffq_scan_device(c, c->stage_d, n_bytes, sentinel, offset, eof, add, flags, qual_add, c->tab_d,
                         table_cap, decode ? c->qual_d : nullptr, qual_cap, decode ? c->qoff_d : nullptr, res);
    if (rc != FFQ_OK && rc != FFQ_E_TABLE_FULL) return rc;
    const int64_t rows = std::min<int64_t>(res->n_records, table_cap);
    int rc2 = stage_d2h(c, h_table, c->tab_d, rows * 48);
    if (!rc2 && decode) {
        rc2 = stage_d2h(c, h_qual, c->qual_d, std::min<int64_t>(res->n_qual_bytes, qual_cap));
        if (!rc2 && res->n_records <= table_cap) rc2 = stage_d2h(c, h_qoff, c->qoff_d, (rows + 1) * 8);
    }
    return rc2 ? rc2 : rc;
}

// ---- FASTA (ffq_fasta.h) --------------------------------------------------------------------
extern "C" int ffq_scan_fasta_device(ffq_ctx *c, const uint8_t *d_buf, int64_t n_bytes, int sentinel,
                                     int64_t offset, int64_t add, int64_t *d_table, int64_t table_cap,
                                     ffq_scan_result *res)
{
    mark_other(c);
    if (!c || !res) return fail(FFQ_E_ARG, "ffq_scan_fasta: ctx/res is NULL");
    if (n_bytes < 0 || offset < 0 || table_cap < 0) return fail(FFQ_E_ARG, "ffq_scan_fasta: negative size");
    if (n_bytes > 0 && !d_buf) return fail(FFQ_E_ARG, "ffq_scan_fasta: d_buf is NULL");
    if ((reinterpret_cast<uintptr_t>(d_buf) & 15) != 0) return fail(FFQ_E_ARG, "ffq_scan_fasta: d_buf must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_table) & 15) != 0) return fail(FFQ_E_ARG, "ffq_scan_fasta: d_table must be 16-byte aligned");
    if (table_cap > 0 && !d_table) return fail(FFQ_E_ARG, "ffq_scan_fasta: d_table is NULL");
    if (c->pend.active) return fail(FFQ_E_ARG, "ffq_scan_fasta: a scan is pending on this context");
    memset(res, 0, sizeof *res);
    HIPCHK(hipSetDevice(c->device));
    const int64_t ntiles = tiles_for(n_bytes);
    if (ntiles == 0) {
        // nothing but (at most) the sentinel: no "\n>" can match
        res->last_status = FFQ_POS_HEAD_BEG;
        res->end_offset = offset;
        for (int i = 0; i < 6; i++) res->last_pos[i] = -1;
        res->path = 4;
        return FFQ_OK;
    }
    if (ntiles > 0x7FFFFFF0) return fail(FFQ_E_ARG, "buffer too large");
    int rc = reserve_tiles(c, ntiles);
    if (!rc) rc = reserve_pool(c, POOL_MIN);
    if (!rc) rc = grow_dev(c, c->sel_cnt, ntiles);
    if (!rc) rc = grow_dev(c, c->sel_base, ntiles);
    if (rc) return rc;
    hipStream_t sA = c->stream;
    ScanArgs a{};
    a.d_buf = d_buf; a.n_bytes = n_bytes; a.s = sentinel ? 1 : 0;
    int attempt = 0;
    for (;; attempt++) {
        const LineIndex L = make_index(c, a, ntiles);
        if (!c->ctl_clean) HIPCHK(hipMemsetAsync(c->ctl, 0, sizeof(Ctl), sA));
        c->ctl_clean = false;
        HIPCHK(hipEventRecord(c->ev[0], sA));
        launch_scan_lines(c, sA, d_buf, n_bytes, ntiles, L, (uint32_t)'>');
        HIPCHK(hipEventRecord(c->ev[1], sA));
        const unsigned tb = (unsigned)((ntiles + 3) / 4);
        hipLaunchKernelGGL(k_fa_count, dim3(tb), dim3(256), 0, sA, L, offset, c->sel_cnt);
        { const int rs = launch_scan(c, sA, (const unsigned int *)c->sel_cnt, ntiles, c->sel_base, ScanToWord{(long long *)c->d_word.p}); if (rs) return rs; }
        hipLaunchKernelGGL(k_fa_rows, dim3(tb), dim3(256), 0, sA, L, offset, add, (const long long *)c->sel_base,
                           (const long long *)c->d_word.p, d_table, table_cap, c->fa_hdr, (const unsigned int *)c->sel_cnt);
        hipLaunchKernelGGL(k_fa_fix, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, sA, L, offset, add,
                           (const FaHdr *)c->fa_hdr, (const unsigned int *)c->sel_cnt, (const long long *)c->sel_base, d_table,
                           table_cap, c->dres, make_pub(c));
        c->ctl_clean = true;
        HIPCHK(hipEventRecord(c->ev[3], sA));
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventSynchronize(c->ev[3]));
        if (c->h_ctl->err & ERR_POOL) {
            if (attempt >= 2) return fail(FFQ_E_INTERNAL, "line-index pool overflow persists");
            rc = reserve_pool(c, std::max<unsigned long long>(c->h_ctl->pool_head + (c->h_ctl->pool_head >> 4), POOL_MIN));
            if (rc) return rc;
            continue;
        }
        break;
    }
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1])); res->ms_index = ms;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[1], c->ev[3])); res->ms_chain = ms;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[3])); res->ms_total = ms;
    fill_result(res, *c->h_res, 4, attempt);
    if (res->n_records > table_cap)
        return fail(FFQ_E_TABLE_FULL, "table holds %lld rows, the buffer has %lld FASTA entries", (long long)table_cap,
                    (long long)res->n_records);
    return FFQ_OK;
}

extern "C" int ffq_scan_fasta_host(ffq_ctx *c, const uint8_t *h_buf, int64_t n_bytes, int sentinel, int64_t offset,
                                   int64_t add, int64_t *h_table, int64_t table_cap, ffq_scan_result *res)
{
    mark_other(c);
    if (!c || !res) return fail(FFQ_E_ARG, "ffq_scan_fasta_host: ctx/res is NULL");
    if (n_bytes < 0 || table_cap < 0) return fail(FFQ_E_ARG, "ffq_scan_fasta_host: negative size");
    if (n_bytes > 0 && !h_buf) return fail(FFQ_E_ARG, "ffq_scan_fasta_host: h_buf is NULL");
    HIPCHK(hipSetDevice(c->device));
    int rc;
    if ((rc = grow_dev(c, c->stage_d, n_bytes + 16))) return rc;
    if ((rc = grow_dev(c, c->tab_d, std::max<int64_t>(table_cap, 1) * 6))) return rc;
    if (n_bytes > 0) HIPCHK(hipMemcpyAsync(c->stage_d, h_buf, (size_t)n_bytes, hipMemcpyHostToDevice, c->stream));
    rc = ffq_scan_fasta_device(c, c->stage_d, n_bytes, sentinel, offset, add, c->tab_d, table_cap, res);
    if (rc != FFQ_OK && rc != FFQ_E_TABLE_FULL) return rc;
    const int64_t rows = std::min<int64_t>(res->n_records, table_cap);
    if (rows > 0) HIPCHK(hipMemcpy(h_table, c->tab_d, (size_t)rows * 48, hipMemcpyDeviceToHost));
    return rc;
}

// ---- arrayadd ----------------------------------------------------------------
extern "C" int ffq_arrayadd_b_device(ffq_ctx *c, int8_t *d_a, int64_t n, int value)
{
    mark_other(c);
    if (!c || n < 0 || (n > 0 && !d_a)) return fail(FFQ_E_ARG, "ffq_arrayadd_b_device: bad argument");
    HIPCHK(hipSetDevice(c->device));
    if (n == 0) return FFQ_OK;
    const int64_t nv = (n + 15) / 16;
    const unsigned grid = (unsigned)std::min<int64_t>((nv + 255) / 256, 256 * 8);
    hipLaunchKernelGGL(k_arrayadd_b, dim3(std::max(grid, 1u)), dim3(256), 0, c->stream, (uint8_t *)d_a, n,
                       (uint32_t)(uint8_t)value);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return FFQ_OK;
}

extern "C" int ffq_arrayadd_q_device(ffq_ctx *c, int64_t *d_a, int64_t n, int64_t value)
{
    mark_other(c);
    if (!c || n < 0 || (n > 0 && !d_a)) return fail(FFQ_E_ARG, "ffq_arrayadd_q_device: bad argument");
    if ((reinterpret_cast<uintptr_t>(d_a) & 7) != 0) return fail(FFQ_E_ARG, "ffq_arrayadd_q_device: unaligned");
    HIPCHK(hipSetDevice(c->device));
    if (n == 0) return FFQ_OK;
    const unsigned grid = (unsigned)std::min<int64_t>((n / 2 + 255) / 256 + 1, 256 * 8);
    hipLaunchKernelGGL(k_arrayadd_q, dim3(grid), dim3(256), 0, c->stream, (unsigned long long *)d_a, n,
                       (unsigned long long)value);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return FFQ_OK;
}

extern "C" int ffq_arrayadd_b(ffq_ctx *c, int8_t *h_a, int64_t n, int value)
{
    mark_other(c);
    if (!c || n < 0 || (n > 0 && !h_a)) return fail(FFQ_E_ARG, "ffq_arrayadd_b: bad argument");
    HIPCHK(hipSetDevice(c->device));
    if (n == 0) return FFQ_OK;
    int rc = grow_dev(c, c->stage_d, n + 16);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c->stage_d, h_a, (size_t)n, hipMemcpyHostToDevice, c->stream));
    rc = ffq_arrayadd_b_device(c, (int8_t *)c->stage_d.p, n, value);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h_a, c->stage_d, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FFQ_OK;
}

extern "C" int ffq_arrayadd_q(ffq_ctx *c, int64_t *h_a, int64_t n, int64_t value)
{
    mark_other(c);
    if (!c || n < 0 || (n > 0 && !h_a)) return fail(FFQ_E_ARG, "ffq_arrayadd_q: bad argument");
    HIPCHK(hipSetDevice(c->device));
    if (n == 0) return FFQ_OK;
    int rc = grow_dev(c, c->stage_d, n * 8 + 16);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c->stage_d, h_a, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    rc = ffq_arrayadd_q_device(c, (int64_t *)c->stage_d.p, n, value);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h_a, c->stage_d, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FFQ_OK;
}

// ---- synthetic inputs ------------------------------------------------------------
extern "C" int ffq_synth_single(ffq_ctx *c, uint8_t *d_out, int64_t first, int64_t count, uint64_t seed)
{
    mark_other(c);
    if (!c || count < 0 || (count > 0 && !d_out)) return fail(FFQ_E_ARG, "ffq_synth_single: bad argument");
    HIPCHK(hipSetDevice(c->device));
    if (count == 0) return FFQ_OK;
    hipLaunchKernelGGL(k_synth_single, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream, d_out,
                       first, count, seed);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return FFQ_OK;
}

extern "C" int64_t ffq_synth_wrapped_size(int64_t i, uint64_t seed) { return synth_wrapped_size(i, seed); }

extern "C" int ffq_synth_wrapped(ffq_ctx *c, uint8_t *d_out, const int64_t *d_start, int64_t first,
                                 int64_t count, uint64_t seed)
{
    mark_other(c);
    if (!c || count < 0 || (count > 0 && (!d_out || !d_start))) return fail(FFQ_E_ARG, "ffq_synth_wrapped: bad argument");
    HIPCHK(hipSetDevice(c->device));
    if (count == 0) return FFQ_OK;
    hipLaunchKernelGGL(k_synth_wrapped, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream, d_out,
                       d_start, first, count, seed);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return FFQ_OK;
}

#ifdef FFQ_PROBES
// ---- probes: only in the instrumented build, libffq_probe.so (include/ffq_probe.h) ----------------------------------
// mode 6: the streaming-read ceiling of the device in the scan kernel's launch geometry with its non-temporal loads
// (k_read_probe), average ms over `reps` launches; every other mode is refused
extern "C" int ffq_read_probe(ffq_ctx *c, const uint8_t *d_buf, int64_t n_bytes, int mode, int reps, float *ms_avg)
{
    mark_other(c);
    if (!c || !d_buf || !ms_avg || n_bytes < TILE || reps < 1) return fail(FFQ_E_ARG, "ffq_read_probe: bad argument");
    if (mode != 6) return fail(FFQ_E_ARG, "ffq_read_probe: mode %d does not exist (6: the non-temporal read)", mode);
    HIPCHK(hipSetDevice(c->device));
    const int64_t ntiles = n_bytes >> TILE_SHIFT;
    uint32_t *sink = reinterpret_cast<uint32_t *>(c->ctl.p);
    for (int r = 0; r < reps + 2; r++) {
        if (r == 2) HIPCHK(hipEventRecord(c->ev[0], c->stream));
        hipLaunchKernelGGL(k_read_probe, dim3((unsigned)ntiles), dim3(256), 0, c->stream, d_buf, sink);
    }
    HIPCHK(hipEventRecord(c->ev[1], c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    *ms_avg = ms / reps;
    return FFQ_OK;
}
#endif  // FFQ_PROBES

// ---- diagnostics ---------------------------------------------------------------------
extern "C" int ffq_selftest(ffq_ctx *c)
{
    mark_other(c);
    if (!c) return fail(FFQ_E_ARG, "ffq_selftest: ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    const int NB = 256 * 16;
    uint8_t host[NB];
    uint64_t x = 12345;
    for (int i = 0; i < NB; i++) {
        x = splitmix64(x);
        const unsigned r = (unsigned)(x & 7);
        host[i] = (r == 0) ? '\n' : (r == 1) ? 0x0B : (r == 2) ? 0x8A : (r == 3) ? 0x00 : (uint8_t)(x >> 8);
    }
    uint8_t *d = nullptr;
    uint32_t *bad = nullptr;
    HIPCHK(hipMalloc((void **)&d, NB));
    HIPCHK(hipMalloc((void **)&bad, 4));
    HIPCHK(hipMemcpyAsync(d, host, NB, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(bad, 0, 4, c->stream));
    hipLaunchKernelGGL(k_selftest, dim3(1), dim3(256), 0, c->stream, d, bad);
    uint32_t hb = 0;
    HIPCHK(hipMemcpyAsync(&hb, bad, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    (void)hipFree(d);
    (void)hipFree(bad);
    if (hb) return fail(FFQ_E_INTERNAL, "device self-test: %u mismatches (wave scan / newline mask)", hb);
    return FFQ_OK;
}

#include "ffq_tables.h"
#include "ffq_gzread.h"
#include "ffq_stream.h"
#include "ffq_bgzf.h"
#include "ffq_shard.h"
#include "ffq_shard_host.h"

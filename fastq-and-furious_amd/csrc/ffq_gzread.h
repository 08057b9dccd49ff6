// ffq_gzread.h -- a gzip file behind a descriptor as a source of DECOMPRESSED bytes (host code of libffq_hip.so, no HIP
// in it; included by ffq_hip.hip, whose `fail` words the errors of ffq_bgzf.h behind it).  GzReader owns everything the
// inflate needs -- the compressed window, the zlib states, ONE BatchPool (ffq_pool.h) that the batch of BGZF members and
// the several-thread engine of ffq_pgz.h both run on -- and frees it in its destructor.  It is the feeder stage of a
// gzip stream (ffq_stream.h) and all of ffq_gunzip_fd; the batch (BgzfBatch) and the member parser serve the BGZF range
// walker (ffq_bgzf.h) as well.
#pragma once
#include <poll.h>
#include <sys/stat.h>
#include <zlib.h>
#include <memory>

#include "ffq_pool.h"
#include "ffq_pgz.h"

constexpr int64_t GZ_IN = 4 << 20;      // compressed bytes held at a time

// ---- BGZF members inflated side by side ------------------------------------------------------------
// A gzip member says how long it is only if its writer put that into the header: bgzip does (the "BC" extra field of the
// BGZF format, SAM specification section 4.1: BSIZE = length of the member - 1, at most 64 KiB of data per member, the
// uncompressed length in the member's last four bytes).  Members of such a file are found without inflating anything and
// inflated independently, each straight into its place in the pinned chunk.  Anything else -- and any member that does not
// hold what its header and trailer promise -- goes through the one-member-at-a-time inflate below, which has the last word.
struct GzJob {
    const uint8_t *src;     // raw deflate data of the member
    uint32_t clen;
    uint8_t *dst;
    uint32_t isize, crc;    // from the member's trailer
};

static bool inflate_one(z_stream *z, const GzJob &j)
{
    uint8_t none[8];
    if (inflateReset(z) != Z_OK) return false;
    z->next_in = const_cast<Bytef *>(j.src);
    z->avail_in = j.clen;
    z->next_out = j.isize ? j.dst : none;
    z->avail_out = j.isize ? j.isize : (uInt)sizeof none;
    const int r = inflate(z, Z_FINISH);
    if (r != Z_STREAM_END || z->avail_in != 0 || z->total_out != j.isize) return false;
    return (uint32_t)crc32(crc32(0L, Z_NULL, 0), j.dst, j.isize) == j.crc;
}
// The same member through this build's own decoder (ffq_pgz.h; about twice zlib's rate on FASTQ), into a scratch
// buffer of the thread (a match is copied a word at a time: the bytes behind a member's end belong to the next
// member, which another thread is writing); whatever it does not like is zlib's (inflate_one).
struct GzScratch { pgz::Inflater<uint8_t> inf; std::vector<uint8_t> buf; };
static bool inflate_fast(const GzJob &j)
{
    thread_local std::unique_ptr<GzScratch> sc;
    try {
        if (!sc) sc.reset(new GzScratch());
        const int64_t cap = (int64_t)j.isize + pgz::OUT_SLACK + 8;
        if ((int64_t)sc->buf.size() < cap) sc->buf.resize((size_t)cap);
    } catch (const std::bad_alloc &) { return false; }
    pgz::Inflater<uint8_t> &f = sc->inf;
    f.win_valid = 0;
    f.limit_bit = INT64_MAX;
    f.set_out(sc->buf.data(), 0, (int64_t)j.isize + pgz::OUT_SLACK + 8);
    f.start(j.src, j.clen, 0);
    if (f.run() != pgz::R_FINAL || f.b_out != (int64_t)j.isize || ((f.b_bit + 7) >> 3) != (int64_t)j.clen) return false;
    if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), sc->buf.data(), j.isize) != j.crc) return false;
    memcpy(j.dst, sc->buf.data(), j.isize);
    return true;
}

// The members gathered for one side-by-side inflate, and what inflating them takes: a BatchPool (the owner's, or one of
// its own; started when a batch first has two jobs for it) and one raw-deflate zlib state per worker (header and trailer
// are read by the parser), made when that worker first needs zlib.
struct BgzfBatch {
    struct ZState { z_stream z; bool init; };
    std::vector<GzJob> jobs;
    const int threads;                  // the caller's included
    BatchPool own, *const pool;
    std::unique_ptr<ZState[]> zs;       // [threads], by worker

    explicit BgzfBatch(int threads_, BatchPool *shared = nullptr) : threads(threads_), pool(shared ? shared : &own) {}
    BgzfBatch(const BgzfBatch &) = delete;
    ~BgzfBatch()
    {
        for (int w = 0; zs && w < threads; w++)
            if (zs[w].init) (void)inflateEnd(&zs[w].z);
    }
    // The member of `total` bytes at `member` (extra field of xlen bytes) as a job that inflates to dst: the ONE place a
    // trailer (CRC-32, ISIZE) is read.  The caller looks at what it promises, then adds it.
    static GzJob job(const uint8_t *member, int64_t total, int xlen, uint8_t *dst)
    {
        const uint8_t *e = member + total;
        return GzJob{member + 12 + xlen, (uint32_t)(total - xlen - 20), dst, pgz::le32(e - 4), pgz::le32(e - 8)};
    }
    void add(const GzJob &j) { jobs.push_back(j); }
    // zlib's state of a worker (0: the caller; the array itself is made by the caller: run() asks for it first); NULL: zlib could not be initialised
    z_stream *zstate(int worker)
    {
        if (!zs) zs.reset(new (std::nothrow) ZState[(size_t)threads]());
        if (!zs || worker >= threads) return nullptr;
        ZState &s = zs[worker];
        if (!s.init) s.init = inflateInit2(&s.z, -15) == Z_OK;
        return s.init ? &s.z : nullptr;
    }
    // Every job inflated (and forgotten), by the pool's threads and the caller; false: a member did not inflate to what
    // its trailer says.
    bool run()
    {
        std::atomic<int> failed{zstate(0) ? 0 : 1};
        if (threads > 1 && jobs.size() > 1) (void)pool->start(threads - 1);      // (fewer threads than asked for: the rest do it)
        for (size_t j0 = 0; j0 < jobs.size() && !failed.load(); j0 += (size_t)1 << 20) {       // (in batches the pool's counter can hold)
            const GzJob *js = jobs.data() + j0;
            pool->run((int)std::min<size_t>((size_t)1 << 20, jobs.size() - j0), [&](int j, int w) {
                if (inflate_fast(js[j])) return;
                z_stream *z = zstate(w);
                if (!z || !inflate_one(z, js[j])) failed.store(1);
            });
        }
        jobs.clear();
        return failed.load() == 0;
    }
};

// threads that inflate (FFQ_GZ_THREADS; default: this process's share of the host's cores -- cores / LOCAL_WORLD_SIZE
// when a launcher runs one rank per GPU --, at most 32): 1 = no pool
static int gz_threads_default()
{
    const char *e = getenv("FFQ_GZ_THREADS");
    if (e && atoi(e) > 0) return std::min(atoi(e), 256);
    unsigned hw = std::max<unsigned>(std::thread::hardware_concurrency(), 1u);
    const char *lw = getenv("LOCAL_WORLD_SIZE");
    if (lw && atoi(lw) > 1) hw = std::max<unsigned>(hw / (unsigned)atoi(lw), 1u);
    return (int)std::min<unsigned>(hw, 32u);
}

// Length of the BGZF member at p; 0: not one; -1: its header is not all there yet.  A BGZF member: gzip magic,
// deflate, FLG = FEXTRA alone, a "BC" subfield of two bytes.  *xlen: length of the extra field.
static int64_t bgzf_member_len(const uint8_t *p, int64_t avail, int *xlen)
{
    if (avail >= 4 && !(p[0] == 0x1f && p[1] == 0x8b && p[2] == 8 && p[3] == 4)) return 0;
    if (avail < 12) return -1;
    const int xl = p[10] | (p[11] << 8);
    if (avail < 12 + xl) return -1;
    for (int q = 0; q + 4 <= xl;) {
        const uint8_t *f = p + 12 + q;
        const int sl = f[2] | (f[3] << 8);
        if (f[0] == 'B' && f[1] == 'C' && sl == 2 && q + 6 <= xl) {
            const int64_t total = (int64_t)(f[4] | (f[5] << 8)) + 1;
            *xlen = xl;
            return total >= xl + 20 ? total : 0;
        }
        q += 4 + sl;
    }
    return 0;
}

namespace {      // (internal linkage: what is new here adds nothing to the library's exports)

// What a blocking source asks its owner.  The two questions differ: the inflate loop ends early only for stop(); a
// read behind poll() gives way to a request to park as well (stream_grow_room).  No Interrupt: never interrupted.
struct Interrupt {
    bool (*asked)(void *owner, bool or_park);
    void *owner;
    bool stop() const { return asked(owner, false); }
    bool stop_or_park() const { return asked(owner, true); }
};

// One chunk from a descriptor that cannot seek (a pipe, a socket): read() behind poll(), so that a request to stop or to
// park is seen within 50 ms even when the writer keeps the pipe open and idle.  Returns the bytes read; *eof: read()
// returned 0.  A chunk is handed over SHORT (not eof) when something was read and then nothing arrived for 50 ms, or a
// pause was asked for: records reach the caller as they come in.  -2: asked to stop / park before anything was read.
// -1: error (errno).
static int64_t stream_fd_read(int fd, const Interrupt *irq, uint8_t *dst, int64_t n, bool *eof)
{
    int64_t got = 0;
    *eof = false;
    while (got < n) {
        if (irq && irq->stop_or_park()) return got > 0 ? got : -2;
        struct pollfd pf = {fd, POLLIN, 0};
        const int pr = poll(&pf, 1, 50);
        if (pr < 0) { if (errno == EINTR) continue; return -1; }
        if (pr == 0) { if (got > 0) return got; continue; }
        const ssize_t r = read(fd, dst + got, (size_t)(n - got));
        if (r < 0) { if (errno == EINTR || errno == EAGAIN) continue; return -1; }
        if (r == 0) { *eof = true; break; }
        got += r;
    }
    return got;
}

// The DECOMPRESSED stream of a gzip file (RFC 1952; members may be concatenated, as bgzip and `cat a.gz b.gz` produce
// them; zero padding behind the last member is ignored), read by ONE thread.
struct GzReader {
    const int fd;
    const bool seekable;
    const Interrupt *const irq;         // (not owned; may be NULL)
    const int threads;                  // > 1: BGZF members are inflated side by side
    z_stream zs{};                      // the members one at a time
    bool z_init = false, z_member = false, z_in_eof = false;
    uint8_t *zin = nullptr;
    int64_t zin_len = 0, zin_pos = 0, z_filepos;
    std::string z_msg;
    bool bgzf_ok = true;                // cleared when a member did not hold what it promised: one at a time from there
    BatchPool pool;                     // threads - 1 threads, started on first use: the batch's and the engine's
    BgzfBatch batch;
    int64_t bgzf_members = 0;           // members inflated by the pool (statistics)
    // one member inflated by several threads (ffq_pgz.h: a regular file that is not BGZF), and zlib going on from
    // the block boundary the engine gave up at
    pgz::Engine *engine = nullptr;
    bool pgz_ok = true, pgz_active = false;
    int pgz_small = 0;
    int64_t pgz_member_off = 0, file_size = -1;
    bool z_raw = false;                 // zs is a raw deflate stream: the member's trailer is checked here
    uint32_t z_crc = 0;
    uint64_t z_isize = 0;

    // the compressed bytes are read from `pos` on (a descriptor that seeks: pread), by nthreads threads (<= 0: the default)
    GzReader(int fd_, int64_t pos, bool seekable_, int nthreads, const Interrupt *irq_)
        : fd(fd_), seekable(seekable_), irq(irq_), threads(nthreads > 0 ? std::min(nthreads, 256) : gz_threads_default()), z_filepos(pos),
          batch(threads, &pool)
    {
        zin = static_cast<uint8_t *>(malloc((size_t)GZ_IN + 16));      // (+16: the decoders read whole words)
        z_init = zin && inflateInit2(&zs, 15 + 16) == Z_OK;            // 16: gzip wrapper (header, CRC-32, length)
    }
    GzReader(const GzReader &) = delete;                     // (the assignment: ruled out by the const members)
    ~GzReader()
    {
        if (z_init) (void)inflateEnd(&zs);
        delete engine;
        free(zin);
    }
    bool ok() const { return z_init; }                       // false: "zlib could not be initialised"
    const char *msg() const { return z_msg.c_str(); }        // what read() failed with
    int64_t parallel_members() const { return bgzf_members; }
    // the file offset behind what has been inflated (inside a member the engine inflates: the block boundary it has committed)
    int64_t file_pos() const { return pgz_active ? (engine->pos_bit >> 3) : z_filepos - (zin_len - zin_pos); }

    // More compressed bytes behind what is left in zin (moved to the front).  1: something was added, 0: nothing
    // (end of the file, or zin is full), -1: error (z_msg), -2: asked to stop / park with nothing read.
    int more_input()
    {
        const int64_t rem = zin_len - zin_pos;
        if (z_in_eof || rem >= GZ_IN) return 0;
        if (rem > 0 && zin_pos > 0) memmove(zin, zin + zin_pos, (size_t)rem);
        zin_pos = 0; zin_len = rem;
        int64_t r;
        bool in_eof = false;
        if (seekable) { r = ReadPool::read_full(fd, zin + rem, GZ_IN - rem, z_filepos, true); in_eof = r >= 0 && r < GZ_IN - rem; }
        else {
            // a pipe: behind poll(), like the uncompressed case (a stop request is seen within 50 ms)
            r = stream_fd_read(fd, irq, zin + rem, GZ_IN - rem, &in_eof);
            if (r == -2) return -2;
        }
        if (r < 0) { z_msg = std::string("read failed: ") + strerror(errno); return -1; }
        z_filepos += r;
        zin_len += r;
        if (in_eof) z_in_eof = true;
        return r > 0 ? 1 : 0;
    }

    // At a member boundary: as many whole BGZF members as zin holds and dst has room for, inflated side by side.
    // Returns the bytes written (zin_pos is behind those members then), 0 if there is nothing to do here (not
    // BGZF, a member that is not all there at the end of the file, no room for even one: the serial inflate
    // takes it from the same place), -1 / -2 as more_input.
    int64_t bgzf_batch(uint8_t *dst, int64_t room)
    {
        int xl = 0;
        for (;;) {        // the first member whole in zin
            const int64_t avail = zin_len - zin_pos;
            const int64_t total = bgzf_member_len(zin + zin_pos, avail, &xl);
            if (total == 0) return 0;
            if (total > 0 && total <= avail) break;
            const int r = more_input();
            if (r <= 0) return r;
        }
        batch.jobs.clear();
        int64_t p = zin_pos, out = 0;
        while (p < zin_len) {
            const int64_t total = bgzf_member_len(zin + p, zin_len - p, &xl);
            if (total <= 0 || total > zin_len - p) break;
            const GzJob j = BgzfBatch::job(zin + p, total, xl, dst + out);
            if ((int64_t)j.isize > room - out) break;
            batch.add(j);
            out += j.isize;
            p += total;
        }
        const int64_t n = (int64_t)batch.jobs.size();
        if (n < 2) return 0;                      // (one member: the serial inflate is as good)
        if (!batch.run()) { bgzf_ok = false; return 0; }
        bgzf_members += n;
        zin_pos = p;
        return out;
    }

    // The compressed input goes on at file offset `off` (what zin held is dropped).
    void reposition(int64_t off)
    {
        z_filepos = off;
        zin_len = zin_pos = 0;
        z_in_eof = file_size >= 0 && off >= file_size;
    }

    // At a member boundary of a regular file: the member is handed to the several-thread engine if enough of the file
    // lies behind it to be worth a batch (FFQ_PGZ_MIN compressed bytes, default 4 MiB).  false: zlib takes the member.
    bool pgz_begin()
    {
        if (file_size < 0) {
            struct stat st;
            if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { pgz_ok = false; return false; }
            file_size = (int64_t)st.st_size;
        }
        int xl = 0;
        if (bgzf_member_len(zin + zin_pos, zin_len - zin_pos, &xl) != 0) return false;      // (a BGZF member: 64 KiB at most)
        const int64_t member_off = z_filepos - (zin_len - zin_pos);
        if (file_size - member_off < pgz::env_i64("FFQ_PGZ_MIN", 4 << 20)) return false;
        if (!engine) {
            engine = new (std::nothrow) pgz::Engine();
            if (!engine || !engine->init(fd, threads, file_size, &pool)) { delete engine; engine = nullptr; pgz_ok = false; return false; }
        }
        if (!engine->begin(member_off)) return false;
        pgz_member_off = member_off;
        pgz_active = true;
        return true;
    }

    // The engine gave up at a block boundary: zlib goes on from that bit with the window the engine holds, as a raw
    // deflate stream; the CRC-32 and the length run on here and are compared with the trailer (raw_trailer).
    bool handoff()
    {
        pgz::Engine &e = *engine;
        if (inflateReset2(&zs, -15) != Z_OK) { z_msg = "inflateReset failed"; return false; }
        if (e.win_valid > 0 && inflateSetDictionary(&zs, e.window + pgz::WSIZE - e.win_valid, (uInt)e.win_valid) != Z_OK) {
            z_msg = "inflateSetDictionary failed";
            return false;
        }
        int64_t byte = e.pos_bit >> 3;
        const int r = (int)(e.pos_bit & 7);
        if (r) {
            uint8_t b = 0;
            if (e.pread_full(&b, 1, byte) != 1) { z_msg = "compressed file ended before the end-of-stream marker was reached"; return false; }
            if (inflatePrime(&zs, 8 - r, b >> r) != Z_OK) { z_msg = "inflatePrime failed"; return false; }
            byte++;
        }
        reposition(byte);
        z_raw = true; z_crc = e.crc; z_isize = e.isize;
        z_member = true;
        return true;
    }

    bool raw_trailer()
    {
        while (zin_len - zin_pos < 8) {
            if (z_in_eof) { z_msg = "compressed file ended before the end-of-stream marker was reached"; return false; }
            if (more_input() < 0) return false;
        }
        const uint8_t *t = zin + zin_pos;
        const uint32_t fcrc = pgz::le32(t), flen = pgz::le32(t + 4);
        zin_pos += 8;
        z_raw = false;
        if (fcrc != z_crc) { z_msg = "incorrect data check"; return false; }
        if (flen != (uint32_t)z_isize) { z_msg = "incorrect length check"; return false; }
        return true;
    }

    // One chunk: fills dst completely unless the stream ends (*eof) or the owner asks to stop.  -1: error, msg() says what.
    int64_t read(uint8_t *dst, int64_t n, bool *eof)
    {
        int64_t got = 0;
        *eof = false;
        while (got < n) {
            if (irq && irq->stop()) break;
            if (pgz_active) {
                got += engine->read(dst + got, n - got);
                if (engine->pending()) continue;                           // (the chunk is full)
                if (engine->failed) { z_msg = engine->msg; return -1; }
                if (engine->member_done) {
                    pgz_active = false;
                    if (engine->end_off - pgz_member_off < (2 << 20) && ++pgz_small >= 4) pgz_ok = false;   // (a file of small members)
                    reposition(engine->end_off);
                } else if (engine->gave_up) {
                    pgz_active = false;
                    if (!handoff()) return -1;
                }
                continue;
            }
            if (zin_pos == zin_len && !z_in_eof) {
                const int r = more_input();
                if (r == -2) break;                                  // asked to stop / park with nothing read
                if (r < 0) return -1;
            }
            if (!z_member) {
                // between members: zero padding, then the next member or the end of the file
                while (zin_pos < zin_len && zin[zin_pos] == 0) zin_pos++;
                if (zin_pos == zin_len) {
                    if (z_in_eof) { *eof = true; break; }
                    continue;
                }
                if (threads > 1 && bgzf_ok) {
                    const int64_t r = bgzf_batch(dst + got, n - got);
                    if (r == -2) break;
                    if (r < 0) return -1;
                    if (r > 0) { got += r; continue; }
                }
                if (threads > 1 && seekable && pgz_ok && pgz_begin()) continue;
                if (inflateReset2(&zs, 15 + 16) != Z_OK) { z_msg = "inflateReset failed"; return -1; }
                z_member = true;
            } else if (zin_pos == zin_len && z_in_eof) {
                z_msg = "compressed file ended before the end-of-stream marker was reached";
                return -1;
            }
            zs.next_in = zin + zin_pos;
            zs.avail_in = (uInt)(zin_len - zin_pos);
            zs.next_out = dst + got;
            zs.avail_out = (uInt)std::min<int64_t>(n - got, 1 << 30);
            const uInt out0 = zs.avail_out;
            const int zr = inflate(&zs, Z_NO_FLUSH);
            zin_pos = zin_len - (int64_t)zs.avail_in;
            if (z_raw) {
                const int64_t made = (int64_t)(out0 - zs.avail_out);
                z_crc = (uint32_t)crc32(z_crc, dst + got, (uInt)made);
                z_isize += (uint64_t)made;
            }
            got += (int64_t)(out0 - zs.avail_out);
            if (zr == Z_STREAM_END) {
                if (z_raw && !raw_trailer()) return -1;
                z_member = false;
            }
            else if (zr != Z_OK && zr != Z_BUF_ERROR) {
                z_msg = zs.msg ? zs.msg : (zr == Z_DATA_ERROR ? "not a gzip file / corrupt data" : "inflate failed");
                return -1;
            }
        }
        if (got == n && !*eof && zin_pos == zin_len && z_in_eof && !z_member) *eof = true;   // ended exactly at the chunk's end
        return got;
    }
};

}  // namespace

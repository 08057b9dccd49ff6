// The window walk of k_decode_stream (csrc/ffq_dqwalk.h: the functions the kernel itself calls), driven on the host over
// offset arrays with long runs of EMPTY records -- what a quality trim leaves of a bad tile, and what no GPU test could
// be allowed to try first: before the walk had its slow step, such a run under one 16-byte chunk made a workgroup repeat
// the same window for ever.
//
// For a vector of component lengths, an output alignment and a capacity, every block is walked exactly as the kernel
// walks it (same state, same functions, same order), with a cap on the turns of the loop.  Checked:
//   * the walk ends (within 2 nchunk + 2 turns);
//   * every chunk of the block is handed out exactly once;
//   * for every chunk a window hands out, every index the kernel would touch in the cache (s_q[a + 1], s_q[a + 2], the
//     tail's s_q[m + 1], s_adj of every record it copies from) lies inside the window, and the record the kernel's
//     selection takes each byte from is the record that owns the byte (found independently: upper_bound over the
//     offsets) -- i.e. the window caches every record with a byte under the chunk;
//   * the slow step finds the owner of each of its bytes too.
//
//   clang++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I <package>/csrc tests/dq_windows_host.cpp -o dq_windows_host
// Exit status 0 and "ok" on the last line, or 1 and a line per failure (the first 20).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ffq_dqwalk.h"

using namespace ffq;

static int g_fail = 0;
static long g_walks = 0, g_windows = 0, g_slow = 0, g_retries = 0;

static void fail(const std::string &name, int shift, int64_t blk, const char *what, long a = 0, long b = 0, long c = 0)
{
    if (++g_fail <= 20)
        std::printf("FAIL %s  shiftA=%d block=%lld: %s (%ld, %ld, %ld)\n", name.c_str(), shift, (long long)blk, what, a, b, c);
}

// owner[x] = the record that owns stream byte x (qoff[r] <= x < qoff[r + 1], never an empty one), written down from the
// lengths alone
struct Owners {
    std::vector<int32_t> of;
    int64_t operator()(int64_t x) const { return of[(size_t)x]; }
};

// one table: lens -> qoff, qdir (by qdir_mark, as k_col_offsets writes it), then every block at alignment `align`
static void walk_table(const std::string &name, const std::vector<int64_t> &lens, const Owners &owner, int align, int64_t out_cap = -1)
{
    const int64_t n = (int64_t)lens.size();
    std::vector<int64_t> qoff(n + 1, 0);
    for (int64_t i = 0; i < n; i++) qoff[i + 1] = qoff[i] + lens[i];
    const int64_t qtotal = qoff[n];
    if (out_cap < 0) out_cap = qtotal;
    const int64_t total = std::min(qtotal, out_cap);
    if (n <= 0 || total <= 0) return;
    const int64_t nblk = (total + DQ_BLK - 1) / DQ_BLK;
    std::vector<int64_t> qdir(nblk + 1, -1);
    for (int64_t i = 0; i < n; i++) qdir_mark(qdir.data(), nblk + 1, qoff[i], lens[i], i);
    const int mean = dq_mean(qtotal, n);
    std::vector<int32_t> s_q(DQ_REC);

    for (int64_t blk = 0; blk < nblk; blk++) {
        const int64_t ob = blk << DQ_SHIFT;
        const int oe = (int)std::min<int64_t>(DQ_BLK, total - ob);
        const int shiftA = (int)((align + ob) & 15);
        const int nchunk = dq_nchunk(oe, shiftA);
        std::vector<int> handed(nchunk, 0);
        DqWalk w;
        w.rbase = qdir[blk];
        w.done = 0;
        w.want = 0;
        g_walks++;
        if (w.rbase < 0 || w.rbase >= n || qoff[w.rbase] > ob || qoff[w.rbase + 1] <= ob) {
            fail(name, shiftA, blk, "the directory does not name the record under the block's first byte", (long)w.rbase);
            continue;
        }
        const int cap = 2 * nchunk + 2;
        int turn = 0;
        bool ended = false;
        for (; turn < cap && !ended; turn++) {
            const int64_t rbase = w.rbase;
            const int done = w.done;
            const int nrec = dq_window_nrec(dq_window_want(w.want, done, oe, shiftA, mean), n, rbase);
            if (nrec < 1 || nrec > DQ_REC - 1) { fail(name, shiftA, blk, "window size", nrec); break; }
            for (int i = 0; i <= nrec; i++) s_q[i] = dq_rel(qoff[rbase + i], ob);
            g_windows++;
            const int cend = s_q[nrec];
            const int klim = dq_klim(rbase, nrec, n, cend, oe, shiftA, nchunk);
            const float inv_mean = (float)nrec / (float)(cend - s_q[0]);
            for (int k = done; k < klim; k++) {
                const int clo = dq_clo(k, shiftA);
                const int vlo = std::max(clo, 0), vhi = std::min(clo + 16, oe);
                if (vlo >= vhi) { fail(name, shiftA, blk, "an empty chunk", k); continue; }
                handed[k]++;
                // every record with a byte under the chunk is cached
                const int64_t r_lo = owner(ob + vlo), r_hi = owner(ob + vhi - 1);
                if (r_lo < rbase || r_hi > rbase + nrec - 1) {
                    fail(name, shiftA, blk, "a chunk handed out by a window that does not cache its records", k, (long)r_lo, (long)r_hi);
                    continue;
                }
                // the kernel's selection, index by index
                int src[16];                             // cached index chunk byte j is taken from
                std::fill(src, src + 16, -1);
                const int a = dq_chunk_record(s_q.data(), nrec, vlo, inv_mean);
                if (a < 0 || a > nrec - 1) { fail(name, shiftA, blk, "chunk record outside the window", k, a, nrec); continue; }
                const int h0 = std::min((int)s_q[a + 1], vhi) - clo;
                int h1 = h0;
                bool bad = false;
                if (h0 < vhi - clo) {
                    if (a + 2 > nrec) { fail(name, shiftA, blk, "s_q[a + 2] outside the window", k, a, nrec); continue; }
                    h1 = std::min((int)s_q[a + 2], vhi) - clo;
                }
                for (int j = vlo - clo; j < h0; j++) src[j] = a;
                for (int j = std::max(h0, vlo - clo); j < h1; j++) src[j] = a + 1;      // (s_adj[a + 1]: a + 1 <= nrec - 1 here)
                if (h1 > h0 && a + 1 > nrec - 1) { fail(name, shiftA, blk, "s_adj[a + 1] outside the window", k, a, nrec); continue; }
                if (h1 < vhi - clo) {                   // gather_tail(m = a + 2, kb = h1, kend = vhi - clo)
                    int m = a + 2, kb = h1;
                    const int kend = vhi - clo;
                    while (kb < kend) {
                        if (m + 1 > nrec) { fail(name, shiftA, blk, "the tail walks out of the window", k, m, nrec); bad = true; break; }
                        const int he = std::min((int)s_q[m + 1], vhi) - clo;
                        for (; kb < he; kb++) src[kb] = m;
                        m++;
                    }
                }
                if (bad) continue;
                for (int x = vlo; x < vhi; x++) {
                    const int64_t got = src[x - clo] < 0 ? -1 : rbase + src[x - clo];
                    if (got != owner(ob + x)) {
                        fail(name, shiftA, blk, "a byte taken from the wrong record", x, (long)got, (long)owner(ob + x));
                        break;
                    }
                }
            }
            if (klim >= nchunk) { ended = true; break; }
            const int nxt = dq_next(w, s_q.data(), nrec, klim, shiftA);
            if (nxt == DQ_NEXT_SLOW) {
                // decode_chunk_slow: thread t < 16 writes byte clo + t if it lies in [0, oe)
                g_slow++;
                const int clo = dq_clo(done, shiftA);
                handed[done]++;
                for (int t = 0; t < 16; t++) {
                    const int x = clo + t;
                    if (x < 0 || x >= oe) continue;
                    if (qoff[rbase] > ob + x) { fail(name, shiftA, blk, "slow step: the search's lower end is above the byte", x); break; }
                    const int64_t r = dq_find_record(qoff.data(), rbase, n - 1, ob + x);
                    if (r != owner(ob + x)) { fail(name, shiftA, blk, "slow step: wrong record", x, (long)r, (long)owner(ob + x)); break; }
                }
                if (dq_after_slow(w, qoff.data(), n, ob, shiftA, nchunk)) { ended = true; break; }
            } else if (w.want < 0) {
                g_retries++;
            }
            if (w.rbase < rbase || w.rbase >= n || w.done < done) { fail(name, shiftA, blk, "the walk went backwards", (long)w.rbase, w.done); break; }
        }
        if (!ended) {
            if (turn >= cap)
                fail(name, shiftA, blk, "NON-TERMINATION: the walk did not end within 2 nchunk + 2 turns; stuck at (done, rbase, want)",
                     w.done, (long)w.rbase, w.want);
            continue;
        }
        for (int k = 0; k < nchunk; k++)
            if (handed[k] != 1) { fail(name, shiftA, blk, "a chunk handed out other than once", k, handed[k]); break; }
    }
}

static void all_alignments(const std::string &name, const std::vector<int64_t> &lens)
{
    int64_t total = 0;
    for (int64_t v : lens) total += v;
    Owners owner;
    owner.of.reserve((size_t)total);
    for (size_t i = 0; i < lens.size(); i++) owner.of.insert(owner.of.end(), (size_t)lens[i], (int32_t)i);
    for (int align = 0; align < 16; align++) {
        walk_table(name, lens, owner, align);
        if (align == 0 || align == 5) {                  // an output that is too small: the walk stops at out_cap
            walk_table(name + " cap-1", lens, owner, align, total - 1);
            walk_table(name + " cap/2", lens, owner, align, total / 2);
        }
    }
}

static std::vector<int64_t> cat(std::initializer_list<std::vector<int64_t>> parts)
{
    std::vector<int64_t> v;
    for (const auto &p : parts) v.insert(v.end(), p.begin(), p.end());
    return v;
}

static std::vector<int64_t> rep(int64_t value, int64_t count) { return std::vector<int64_t>((size_t)count, value); }

// records of 32 bytes (and one shorter) that sum to `total`
static std::vector<int64_t> fill(int64_t total)
{
    std::vector<int64_t> v = rep(32, total / 32);
    if (total % 32) v.push_back(total % 32);
    return v;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return g_rng;
}

int main()
{
    const int Z[] = {0, 1, 1021, 1022, 1023, 1024, 2047, 3000};
    const int FIRST[] = {1, 15, 16, 17, 20, 33};
    const std::vector<int64_t> tail = cat({{20}, rep(30, 50)});
    // a record that ends inside a chunk (or at its end), Z empty records, more bytes in the same block
    for (int z : Z)
        for (int first : FIRST)
            all_alignments("table first=" + std::to_string(first) + " Z=" + std::to_string(z), cat({{first}, rep(0, z), tail}));
    for (int z : Z) {
        for (int first : FIRST) {
            const std::string id = "first=" + std::to_string(first) + " Z=" + std::to_string(z);
            all_alignments("run at the end " + id, cat({{first}, rep(30, 50), rep(0, z)}));
            // the run sits exactly on the boundary between two blocks (it begins and ends at 65536) ...
            all_alignments("run at 65536 " + id, cat({fill(DQ_BLK - first), {first}, rep(0, z), tail}));
            // ... the record BEHIND it ends exactly at the boundary ...
            all_alignments("run ends before 65536 " + id, cat({fill(DQ_BLK - first - 40), {40}, rep(0, z), {first}, tail}));
            // ... the record IN FRONT of it begins exactly there
            all_alignments("run begins behind 65536 " + id, cat({fill(DQ_BLK), {first}, rep(0, z), tail}));
        }
        all_alignments("run at the start Z=" + std::to_string(z), cat({rep(0, z), tail}));
        all_alignments("two runs in one block Z=" + std::to_string(z), cat({{20}, rep(0, z), {7}, rep(0, z + 1), tail}));
        all_alignments("two runs under one chunk Z=" + std::to_string(z), cat({{3}, rep(0, z), {2}, rep(0, z), {1}, rep(0, z), tail}));
        all_alignments("a 70000-byte record between runs Z=" + std::to_string(z), cat({{5}, rep(0, z), {70000}, rep(0, z), {9}, rep(30, 10)}));
    }
    all_alignments("1-byte records", rep(1, 5000));
    all_alignments("1-byte records, a block and more", rep(1, 70000));
    {
        std::vector<int64_t> v;
        for (int i = 0; i < 3000; i++) { v.push_back(1); v.push_back(0); v.push_back(0); }
        all_alignments("1-byte records between empty ones", v);
        v.clear();
        for (int i = 0; i < 40; i++) { v.push_back(1); for (int j = 0; j < 1022 + i % 3; j++) v.push_back(0); }
        all_alignments("a run behind every byte", v);
    }
    all_alignments("equal records", rep(151, 3000));
    const int64_t PICK[] = {0, 0, 0, 1, 15, 16, 17, 300};
    for (int it = 0; it < 300; it++) {
        // even: independent draws; odd: runs of one drawn value among them, so that runs of empty records get long
        std::vector<int64_t> v;
        const int64_t n = 1 + (int64_t)(rnd() % 6000);
        while ((int64_t)v.size() < n) {
            const int64_t val = PICK[rnd() % 8];
            int64_t run = ((it & 1) && rnd() % 4 == 0) ? 1 + (int64_t)(rnd() % 2500) : 1;
            if (val == 300 && run > 300) run = 300;
            for (; run > 0 && (int64_t)v.size() < n; run--) v.push_back(val);
        }
        all_alignments("random #" + std::to_string(it), v);
    }
    std::printf("%ld walks, %ld windows, %ld retried at full size, %ld slow steps, %d failures\n", g_walks, g_windows, g_retries, g_slow, g_fail);
    if (g_fail) return 1;
    if (g_slow == 0 || g_retries == 0) { std::printf("the inputs never reached the slow step\n"); return 1; }
    std::printf("ok\n");
    return 0;
}

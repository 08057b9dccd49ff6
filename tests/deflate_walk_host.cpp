// The parts of the BGZF deflate that have no device in them (csrc/ffq_deflatewalk.h: the functions k_deflate_members itself
// calls), driven on the host.  A workgroup is emulated lane by lane: the rounds of lookups and inserts, every lane's walk,
// the counts, the ranks, the code lengths, the codes, the header, the lanes' bit offsets and their packing are the header's
// functions; the barriers, the prefix sum and the atomics of the kernel are plain loops here.  What comes out is a whole
// gzip member, and zlib judges it: inflate (raw, -15) must give the block back, crc32() must agree.  Every block lives in a
// heap block of exactly its length, so a load that leaves it is an out-of-bounds read AddressSanitizer reports.
//
//   clang++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I <package>/csrc tests/deflate_walk_host.cpp -lz -o deflate_walk_host
// Exit status 0 and "ok" on the last line, or 1 and a line per failure.
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "ffq_deflatewalk.h"

using namespace ffq;

static int g_fail = 0;
static long g_checks = 0;
#define CHECK(cond, ...) do { g_checks++; if (!(cond)) { if (g_fail++ < 20) { std::printf("FAIL %s:%d: %s  [", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("]\n"); } } } while (0)

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17;
    return (uint32_t)(g_seed >> 24);
}

// the words a member is built in: on the host an OR is an OR
struct Words {
    std::vector<uint32_t> w = std::vector<uint32_t>(DFL_SLOT / 4, 0u);
    std::vector<uint8_t> plain_seen = std::vector<uint8_t>(DFL_SLOT / 4, 0);
    void plain(uint32_t i, uint32_t v)
    {
        CHECK(w.at(i) == 0 && !plain_seen.at(i), "a plain store into word %u that is not all the lane's", i);
        plain_seen[i] = 1; w[i] = v;
    }
    void shared(uint32_t i, uint32_t v) { CHECK(!plain_seen.at(i), "an OR into word %u that a lane stored plainly", i); w.at(i) |= v; }
};

// 2^15 times the Kraft sum of len[0, n), the number of used codes, the longest
static long kraft(const uint8_t *len, int n, int *used = nullptr, int *longest = nullptr)
{
    long k = 0;
    int u = 0, mx = 0;
    for (int s = 0; s < n; s++)
        if (len[s]) { k += 1L << (15 - len[s]); u++; mx = std::max<int>(mx, len[s]); }
    if (used) *used = u;
    if (longest) *longest = mx;
    return k;
}

struct Code {
    std::vector<uint32_t> freq;
    std::vector<uint16_t> sorted, code;
    std::vector<int32_t> work;
    std::vector<uint8_t> len;
    int n, used = 0;
    explicit Code(int n_) : freq(n_, 0u), sorted(n_, 0), code(n_, 0), work(n_, 0), len(n_, 0xEE), n(n_) {}
    void build(int maxbits, bool pad_single)
    {
        for (int lane = 0; lane < DFL_LANES; lane++) dfl_rank_lane(freq.data(), n, lane, DFL_LANES, sorted.data(), work.data(), len.data());
        used = dfl_lengths(freq.data(), n, maxbits, pad_single, sorted.data(), work.data(), len.data());
        dfl_codes(len.data(), n, code.data());
    }
};

struct Member {
    std::vector<uint8_t> bytes;
    bool stored = false;
    int n_match = 0, max_dist = 0, llongest = 0, dused = 0;
    std::vector<uint8_t> dist_seen = std::vector<uint8_t>(65536, 0);      // the distances the member's matches use
};

// a workgroup, lane by lane
static Member build_member(const uint8_t *src, int n)
{
    Member m;
    std::unique_ptr<uint8_t[]> b(new uint8_t[n]);
    std::memcpy(b.get(), src, (size_t)n);
    std::vector<uint32_t> slot((size_t)n, 0u), table(1u << DFL_HASH_BITS, 0u);
    // 1. the rounds: every position looks up, then every position is entered
    for (int r0 = 0; r0 < n; r0 += DFL_ROUND) {
        const int r1 = std::min(n, r0 + DFL_ROUND);
        for (int p = r0; p < r1; p++) slot[p] = p + 4 <= n ? dfl_candidate(p, table[dfl_hash(dfl_load4(b.get(), p))]) : 0;
        for (int p = r0; p < r1; p++)
            if (p + 4 <= n) { uint32_t &e = table[dfl_hash(dfl_load4(b.get(), p))]; e = std::max<uint32_t>(e, (uint32_t)p + 1); }
    }
    // 2. the walk
    const int nseg = (n + DFL_SEG - 1) / DFL_SEG;
    std::vector<int> ntok(DFL_LANES, 0);
    for (int lane = 0; lane < nseg; lane++) ntok[lane] = dfl_walk(b.get(), lane * DFL_SEG, std::min(n, (lane + 1) * DFL_SEG), slot.data());
    // 3. counts, lengths, codes
    Code L(DFL_NLIT), D(DFL_NDIST), C(DFL_NCL);
    for (int lane = 0; lane < nseg; lane++)
        for (int k = 0; k < ntok[lane]; k++) {
            int ls, ds;
            const uint32_t t = slot[lane * DFL_SEG + k];
            dfl_token_syms(t, ls, ds);
            L.freq.at(ls)++;
            if (ds >= 0) { D.freq.at(ds)++; m.n_match++; m.max_dist = std::max(m.max_dist, dfl_tok_dist(t)); m.dist_seen.at(dfl_tok_dist(t)) = 1; }
        }
    L.freq[DFL_EOB] = 1;
    L.build(DFL_LIT_BITS, true);
    D.build(DFL_LIT_BITS, false);
    CHECK(kraft(L.len.data(), DFL_NLIT, nullptr, &m.llongest) == 1L << 15 && L.used >= 2, "literal/length code: Kraft %ld", kraft(L.len.data(), DFL_NLIT));
    const long dk = kraft(D.len.data(), DFL_NDIST, &m.dused);
    // (no match: one distance code of length 0; one distance symbol: one code of length 1; else a complete code)
    CHECK(D.used == 0 ? dk == 0 : D.used == 1 ? (dk == 1L << 14 && m.dused == 1) : dk == 1L << 15, "distance code: %d used, Kraft %ld", D.used, dk);
    CHECK((D.used == 0) == (m.n_match == 0), "%d matches, %d distance symbols", m.n_match, D.used);
    // 4. the header's code
    DflPlan pl;
    dfl_header_counts(L.len.data(), D.len.data(), pl);
    for (int s = 0; s < pl.hlit; s++) C.freq[L.len[s]]++;
    for (int s = 0; s < pl.hdist; s++) C.freq[D.len[s]]++;
    C.build(DFL_CL_BITS, true);
    CHECK(kraft(C.len.data(), DFL_NCL) == 1L << 15, "the header's code: Kraft %ld", kraft(C.len.data(), DFL_NCL));
    dfl_header_plan(C.freq.data(), C.len.data(), pl);
    // 5. sizes
    std::vector<int64_t> at(DFL_LANES + 1, 0);
    for (int lane = 0; lane < nseg; lane++) {
        int64_t bits = 0;
        for (int k = 0; k < ntok[lane]; k++) bits += dfl_token_bits(slot[lane * DFL_SEG + k], L.len.data(), D.len.data());
        if (lane == nseg - 1) bits += L.len[DFL_EOB];
        at[lane + 1] = at[lane] + bits;
    }
    const int64_t stream_bits = pl.head_bits + at[nseg];
    m.stored = dfl_stored(stream_bits, n);
    const int stream_bytes = m.stored ? n + DFL_STORED_HEAD : (int)((stream_bits + 7) / 8);
    const int member_bytes = dfl_member_bytes(stream_bytes);
    CHECK(member_bytes <= DFL_SLOT && member_bytes <= n + DFL_OVERHEAD, "a member of %d bytes for %d", member_bytes, n);
    // 6. emit
    Words w;
    if (m.stored) {
        dfl_put_stored_head(w, n);
        for (int i = 0; i < n; i++) dfl_put_byte(w, DFL_HEAD + DFL_STORED_HEAD + i, b[i]);
    } else {
        {
            DflBits<Words> o(w, 8 * DFL_HEAD);
            dfl_put_header(o, pl, L.len.data(), D.len.data(), C.code.data(), C.len.data());
            CHECK((int64_t)o.wi * 32 + o.nb == 8 * DFL_HEAD + pl.head_bits, "the header has %lld bits, planned %d", (long long)o.wi * 32 + o.nb - 8 * DFL_HEAD, pl.head_bits);
            o.finish();
        }
        for (int lane = 0; lane < nseg; lane++) {
            DflBits<Words> o(w, 8 * DFL_HEAD + pl.head_bits + at[lane]);
            for (int k = 0; k < ntok[lane]; k++) dfl_put_token(o, slot[lane * DFL_SEG + k], L.code.data(), L.len.data(), D.code.data(), D.len.data());
            if (lane == nseg - 1) o.put(L.code[DFL_EOB], L.len[DFL_EOB]);
            CHECK((int64_t)o.wi * 32 + o.nb == 8 * DFL_HEAD + pl.head_bits + at[lane + 1], "lane %d packed other bits than it counted", lane);
            o.finish();
        }
    }
    // the CRC: a lane's own, moved by the bytes behind it
    uint32_t tab[256], x2n[32], crc = 0;
    for (int i = 0; i < 256; i++) tab[i] = dfl_crc_entry(i);
    dfl_crc_x2n(x2n);
    for (int lane = 0; lane < nseg; lane++) {
        const int s0 = lane * DFL_SEG, s1 = std::min(n, s0 + DFL_SEG);
        crc ^= dfl_crc_shift(x2n, dfl_crc(tab, b.get() + s0, s1 - s0), (uint32_t)(n - s1));
    }
    CHECK(crc == (uint32_t)crc32(0L, src, (uInt)n), "CRC of %d bytes: %08x, zlib %08lx", n, crc, crc32(0L, src, (uInt)n));
    dfl_put_frame(w, member_bytes, crc, n);
    m.bytes.resize((size_t)member_bytes);
    for (int i = 0; i < member_bytes; i++) m.bytes[i] = (uint8_t)(w.w[i >> 2] >> (8 * (i & 3)));
    return m;
}

// the member as zlib sees it
static void check_member(const char *what, const std::vector<uint8_t> &src, Member *out = nullptr)
{
    const int n = (int)src.size();
    Member m = build_member(src.data(), n);
    const std::vector<uint8_t> &g = m.bytes;
    static const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    CHECK(g.size() >= 26 && !std::memcmp(g.data(), head, 16), "%s: the fixed header bytes", what);
    CHECK((size_t)(g[16] | (g[17] << 8)) + 1 == g.size(), "%s: BSIZE", what);
    std::unique_ptr<uint8_t[]> back(new uint8_t[n + 1]);
    z_stream z;
    std::memset(&z, 0, sizeof z);
    CHECK(inflateInit2(&z, -15) == Z_OK, "inflateInit2");
    z.next_in = const_cast<Bytef *>(g.data()) + DFL_HEAD; z.avail_in = (uInt)(g.size() - DFL_HEAD - DFL_TAIL);
    z.next_out = back.get(); z.avail_out = (uInt)n + 1;
    const int rc = inflate(&z, Z_FINISH);
    CHECK(rc == Z_STREAM_END && z.avail_in == 0 && (int)z.total_out == n, "%s (%d bytes): inflate %d (%s), %u left, %lu out", what, n, rc,
          z.msg ? z.msg : "", z.avail_in, z.total_out);
    CHECK(!std::memcmp(back.get(), src.data(), (size_t)n), "%s: the inflated bytes differ", what);
    inflateEnd(&z);
    const uint8_t *t = g.data() + g.size() - 8;
    const uint32_t crc = t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24), isize = t[4] | (t[5] << 8) | (t[6] << 16) | ((uint32_t)t[7] << 24);
    CHECK(crc == (uint32_t)crc32(0L, src.data(), (uInt)n) && isize == (uint32_t)n, "%s: trailer %08x %u", what, crc, isize);
    CHECK(m.max_dist <= DFL_MAX_DIST, "%s: a distance of %d", what, m.max_dist);
    if (out) *out = m;
}

static std::vector<uint8_t> noise(int n)
{
    std::vector<uint8_t> v((size_t)n);
    for (auto &x : v) x = (uint8_t)rnd();
    return v;
}

static std::vector<uint8_t> fastq_like(int n)
{
    std::string s;
    long x = 1000, y = 2000;
    while ((int)s.size() < n) {
        char h[128];
        x += rnd() % 30; y += rnd() % 50;
        std::snprintf(h, sizeof h, "@A00123:45:HXXXXDSXY:1:1101:%ld:%ld 1:N:0:ATCACGTT+AGGCTATA\n", x, y);
        s += h;
        for (int i = 0; i < 150; i++) s += "ACGT"[rnd() & 3];
        s += "\n+\n";
        for (int i = 0; i < 150; i++) { const uint32_t r = rnd() % 100; s += r < 90 ? 'F' : r < 96 ? ':' : r < 99 ? ',' : '#'; }
        s += "\n";
    }
    s.resize((size_t)n);
    return std::vector<uint8_t>(s.begin(), s.end());
}

// a phrase of 100 bytes no four of which come twice
static const struct Phrase { uint8_t b[100]; Phrase() { for (int i = 0; i < 100; i++) b[i] = (uint8_t)(32 + i); } } PHRASE;

// the phrase at `first` and again `dist` behind it; around them noise, or with `quiet` one byte repeated: no position between
// the two then takes the phrase's places in the table, so the second phrase is SURE to be offered the first
static std::vector<uint8_t> phrase_twice(int n, int first, int dist, bool quiet = false)
{
    std::vector<uint8_t> v = quiet ? std::vector<uint8_t>((size_t)n, (uint8_t)'x') : noise(n);
    std::memcpy(v.data() + first, PHRASE.b, 100);
    std::memcpy(v.data() + first + dist, PHRASE.b, 100);
    return v;
}

static void test_symbols()
{
    static const int lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const int lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const int dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    static const int dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    for (int len = 3; len <= 258; len++) {
        int eb, ev;
        const int s = dfl_len_sym(len, eb, ev) - 257;
        CHECK(s >= 0 && s < 29 && eb == lext[s] && lbase[s] + ev == len && ev < (1 << eb), "length %d: symbol %d, %d extra bits, value %d", len, s + 257, eb, ev);
    }
    for (int d = 1; d <= 32768; d++) {
        int eb, ev;
        const int s = dfl_dist_sym(d, eb, ev);
        CHECK(s >= 0 && s < 30 && eb == dext[s] && dbase[s] + ev == d && ev < (1 << eb), "distance %d: symbol %d, %d extra bits, value %d", d, s, eb, ev);
    }
    static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int i = 0; i < 19; i++) CHECK(dfl_cl_order(i) == order[i], "order of the header's lengths at %d", i);
    uint8_t eof[28];
    static const uint8_t want[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    dfl_eof_member(eof);
    CHECK(!std::memcmp(eof, want, 28), "the EOF member");
}

// the cost of an unlimited Huffman code, by merging the two smallest again and again
static long huffman_cost(std::vector<long> f)
{
    long cost = 0;
    while (f.size() > 1) {
        std::sort(f.begin(), f.end());
        const long s = f[0] + f[1];
        cost += s;
        f.erase(f.begin(), f.begin() + 2);
        f.push_back(s);
    }
    return cost;
}

static void test_lengths()
{
    // Fibonacci counts: 22 terms sum to 46367, under a block's bytes, and an unlimited code is 21 deep
    for (int pass = 0; pass < 2; pass++) {
        const int n = pass ? DFL_NCL : DFL_NLIT, limit = pass ? DFL_CL_BITS : DFL_LIT_BITS, terms = pass ? 19 : 22;
        Code c(n);
        uint32_t a = 1, b2 = 1;
        for (int i = 0; i < terms; i++) { c.freq[(i * 7) % n] = a; const uint32_t t = a + b2; a = b2; b2 = t; }
        c.build(limit, true);
        int used, longest;
        const long k = kraft(c.len.data(), n, &used, &longest);
        CHECK(k == 1L << 15 && used == terms && longest == limit, "Fibonacci counts against %d bits: Kraft %ld, %d used, longest %d", limit, k, used, longest);
        // a code that is no prefix code would show here: all codes differ, none is the head of another
        for (int s = 0; s < n; s++)
            for (int t = 0; t < n; t++)
                if (s != t && c.len[s] && c.len[t] && c.len[s] <= c.len[t])
                    CHECK((c.code[t] & ((1u << c.len[s]) - 1)) != c.code[s], "codes %d and %d", s, t);
    }
    // a single symbol: two codes of length 1; with the distance code's rule, one
    for (int s : {0, 5}) {
        Code c(DFL_NDIST);
        c.freq[s] = 9;
        c.build(DFL_LIT_BITS, true);
        int used;
        CHECK(kraft(c.len.data(), DFL_NDIST, &used) == 1L << 15 && used == 2 && c.len[s] == 1 && c.code[s] != c.code[s ? 0 : 1], "one symbol, padded");
        c.build(DFL_LIT_BITS, false);
        CHECK(kraft(c.len.data(), DFL_NDIST, &used) == 1L << 14 && used == 1 && c.len[s] == 1, "one symbol, alone");
    }
    {
        Code c(DFL_NDIST);
        c.build(DFL_LIT_BITS, false);
        CHECK(c.used == 0 && kraft(c.len.data(), DFL_NDIST) == 0, "no symbol");
    }
    // seeded counts: complete, within the limit, and as cheap as Huffman's where the limit does not bind
    for (int it = 0; it < 300; it++) {
        const int n = it % 3 == 0 ? DFL_NCL : it % 3 == 1 ? DFL_NDIST : DFL_NLIT, limit = n == DFL_NCL ? DFL_CL_BITS : DFL_LIT_BITS;
        Code c(n);
        const int used_want = 2 + (int)(rnd() % (uint32_t)(n - 1));
        const int skew = (int)(rnd() % 12);
        std::vector<long> f;
        for (int i = 0; i < used_want; i++) {
            int s;
            do s = (int)(rnd() % (uint32_t)n); while (c.freq[s]);
            c.freq[s] = 1 + (rnd() % (1u << skew)) % 200;
            f.push_back(c.freq[s]);
        }
        c.build(limit, true);
        int used, longest;
        const long k = kraft(c.len.data(), n, &used, &longest);
        CHECK(k == 1L << 15 && used == used_want && longest <= limit, "seeded counts %d: Kraft %ld, %d of %d used, longest %d", it, k, used, used_want, longest);
        long cost = 0;
        for (int s = 0; s < n; s++) cost += (long)c.freq[s] * c.len[s];
        const long best = huffman_cost(f);
        CHECK(cost >= best && (longest == limit || cost == best), "seeded counts %d: cost %ld, Huffman %ld, longest %d", it, cost, best, longest);
        for (int s = 0; s < n; s++) CHECK((c.len[s] != 0) == (c.freq[s] != 0), "a length for an unused symbol");
    }
}

static void test_crc()
{
    uint32_t tab[256], x2n[32];
    for (int i = 0; i < 256; i++) tab[i] = dfl_crc_entry(i);
    dfl_crc_x2n(x2n);
    CHECK(tab[1] == 0x77073096u && tab[255] == 0x2D02EF8Du, "the CRC table");
    // 1, 2 and 255 segments, and a short last one
    for (int n : {1, 100, DFL_SEG, DFL_SEG + 1, 2 * DFL_SEG, 2 * DFL_SEG - 1, 255 * DFL_SEG, 254 * DFL_SEG + 7}) {
        const std::vector<uint8_t> v = noise(n);
        std::unique_ptr<uint8_t[]> b(new uint8_t[n]);
        std::memcpy(b.get(), v.data(), (size_t)n);
        uint32_t crc = 0;
        uLong z = crc32(0L, Z_NULL, 0);
        for (int s0 = 0; s0 < n; s0 += DFL_SEG) {
            const int len = std::min(DFL_SEG, n - s0);
            const uint32_t piece = dfl_crc(tab, b.get() + s0, len);
            CHECK(piece == (uint32_t)crc32(0L, b.get() + s0, (uInt)len), "a segment's CRC");
            crc ^= dfl_crc_shift(x2n, piece, (uint32_t)(n - s0 - len));
            z = crc32_combine(z, piece, len);
        }
        CHECK(crc == (uint32_t)crc32(0L, b.get(), (uInt)n) && crc == (uint32_t)z, "CRC of %d bytes in segments: %08x, zlib %08lx, combined %08lx", n, crc,
              crc32(0L, b.get(), (uInt)n), z);
    }
}

static void test_members()
{
    const int S = DFL_SEG, B = DFL_BLOCK;
    Member m;
    for (int n : {1, 3, 4, 5, S - 1, S, S + 1, DFL_ROUND + 3, B - 1, B}) {
        check_member("one byte repeated", std::vector<uint8_t>((size_t)n, (uint8_t)'F'), &m);
        CHECK(n < 5 || (m.n_match > 0 && m.dused == 1 && (n < 64 || !m.stored)), "one byte repeated, %d bytes: %d matches, %d distance codes", n, m.n_match, m.dused);
        std::vector<uint8_t> alt((size_t)n);
        for (int i = 0; i < n; i++) alt[i] = i & 1 ? 'A' : 'C';
        check_member("two bytes alternating", alt);
        check_member("noise", noise(n), &m);
        CHECK(n < 64 || (m.stored && (int)m.bytes.size() == n + DFL_OVERHEAD), "noise of %d bytes: stored %d, %zu bytes", n, (int)m.stored, m.bytes.size());
        check_member("FASTQ-like", fastq_like(n), &m);
        CHECK(n < B || (!m.stored && m.n_match > 500), "FASTQ-like: %d matches", m.n_match);
    }
    // bytes with Fibonacci counts, shuffled (runs become matches, so the counts of the symbols are not quite these)
    {
        std::vector<uint8_t> v;
        uint32_t a = 1, b2 = 1;
        for (int i = 0; i < 22; i++) { v.insert(v.end(), a, (uint8_t)(i * 11 + 1)); const uint32_t t = a + b2; a = b2; b2 = t; }
        for (size_t i = v.size() - 1; i > 0; i--) std::swap(v[i], v[rnd() % (i + 1)]);
        check_member("Fibonacci counts", v, &m);
        CHECK(m.llongest >= 12 && m.llongest <= DFL_LIT_BITS && !m.stored, "Fibonacci counts: the longest literal code has %d bits", m.llongest);
    }
    // a repeat too far back to be used, one as far as a distance reaches, one a byte farther
    check_member("phrase 40000 apart, noise", phrase_twice(B, 1000, 40000));
    check_member("phrase 40000 apart", phrase_twice(B, 1000, 40000, true), &m);
    CHECK(!m.dist_seen[40000] && m.max_dist < 32768, "a repeat at 40000 (farthest %d)", m.max_dist);
    check_member("phrase 32768 apart, noise", phrase_twice(B, 1024, 32768));
    check_member("phrase 32768 apart", phrase_twice(B, 1024, 32768, true), &m);
    CHECK(m.max_dist == 32768, "the repeat at 32768 was not used (farthest %d)", m.max_dist);
    check_member("phrase 32769 apart, noise", phrase_twice(B, 1024, 32769));
    check_member("phrase 32769 apart", phrase_twice(B, 1024, 32769, true), &m);
    CHECK(!m.dist_seen[32769] && m.max_dist < 32768, "a repeat at 32769 (farthest %d)", m.max_dist);
    // a repeat across the end of a round, and across the end of a segment
    check_member("across a round", phrase_twice(8192, DFL_ROUND - 50, 2 * DFL_ROUND));
    check_member("across a segment", phrase_twice(8192, 3 * S - 50, 2048 + 17));
    for (int it = 0; it < 40; it++) {
        const int n = 1 + (int)(rnd() % 6000);
        std::vector<uint8_t> v((size_t)n);
        const int alpha = 1 + (int)(rnd() % 6);
        for (auto &x : v) x = (uint8_t)('a' + rnd() % (uint32_t)alpha);
        check_member("seeded small alphabet", v);
    }
}

int main()
{
    test_symbols();
    test_lengths();
    test_crc();
    test_members();
    std::printf("%ld checks, %d failures\n", g_checks, g_fail);
    if (g_fail) return 1;
    std::printf("ok\n");
    return 0;
}

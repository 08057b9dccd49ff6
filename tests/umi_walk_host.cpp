// The lane work of the UMI take and of the tagged render (csrc/ffq_umiwalk.h: the functions the kernels of csrc/ffq_umi.h
// themselves call), driven on the host against loops over bytes (include/ffq.h, ffq_table_take_umi and
// ffq_table_render_fastq_umi): the first blank and the newline look over sixteen bytes, the cut, the carrier's positions, and
// the chunk-relative spans of a tagged row's pieces.  A row is assembled the way render's copy does it -- the output cut into
// 16-byte chunks aligned on the output address, every piece merged into the chunks it lies under -- for every shift 0..15, and
// compared with the plain concatenation.  Every piece lives in a heap block of exactly its length, so a span that leaves its
// piece is an out-of-bounds read AddressSanitizer reports.
//
//   clang++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I <package>/csrc tests/umi_walk_host.cpp -o umi_walk_host
// Exit status 0 and "ok" on the last line, or 1 and a line per failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "ffq_umiwalk.h"

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

// a heap block of exactly n bytes
struct Block {
    std::unique_ptr<uint8_t[]> p;
    int64_t n;
    explicit Block(const std::string &s) : p(new uint8_t[s.size() ? s.size() : 1]), n((int64_t)s.size()) { std::memcpy(p.get(), s.data(), s.size()); }
};

static void sixteen(const uint8_t *b, uint32_t w[4])
{
    for (int j = 0; j < 4; j++) w[j] = (uint32_t)b[4 * j] | ((uint32_t)b[4 * j + 1] << 8) | ((uint32_t)b[4 * j + 2] << 16) | ((uint32_t)b[4 * j + 3] << 24);
}

static void test_sixteen_bytes()
{
    static const uint8_t pool[] = {' ', '\t', '\n', 'A', 'a', 0, 0x80, 0x89, 0xA0, 0x0B, 0x1F, 0x21, 0x8A, 0xFF, 0x08, 0x0A ^ 0x80};
    for (int it = 0; it < 20000; it++) {
        uint8_t b[16];
        const int dense = it % 3;                            // few special bytes, some, many
        for (int j = 0; j < 16; j++) b[j] = dense == 0 && rnd() % 8 ? (uint8_t)('A' + rnd() % 26) : pool[rnd() % (dense == 2 ? 3 : sizeof pool)];
        uint32_t w[4];
        sixteen(b, w);
        for (int nv = 0; nv <= 16; nv++) {
            int blank = 16;
            bool nl = false;
            for (int j = nv - 1; j >= 0; j--) {
                if (b[j] == ' ' || b[j] == '\t') blank = j;
                nl |= b[j] == '\n';
            }
            CHECK(umi_blank16(w[0], w[1], w[2], w[3], nv) == blank, "it %d nvalid %d: %d != %d", it, nv, umi_blank16(w[0], w[1], w[2], w[3], nv), blank);
            CHECK(umi_nl16(w[0], w[1], w[2], w[3], nv) == nl, "it %d nvalid %d", it, nv);
        }
    }
}

static void test_cut_and_carrier()
{
    // the issue's read lengths: len - 1, len, len + skip - 1, len + skip, 0
    CHECK(umi_cut(7, 8, 3) == 0 && umi_cut(8, 8, 3) == 8 && umi_cut(10, 8, 3) == 10 && umi_cut(11, 8, 3) == 11 && umi_cut(12, 8, 3) == 11, "cut");
    CHECK(umi_cut(0, 8, 3) == 0 && umi_cut(0, 1, 0) == 0 && umi_cut(1, 1, 0) == 1 && umi_cut(129, 64, 64) == 128 && umi_cut(100, 64, 64) == 100, "cut");
    for (int n = 0; n < 200; n++)
        for (int len = 1; len <= 64; len += 7)
            for (int skip = 0; skip <= 64; skip += 9) {
                const int64_t want = n < len ? 0 : (len + skip < n ? len + skip : n);
                CHECK(umi_cut(n, len, skip) == want, "n %d len %d skip %d", n, len, skip);
            }
    // c1 = pos1, c2 = pos2, L = the buffer's coordinates
    CHECK(umi_carrier_pos(5, 14, 100, 8) && !umi_carrier_pos(5, 13, 100, 8) && !umi_carrier_pos(5, 6, 100, 1) && umi_carrier_pos(5, 7, 100, 1), "pos2");
    CHECK(umi_carrier_pos(0, 9, 100, 8) && !umi_carrier_pos(-1, 9, 100, 8) && !umi_carrier_pos(5, -1, 100, 8), "negative");
    CHECK(umi_carrier_pos(91, 100, 100, 8) && !umi_carrier_pos(92, 200, 100, 8) && !umi_carrier_pos(INT64_MAX - 2, INT64_MAX, 100, 1), "the buffer's end");
    CHECK(!umi_carrier_pos(INT64_MIN, INT64_MAX, 100, 8) && !umi_carrier_pos(0, INT64_MAX, 0, 1) && umi_carrier_pos(0, INT64_MAX, 2, 1), "wild positions");
    CHECK(umi_ins_len(UMI_READ1, 8, 0) == 9 && umi_ins_len(UMI_READ2, 8, 3) == 13 && umi_ins_len(UMI_PER_READ, 8, 16) == 35, "insert");
}

static std::string letters(int64_t n, const char *from)
{
    std::string s;
    const size_t k = std::strlen(from);
    for (int64_t i = 0; i < n; i++) s.push_back(from[rnd() % k]);
    return s;
}

// one tagged row, chunk by chunk, at every shift; `total` rows so far
static void one_row(int64_t h, int64_t k, int64_t sn, int loc, int len, int prefix_len)
{
    std::string head = letters(h, "ABCxyz0189:/#");
    if (k < h) head[(size_t)k] = rnd() & 1 ? ' ' : '\t';
    const std::string seq = letters(sn, "ACGTN"), qual = letters(sn, "!#5?AFI"), tag1 = letters(len, "ACGT"), tag2 = letters(len, "acgt");
    const std::string prefix = letters(prefix_len, "PQRpqr019");
    uint8_t lit[UMI_LIT_MAX];
    const int lit_n = umi_literal(lit, (uint8_t)':', reinterpret_cast<const uint8_t *>(prefix.data()), prefix_len);
    std::string tag = loc == UMI_READ1 ? tag1 : loc == UMI_READ2 ? tag2 : tag1 + "_" + tag2;
    const std::string want = "@" + head.substr(0, (size_t)k) + ":" + (prefix_len ? prefix + "_" : "") + tag + head.substr((size_t)k) + "\n" + seq + "\n+\n" + qual + "\n";
    const UmiLayout Y = umi_layout(h, k, sn, sn, loc, len, prefix_len);
    CHECK(Y.len == (int64_t)want.size() && lit_n == Y.lit_n && Y.len == h + 2 * sn + 6 + umi_ins_len(loc, len, prefix_len), "h %lld k %lld s %lld loc %d len %d",
          (long long)h, (long long)k, (long long)sn, loc, len);
    // the pieces, each in a block of its own: header (head and tail are two spans of it), tags, sequence, quality
    const Block bh(head), b1(tag1), b2(tag2), bs(seq), bq(qual);
    struct Piece { int64_t at, n; const uint8_t *src; int64_t src_n; };
    const Piece pieces[6] = {{1, k, bh.p.get(), k}, {Y.o_t1, Y.t1_n, b1.p.get(), b1.n}, {Y.o_t2, Y.t2_n, b2.p.get(), b2.n},
                             {Y.o_tail, Y.tail_n, bh.p.get() + k, h - k}, {Y.o_s, sn, bs.p.get(), bs.n}, {Y.o_q, sn, bq.p.get(), bq.n}};
    for (int shift = 0; shift < 16; shift++) {
        std::string got((size_t)Y.len, '?');
        const int64_t nchunk = (Y.len + shift + 15) >> 4;
        for (int64_t c = 0; c < nchunk; c++) {
            const int64_t clo = 16 * c - shift;
            uint8_t y[16];
            bool set[16] = {false};
            int a, b;
            for (const Piece &p : pieces) {
                umi_span(p.at - clo, p.n, a, b);
                for (int t = a; t < b; t++) {
                    const int64_t i = clo + t - p.at;            // byte of the piece: inside its block, or ASan says so
                    CHECK(i >= 0 && i < p.src_n && !set[t], "piece at %lld byte %lld", (long long)p.at, (long long)i);
                    y[t] = p.src[i]; set[t] = true;
                }
            }
            umi_span(Y.o_lit - clo, Y.lit_n, a, b);
            for (int t = a; t < b; t++) { CHECK(!set[t], "literal"); y[t] = lit[t - (int)(Y.o_lit - clo)]; set[t] = true; }
            const int64_t puts[7][2] = {{0, '@'}, {loc == UMI_PER_READ ? Y.o_t2 - 1 : -1, '_'}, {Y.o_s - 1, '\n'}, {Y.o_p, '\n'}, {Y.o_p + 1, '+'},
                                        {Y.o_p + 2, '\n'}, {Y.len - 1, '\n'}};
            for (const auto &pt : puts) {
                const int64_t t = pt[0] - clo;
                if (pt[0] < 0 || t < 0 || t >= 16) continue;
                CHECK(!set[t], "literal byte %lld", (long long)pt[0]);
                y[t] = (uint8_t)pt[1]; set[t] = true;
            }
            const int kb = (int)(clo < 0 ? -clo : 0), ke = (int)(Y.len - clo < 16 ? Y.len - clo : 16);
            for (int t = 0; t < 16; t++) CHECK(set[t] == (t >= kb && t < ke), "chunk %lld byte %d of a row of %lld, shift %d", (long long)c, t, (long long)Y.len, shift);
            for (int t = kb; t < ke; t++) got[(size_t)(clo + t)] = (char)y[t];
        }
        CHECK(got == want, "h %lld k %lld s %lld loc %d len %d prefix %d shift %d", (long long)h, (long long)k, (long long)sn, loc, len, prefix_len, shift);
    }
}

static void test_rows()
{
    static const int lens[] = {1, 7, 16, 17, 64};
    static const int prefixes[] = {0, 3, 16};
    for (int64_t h = 1; h <= 40; h++)
        for (int kk = 0; kk < 4; kk++) {
            const int64_t k = kk == 0 ? h : kk == 1 ? 0 : kk == 2 ? h / 2 : h - 1;
            for (int64_t sn = 0; sn <= 40; sn += (h % 3) + 1)
                one_row(h, k, sn, 1 + (int)((h + sn + kk) % 3), lens[(h + kk) % 5], prefixes[(sn + kk) % 3]);
        }
    for (int it = 0; it < 300; it++) {
        const int64_t h = 1 + rnd() % 200;
        one_row(h, rnd() % (h + 1), rnd() % 300, 1 + (int)(rnd() % 3), 1 + (int)(rnd() % 64), (int)(rnd() % 17));
    }
    one_row(3000, 2900, 100, UMI_READ1, 12, 3);
    one_row(1, 1, 6000, UMI_PER_READ, 64, 16);
}

int main()
{
    test_sixteen_bytes();
    test_cut_and_carrier();
    test_rows();
    std::printf("%ld checks, %d failures\n", g_checks, g_fail);
    std::printf(g_fail ? "FAILED\n" : "ok\n");
    return g_fail ? 1 : 0;
}

// The lane and chunk work of the poly-tail walk (csrc/ffq_polywalk.h: the functions k_poly_rows and k_poly_long themselves
// call), driven on the host against the rule's loop over bytes (include/ffq.h, ffq_table_trim_poly).  A group is emulated
// lane by lane: every lane classifies and sums its bytes, the prefix sum and the maxima that the kernel takes with DPP moves
// are plain loops here, and poly_chunk_end moves the state on -- in both shapes, eight lanes of eight bytes (chunks of 64) and
// sixty-four lanes of sixteen (chunks of 1024).  Every sequence lives in a heap block of exactly its length, so a load that
// leaves the sequence is an out-of-bounds read AddressSanitizer reports.
//
//   clang++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I <package>/csrc tests/poly_walk_host.cpp -o poly_walk_host
// Exit status 0 and "ok" on the last line, or 1 and a line per failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "ffq_polywalk.h"

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

// ---- the rule over bytes (include/ffq.h) ----
static int cls(uint8_t b)
{
    switch (b) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
    }
}

static int64_t loop_cut(const uint8_t *seq, int64_t n, int base, int min_len)
{
    int64_t mm[4] = {0, 0, 0, 0}, hit[4] = {0, 0, 0, 0}, last[4] = {-1, -1, -1, -1}, stop = n;
    bool in_s[4];
    for (int b = 0; b < 4; b++) in_s[b] = base == POLY_ANY || b == base;
    for (int64_t i = 0; i < n; i++) {
        const int k = cls(seq[n - 1 - i]);
        const int64_t allowed = (i + 1) / 8 < 5 ? (i + 1) / 8 : 5;
        int64_t t[4];
        bool every = true;
        for (int b = 0; b < 4; b++) {
            t[b] = mm[b] + (k != b);
            if (in_s[b] && t[b] <= allowed) every = false;
        }
        if (i >= min_len - 1 && every) { stop = i; break; }
        for (int b = 0; b < 4; b++) mm[b] = t[b];
        if (k < 4 && in_s[k]) { hit[k]++; last[k] = i; }
    }
    if (stop < min_len) return n;
    int best = -1;
    for (int b = 0; b < 4; b++)
        if (in_s[b] && (best < 0 || hit[b] > hit[best])) best = b;
    return n - 1 - last[best];
}

// ---- a group of G lanes with B bytes each, lane by lane ----
template <int G, int B>
static int64_t group_cut(const uint8_t *seq, int64_t n, int base, int min_len, int *chunks)
{
    constexpr int C = G * B;
    typedef PolyOps<C> P;
    typedef typename P::T T;
    PolyState<C> s = {P::begin(base), -1, 0};
    int64_t newlen = n;
    bool act = n >= min_len;
    *chunks = 0;
    while (act) {
        ++*chunks;
        static int k[G][B];
        typename PolyHits<B>::T hits[G];
        T t[G], at[G];
        int avail[G], stop_j[G];
        for (int gl = 0; gl < G; gl++) {
            const int64_t i0 = s.w0 + (int64_t)gl * B;
            const int64_t left = n - i0;
            avail[gl] = (int)(left < 0 ? 0 : left < B ? left : B);
            int qv[B];                                  // ascending addresses, -1 where the read has no byte
            for (int j = 0; j < B; j++) qv[j] = j >= B - avail[gl] ? (int)seq[n - i0 - B + j] : -1;
            const bool nl = poly_classify<B>(qv, k[gl], hits[gl]);
            bool has_nl = false;
            for (int j = 0; j < B; j++) has_nl |= qv[j] == 10;
            CHECK(nl == has_nl, "newline flag, lane %d", gl);
            t[gl] = poly_lane_sum<C, B>(k[gl], avail[gl]);
        }
        T run = 0;
        int skey = 0;
        for (int gl = 0; gl < G; gl++) {
            const T start = s.mm + run;                 // carried + the exclusive prefix
            run += t[gl];
            poly_lane_walk<C, B>(k[gl], avail[gl], s.w0 + (int64_t)gl * B, min_len, start, stop_j[gl], at[gl]);
            const int key = poly_stop_key<C, B>(gl, stop_j[gl]);
            if (key > skey) skey = key;
        }
        const int el = poly_end_lane<C, B>(skey, s.w0, n);
        CHECK(el >= 0 && el < G, "end lane %d", el);
        int g[4];
        for (int b = 0; b < 4; b++) {
            g[b] = 0;
            if (P::field(s.mm, b) >= POLY_DEAD) continue;      // (the kernel skips a base no row of the wave has alive)
            for (int gl = 0; gl < G; gl++) {
                const int key = poly_hit_key<B>(hits[gl], b, poly_hit_upto<C, B>(skey, gl, avail[gl]), gl);
                if (key > g[b]) g[b] = key;
            }
        }
        for (int b = 0; b < 4; b++) CHECK(P::field(at[el], b) <= POLY_DEAD + C, "field %d", b);
        act = poly_chunk_end<C>(s, n, min_len, skey, at[el], g, &newlen);
    }
    return newlen;
}

static void one(const std::vector<uint8_t> &v, int base, int min_len, const char *what)
{
    const int64_t n = (int64_t)v.size();
    std::unique_ptr<uint8_t[]> block(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(block.get(), v.data(), (size_t)n);
    const int64_t want = loop_cut(block.get(), n, base, min_len);
    int c8 = 0, c64 = 0;
    const int64_t got8 = group_cut<8, 8>(block.get(), n, base, min_len, &c8);
    const int64_t got64 = group_cut<64, 16>(block.get(), n, base, min_len, &c64);
    CHECK(got8 == want, "%s: n %lld base %d min_len %d: chunks of 64 give %lld, the loop %lld", what, (long long)n, base, min_len, (long long)got8, (long long)want);
    CHECK(got64 == want, "%s: n %lld base %d min_len %d: chunks of 1024 give %lld, the loop %lld", what, (long long)n, base, min_len, (long long)got64, (long long)want);
    CHECK(c8 <= n / 64 + 1 && c64 <= n / 1024 + 1, "%s: %d and %d chunks for %lld bytes", what, c8, c64, (long long)n);
}

static const char LET[] = "ACGT", LOW[] = "acgt", OTHER[] = "N*.-n";

static uint8_t not_base(int b)
{
    const uint32_t r = rnd() % 8;
    if (r < 5) return (uint8_t)OTHER[r];
    return (uint8_t)LET[(b + 1 + r % 3) & 3];
}

static void body(std::vector<uint8_t> &v, int n)
{
    for (int i = 0; i < n; i++) {
        const uint32_t r = rnd();
        v.push_back(r % 50 == 0 ? (uint8_t)'N' : r % 17 == 0 ? (uint8_t)LOW[(r >> 8) & 3] : (uint8_t)LET[(r >> 8) & 3]);
    }
}

int main()
{
    // the functions on their own
    for (int i = 0; i < 200; i++) CHECK(poly_allowed(i) == ((i + 1) / 8 < 5 ? (i + 1) / 8 : 5), "allowed(%d)", i);
    for (int c = -1; c < 256; c++) CHECK(poly_cls(c) == (c < 0 ? 4 : cls((uint8_t)c)), "class of %d", c);
    for (int a = 0; a <= 5; a++)
        for (int f = 0; f <= POLY_DEAD + 64; f++) {
            const uint32_t x = (uint32_t)f * PolyOps<64>::ONES;
            CHECK(PolyOps<64>::all_above(x, a) == (f > a), "all_above(%d, %d)", f, a);
            CHECK(PolyOps<64>::all_above(x - (uint32_t)(f ? 1 : 0) * (1u << 16), a) == (f > a && f - 1 > a), "one field below");
        }
    for (int a = 0; a <= 5; a++)
        for (int f = 0; f <= POLY_DEAD + 1024; f += (f < 20 ? 1 : 37)) {
            const uint64_t x = (uint64_t)f * PolyOps<1024>::ONES;
            CHECK(PolyOps<1024>::all_above(x, a) == (f > a), "wide all_above(%d, %d)", f, a);
        }
    CHECK(PolyOps<64>::saturate(0x46000506u) == 0x06000506u, "saturate");
    CHECK(PolyOps<64>::begin(2) == 0x06000606u && PolyOps<64>::begin(POLY_ANY) == 0u, "begin");

    // the issue's hand vectors
    struct { const char *seq; int base, want; } hand[] = {
        {"ACGTACGTACGGGGGGGGGG", 2, 10}, {"ACGTACGTACGGGGGGGGG", 2, 10}, {"ACGTACGTACGGGGGGGG", 2, 18}, {"GGGGGGGGGG", 2, 0},
        {"GGGGGGGGG", 2, 9}, {"ACGTACGTATGGGAGGGGGGGGGGAG", 2, 14}, {"ACGTACGTATGAGAGGGGGGGGGGGG", 2, 12},
        {"ACGTACGTACTTTTNTTTTTTT", POLY_ANY, 10}, {"ACGTACGTACNNNNNNNNNNNN", POLY_ANY, 22}, {"ACGTTTTTTTAAAAAAAAAA", POLY_ANY, 10},
        {"ACGTTTTTTTTAAAAAAAAAA", POLY_ANY, 11}, {"acgtacgtacgggggggggggg", 2, 10},
    };
    for (const auto &h : hand) {
        std::vector<uint8_t> v(h.seq, h.seq + std::strlen(h.seq));
        CHECK(loop_cut(v.data(), (int64_t)v.size(), h.base, 10) == h.want, "the loop on %s", h.seq);
        one(v, h.base, 10, "hand");
    }

    // every tail length 0..140 for each base with 0..7 planted mismatches, behind a body of 0..40 bytes
    for (int len = 0; len <= 140; len++)
        for (int b = 0; b < 4; b++)
            for (int mism = 0; mism <= 7; mism++) {
                std::vector<uint8_t> v;
                body(v, (int)(rnd() % 41));
                const size_t at = v.size();
                for (int i = 0; i < len; i++) v.push_back((uint8_t)(rnd() % 9 ? LET[b] : LOW[b]));
                for (int m = 0; m < mism && len > 0; m++) {
                    // a walk position: in the grace zone, or anywhere in the tail
                    const int i = (int)(rnd() % (uint32_t)((m & 1) && len > 9 ? 9 : len));
                    v[at + (size_t)(len - 1 - i)] = not_base(b);
                }
                const int min_len = mism == 7 ? 2 + (int)(rnd() % 30) : 10;
                one(v, b, min_len, "tail");
                one(v, POLY_ANY, min_len, "tail, any base");
                one(v, (b + 1) & 3, min_len, "tail, another base");
            }

    // seeded cases up to 5000 positions: long tails whose mismatches come about one in eight, one in sixteen, or in a burst;
    // min_len from 2 to beyond the read
    static const int MIN_LENS[] = {2, 10, 10, 10, 33, 64, 65, 200, 1024, 1025, 3000, 65535};
    for (int it = 0; it < 1500; it++) {
        std::vector<uint8_t> v;
        const int b = (int)(rnd() % 4);
        body(v, (int)(rnd() % 300));
        const int len = (int)(rnd() % (it % 3 == 0 ? 5000u : 1300u));
        const uint32_t every = it % 5 == 0 ? 8 : it % 5 == 1 ? 16 : 400;
        const int burst = (int)(rnd() % (uint32_t)(len + 1));
        for (int i = 0; i < len; i++) {
            uint8_t c = (uint8_t)LET[b];
            if (rnd() % every == 0) c = not_base(b);
            if (it % 7 == 0 && i >= burst && i < burst + 6) c = not_base(b);
            v.push_back(c);
        }
        const int min_len = MIN_LENS[rnd() % (sizeof MIN_LENS / sizeof MIN_LENS[0])];
        one(v, it % 2 ? b : POLY_ANY, min_len, "seeded");
    }
    // a read of nothing but tail, at the chunk edges
    for (int n : {0, 1, 2, 9, 10, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2048, 4096, 4097, 5000}) {
        std::vector<uint8_t> v((size_t)n, (uint8_t)'G');
        one(v, 2, 10, "all tail");
        one(v, POLY_ANY, 10, "all tail, any base");
        one(v, 0, 10, "all of another base");
        if (n > 70) { v[(size_t)n - 65] = 'A'; v[(size_t)n - 64] = 'A'; one(v, 2, 10, "mismatches on the chunk edge"); }
    }

    std::printf("%ld checks, %d failures\n", g_checks, g_fail);
    if (g_fail) return 1;
    std::printf("ok\n");
    return 0;
}

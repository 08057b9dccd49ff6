// The word work of the overlap analysis (csrc/ffq_overlapwalk.h: the functions k_pair_overlap itself calls), driven on the
// host against a loop over bytes: the packing of both mates (two bits per base and a `bad` bit, mate 2 reversed and
// complemented), the mismatch count of a candidate at every offset, its early exit, the order of the candidates and the
// first accepted one.  Every sequence lives in a heap block of exactly its length, so a load that leaves the sequence is an
// out-of-bounds read AddressSanitizer reports.
//
//   clang++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I <package>/csrc tests/overlap_pack_host.cpp -o overlap_pack_host
// Exit status 0 and "ok" on the last line, or 1 and a line per failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "ffq_overlapwalk.h"

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
static int rb_at(const uint8_t *b, int n2, int j) { const int c = cls(b[n2 - 1 - j]); return c < 4 ? 3 - c : 4; }
static int loop_mm(const uint8_t *a, const uint8_t *b, int n2, int o, int lo, int hi)
{
    int mm = 0;
    for (int i = lo; i < hi; i++) {
        const int ca = cls(a[i]);
        mm += !(ca < 4 && ca == rb_at(b, n2, i - o));
    }
    return mm;
}
// the first accepted candidate's offset; false: none
static bool loop_find(const uint8_t *a, int n1, const uint8_t *b, int n2, int mo, int max_diff, int permille, int &ostar)
{
    if (n1 < mo || n2 < mo) return false;
    std::vector<int> cand;
    for (int o = 0; o <= n1 - mo; o++) cand.push_back(o);
    for (int o = 1; o <= n2 - mo; o++) cand.push_back(-o);
    for (int o : cand) {
        const int lo = o > 0 ? o : 0, hi = n1 < n2 + o ? n1 : n2 + o, ov = hi - lo;
        const int lim = max_diff < ov * permille / 1000 ? max_diff : ov * permille / 1000;
        if (loop_mm(a, b, n2, o, lo, hi) <= lim) { ostar = o; return true; }
    }
    return false;
}

// ---- the packed side ----
struct Planes { uint32_t ac[OVL_PLANE], ab[OVL_PLANE], rc[OVL_PLANE], rbad[OVL_PLANE]; };

// exact-size copies: a[-1], a[n] do not exist
static std::unique_ptr<uint8_t[]> exact(const std::vector<uint8_t> &v)
{
    std::unique_ptr<uint8_t[]> p(new uint8_t[v.size() ? v.size() : 1]);
    if (!v.empty()) std::memcpy(p.get(), v.data(), v.size());
    return p;
}

static void pack(const uint8_t *a, int n1, const uint8_t *b, int n2, Planes &P)
{
    // (garbage where the kernel's planes hold a former pair's words)
    for (int i = 0; i < OVL_PLANE; i++) P.ac[i] = P.ab[i] = P.rc[i] = P.rbad[i] = 0xDEADBEEFu ^ (uint32_t)i;
    P.ac[0] = P.ab[0] = P.rc[0] = P.rbad[0] = 0;
    P.ac[OVL_PLANE - 1] = P.ab[OVL_PLANE - 1] = P.rc[OVL_PLANE - 1] = P.rbad[OVL_PLANE - 1] = 0;
    uint32_t x[4];
    for (int W = 0; W < (n1 + 15) / 16; W++) ovl_pack_fwd(a, n1, W, P.ac[W + 1], P.ab[W + 1], x);
    const int nw2 = ovl_imin((n2 + 15) / 16 + 1, OVL_WORDS);
    for (int W = 0; W < nw2; W++) ovl_pack_rc(b, n2, W, P.rc[W + 1], P.rbad[W + 1], x);
}

// internal code of a class: the header's bijection (A 0, C 1, T 2, G 3)
static uint32_t code_of(int c) { static const uint32_t k[4] = {0, 1, 3, 2}; return k[c]; }

static void check_planes(const uint8_t *a, int n1, const uint8_t *b, int n2, const Planes &P)
{
    for (int p = 0; p < n1; p++) {
        const int c = cls(a[p]);
        const uint32_t bad = (P.ab[1 + (p >> 4)] >> (2 * (p & 15))) & 3u, code = (P.ac[1 + (p >> 4)] >> (2 * (p & 15))) & 3u;
        CHECK(bad == (c == 4 ? 1u : 0u), "a bad p=%d n1=%d", p, n1);
        if (c < 4) CHECK(code == code_of(c), "a code p=%d n1=%d", p, n1);
    }
    for (int p = n1; p < ((n1 + 15) / 16) * 16; p++)
        CHECK(((P.ab[1 + (p >> 4)] >> (2 * (p & 15))) & 3u) == 1u, "a pad p=%d n1=%d", p, n1);
    for (int j = 0; j < n2; j++) {
        const int c = rb_at(b, n2, j);
        const uint32_t bad = (P.rbad[1 + (j >> 4)] >> (2 * (j & 15))) & 3u, code = (P.rc[1 + (j >> 4)] >> (2 * (j & 15))) & 3u;
        CHECK(bad == (c == 4 ? 1u : 0u), "rb bad j=%d n2=%d", j, n2);
        if (c < 4) CHECK(code == code_of(c), "rb code j=%d n2=%d", j, n2);
    }
    for (int j = n2; j < ((n2 + 15) / 16) * 16; j++)
        CHECK(((P.rbad[1 + (j >> 4)] >> (2 * (j & 15))) & 3u) == 1u, "rb pad j=%d n2=%d", j, n2);
}

static const char ALPHA[] = "ACGTACGTACGTacgtNn.\n";

static std::vector<uint8_t> random_seq(int n, int alpha)
{
    std::vector<uint8_t> v((size_t)n);
    for (auto &c : v) c = (uint8_t)ALPHA[rnd() % (uint32_t)alpha];
    return v;
}

static uint8_t comp(uint8_t c)
{
    switch (c) {
    case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A';
    case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a';
    default: return c;
    }
}

// every offset with at least one position in the overlap: the count without a limit, and mm <= limit for some limits
static void every_offset(const uint8_t *a, int n1, const uint8_t *b, int n2, const Planes &P, int stride)
{
    for (int o = -(n2 - 1); o <= n1 - 1; o += stride) {
        const int lo = o > 0 ? o : 0, hi = n1 < n2 + o ? n1 : n2 + o;
        if (hi <= lo) continue;
        const int want = loop_mm(a, b, n2, o, lo, hi);
        CHECK(ovl_count(P.ac, P.ab, P.rc, P.rbad, o, lo, hi, 1 << 20) == want, "n1=%d n2=%d o=%d want %d", n1, n2, o, want);
        for (int limit : {0, 1, want - 1, want, 5})
            if (limit >= 0)
                CHECK((ovl_count(P.ac, P.ab, P.rc, P.rbad, o, lo, hi, limit) <= limit) == (want <= limit), "n1=%d n2=%d o=%d limit=%d", n1, n2, o, limit);
    }
}

static void search(const uint8_t *a, int n1, const uint8_t *b, int n2, const Planes &P, int mo, int max_diff, int permille)
{
    int want_o = 0;
    const bool want = loop_find(a, n1, b, n2, mo, max_diff, permille, want_o);
    const int nc = ovl_ncand(n1, n2, mo);
    bool got = false;
    int got_o = 0;
    for (int c = 0; c < nc && !got; c++) {
        const int o = ovl_cand(c, n1, mo), lo = ovl_imax(0, o), hi = ovl_imin(n1, n2 + o);
        CHECK(hi - lo >= mo, "ov n1=%d n2=%d o=%d", n1, n2, o);
        const int limit = ovl_limit(hi - lo, max_diff, permille);
        if (ovl_count(P.ac, P.ab, P.rc, P.rbad, o, lo, hi, limit) <= limit) { got = true; got_o = o; }
    }
    CHECK(got == want && (!got || got_o == want_o), "search n1=%d n2=%d mo=%d: %d %d / %d %d", n1, n2, mo, (int)got, got_o, (int)want, want_o);
}

int main()
{
    // the order of the candidates
    for (int n1 = 0; n1 <= 12; n1++)
        for (int n2 = 0; n2 <= 12; n2++)
            for (int mo = 1; mo <= 6; mo++) {
                std::vector<int> cand;
                if (n1 >= mo && n2 >= mo) {
                    for (int o = 0; o <= n1 - mo; o++) cand.push_back(o);
                    for (int o = 1; o <= n2 - mo; o++) cand.push_back(-o);
                }
                CHECK(ovl_ncand(n1, n2, mo) == (int)cand.size(), "ncand %d %d %d", n1, n2, mo);
                for (int c = 0; c < (int)cand.size(); c++) CHECK(ovl_cand(c, n1, mo) == cand[(size_t)c], "cand %d %d %d %d", n1, n2, mo, c);
            }

    // all length pairs up to 40 x 40, every offset: random bytes (bases of both cases, N, other bytes), and mates that overlap
    Planes P;
    for (int n1 = 0; n1 <= 40; n1++)
        for (int n2 = 0; n2 <= 40; n2++) {
            for (int kind = 0; kind < 2; kind++) {
                std::vector<uint8_t> va = random_seq(n1, kind ? 4 : 20), vb = random_seq(n2, kind ? 4 : 20);
                if (kind) {
                    // mate 2 = reverse complement of mate 1's beginning, a few bytes changed
                    for (int j = 0; j < n2; j++)
                        if (n2 - 1 - j < n1 && rnd() % 8) vb[(size_t)j] = comp(va[(size_t)(n2 - 1 - j)]);
                }
                auto a = exact(va), b = exact(vb);
                pack(a.get(), n1, b.get(), n2, P);
                check_planes(a.get(), n1, b.get(), n2, P);
                every_offset(a.get(), n1, b.get(), n2, P, 1);
                for (int mo : {1, 3, 8}) search(a.get(), n1, b.get(), n2, P, mo, 5, 200);
            }
        }

    // seeded cases up to 512: a fragment read from both ends, mismatches, an adapter tail
    for (int t = 0; t < 300; t++) {
        const int n1 = t < 8 ? 512 - (t & 3) : 1 + (int)(rnd() % 512), n2 = t < 8 ? 512 - (t >> 2) : 1 + (int)(rnd() % 512);
        const int frag = 1 + (int)(rnd() % 700);
        std::vector<uint8_t> f = random_seq(frag, 4), va = random_seq(n1, 4), vb = random_seq(n2, 4);
        for (int i = 0; i < n1 && i < frag; i++) va[(size_t)i] = f[(size_t)i];
        for (int j = 0; j < n2 && j < frag; j++) vb[(size_t)j] = comp(f[(size_t)(frag - 1 - j)]);
        for (int k = (int)(rnd() % 8); k > 0; k--) va[rnd() % (uint32_t)n1] = (uint8_t)ALPHA[rnd() % 18];
        auto a = exact(va), b = exact(vb);
        pack(a.get(), n1, b.get(), n2, P);
        check_planes(a.get(), n1, b.get(), n2, P);
        every_offset(a.get(), n1, b.get(), n2, P, 1 + (int)(rnd() % 13));
        search(a.get(), n1, b.get(), n2, P, 30, 5, 200);
        search(a.get(), n1, b.get(), n2, P, 1 + (int)(rnd() % 40), (int)(rnd() % 8), (int)(rnd() % 300));
    }

    std::printf("%ld checks, %d failures\n", g_checks, g_fail);
    std::printf(g_fail ? "FAILED\n" : "ok\n");
    return g_fail ? 1 : 0;
}

// The chunk functions of csrc/ffq_correctwalk.h on a CPU, against a loop over bytes (the rule of include/ffq.h at
// ffq_table_pair_correct).  Every n1, n2 up to 40 with every valid o, then seeded cases up to 512.  Both buffers are allocated
// exactly and hold nothing but the pair's two lines, in either order: every line begins at the first byte of an allocation in
// some cases and ends at the last in others, so a load that under-reads or over-reads is a report under AddressSanitizer.  The
// corrections are applied the way the kernel applies them -- one byte store per corrected byte -- and both whole buffers are
// compared; a second pass over the result must correct nothing.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ffq_correctwalk.h"

using namespace ffq;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static uint8_t comp(uint8_t c)
{
    switch (c) {
    case 'A': return 'T'; case 'T': return 'A'; case 'C': return 'G'; case 'G': return 'C';
    case 'a': return 't'; case 't': return 'a'; case 'c': return 'g'; case 'g': return 'c';
    default: return c;
    }
}

static int cls(uint8_t c)
{
    switch (c) {
    case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3;
    default: return 4;
    }
}

static uint8_t rnd_base()
{
    static const char alphabet[] = "ACGTACGTACGTacgtN.";
    return (uint8_t)alphabet[rnd() % (sizeof alphabet - 1)];
}

// qualities around both thresholds (G - 1, G, B, B + 1 among them), sometimes any byte
static uint8_t rnd_qual(uint32_t G, uint32_t B)
{
    switch (rnd() % 8) {
    case 0: return (uint8_t)rnd();
    case 1: return (uint8_t)G;
    case 2: return (uint8_t)(G - 1);
    case 3: return (uint8_t)B;
    case 4: return (uint8_t)(B + 1);
    case 5: return (uint8_t)(G + rnd() % 3);
    default: return (uint8_t)(B - (B ? rnd() % 2 : 0));
    }
}

static long failures = 0, cases = 0, total_fix1 = 0, total_fix2 = 0, total_mism = 0;

struct Counts { long mism, fix1, fix2; };

// the kernel's way: chunk by chunk, a byte store per corrected byte
static Counts walk(uint8_t *d1, uint8_t *d2, const CorPair &P, uint32_t G, uint32_t B)
{
    Counts c = {0, 0, 0};
    const int nchunk = cor_nchunk(P);
    for (int k = 0; k < nchunk; k++) {
        CorLoads X;
        CorChunk Y;
        cor_chunk_load(d1, d2, P, k, X);
        cor_chunk_build(P, k, X, G, B, Y);
        c.mism += Y.mism;
        const int p0 = cor_lo(P) + 16 * k;
        for (uint32_t m = cor_bits16(Y.fix1); m; m &= m - 1) {
            const int i = __builtin_ctz(m);
            d1[P.asrc + p0 + i] = cor_byte(Y.na, i); d1[P.qasrc + p0 + i] = cor_byte(Y.nqa, i);
            c.fix1++;
        }
        for (uint32_t m = cor_bits16(Y.fix2); m; m &= m - 1) {
            const int i = __builtin_ctz(m), bi = cor_bi(P, p0 + i);
            d2[P.bsrc + bi] = cor_byte(Y.nb, i); d2[P.qbsrc + bi] = cor_byte(Y.nqb, i);
            c.fix2++;
        }
    }
    return c;
}

static void one_case(int n1, int n2, int o, int layout, uint32_t G, uint32_t B)
{
    cases++;
    std::vector<uint8_t> a(n1), qa(n1), b(n2), qb(n2);
    for (auto &x : a) x = rnd_base();
    for (auto &x : qa) x = rnd_qual(G, B);
    for (auto &x : qb) x = rnd_qual(G, B);
    // mate 2 mostly agrees with mate 1 where they face each other
    for (int j = 0; j < n2; j++) {
        const int p = (n2 - 1 - j) + o;
        b[j] = (p >= 0 && p < n1 && rnd() % 4) ? comp(a[p]) : rnd_base();
    }
    const int64_t nb1 = 2 * (int64_t)n1, nb2 = 2 * (int64_t)n2;
    uint8_t *d1 = (uint8_t *)malloc((size_t)nb1), *d2 = (uint8_t *)malloc((size_t)nb2);
    CorPair P;
    P.n1 = n1; P.n2 = n2; P.o = o;
    if (layout & 1) { P.asrc = 0; P.qasrc = n1; } else { P.qasrc = 0; P.asrc = n1; }
    if (layout & 2) { P.bsrc = 0; P.qbsrc = n2; } else { P.qbsrc = 0; P.bsrc = n2; }
    memcpy(d1 + P.asrc, a.data(), (size_t)n1); memcpy(d1 + P.qasrc, qa.data(), (size_t)n1);
    memcpy(d2 + P.bsrc, b.data(), (size_t)n2); memcpy(d2 + P.qbsrc, qb.data(), (size_t)n2);

    // the rule, byte by byte, on copies
    std::vector<uint8_t> w1(d1, d1 + nb1), w2(d2, d2 + nb2);
    Counts want = {0, 0, 0};
    const int lo = o > 0 ? o : 0, hi = n1 < n2 + o ? n1 : n2 + o;
    for (int p = lo; p < hi; p++) {
        const int bi = n2 - 1 - (p - o);
        uint8_t &xa = w1[(size_t)(P.asrc + p)], &xqa = w1[(size_t)(P.qasrc + p)], &xb = w2[(size_t)(P.bsrc + bi)], &xqb = w2[(size_t)(P.qbsrc + bi)];
        const int ca = cls(xa), cb = cls(xb);
        if (ca < 4 && cb < 4 && ca == 3 - cb) continue;
        want.mism++;
        if (xqa >= G && xqb <= B && ca < 4) { xb = comp(xa); xqb = xqa; want.fix2++; }
        else if (xqb >= G && xqa <= B && cb < 4) { xa = comp(xb); xqa = xqb; want.fix1++; }
    }
    bool bad = hi - lo < 1 || cor_nchunk(P) != (hi - lo + 15) / 16;
    const Counts got = walk(d1, d2, P, G, B);
    bad = bad || got.mism != want.mism || got.fix1 != want.fix1 || got.fix2 != want.fix2;
    bad = bad || memcmp(d1, w1.data(), (size_t)nb1) != 0 || memcmp(d2, w2.data(), (size_t)nb2) != 0;
    // idempotent: a second pass corrects nothing and meets the mismatches that stayed
    const Counts again = walk(d1, d2, P, G, B);
    bad = bad || again.fix1 != 0 || again.fix2 != 0 || again.mism != want.mism - want.fix1 - want.fix2;
    bad = bad || memcmp(d1, w1.data(), (size_t)nb1) != 0 || memcmp(d2, w2.data(), (size_t)nb2) != 0;
    total_fix1 += want.fix1; total_fix2 += want.fix2; total_mism += want.mism;
    if (bad) {
        failures++;
        if (failures < 20) printf("FAIL n1=%d n2=%d o=%d layout=%d G=%u B=%u\n", n1, n2, o, layout, G, B);
    }
    free(d1); free(d2);
}

int main()
{
    // the small pieces on their own
    for (int t = 0; t < 200000; t++) {
        const uint32_t x = t % 2 ? rnd() : (uint32_t)rnd_base() | ((uint32_t)rnd_base() << 8) | ((uint32_t)rnd_base() << 16) | ((uint32_t)rnd_base() << 24);
        const uint32_t y = t % 3 == 0 ? (x ^ (1u << (rnd() % 32))) : t % 3 == 1 ? x : rnd();
        const uint32_t bm = cor_base4(x), e = cor_eq4(x, y);
        for (int i = 0; i < 4; i++) {
            const uint8_t xb = (uint8_t)(x >> (8 * i)), yb = (uint8_t)(y >> (8 * i));
            if ((uint8_t)(bm >> (8 * i)) != (cls(xb) < 4 ? 0xFF : 0)) { failures++; if (failures < 20) printf("base4 %08x\n", x); }
            if ((uint8_t)(e >> (8 * i)) != (xb == yb ? 0xFF : 0)) { failures++; if (failures < 20) printf("eq4 %08x %08x\n", x, y); }
            if (cor_cls(xb) != cls(xb)) { failures++; if (failures < 20) printf("cls %02x\n", xb); }
        }
        Mrg16 m = {cor_eq4(x, y), bm, e ^ bm, x};
        uint32_t bits = 0;
        uint8_t raw[16];
        memcpy(raw, &m, 16);
        for (int i = 0; i < 16; i++) {
            bits |= (uint32_t)(raw[i] & 1) << i;
            if (cor_byte(m, i) != raw[i]) { failures++; if (failures < 20) printf("byte %d\n", i); }
        }
        if (cor_bits16(m) != bits) { failures++; if (failures < 20) printf("bits16 %08x %08x\n", x, y); }
    }
    // the line-bounded load against a loop, on lines allocated exactly
    for (int n = 0; n <= 48; n++) {
        uint8_t *line = (uint8_t *)malloc((size_t)(n ? n : 1));
        for (int i = 0; i < n; i++) line[i] = (uint8_t)(1 + rnd() % 255);
        for (int a = -20; a <= n + 4; a++) {
            const Mrg16 v = cor_load16(line, n, a);
            for (int i = 0; i < 16; i++) {
                const uint8_t want = (a + i >= 0 && a + i < n) ? line[a + i] : 0;
                if (cor_byte(v, i) != want) { failures++; if (failures < 20) printf("load16 n=%d a=%d byte %d\n", n, a, i); }
            }
        }
        free(line);
    }
    static const uint32_t thr[][2] = {{33 + 30, 33 + 14}, {64 + 30, 64 + 14}, {200, 130}, {255, 0}, {1, 0}, {129, 128}};
    for (int n1 = 1; n1 <= 40; n1++)
        for (int n2 = 1; n2 <= 40; n2++)
            for (int o = -(n2 - 1); o <= n1 - 1; o++) {
                const int t = (n1 + 3 * n2 + o + 80) % 6;
                one_case(n1, n2, o, (n1 + n2 + o + 80) & 3, thr[t][0], thr[t][1]);
            }
    static const int lens[] = {1, 2, 15, 16, 17, 31, 32, 33, 150, 511, 512};
    for (int t = 0; t < 800; t++) {
        const int n1 = t % 3 ? lens[rnd() % 11] : 1 + (int)(rnd() % 512), n2 = t % 5 ? lens[rnd() % 11] : 1 + (int)(rnd() % 512);
        int o = -(n2 - 1) + (int)(rnd() % (uint32_t)(n1 + n2 - 1));
        if (t % 7 == 0) o = n1 - 1;
        if (t % 7 == 1) o = -(n2 - 1);
        if (t % 7 == 2) o = 0;
        one_case(n1, n2, o, (int)(rnd() & 3), thr[t % 6][0], thr[t % 6][1]);
    }
    if (total_fix1 < 1000 || total_fix2 < 1000 || total_mism < 2 * (total_fix1 + total_fix2)) {
        failures++;
        printf("the cases show too little: %ld mismatches, %ld + %ld corrections\n", total_mism, total_fix1, total_fix2);
    }
    printf("%ld cases, %ld mismatches, %ld + %ld corrections, %ld failures\n", cases, total_mism, total_fix1, total_fix2, failures);
    if (failures) return 1;
    printf("ok\n");
    return 0;
}

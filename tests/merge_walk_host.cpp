// The chunk builders of csrc/ffq_mergewalk.h on a CPU, against a loop over bytes (the rule of include/ffq.h at
// ffq_table_pair_merge).  Every n1, n2 up to 40 with every valid o and every destination shift 0..15, then seeded cases up to
// 512.  Both buffers are allocated exactly: mate 2's lines begin at its first byte or end at its last, mate 1's end at its
// last, so a load that under-reads or over-reads is a report under AddressSanitizer.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ffq_mergewalk.h"

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

static uint8_t rnd_base()
{
    static const char alphabet[] = "ACGTACGTACGTacgtN.";
    return (uint8_t)alphabet[rnd() % (sizeof alphabet - 1)];
}

// qualities: mostly a narrow band (ties are frequent), sometimes any byte, 0x80 and above among them
static uint8_t rnd_qual() { return rnd() % 8 == 0 ? (uint8_t)rnd() : (uint8_t)(33 + rnd() % 6); }

static long failures = 0, cases = 0;

static void one_case(int n1, int n2, int o, int h, int layout)
{
    cases++;
    // mate 1's buffer: [pad] header a qa, exactly; mate 2's: layout 0: qb b (qb at the first byte), 1: b qb (b at the first byte)
    const int pad1 = layout & 2 ? 0 : 3;
    std::vector<uint8_t> hdr(h), a(n1), qa(n1), b(n2), qb(n2);
    for (auto &x : hdr) x = (uint8_t)(33 + rnd() % 90);
    for (auto &x : a) x = rnd_base();
    for (auto &x : b) x = rnd_base();
    for (auto &x : qa) x = rnd_qual();
    for (auto &x : qb) x = rnd_qual();
    const int64_t nb1 = pad1 + h + 2 * n1, nb2 = 2 * n2;
    uint8_t *d1 = (uint8_t *)malloc((size_t)nb1 ? (size_t)nb1 : 1), *d2 = (uint8_t *)malloc((size_t)nb2 ? (size_t)nb2 : 1);
    memset(d1, '#', (size_t)pad1);
    if (h) memcpy(d1 + pad1, hdr.data(), (size_t)h);
    memcpy(d1 + pad1 + h, a.data(), (size_t)n1);
    memcpy(d1 + pad1 + h + n1, qa.data(), (size_t)n1);
    MrgPair P;
    P.hsrc = pad1; P.asrc = pad1 + h; P.qasrc = pad1 + h + n1; P.h = h;
    if (layout & 1) { memcpy(d2, b.data(), (size_t)n2); memcpy(d2 + n2, qb.data(), (size_t)n2); P.bsrc = 0; P.qbsrc = n2; }
    else { memcpy(d2, qb.data(), (size_t)n2); memcpy(d2 + n2, b.data(), (size_t)n2); P.qbsrc = 0; P.bsrc = n2; }
    P.n1 = n1; P.n2 = n2; P.o = o; P.L = mrg_L(n1, n2, o);

    // the rule, byte by byte
    const int L = o < 0 ? n2 + o : (n1 > n2 + o ? n1 : n2 + o);
    std::vector<uint8_t> want;
    want.push_back('@');
    want.insert(want.end(), hdr.begin(), hdr.end());
    want.push_back('\n');
    std::vector<uint8_t> base(L), qual(L);
    int want_taken = 0, want_ov = 0;
    for (int p = 0; p < L; p++) {
        const bool inA = p < n1;
        const int j2 = p - o;
        const bool inB = j2 >= 0 && j2 < n2;
        const int bi = n2 - 1 - j2;
        if (!inA && !inB) { failures++; printf("no mate at p=%d (n1=%d n2=%d o=%d)\n", p, n1, n2, o); }
        const bool takeB = (inA && inB) ? qb[bi] > qa[p] : !inA;
        if (inA && inB) { want_ov++; if (takeB) want_taken++; }
        base[p] = takeB ? comp(b[bi]) : a[p];
        qual[p] = takeB ? qb[bi] : qa[p];
    }
    want.insert(want.end(), base.begin(), base.end());
    want.push_back('\n'); want.push_back('+'); want.push_back('\n');
    want.insert(want.end(), qual.begin(), qual.end());
    want.push_back('\n');
    const int64_t len = (int64_t)want.size();
    bool bad = len != mrg_len(P) || L != P.L || want_ov != mrg_overlap(n1, n2, o);

    for (int shift = 0; shift < 16 && !bad; shift++) {
        const int64_t nchunk = (len + shift + 15) >> 4;
        int taken = 0;
        for (int64_t k = 0; k < nchunk; k++) {
            const int64_t clo = 16 * k - shift;
            MrgLoads X;
            Mrg16 y;
            mrg_chunk_load(d1, nb1, d2, nb2, P, clo, X);
            taken += mrg_chunk_build(P, clo, X, y);
            uint8_t got[16];
            memcpy(got, &y, 16);
            for (int i = 0; i < 16; i++) {
                const int64_t t = clo + i;
                if (t < 0 || t >= len) continue;
                if (got[i] != want[(size_t)t]) bad = true;
            }
        }
        if (taken != want_taken) bad = true;
    }
    if (bad) {
        failures++;
        if (failures < 20) printf("FAIL n1=%d n2=%d o=%d h=%d layout=%d\n", n1, n2, o, h, layout);
    }
    free(d1); free(d2);
}

int main()
{
    // the small pieces on their own
    for (int t = 0; t < 200000; t++) {
        const uint32_t x = rnd(), y = t % 3 == 0 ? (x ^ (1u << (rnd() % 32))) : rnd();
        const uint32_t g = mrg_gt4(x, y), c = mrg_comp4(x);
        for (int i = 0; i < 4; i++) {
            const uint8_t xb = (uint8_t)(x >> (8 * i)), yb = (uint8_t)(y >> (8 * i));
            if ((uint8_t)(g >> (8 * i)) != (xb > yb ? 0xFF : 0)) { failures++; if (failures < 20) printf("gt4 %08x %08x\n", x, y); }
            if ((uint8_t)(c >> (8 * i)) != comp(xb)) { failures++; if (failures < 20) printf("comp4 %08x\n", x); }
        }
    }
    {
        const uint32_t x = 0x54476141u, c = mrg_comp4(x);     // "AaGT" -> "TtCA"
        if (c != 0x41437454u) { failures++; printf("comp4 letters %08x\n", c); }
    }
    for (int n1 = 1; n1 <= 40; n1++)
        for (int n2 = 1; n2 <= 40; n2++)
            for (int o = -(n2 - 1); o <= n1 - 1; o++)
                one_case(n1, n2, o, (n1 + 3 * n2 + o + 80) % 19, (n1 + n2 + o + 80) & 3);
    static const int lens[] = {1, 2, 15, 16, 17, 31, 32, 33, 150, 511, 512};
    for (int t = 0; t < 600; t++) {
        const int n1 = t % 3 ? lens[rnd() % 11] : 1 + (int)(rnd() % 512), n2 = t % 5 ? lens[rnd() % 11] : 1 + (int)(rnd() % 512);
        int o = -(n2 - 1) + (int)(rnd() % (uint32_t)(n1 + n2 - 1));
        if (t % 7 == 0) o = n1 - 1;
        if (t % 7 == 1) o = -(n2 - 1);
        if (t % 7 == 2) o = 0;
        one_case(n1, n2, o, t % 11 == 0 ? 5000 : (int)(rnd() % 40), (int)(rnd() & 3));
    }
    printf("%ld cases, %ld failures\n", cases, failures);
    if (failures) return 1;
    printf("ok\n");
    return 0;
}

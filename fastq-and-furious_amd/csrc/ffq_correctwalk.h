// ffq_correctwalk.h -- the byte work of correcting mismatched bases inside the overlap of a pair's mates (csrc/ffq_correct.h,
// ffq_table_pair_correct; include/ffq.h states the rule): sixteen overlap positions at a time, judged in registers.  Inline
// functions that compile for the host too: the kernel calls them, and tests/correct_walk_host.cpp drives the same functions
// on a CPU against a loop over bytes.
//
// The overlap of a pair is the positions p in [lo, hi), lo = max(0, o), hi = min(n1, n2 + o); CHUNK c is [lo + 16 c, + 16) cut
// to hi.  A chunk takes four loads (cor_load16):
//   mate 1   a + p0 and qa + p0, as they stand
//   mate 2   b + (n2 - 16 - p0 + o) and qb + the same: the sixteen bytes that FACE those positions, reversed in registers
// Every load is bounded by its own LINE, not by the buffer: a byte outside [0, n) of the line reads as zero and is not
// touched.  The pass edits bytes, and the bytes beside a line belong to records another group may be rewriting.
// Everything is judged for the sixteen positions at once with byte masks (0xFF per byte, in POSITION order: byte i is p0 + i):
//   match   a and comp(rb) agree without their case bit, and a is a base (then rb is the complementary base: comp maps bases
//           to bases and nothing else onto one) -- the overlap rule's MATCH, N matching nothing
//   fix2    a mismatch with qa >= G, qb <= B and a a base: mate 2's byte becomes comp(a), its quality qa
//   fix1    else a mismatch with qb >= G, qa <= B and rb a base: mate 1's byte becomes comp(rb), its quality qb
// The new bytes of mate 2 are in position order too: byte i goes to b[cor_bi(P, p0 + i)].
#pragma once
#include "ffq_mergewalk.h"

namespace ffq {

// a pair that is looked at: where its four lines begin in their buffers (byte index) and the alignment, -n2 < o < n1
struct CorPair {
    int64_t asrc, qasrc;                          // mate 1's buffer: sequence, quality
    int64_t bsrc, qbsrc;                          // mate 2's buffer
    int32_t n1, n2, o;
};

MRG_HD int cor_lo(const CorPair &P) { return P.o > 0 ? P.o : 0; }
MRG_HD int cor_hi(const CorPair &P) { return P.n1 < P.n2 + P.o ? P.n1 : P.n2 + P.o; }
MRG_HD int cor_nchunk(const CorPair &P) { return (cor_hi(P) - cor_lo(P) + 15) >> 4; }
// the byte of mate 2 that faces position p
MRG_HD int cor_bi(const CorPair &P, int p) { return P.n2 - 1 - (p - P.o); }

// the class of ffq_table_stats: 0 / 1 / 2 / 3 for A a / C c / G g / T t, 4 for every other byte
MRG_HD int cor_cls(uint8_t x)
{
    const uint8_t u = x & 0xDFu;
    return u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : 4;
}

// 0xFF in every byte of x that is a base (either case)
MRG_HD uint32_t cor_base4(uint32_t x)
{
    const uint32_t u = x & 0xDFDFDFDFu;
    const uint32_t m = mrg_zero7(u ^ 0x41414141u) | mrg_zero7(u ^ 0x43434343u) | mrg_zero7(u ^ 0x47474747u) | mrg_zero7(u ^ 0x54545454u);
    return (m >> 7) * 0xFFu;
}

// 0xFF in every byte in which x and y are equal
MRG_HD uint32_t cor_eq4(uint32_t x, uint32_t y) { return (mrg_zero7(x ^ y) >> 7) * 0xFFu; }

// Bytes [a, a + 16) of a LINE of n bytes; those outside [0, n) read as zero and are not touched.  A chunk that sticks out of a
// line of sixteen bytes or more -- the last chunk of nearly every overlap, and mate 2's at the mirrored address -- is ONE load
// of the sixteen bytes at the line's edge, shifted into place in registers: no loop over bytes.  Only a line below sixteen
// bytes takes the merge's byte loop.
MRG_HD Mrg16 cor_load16(const uint8_t *line, int n, int64_t a)
{
    if (a >= 0 && a + 16 <= n) {
        Mrg16 v;
        __builtin_memcpy(&v, line + a, 16);
        return v;
    }
    if (n < 16) return mrg_load16_edge(line, n, a);
    const Mrg16 zero = {0, 0, 0, 0};
    if (a <= -16 || a >= n) return zero;
    uint64_t h[2];
    __builtin_memcpy(h, line + (a < 0 ? 0 : n - 16), 16);
    uint64_t lo = h[0], hi = h[1];
    if (a < 0) {                                   // byte j of the result is byte j + a of the line: up by s = -a bytes, 0 < s < 16
        const int s = (int)-a;
        if (s < 8) { hi = (hi << (8 * s)) | (lo >> (64 - 8 * s)); lo <<= 8 * s; }
        else { hi = lo << (8 * (s - 8)); lo = 0; }
    } else {                                       // the load began s = a - (n - 16) bytes in front of a: down by s bytes, 0 < s < 16
        const int s = (int)(a - (n - 16));
        if (s < 8) { lo = (lo >> (8 * s)) | (hi << (64 - 8 * s)); hi >>= 8 * s; }
        else { lo = hi >> (8 * (s - 8)); hi = 0; }
    }
    Mrg16 v;
    v.x = (uint32_t)lo; v.y = (uint32_t)(lo >> 32); v.z = (uint32_t)hi; v.w = (uint32_t)(hi >> 32);
    return v;
}

struct CorLoads { Mrg16 a, qa, b, qb; };           // as loaded: mate 2's at the mirrored address, not yet reversed

MRG_HD void cor_chunk_load(const uint8_t *d1, const uint8_t *d2, const CorPair &P, int c, CorLoads &X)
{
    const int64_t p0 = cor_lo(P) + 16 * (int64_t)c, m0 = (int64_t)P.n2 - 16 - p0 + P.o;
    X.a = cor_load16(d1 + P.asrc, P.n1, p0); X.qa = cor_load16(d1 + P.qasrc, P.n1, p0);
    X.b = cor_load16(d2 + P.bsrc, P.n2, m0); X.qb = cor_load16(d2 + P.qbsrc, P.n2, m0);
}

// What chunk c does to the pair.  fix1 / fix2: the positions whose byte of mate 1 / mate 2 is rewritten; na, nqa: mate 1's new
// base and quality there; nb, nqb: mate 2's (position order); mism: the chunk's mismatch positions.
struct CorChunk { Mrg16 fix1, fix2, na, nqa, nb, nqb; int mism; };

MRG_HD void cor_word(uint32_t a, uint32_t qa, uint32_t rb, uint32_t rqb, uint32_t in, uint32_t G4, uint32_t B4, uint32_t &f1, uint32_t &f2,
                     uint32_t &ca, uint32_t &crb, uint32_t &mm)
{
    ca = mrg_comp4(a); crb = mrg_comp4(rb);
    const uint32_t baseA = cor_base4(a), baseB = cor_base4(rb);
    const uint32_t match = cor_eq4(a & 0xDFDFDFDFu, crb & 0xDFDFDFDFu) & baseA;
    mm = in & ~match;
    // x >= G: not G > x; x <= B: not x > B
    f2 = mm & ~mrg_gt4(G4, qa) & ~mrg_gt4(rqb, B4) & baseA;
    f1 = mm & ~f2 & ~mrg_gt4(G4, rqb) & ~mrg_gt4(qa, B4) & baseB;
}

// G, B: the two threshold bytes, qual_base + good_quality and qual_base + bad_quality
MRG_HD void cor_chunk_build(const CorPair &P, int c, const CorLoads &X, uint32_t G, uint32_t B, CorChunk &Y)
{
    const int64_t p0 = cor_lo(P) + 16 * (int64_t)c;
    const Mrg16 in = mrg_range(0, mrg_clamp16((int64_t)cor_hi(P) - p0));
    const Mrg16 rb = mrg_rev16(X.b), rqb = mrg_rev16(X.qb);
    const uint32_t G4 = G * 0x01010101u, B4 = B * 0x01010101u;
    Mrg16 mm;
    cor_word(X.a.x, X.qa.x, rb.x, rqb.x, in.x, G4, B4, Y.fix1.x, Y.fix2.x, Y.nb.x, Y.na.x, mm.x);
    cor_word(X.a.y, X.qa.y, rb.y, rqb.y, in.y, G4, B4, Y.fix1.y, Y.fix2.y, Y.nb.y, Y.na.y, mm.y);
    cor_word(X.a.z, X.qa.z, rb.z, rqb.z, in.z, G4, B4, Y.fix1.z, Y.fix2.z, Y.nb.z, Y.na.z, mm.z);
    cor_word(X.a.w, X.qa.w, rb.w, rqb.w, in.w, G4, B4, Y.fix1.w, Y.fix2.w, Y.nb.w, Y.na.w, mm.w);
    Y.nqa = rqb; Y.nqb = X.qa;
    Y.mism = mrg_count(mm);
}

// a byte mask as sixteen bits, bit i for byte i (bit 0 of every byte gathered by a multiplication without carries)
MRG_HD uint32_t cor_bits4(uint32_t m) { return ((m & 0x01010101u) * 0x01020408u) >> 24; }
MRG_HD uint32_t cor_bits16(Mrg16 m) { return cor_bits4(m.x) | (cor_bits4(m.y) << 4) | (cor_bits4(m.z) << 8) | (cor_bits4(m.w) << 12); }

// byte i of sixteen (selects: no array indexed by a variable)
MRG_HD uint8_t cor_byte(Mrg16 v, int i)
{
    const int w = i >> 2;
    const uint32_t x = w == 0 ? v.x : w == 1 ? v.y : w == 2 ? v.z : v.w;
    return (uint8_t)(x >> (8 * (i & 3)));
}

}  // namespace ffq

// ffq_mergewalk.h -- the byte work of merging the two mates of a pair into one read (csrc/ffq_merge.h, ffq_table_pair_merge;
// include/ffq.h states the rule): sixteen bytes of the merged record's text at a time, built in registers.  Inline functions
// that compile for the host too: the kernel calls them, and tests/merge_walk_host.cpp drives the same functions on a CPU against
// a loop over bytes.
//
// The text of a merged pair is  '@' header '\n' base[0 .. L) "\n+\n" qual[0 .. L) '\n'  (len = h + 2 L + 6 bytes).  A CHUNK is
// sixteen of its bytes, [clo, clo + 16) row-relative; clo may be negative and the chunk may reach behind len: those bytes are
// the caller's to leave out.  Under a chunk lie up to three spans with bytes from memory -- header, bases, qualities -- and
// the six literals.  A span of merged positions [p0, p0 + 16) is built from four loads:
//   mate 1   a + p0 and qa + p0, as they stand
//   mate 2   b + (n2 - 16 - p0 + o) and qb + the same: the sixteen bytes that FACE those positions, at the mirrored address,
//            reversed in registers (a byte swap per dword, then the dwords swapped) -- and the bases complemented with byte masks
// and the choice `takeB = inA && inB ? qb > qa : !inA` is made for all sixteen at once: inA / inB are ranges of chunk bytes,
// qb > qa an unsigned compare of every byte of a dword without a carry between bytes.  Bytes outside a mate's line are loaded
// (where the BUFFER has them: mrg_load16 reads nothing outside it, in front of mate 2's first byte in particular) and masked.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MRG_HD __host__ __device__ __forceinline__
#define MRG_EDGE __host__ __device__ __noinline__
#else
#define MRG_HD inline
#define MRG_EDGE inline
#endif

namespace ffq {

constexpr int MRG_MAX_LEN = 512;                  // FFQ_OVERLAP_MAX_LEN

struct Mrg16 { uint32_t x, y, z, w; };            // sixteen bytes in memory order, first byte lowest in x

// a mergeable pair: where its five slices begin in their buffers (byte index), the header's length, and the alignment
struct MrgPair {
    int64_t hsrc, asrc, qasrc;                    // mate 1's buffer: header, sequence, quality
    int64_t bsrc, qbsrc;                          // mate 2's buffer: sequence, quality
    int64_t h;                                    // header bytes
    int32_t n1, n2, o, L;                         // -n2 < o < n1; L = o < 0 ? n2 + o : max(n1, n2 + o)
};

MRG_HD int64_t mrg_len(const MrgPair &P) { return P.h + 2 * (int64_t)P.L + 6; }
MRG_HD int mrg_L(int n1, int n2, int o) { return o < 0 ? n2 + o : (n1 > n2 + o ? n1 : n2 + o); }
// positions at which both mates have a base
MRG_HD int mrg_overlap(int n1, int n2, int o) { return (n1 < n2 + o ? n1 : n2 + o) - (o > 0 ? o : 0); }

MRG_HD int mrg_clamp16(int64_t v) { return v < 0 ? 0 : (v > 16 ? 16 : (int)v); }

// dword w of the 16-byte mask with bytes [0, nb) set
MRG_HD uint32_t mrg_lt(int nb, int w)
{
    const int t = nb - 4 * w;
    return t <= 0 ? 0u : (t >= 4 ? 0xFFFFFFFFu : ((1u << (8 * t)) - 1u));
}

// the mask with chunk bytes [a, b) set (a > b: empty)
MRG_HD Mrg16 mrg_range(int a, int b)
{
    Mrg16 m;
    m.x = mrg_lt(b, 0) & ~mrg_lt(a, 0); m.y = mrg_lt(b, 1) & ~mrg_lt(a, 1);
    m.z = mrg_lt(b, 2) & ~mrg_lt(a, 2); m.w = mrg_lt(b, 3) & ~mrg_lt(a, 3);
    return m;
}

// chunk bytes [a, b) that a span of xl bytes, whose first byte is chunk byte rel, covers
MRG_HD void mrg_span(int64_t rel, int64_t xl, int &a, int &b)
{
    a = mrg_clamp16(rel);
    b = mrg_clamp16(rel + xl);
}

// 16 bytes at buffer offset a that do not all lie inside [0, nbytes): those outside read as zero and are not touched
MRG_EDGE Mrg16 mrg_load16_edge(const uint8_t *d, int64_t nbytes, int64_t a)
{
    // (two 64-bit halves: no array indexed by a variable)
    uint64_t lo = 0, hi = 0;
    const int j0 = mrg_clamp16(-a), j1 = mrg_clamp16(nbytes - a);
    for (int j = j0; j < j1; j++) {
        const uint64_t b = (uint64_t)d[a + j] << (8 * (j & 7));
        if (j < 8) lo |= b; else hi |= b;
    }
    Mrg16 v;
    v.x = (uint32_t)lo; v.y = (uint32_t)(lo >> 32); v.z = (uint32_t)hi; v.w = (uint32_t)(hi >> 32);
    return v;
}

// 16 bytes at buffer offset a; bytes outside [0, nbytes) read as zero and are not touched
MRG_HD Mrg16 mrg_load16(const uint8_t *d, int64_t nbytes, int64_t a)
{
    if (a >= 0 && a + 16 <= nbytes) {
        Mrg16 v;
        __builtin_memcpy(&v, d + a, 16);
        return v;
    }
    return mrg_load16_edge(d, nbytes, a);
}

// the sixteen bytes back to front: a byte permute per dword, then the dwords swapped
MRG_HD Mrg16 mrg_rev16(Mrg16 v)
{
    Mrg16 r;
    r.x = __builtin_bswap32(v.w); r.y = __builtin_bswap32(v.z); r.z = __builtin_bswap32(v.y); r.w = __builtin_bswap32(v.x);
    return r;
}

// bit 7 of every byte of z that is zero (exact: no carry between bytes)
MRG_HD uint32_t mrg_zero7(uint32_t z)
{
    const uint32_t L7 = 0x7F7F7F7Fu;
    return ~(((z & L7) + L7) | z) & 0x80808080u;
}

// four bases complemented: A <-> T (0x41 ^ 0x54 = 0x15), C <-> G (0x43 ^ 0x47 = 0x04), either case; every other byte as it is
MRG_HD uint32_t mrg_comp4(uint32_t x)
{
    const uint32_t u = x & 0xDFDFDFDFu;            // (u == 'A' exactly for 'A' and 'a')
    const uint32_t at = (mrg_zero7(u ^ 0x41414141u) | mrg_zero7(u ^ 0x54545454u)) >> 7;
    const uint32_t cg = (mrg_zero7(u ^ 0x43434343u) | mrg_zero7(u ^ 0x47474747u)) >> 7;
    return x ^ (at * 0x15u) ^ (cg * 0x04u);        // (a 1 per byte times a byte: nothing crosses into the next)
}

MRG_HD Mrg16 mrg_comp16(Mrg16 v)
{
    v.x = mrg_comp4(v.x); v.y = mrg_comp4(v.y); v.z = mrg_comp4(v.z); v.w = mrg_comp4(v.w);
    return v;
}

// 0xFF in every byte in which x > y, both unsigned.  The low seven bits are compared by a subtraction that cannot borrow
// from the byte above ((y | 0x80) - (x & 0x7F) >= 1 per byte; its bit 7 says y7 >= x7), the top bits decide unless equal.
MRG_HD uint32_t mrg_gt4(uint32_t x, uint32_t y)
{
    const uint32_t d = (y | 0x80808080u) - (x & 0x7F7F7F7Fu);
    const uint32_t g = ((x & ~y) | (~(x ^ y) & ~d)) & 0x80808080u;
    return (g >> 7) * 0xFFu;
}

MRG_HD Mrg16 mrg_and(Mrg16 a, Mrg16 b) { a.x &= b.x; a.y &= b.y; a.z &= b.z; a.w &= b.w; return a; }

// m ? x : y, byte by byte
MRG_HD Mrg16 mrg_sel(Mrg16 m, Mrg16 x, Mrg16 y)
{
    Mrg16 r;
    r.x = (x.x & m.x) | (y.x & ~m.x); r.y = (x.y & m.y) | (y.y & ~m.y);
    r.z = (x.z & m.z) | (y.z & ~m.z); r.w = (x.w & m.w) | (y.w & ~m.w);
    return r;
}

MRG_HD int mrg_popc(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(x);
#else
    return __builtin_popcount(x);
#endif
}

// bytes set in a byte mask
MRG_HD int mrg_count(Mrg16 m)
{
    const uint32_t one = 0x01010101u;
    return mrg_popc(m.x & one) + mrg_popc(m.y & one) + mrg_popc(m.z & one) + mrg_popc(m.w & one);
}

// literal byte v at chunk byte k, if the chunk has it
MRG_HD Mrg16 mrg_put(Mrg16 y, int64_t k, uint32_t v)
{
    if (k < 0 || k >= 16) return y;
    const uint32_t sh = 8u * ((uint32_t)k & 3u), val = v << sh, msk = ~(0xFFu << sh);
    const int w = (int)k >> 2;
    if (w == 0) y.x = (y.x & msk) | val;
    if (w == 1) y.y = (y.y & msk) | val;
    if (w == 2) y.z = (y.z & msk) | val;
    if (w == 3) y.w = (y.w & msk) | val;
    return y;
}

// what a chunk takes from memory: the header's bytes; for the bases under it mate 1's bases and qualities and the bytes of
// mate 2 that face them; for the qualities under it the two quality loads again, at THEIR positions
struct MrgLoads { Mrg16 h, sa, sqa, sb, sqb, qa, qb; };

// where in the text the spans begin: '@' 0, header 1, '\n' o_s - 1, bases o_s, "\n+\n" o_p, qualities o_q, '\n' len - 1
MRG_HD int64_t mrg_os(const MrgPair &P) { return 2 + P.h; }
MRG_HD int64_t mrg_op(const MrgPair &P) { return 2 + P.h + P.L; }
MRG_HD int64_t mrg_oq(const MrgPair &P) { return 5 + P.h + P.L; }

// every load of the chunk at clo (d1 / nb1, d2 / nb2: the two buffers); a span without a byte under the chunk loads nothing
MRG_HD void mrg_chunk_load(const uint8_t *d1, int64_t nb1, const uint8_t *d2, int64_t nb2, const MrgPair &P, int64_t clo, MrgLoads &X)
{
    const Mrg16 zero = {0, 0, 0, 0};
    X.h = X.sa = X.sqa = X.sb = X.sqb = X.qa = X.qb = zero;
    int a, b;
    mrg_span(1 - clo, P.h, a, b);
    if (b > a) X.h = mrg_load16(d1, nb1, P.hsrc + (clo - 1));
    mrg_span(mrg_os(P) - clo, P.L, a, b);
    if (b > a) {
        const int64_t p0 = clo - mrg_os(P), m0 = (int64_t)P.n2 - 16 - p0 + P.o;
        X.sa = mrg_load16(d1, nb1, P.asrc + p0); X.sqa = mrg_load16(d1, nb1, P.qasrc + p0);
        X.sb = mrg_load16(d2, nb2, P.bsrc + m0); X.sqb = mrg_load16(d2, nb2, P.qbsrc + m0);
    }
    mrg_span(mrg_oq(P) - clo, P.L, a, b);
    if (b > a) {
        const int64_t p0 = clo - mrg_oq(P), m0 = (int64_t)P.n2 - 16 - p0 + P.o;
        X.qa = mrg_load16(d1, nb1, P.qasrc + p0);
        X.qb = mrg_load16(d2, nb2, P.qbsrc + m0);
    }
}

// The merged positions [p0, p0 + 16): who is taken.  xqa: mate 1's qualities there; xqb: mate 2's as loaded (mirrored address).
// takeB: the bytes that come from mate 2; both: the overlap's bytes that do (a subset: inA && inB && qb > qa); rqb: xqb reversed.
MRG_HD void mrg_choose(const MrgPair &P, int64_t p0, Mrg16 xqa, Mrg16 xqb, Mrg16 &takeB, Mrg16 &both, Mrg16 &rqb)
{
    rqb = mrg_rev16(xqb);
    const Mrg16 inA = mrg_range(mrg_clamp16(-p0), mrg_clamp16((int64_t)P.n1 - p0));
    const Mrg16 inB = mrg_range(mrg_clamp16((int64_t)P.o - p0), mrg_clamp16((int64_t)P.o + P.n2 - p0));
    Mrg16 gt;
    gt.x = mrg_gt4(rqb.x, xqa.x); gt.y = mrg_gt4(rqb.y, xqa.y); gt.z = mrg_gt4(rqb.z, xqa.z); gt.w = mrg_gt4(rqb.w, xqa.w);
    both = mrg_and(mrg_and(inA, inB), gt);
    // inB && (!inA || qb > qa)
    takeB.x = inB.x & (~inA.x | gt.x); takeB.y = inB.y & (~inA.y | gt.y); takeB.z = inB.z & (~inA.z | gt.z); takeB.w = inB.w & (~inA.w | gt.w);
}

// The chunk at clo from its loads; bytes outside [0, len) of the text are unspecified.  Returns how many positions of the
// overlap, among the QUALITY bytes of this chunk, were taken from mate 2 (every position is some chunk's: the sum over a
// record's chunks is counts[5]'s share of the pair).
MRG_HD int mrg_chunk_build(const MrgPair &P, int64_t clo, const MrgLoads &X, Mrg16 &out)
{
    Mrg16 y = {0, 0, 0, 0};
    int a, b, taken = 0;
    mrg_span(1 - clo, P.h, a, b);
    if (b > a) y = mrg_sel(mrg_range(a, b), X.h, y);
    mrg_span(mrg_os(P) - clo, P.L, a, b);
    if (b > a) {
        Mrg16 takeB, both, rqb;
        mrg_choose(P, clo - mrg_os(P), X.sqa, X.sqb, takeB, both, rqb);
        const Mrg16 v = mrg_sel(takeB, mrg_comp16(mrg_rev16(X.sb)), X.sa);
        y = mrg_sel(mrg_range(a, b), v, y);
    }
    mrg_span(mrg_oq(P) - clo, P.L, a, b);
    if (b > a) {
        Mrg16 takeB, both, rqb;
        mrg_choose(P, clo - mrg_oq(P), X.qa, X.qb, takeB, both, rqb);
        const Mrg16 v = mrg_sel(takeB, rqb, X.qa);
        y = mrg_sel(mrg_range(a, b), v, y);
        taken = mrg_count(mrg_and(both, mrg_range(a, b)));
    }
    const int64_t len = mrg_len(P);
    y = mrg_put(y, 0 - clo, '@');
    y = mrg_put(y, mrg_os(P) - 1 - clo, '\n');
    y = mrg_put(y, mrg_op(P) - clo, '\n');
    y = mrg_put(y, mrg_op(P) + 1 - clo, '+');
    y = mrg_put(y, mrg_op(P) + 2 - clo, '\n');
    y = mrg_put(y, len - 1 - clo, '\n');
    out = y;
    return taken;
}

}  // namespace ffq

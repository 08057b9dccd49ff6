// ffq_polywalk.h -- what ONE LANE does with its bytes in the poly-tail walk (csrc/ffq_poly.h, ffq_table_trim_poly; include/ffq.h
// states the rule), and what its group does with a chunk once the lanes' results are reduced.  Nothing here has a ballot or a
// DPP move in it: inline functions that compile for the host too.  The kernels call them, and tests/poly_walk_host.cpp drives
// the same functions on a CPU, a group lane by lane, against the rule's loop over bytes.
//
// The walk goes from the 3' end in CHUNKS of C = G * B walk positions, B consecutive ones per lane.  Per base b the rule keeps
// mm[b], the positions so far that are not b.  The four counts live in ONE packed word, a field each (PolyPack<C>: four 8-bit
// fields in 32 bits for the chunk of 64, four 16-bit fields in 64 bits for the chunk of 1024), so that the sum of a lane's
// mismatch indicators, the prefix sum over the lanes and the carry from chunk to chunk are one addition each for all four
// bases.  A count that has passed 5 can never pass `allowed` again (allowed(i) <= 5): the base is DEAD for good, and the
// carried counts saturate at POLY_DEAD.  A base outside the set S the caller asked for starts dead; that is all S is.
//
// A chunk, for its group:
//   1. every lane: poly_classify (classes and hit nibbles of its B bytes), poly_lane_sum (its packed indicator sums)
//   2. the group:  an inclusive prefix sum of the lanes' sums; start = carried + (inclusive - own)
//   3. every lane: poly_lane_walk from `start`: its first stopping position, the counts in front of it
//   4. the group:  the FIRST stopping position of the chunk (a maximum of poly_stop_key), the counts in front of that
//                  position -- or, without a stop, at the chunk's last position -- from the lane poly_end_lane names, and per
//                  base the deepest exact hit in front of the stop (a maximum of poly_hit_key)
//   5. the group:  poly_chunk_end: the row's new length if the walk ends here, the carried state if it goes on
// After a full chunk of 64 or more positions at most one base is alive (two bases mismatch each other everywhere, so their
// counts sum to the position), which is why ONE carried `last` is enough: it belongs to the base that is still alive.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define POLY_HD __host__ __device__ __forceinline__
#else
#define POLY_HD inline
#endif

namespace ffq {

constexpr int POLY_ANY = -1;          // FFQ_POLY_ANY
constexpr int POLY_DEAD = 6;          // a count that has passed 5
constexpr int POLY_MIN_LEN_LO = 2, POLY_MIN_LEN_HI = 65535;

// class of a base: A a / C c / G g / T t = 0..3, any other byte (and -1, no byte) 4
POLY_HD int poly_cls(int byte)
{
    const int u = byte & 0xDF;
    if (byte < 0) return 4;
    return u == 0x41 ? 0 : u == 0x43 ? 1 : u == 0x47 ? 2 : u == 0x54 ? 3 : 4;
}

// mismatches the rule allows among walk positions 0 .. i (ic: i, or anything >= 40 in its place)
POLY_HD int poly_allowed(int ic)
{
    const int a = (ic + 1) >> 3;
    return a < 5 ? a : 5;
}

// the four counts of a chunk of C positions, packed
template <int C> struct PolyPack;
template <> struct PolyPack<64> { typedef uint32_t T; static constexpr int FB = 8; };
template <> struct PolyPack<1024> { typedef uint64_t T; static constexpr int FB = 16; };

template <int C> struct PolyOps {
    typedef typename PolyPack<C>::T T;
    static constexpr int FB = PolyPack<C>::FB;
    static constexpr T FIELD = ((T)1 << FB) - 1;
    static constexpr T ONES = (T)1 | ((T)1 << FB) | ((T)1 << (2 * FB)) | ((T)1 << (3 * FB));
    static constexpr T TOPS = ONES << (FB - 1);
    // a field holds at most POLY_DEAD + C, and all_above adds up to 2^(FB-1) - 1 to it
    static_assert(POLY_DEAD + C + (1 << (FB - 1)) - 1 <= (1 << FB) - 1, "a field of the packed counts overflows");

    static POLY_HD int field(T x, int b) { return (int)((x >> (FB * b)) & FIELD); }
    // one position of class k: a mismatch for every base but k
    static POLY_HD T step(int k) { return ONES - (k < 4 ? (T)1 << (FB * (k & 3)) : (T)0); }
    // every field of x is above a (0 <= a <= 5): the top bit of field + (2^(FB-1) - 1 - a) is set iff field > a
    static POLY_HD bool all_above(T x, int a) { return ((x + ONES * (T)((1 << (FB - 1)) - 1 - a)) & TOPS) == TOPS; }
    // every field min(field, POLY_DEAD)
    static POLY_HD T saturate(T x)
    {
        T r = 0;
        for (int b = 0; b < 4; b++) {
            const int f = field(x, b);
            r |= (T)(f < POLY_DEAD ? f : POLY_DEAD) << (FB * b);
        }
        return r;
    }
    // the counts a walk begins with: 0 for the bases of S (base 0..3, or POLY_ANY for all four), dead for the others
    static POLY_HD T begin(int base)
    {
        T r = 0;
        for (int b = 0; b < 4; b++)
            if (base != POLY_ANY && b != base) r |= (T)POLY_DEAD << (FB * b);
        return r;
    }
    static POLY_HD bool any_alive(T x)
    {
        bool a = false;
        for (int b = 0; b < 4; b++) a |= field(x, b) < POLY_DEAD;
        return a;
    }
};

// a nibble per position of a lane, bit b of nibble j set where position j is an exact b
template <int B> struct PolyHits;
template <> struct PolyHits<8> { typedef uint32_t T; static constexpr T EACH = 0x11111111u; };
template <> struct PolyHits<16> { typedef uint64_t T; static constexpr T EACH = 0x1111111111111111ull; };

// qv: the lane's B bytes in ascending ADDRESS order, -1 where there is none (the low indices: the walk goes backwards).
// k: their classes in WALK order, hits: the nibbles; returns whether one of the bytes is '\n'.
template <int B>
POLY_HD bool poly_classify(const int (&qv)[B], int (&k)[B], typename PolyHits<B>::T &hits)
{
    typedef typename PolyHits<B>::T H;
    bool nl = false;
    hits = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < B; j++) {
        const int x = qv[B - 1 - j];
        nl |= x == 10;
        k[j] = poly_cls(x);
        hits |= (H)((1u << k[j]) & 0xFu) << (4 * j);
    }
    return nl;
}

// the packed indicator sums of the lane's first `avail` positions
template <int C, int B>
POLY_HD typename PolyPack<C>::T poly_lane_sum(const int (&k)[B], int avail)
{
    typename PolyPack<C>::T t = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < B; j++)
        if (j < avail) t += PolyOps<C>::step(k[j]);
    return t;
}

// The lane steps through its positions i0 .. i0 + avail - 1 from the counts `start` in front of them.  stop_j: its first
// stopping position, B if it has none; at: the counts in front of that position -- without a stop, behind its last one.
template <int C, int B>
POLY_HD void poly_lane_walk(const int (&k)[B], int avail, int64_t i0, int min_len, typename PolyPack<C>::T start, int &stop_j,
                            typename PolyPack<C>::T &at)
{
    typedef PolyOps<C> P;
    // (positions as 32 bits: beyond 2^20 nothing depends on them any more, min_len is at most 65535 and allowed is 5 from 39 on)
    const int ic = (int)(i0 < ((int64_t)1 << 20) ? i0 : ((int64_t)1 << 20));
    typename P::T r = start;
    stop_j = B;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < B; j++) {
        if (j < avail && stop_j == B) {
            const typename P::T t = r + P::step(k[j]);
            if (ic + j >= min_len - 1 && P::all_above(t, poly_allowed(ic + j))) stop_j = j;
            else r = t;
        }
    }
    at = r;
}

// what the group takes maxima of: C - (the lane's first stopping position in the chunk), 0 if it has none ...
template <int C, int B>
POLY_HD int poly_stop_key(int gl, int stop_j) { return stop_j < B ? C - (gl * B + stop_j) : 0; }

// ... and 1 + (the lane's deepest exact b among its first `upto` positions, as a position of the chunk), 0 if it has none
template <int B>
POLY_HD int poly_hit_key(typename PolyHits<B>::T hits, int b, int upto, int gl)
{
    typedef typename PolyHits<B>::T H;
    H m = (hits >> b) & PolyHits<B>::EACH;
    if (upto < B) m &= ((H)1 << (4 * (upto < 0 ? 0 : upto))) - 1;
    if (!m) return 0;
    int top = 0;                                       // the highest set bit
#if defined(__HIP_DEVICE_COMPILE__)
    top = sizeof(H) == 8 ? 63 - __clzll((long long)m) : 31 - __clz((int)m);
#else
    top = 63 - __builtin_clzll((unsigned long long)m);
#endif
    return gl * B + (top >> 2) + 1;
}

// the lane whose `at` the group needs: the one that stopped first (skey: the maximum of poly_stop_key) or, without a stop, the
// one that holds the chunk's last position -- the row's last if it ends in this chunk (w0: the chunk's first position)
template <int C, int B>
POLY_HD int poly_end_lane(int skey, int64_t w0, int64_t n)
{
    if (skey > 0) return (C - skey) / B;
    return n - w0 < C ? (int)((n - 1 - w0) / B) : C / B - 1;
}

// how many of its positions a lane looks for exact hits in: those in front of the chunk's first stop
template <int C, int B>
POLY_HD int poly_hit_upto(int skey, int gl, int avail)
{
    if (skey <= 0) return avail;
    const int upto = (C - skey) - gl * B;
    return upto < 0 ? 0 : upto < avail ? upto : avail;
}

// what a group carries from chunk to chunk
template <int C> struct PolyState {
    typename PolyPack<C>::T mm;       // the counts in front of position w0, saturated
    int64_t last;                     // the deepest exact hit so far of the base that is still alive, -1: none
    int64_t w0;                       // the next chunk's first position
};

// The end of a chunk.  skey: the maximum of the lanes' stop keys; at: the end lane's counts; g[b]: the maximum of the lanes' hit
// keys of base b.  The walk ends in this chunk if it stopped or the row has no more positions: then *newlen is the row's new
// length (n: unchanged) and false is returned.  Otherwise the state is moved on; it is also over, unchanged, when no base is
// alive any more (the stop that is still to come can then only leave the row as it is).
template <int C>
POLY_HD bool poly_chunk_end(PolyState<C> &s, int64_t n, int min_len, int skey, typename PolyPack<C>::T at, const int (&g)[4],
                            int64_t *newlen)
{
    typedef PolyOps<C> P;
    *newlen = n;
    if (skey > 0 || n - s.w0 <= C) {
        const int64_t stop = skey > 0 ? s.w0 + (C - skey) : n;
        if (stop < min_len) return false;
        const int a = poly_allowed((int)(stop - 1 < 64 ? stop - 1 : 64));
        for (int b = 0; b < 4; b++)                     // (one base passes at stop - 1, include/ffq.h says why)
            if (P::field(at, b) <= a) *newlen = n - 1 - (g[b] > 0 ? s.w0 + g[b] - 1 : s.last);
        return false;
    }
    for (int b = 0; b < 4; b++)
        if (P::field(at, b) < POLY_DEAD && g[b] > 0) s.last = s.w0 + g[b] - 1;
    s.mm = P::saturate(at);
    s.w0 += C;
    return P::any_alive(s.mm);
}

}  // namespace ffq

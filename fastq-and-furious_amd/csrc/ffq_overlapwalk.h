// ffq_overlapwalk.h -- the word work of the overlap analysis between the mates of a pair (csrc/ffq_overlap.h,
// ffq_table_pair_overlap; include/ffq.h states the rule): packing a mate into two bits per base, and counting the mismatches
// of one candidate alignment sixteen positions at a time.  Inline functions that compile for the host too: the kernel calls
// them, and tests/overlap_pack_host.cpp drives the same functions on a CPU against a loop over bytes.
//
// A PLANE is OVL_PLANE dwords: a zero dword, OVL_WORDS dwords of sixteen positions each, a zero dword -- so that the funnel
// shift of a candidate may take the dword in front of the first and the one behind the last.  A mate has two planes:
//   code   two bits per position, position p at bits 2 (p & 15) of word p >> 4.  The code of a base is (byte >> 1) & 3:
//          A a = 0, C c = 1, T t = 2, G g = 3 -- a bijection whose complement is `code ^ 2`; only equality is ever asked for
//   bad    bit 2 (p & 15) set where the byte is none of the eight (class 4 of include/ffq.h) or lies behind the mate's end
// Mate 1 is packed as it stands (ovl_pack_fwd), mate 2 reversed and complemented (ovl_pack_rc): word W of rb holds
// b[n2 - 16 W - 16 .. n2 - 16 W) back to front.
// A candidate o compares a[i] with rb[i - o] for i in [lo, hi): per word of a, the sixteen positions of rb that face it are
// brought to the word's frame with a funnel shift by 2 ((16 w - o) & 15) bits out of two neighbouring dwords, the codes are
// XORed and the bit pairs folded to one bit, both `bad` planes ORed in, the positions outside [lo, hi) masked off, and the
// set bits counted.  The count stops as soon as it exceeds `limit`: only mm <= limit is observable.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OVL_HD __host__ __device__ __forceinline__
#else
#define OVL_HD inline
#endif

namespace ffq {

constexpr int OVL_MAX_LEN = 512;                  // FFQ_OVERLAP_MAX_LEN
constexpr int OVL_WORDS = OVL_MAX_LEN / 16;       // dwords of a plane that hold positions
constexpr int OVL_PLANE = OVL_WORDS + 2;          // ... and a zero dword at either end
constexpr uint32_t OVL_EVEN = 0x55555555u;

OVL_HD int ovl_imin(int a, int b) { return a < b ? a : b; }
OVL_HD int ovl_imax(int a, int b) { return a > b ? a : b; }

// seq[a .. a + 16) as four dwords in memory order, zero where the byte lies outside seq[0 .. n); no byte outside is read
OVL_HD void ovl_load16(const uint8_t *seq, int a, int n, uint32_t (&x)[4])
{
    x[0] = x[1] = x[2] = x[3] = 0;
    if (a >= 0 && a + 16 <= n) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int w = 0; w < 4; w++) __builtin_memcpy(&x[w], seq + a + 4 * w, 4);
        return;
    }
    // (two 64-bit halves: no array indexed by a variable)
    const int j0 = ovl_imax(0, -a), j1 = ovl_imin(16, n - a);
    uint64_t lo = 0, hi = 0;
    for (int j = j0; j < j1; j++) {
        const uint64_t b = (uint64_t)seq[a + j] << (8 * (j & 7));
        if (j < 8) lo |= b; else hi |= b;
    }
    x[0] = (uint32_t)lo; x[1] = (uint32_t)(lo >> 32); x[2] = (uint32_t)hi; x[3] = (uint32_t)(hi >> 32);
}

// four bytes: their codes in bits 0..7 of `code`, bit 2 k of `bad` set where byte k is no base
OVL_HD void ovl_pack4(uint32_t x, uint32_t &code, uint32_t &bad)
{
    const uint32_t u = x & 0xDFDFDFDFu, L7 = 0x7F7F7F7Fu;
    const uint32_t za = u ^ 0x41414141u, zc = u ^ 0x43434343u, zg = u ^ 0x47474747u, zt = u ^ 0x54545454u;
    // bit 7 of a byte: it is non-zero (exact, no carry between bytes)
    const uint32_t na = ((za & L7) + L7) | za, nc = ((zc & L7) + L7) | zc, ng = ((zg & L7) + L7) | zg, nt = ((zt & L7) + L7) | zt;
    uint32_t v = ((na & nc & ng & nt) >> 7) & 0x01010101u;       // bits 0, 8, 16, 24
    v |= v >> 6;                                                  // bits 0, 2 and 16, 18
    bad = (v & 0x5u) | ((v >> 12) & 0x50u);
    uint32_t t = (u >> 1) & 0x03030303u;
    t |= t >> 6;
    code = (t & 0xFu) | ((t >> 12) & 0xF0u);
}

// sixteen bytes in memory order -> a word of codes and a word of `bad` bits, first byte lowest
OVL_HD void ovl_pack16(const uint32_t (&x)[4], uint32_t &code, uint32_t &bad)
{
    code = bad = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int w = 0; w < 4; w++) {
        uint32_t c, b;
        ovl_pack4(x[w], c, b);
        code |= c << (8 * w);
        bad |= b << (8 * w);
    }
}

OVL_HD uint32_t ovl_bitrev(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bitreverse32(x);
#else
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
    return (x >> 16) | (x << 16);
#endif
}

// word W of mate 1: a[16 W .. 16 W + 16); x: the bytes as they were loaded (for the caller's newline check)
OVL_HD void ovl_pack_fwd(const uint8_t *a, int n, int W, uint32_t &code, uint32_t &bad, uint32_t (&x)[4])
{
    ovl_load16(a, 16 * W, n, x);
    ovl_pack16(x, code, bad);
}

// word W of rb: b[n - 16 W - 16 .. n - 16 W) back to front, complemented
OVL_HD void ovl_pack_rc(const uint8_t *b, int n, int W, uint32_t &code, uint32_t &bad, uint32_t (&x)[4])
{
    ovl_load16(b, n - 16 * W - 16, n, x);
    uint32_t c, m;
    ovl_pack16(x, c, m);
    const uint32_t r = ovl_bitrev(c);                            // the pairs in reverse order, each pair's two bits swapped
    code = (((r >> 1) & OVL_EVEN) | ((r & OVL_EVEN) << 1)) ^ 0xAAAAAAAAu;
    bad = ovl_bitrev(m) >> 1;
}

// (hi : lo) >> sh, sh in 0..31: v_alignbit_b32
OVL_HD uint32_t ovl_funnel(uint32_t hi, uint32_t lo, int sh)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)sh);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
#endif
}

// the candidates of a pair: 0 .. n1 - mo, then -1 .. -(n2 - mo); none if a mate is shorter than mo
OVL_HD int ovl_ncand(int n1, int n2, int mo) { return (n1 < mo || n2 < mo) ? 0 : (n1 - mo + 1) + (n2 - mo); }
OVL_HD int ovl_cand(int c, int n1, int mo) { return c <= n1 - mo ? c : -(c - (n1 - mo)); }

// what a candidate may differ in
OVL_HD int ovl_limit(int ov, int max_diff, int diff_permille) { return ovl_imin(max_diff, (ov * diff_permille) / 1000); }

// Mismatches of candidate o, counted up to the first word behind which they exceed `limit`.  ac, ab: mate 1's planes; rc,
// rbad: rb's.  Planes begin with their zero dword (position p lives in plane[1 + (p >> 4)]).  lo < hi.
OVL_HD int ovl_count(const uint32_t *ac, const uint32_t *ab, const uint32_t *rc, const uint32_t *rbad, int o, int lo, int hi, int limit)
{
    const int w0 = lo >> 4, w1 = (hi - 1) >> 4;
    const int s = 16 * w0 - o;                    // rb's position facing the first position of word w0; >= -15
    int q = (s >> 4) + 1;                         // its dword in the plane (arithmetic shift: floor)
    const int sh = 2 * (s & 15);
    uint32_t cl = rc[q], bl = rbad[q];
    int mm = 0;
    for (int w = w0; w <= w1; w++) {
        q++;
        const uint32_t ch = rc[q], bh = rbad[q];
        const uint32_t x = ac[w + 1] ^ ovl_funnel(ch, cl, sh);
        uint32_t d = ((x | (x >> 1)) & OVL_EVEN) | ab[w + 1] | ovl_funnel(bh, bl, sh);
        uint32_t m = OVL_EVEN;
        if (16 * w < lo) m &= ~((1u << (2 * (lo - 16 * w))) - 1u);
        if (16 * w + 16 > hi) m &= (1u << (2 * (hi - 16 * w))) - 1u;
        d &= m;
#if defined(__HIP_DEVICE_COMPILE__)
        mm += __popc(d);
#else
        mm += __builtin_popcount(d);
#endif
        if (mm > limit) break;
        cl = ch; bl = bh;
    }
    return mm;
}

}  // namespace ffq

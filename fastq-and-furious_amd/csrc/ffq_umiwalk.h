// ffq_umiwalk.h -- what ONE LANE does with its bytes when a UMI is taken off a read and put into its name (csrc/ffq_umi.h:
// ffq_table_take_umi, ffq_table_render_fastq_umi; include/ffq.h states the rule).  Nothing here has a ballot or a DPP move in it:
// inline functions that compile for the host too.  The kernels call them, and tests/umi_walk_host.cpp drives the same functions
// on a CPU against loops over bytes.
//
//   umi_blank16, umi_nl16   sixteen bytes as four little-endian dwords: the first ' ' or '\t', and whether there is a '\n',
//                           among the first `nvalid` of them
//   umi_cut                 the bases the take removes from a read of n
//   umi_carrier_pos         whether a source row's positions let it carry a tag (the newline look is the caller's)
//   umi_layout              where the pieces of a tagged row lie, row-relative:
//                               '@' | header head h[:k] | literal: delim, prefix, '_' | tag 1 | '_' | tag 2 | header tail h[k:] |
//                               '\n' | sequence | "\n+\n" | quality | '\n'
//   umi_span                the bytes [a, b) of a 16-byte chunk that a piece covers
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define UMI_HD __host__ __device__ __forceinline__
#else
#define UMI_HD inline
#endif

namespace ffq {

constexpr int UMI_READ1 = 1, UMI_READ2 = 2, UMI_PER_READ = 3;             // FFQ_UMI_*
constexpr int UMI_LEN_MAX = 64, UMI_SKIP_MAX = 64, UMI_PREFIX_MAX = 16;
constexpr int UMI_LIT_MAX = UMI_PREFIX_MAX + 2;                           // delim, prefix, '_'

// 0x80 in every byte of v that is zero, exactly (no carry runs from one byte into the next)
UMI_HD uint32_t umi_zero_bytes(uint32_t v) { return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu); }

// the low t bytes of a dword
UMI_HD uint32_t umi_low_bytes(int t) { return t <= 0 ? 0u : (t >= 4 ? 0xFFFFFFFFu : ((1u << (8 * t)) - 1u)); }

// index of the first ' ' or '\t' among bytes [0, nvalid) of the sixteen; 16: none
UMI_HD int umi_blank16(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int nvalid)
{
    const uint32_t w[4] = {w0, w1, w2, w3};
    int at = 16;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 3; j >= 0; j--) {
        const uint32_t m = umi_zero_bytes(w[j] ^ 0x20202020u) | umi_zero_bytes(w[j] ^ 0x09090909u);
        if (m) at = 4 * j + (__builtin_ctz(m) >> 3);
    }
    return at < nvalid ? at : 16;
}

// a '\n' among bytes [0, nvalid) of the sixteen
UMI_HD bool umi_nl16(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int nvalid)
{
    const uint32_t w[4] = {w0, w1, w2, w3};
    uint32_t m = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 4; j++) m |= umi_zero_bytes(w[j] ^ 0x0A0A0A0Au) & umi_low_bytes(nvalid - 4 * j);
    return m != 0;
}

// bases the take removes from an eligible read of n: the tag and what is dropped behind it, or nothing from a read that is
// shorter than the tag
UMI_HD int64_t umi_cut(int64_t n, int len, int skip)
{
    if (n < len) return 0;
    const int64_t c = (int64_t)len + skip;
    return c < n ? c : n;
}

// A source row carries a tag of `len` bytes as far as its positions say: c1 = pos1 - add, c2 = pos2 - add, L = the buffer's
// coordinates (bytes + sentinel).  The tag is [c1 + 1, c1 + 1 + len): it begins behind coordinate 0, which a sentinel makes
// virtual.  (Written without a sum that a wild position could overflow.)
UMI_HD bool umi_carrier_pos(int64_t c1, int64_t c2, int64_t L, int len)
{
    return c1 >= 0 && c2 >= 0 && c2 - c1 >= 1 + (int64_t)len && c1 <= L - 1 - (int64_t)len;
}

// bytes of the insert: delim, prefix and '_' if there is a prefix, the tag or tags, '_' between two
UMI_HD int umi_lit_len(int prefix_len) { return 1 + (prefix_len ? prefix_len + 1 : 0); }
UMI_HD int umi_ins_len(int loc, int len, int prefix_len)
{
    return umi_lit_len(prefix_len) + (loc == UMI_PER_READ ? 2 * len + 1 : len);
}

// the literal's bytes into lit[0 .. UMI_LIT_MAX); their number
UMI_HD int umi_literal(uint8_t *lit, uint8_t delim, const uint8_t *prefix, int prefix_len)
{
    int n = 0;
    lit[n++] = delim;
    if (prefix_len) {
        for (int j = 0; j < prefix_len; j++) lit[n++] = prefix[j];
        lit[n++] = (uint8_t)'_';
    }
    return n;
}

// row-relative places of a tagged row's pieces (h, s, q: bytes of header, sequence, quality; k: the header's first blank, h if none)
struct UmiLayout {
    int64_t o_lit, o_t1, o_t2, o_tail, o_s, o_p, o_q, len;   // literal, tags, header tail, sequence, "\n+\n", quality; the row's bytes
    int lit_n, t1_n, t2_n;                                   // bytes of the literal and of the tags (0: the location has none)
    int64_t tail_n;                                          // h - k
};

UMI_HD UmiLayout umi_layout(int64_t h, int64_t k, int64_t s, int64_t q, int loc, int len, int prefix_len)
{
    UmiLayout y;
    y.lit_n = umi_lit_len(prefix_len);
    y.t1_n = loc != UMI_READ2 ? len : 0;
    y.t2_n = loc != UMI_READ1 ? len : 0;
    y.tail_n = h - k;
    y.o_lit = 1 + k;
    y.o_t1 = y.o_lit + y.lit_n;
    y.o_t2 = y.o_t1 + y.t1_n + (loc == UMI_PER_READ ? 1 : 0);
    y.o_tail = y.o_t2 + y.t2_n;
    y.o_s = y.o_tail + y.tail_n + 1;
    y.o_p = y.o_s + s;
    y.o_q = y.o_p + 3;
    y.len = y.o_q + q + 1;
    return y;
}

// chunk bytes [a, b) that a piece of xl bytes, whose first byte is chunk byte rel, covers (b <= a: none)
UMI_HD void umi_span(int64_t rel, int64_t xl, int &a, int &b)
{
    const int64_t lo = rel < 0 ? 0 : (rel > 16 ? 16 : rel), e = rel + xl, hi = e < 0 ? 0 : (e > 16 ? 16 : e);
    a = (int)lo; b = (int)hi;
}

}  // namespace ffq

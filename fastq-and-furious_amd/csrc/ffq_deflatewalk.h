// ffq_deflatewalk.h -- the parts of the BGZF deflate (csrc/ffq_deflate.h, ffq_deflate_bgzf; include/ffq.h states the container,
// the bound and the match rule) that have no device in them: inline functions that compile for the host too.  The kernel calls
// them, and tests/deflate_walk_host.cpp drives the same functions on a CPU, a workgroup lane by lane, and hands what they
// build to zlib.
//
// A BLOCK of at most DFL_BLOCK bytes becomes one gzip member.  Its workgroup of DFL_LANES lanes goes through it like this:
//   1. MATCH CANDIDATES, in rounds of DFL_ROUND positions.  Every position p of a round with four bytes behind it looks up
//      table[dfl_hash(its four bytes)]: the most recent position of an EARLIER round with that hash (dfl_candidate: refused
//      when it is farther than DFL_MAX_DIST), and leaves the distance in slot[p].  After a barrier the round's positions are
//      entered, a maximum per table entry.  Lookup before insert with a barrier between is what makes the result the same
//      on every run.
//   2. THE WALK, dfl_walk: the block is cut into segments of DFL_SEG bytes, one lane each.  A lane goes through its segment
//      greedily: at p it measures the candidate of slot[p] and the candidate at distance 1 (runs, which the rounds cannot
//      see), takes the longer if that has DFL_MIN_MATCH bytes or more, else the literal.  A match never crosses the end of
//      its segment.  The lane's TOKENS go into the slots of its own segment, in place: token k into slot[begin + k], which
//      lies at or in front of the position the lane has just read, as every token takes a byte or more.
//   3. COUNTS of the tokens' symbols (dfl_token_syms), then the code lengths of the two alphabets: dfl_rank -- a symbol's
//      place among the used ones by (count, symbol), a lane per symbol --, and dfl_lengths, ONE lane per alphabet: the
//      in-place minimum-redundancy lengths of Moffat and Katajainen over the sorted counts, cut to the limit level by
//      level, handed out along the sorted order.  dfl_codes: canonical codes, bit-reversed as deflate packs them.
//   4. THE HEADER's own code over the lengths (no run-length symbols: at most about 280 bytes per block), dfl_header_plan.
//   5. SIZES: a lane's bits (dfl_token_bits), their prefix sum; stored or dynamic, dfl_stored.
//   6. EMIT: every lane packs its bits from its own bit offset, DflBits: whole words plainly, the word it shares with a
//      neighbour by an OR into zeroed memory.
// The CRC-32 of the block is the XOR of the lanes' CRCs, each multiplied by x^(8 * bytes behind it) mod P (dfl_crc_shift).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DFL_HD __host__ __device__ __forceinline__
#else
#define DFL_HD inline
#endif

namespace ffq {

constexpr int DFL_BLOCK = 65280;              // FFQ_BGZF_BLOCK_BYTES: what bgzip puts into a member
constexpr int DFL_SEG = 256;                  // bytes of a lane's segment
constexpr int DFL_LANES = 256;                // lanes of a block's workgroup; DFL_BLOCK / DFL_SEG = 255 of them have a segment
constexpr int DFL_ROUND = 1024;               // positions of a round
constexpr int DFL_HASH_BITS = 14;
constexpr int DFL_MIN_MATCH = 4, DFL_MAX_MATCH = 258, DFL_MAX_DIST = 32768;
constexpr int DFL_NLIT = 286, DFL_NDIST = 30, DFL_NCL = 19;       // the three alphabets (the header's without 16, 17, 18 in use)
constexpr int DFL_LIT_BITS = 15, DFL_CL_BITS = 7;
constexpr int DFL_EOB = 256;
constexpr int DFL_HEAD = 18, DFL_TAIL = 8, DFL_STORED_HEAD = 5;
constexpr int DFL_OVERHEAD = DFL_HEAD + DFL_STORED_HEAD + DFL_TAIL;   // 31: a stored member on top of its data
constexpr int DFL_SLOT = 65536;               // the largest member there is, and the bytes a block's member is built in
static_assert(DFL_BLOCK + DFL_OVERHEAD <= DFL_SLOT && (DFL_BLOCK + DFL_SEG - 1) / DFL_SEG <= DFL_LANES, "a member, a workgroup");

// ---- symbols ------------------------------------------------------------------------------------
DFL_HD int dfl_log2(uint32_t x) { return 31 - __builtin_clz(x); }                 // x > 0

// length 3..258 -> symbol 257..285, the number of its extra bits, their value
DFL_HD int dfl_len_sym(int len, int &eb, int &ev)
{
    const int l = len - 3;
    eb = ev = 0;
    if (len == 258) return 285;
    if (l < 8) return 257 + l;
    eb = dfl_log2((uint32_t)l) - 2;
    ev = l & ((1 << eb) - 1);
    return 257 + 4 * (eb + 1) + ((l >> eb) & 3);
}

// distance 1..32768 -> symbol 0..29
DFL_HD int dfl_dist_sym(int dist, int &eb, int &ev)
{
    const int d = dist - 1;
    eb = ev = 0;
    if (d < 4) return d;
    const int k = dfl_log2((uint32_t)d);
    eb = k - 1;
    ev = d & ((1 << eb) - 1);
    return 2 * k + ((d >> eb) & 1);
}

// ---- tokens -------------------------------------------------------------------------------------
// a literal is its byte; a match is length | distance << 9
DFL_HD uint32_t dfl_tok_match(int len, int dist) { return (uint32_t)len | ((uint32_t)dist << 9); }
DFL_HD int dfl_tok_dist(uint32_t t) { return (int)(t >> 9); }
DFL_HD int dfl_tok_len(uint32_t t) { return (int)(t & 511); }

// ---- the match rule -----------------------------------------------------------------------------
DFL_HD uint32_t dfl_load4(const uint8_t *b, int p)
{
    return (uint32_t)b[p] | ((uint32_t)b[p + 1] << 8) | ((uint32_t)b[p + 2] << 16) | ((uint32_t)b[p + 3] << 24);
}

DFL_HD uint32_t dfl_hash(uint32_t four) { return (four * 2654435761u) >> (32 - DFL_HASH_BITS); }

// what a lookup found for position p: entry = 1 + a position in front of p, 0: none.  The distance, 0 if there is no
// candidate or it lies farther back than a deflate distance reaches.
DFL_HD uint32_t dfl_candidate(int p, uint32_t entry)
{
    if (entry == 0) return 0;
    const int dist = p - (int)(entry - 1);
    return dist >= 1 && dist <= DFL_MAX_DIST ? (uint32_t)dist : 0;
}

// bytes that agree at p and p - dist, at most maxlen
DFL_HD int dfl_match_len(const uint8_t *b, int p, int dist, int maxlen)
{
    int n = 0;
    while (n < maxlen && b[p + n] == b[p - dist + n]) n++;
    return n;
}

// One lane's walk through its segment [begin, end) of the block b.  slot[p], begin <= p < end: the candidate distance of p on
// entry, the lane's tokens from slot[begin] on at the end.  Returns the number of tokens.
DFL_HD int dfl_walk(const uint8_t *b, int begin, int end, uint32_t *slot)
{
    int p = begin, k = 0;
    while (p < end) {
        const int maxlen = end - p < DFL_MAX_MATCH ? end - p : DFL_MAX_MATCH;
        int len = 0, dist = 0;
        if (maxlen >= DFL_MIN_MATCH) {
            const int cd = (int)slot[p];
            if (cd > 0 && cd <= p && cd <= DFL_MAX_DIST) {
                const int l = dfl_match_len(b, p, cd, maxlen);
                if (l >= DFL_MIN_MATCH) { len = l; dist = cd; }
            }
            if (p >= 1 && b[p] == b[p - 1]) {
                const int l = dfl_match_len(b, p, 1, maxlen);
                if (l >= DFL_MIN_MATCH && l >= len) { len = l; dist = 1; }      // (a tie: the nearer one, fewer extra bits)
            }
        }
        if (len) { slot[begin + k++] = dfl_tok_match(len, dist); p += len; }
        else { slot[begin + k++] = b[p]; p++; }
    }
    return k;
}

// the symbols of a token
DFL_HD void dfl_token_syms(uint32_t t, int &lsym, int &dsym)
{
    int eb, ev;
    if (dfl_tok_dist(t) == 0) { lsym = (int)t; dsym = -1; return; }
    lsym = dfl_len_sym(dfl_tok_len(t), eb, ev);
    dsym = dfl_dist_sym(dfl_tok_dist(t), eb, ev);
}

// bits of a token under the two codes' lengths
DFL_HD int dfl_token_bits(uint32_t t, const uint8_t *llen, const uint8_t *dlen)
{
    if (dfl_tok_dist(t) == 0) return llen[t];
    int eb1, eb2, ev;
    const int ls = dfl_len_sym(dfl_tok_len(t), eb1, ev), ds = dfl_dist_sym(dfl_tok_dist(t), eb2, ev);
    return llen[ls] + eb1 + dlen[ds] + eb2;
}

// ---- code lengths -------------------------------------------------------------------------------
// the place of symbol s among the used symbols of freq[0, n), by (count, symbol) ascending
DFL_HD int dfl_rank(const uint32_t *freq, int n, int s)
{
    const uint32_t f = freq[s];
    int r = 0;
    for (int j = 0; j < n; j++) {
        const uint32_t g = freq[j];
        r += (g != 0 && (g < f || (g == f && j < s))) ? 1 : 0;
    }
    return r;
}

// what every lane does for its symbols s = lane, lane + lanes, ... in front of dfl_lengths: the length cleared, a used symbol
// and its count put in their place
DFL_HD void dfl_rank_lane(const uint32_t *freq, int n, int lane, int lanes, uint16_t *sorted, int32_t *work, uint8_t *len)
{
    for (int s = lane; s < n; s += lanes) {
        len[s] = 0;
        if (freq[s]) {
            const int r = dfl_rank(freq, n, s);
            sorted[r] = (uint16_t)s;
            work[r] = (int32_t)freq[s];
        }
    }
}

// A[0, n): counts, ascending, n >= 2 -> the depths of a minimum-redundancy code, descending.  In place, three passes
// (A. Moffat, J. Katajainen, "In-place calculation of minimum-redundancy codes", 1995).
DFL_HD void dfl_min_redundancy(int32_t *A, int n)
{
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; next++) {
        if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; }
        else A[next] = A[leaf++];
        if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; }
        else A[next] += A[leaf++];
    }
    A[n - 2] = 0;
    for (int next = n - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
    int avbl = 1, used = 0, dpth = 0, next = n - 1;
    root = n - 2;
    while (avbl > 0) {
        while (root >= 0 && A[root] == dpth) { used++; root--; }
        while (avbl > used) { A[next--] = dpth; avbl--; }
        avbl = 2 * used; dpth++; used = 0;
    }
}

// ONE lane, behind dfl_rank_lane of every lane: len[s] for the used symbols, at most maxbits, the Kraft sum exactly 1.  A
// single used symbol gets a code of length 1 and, with pad_single, so does a second symbol (0, or 1 if the used one is 0):
// the sum is 1 then too.  No used symbol: nothing.  Returns the number of used symbols.
DFL_HD int dfl_lengths(const uint32_t *freq, int n, int maxbits, bool pad_single, const uint16_t *sorted, int32_t *work, uint8_t *len)
{
    int nu = 0;
    for (int s = 0; s < n; s++) nu += freq[s] != 0;
    if (nu == 0) return 0;
    if (nu == 1) {
        const int s = sorted[0];
        len[s] = 1;
        if (pad_single) len[s == 0 ? 1 : 0] = 1;
        return 1;
    }
    dfl_min_redundancy(work, nu);
    int blc[16];
    for (int i = 0; i < 16; i++) blc[i] = 0;
    for (int i = 0; i < nu; i++) blc[work[i] < maxbits ? work[i] : maxbits]++;
    // the leaves that were deeper are at the limit now and the code is over-full, by `total - 2^maxbits` codes of the limit's
    // length.  A step takes one of them away: a leaf of the deepest level above the limit goes one level down, and a leaf of
    // the limit's level moves in beside it.
    int32_t total = 0;
    for (int bits = 1; bits <= maxbits; bits++) total += blc[bits] << (maxbits - bits);
    for (; total > (1 << maxbits); total--) {
        int bits = maxbits - 1;
        while (blc[bits] == 0) bits--;
        blc[bits]--; blc[bits + 1] += 2; blc[maxbits]--;
    }
    int i = 0;
    for (int bits = maxbits; bits >= 1; bits--)
        for (int k = 0; k < blc[bits]; k++) len[sorted[i++]] = (uint8_t)bits;
    return nu;
}

DFL_HD uint32_t dfl_bitrev(uint32_t c, int n)
{
    uint32_t r = 0;
    for (int i = 0; i < n; i++) { r = (r << 1) | (c & 1); c >>= 1; }
    return r;
}

// canonical codes of len[0, n), each bit-reversed: deflate packs a code from its most significant bit
DFL_HD void dfl_codes(const uint8_t *len, int n, uint16_t *code)
{
    int blc[16], nxt[16];
    for (int i = 0; i < 16; i++) blc[i] = 0;
    for (int s = 0; s < n; s++) blc[len[s]]++;
    blc[0] = 0;
    int c = 0;
    nxt[0] = 0;
    for (int b = 1; b < 16; b++) { c = (c + blc[b - 1]) << 1; nxt[b] = c; }
    for (int s = 0; s < n; s++) code[s] = len[s] ? (uint16_t)dfl_bitrev((uint32_t)nxt[len[s]]++, len[s]) : 0;
}

// ---- the header of a dynamic block --------------------------------------------------------------
// the order the header gives the lengths of its own code in
DFL_HD int dfl_cl_order(int i)
{
    switch (i) {
    case 0: return 16; case 1: return 17; case 2: return 18; case 3: return 0; case 4: return 8; case 5: return 7;
    case 6: return 9; case 7: return 6; case 8: return 10; case 9: return 5; case 10: return 11; case 11: return 4;
    case 12: return 12; case 13: return 3; case 14: return 13; case 15: return 2; case 16: return 14; case 17: return 1;
    default: return 15;
    }
}

struct DflPlan {
    int hlit, hdist, hclen;           // the NUMBERS of lengths the header gives: 257.., 1.., 4..
    int head_bits;                    // bits of the header, the three block bits included
};

// the numbers of literal/length and distance lengths the header carries
DFL_HD void dfl_header_counts(const uint8_t *llen, const uint8_t *dlen, DflPlan &pl)
{
    int hl = DFL_NLIT, hd = DFL_NDIST;
    while (hl > 257 && llen[hl - 1] == 0) hl--;
    while (hd > 1 && dlen[hd - 1] == 0) hd--;
    pl.hlit = hl; pl.hdist = hd;
}

// behind the header code's lengths: how many of those are given, the header's bits
DFL_HD void dfl_header_plan(const uint32_t *cfreq, const uint8_t *clen, DflPlan &pl)
{
    int hc = DFL_NCL;
    while (hc > 4 && clen[dfl_cl_order(hc - 1)] == 0) hc--;
    pl.hclen = hc;
    int bits = 3 + 5 + 5 + 4 + 3 * hc;
    for (int s = 0; s < DFL_NCL; s++) bits += (int)cfreq[s] * clen[s];
    pl.head_bits = bits;
}

// stored, not dynamic: the dynamic stream would be longer than a stored block of n bytes
DFL_HD bool dfl_stored(int64_t stream_bits, int n) { return (stream_bits + 7) / 8 > (int64_t)n + DFL_STORED_HEAD; }

// ---- bits ---------------------------------------------------------------------------------------
// A lane's bits, from bit `at` of a zeroed array of 32-bit words.  W: { void plain(uint32_t i, uint32_t w); void shared(uint32_t
// i, uint32_t w); } -- `plain` for a word that is all this lane's, `shared` (an OR) for its first and its last.
template <class W>
struct DflBits {
    W &w;
    uint64_t acc = 0;
    int nb;
    uint32_t wi;
    bool first = true;
    DFL_HD DflBits(W &w_, int64_t at) : w(w_), nb((int)(at & 31)), wi((uint32_t)(at >> 5)) {}
    DFL_HD void put(uint32_t v, int n)            // n <= 16
    {
        acc |= (uint64_t)v << nb;
        nb += n;
        if (nb >= 32) {
            if (first) w.shared(wi, (uint32_t)acc); else w.plain(wi, (uint32_t)acc);
            first = false; wi++; acc >>= 32; nb -= 32;
        }
    }
    DFL_HD void finish() { if (nb > 0 && acc) w.shared(wi, (uint32_t)acc); nb = 0; acc = 0; }
};

template <class W>
DFL_HD void dfl_put_token(DflBits<W> &o, uint32_t t, const uint16_t *lcode, const uint8_t *llen, const uint16_t *dcode, const uint8_t *dlen)
{
    if (dfl_tok_dist(t) == 0) { o.put(lcode[t], llen[t]); return; }
    int eb, ev;
    const int ls = dfl_len_sym(dfl_tok_len(t), eb, ev);
    o.put(lcode[ls], llen[ls]);
    if (eb) o.put((uint32_t)ev, eb);
    const int ds = dfl_dist_sym(dfl_tok_dist(t), eb, ev);
    o.put(dcode[ds], dlen[ds]);
    if (eb) o.put((uint32_t)ev, eb);
}

// the header of a dynamic block, BFINAL set: ONE lane
template <class W>
DFL_HD void dfl_put_header(DflBits<W> &o, const DflPlan &pl, const uint8_t *llen, const uint8_t *dlen, const uint16_t *ccode, const uint8_t *clen)
{
    o.put(1, 1); o.put(2, 2);
    o.put((uint32_t)(pl.hlit - 257), 5); o.put((uint32_t)(pl.hdist - 1), 5); o.put((uint32_t)(pl.hclen - 4), 4);
    for (int i = 0; i < pl.hclen; i++) o.put(clen[dfl_cl_order(i)], 3);
    for (int s = 0; s < pl.hlit; s++) o.put(ccode[llen[s]], clen[llen[s]]);
    for (int s = 0; s < pl.hdist; s++) o.put(ccode[dlen[s]], clen[dlen[s]]);
}

// ---- the member ---------------------------------------------------------------------------------
// the 18 bytes in front of a member's deflate stream (SAM specification 4.1); member_bytes: all of it, at most 65536
DFL_HD void dfl_member_head(uint8_t out[DFL_HEAD], int member_bytes)
{
    const uint8_t h[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    for (int i = 0; i < 16; i++) out[i] = h[i];
    out[16] = (uint8_t)((member_bytes - 1) & 255);
    out[17] = (uint8_t)((member_bytes - 1) >> 8);
}

// bytes of a member whose deflate stream has stream_bytes
DFL_HD int dfl_member_bytes(int stream_bytes) { return DFL_HEAD + stream_bytes + DFL_TAIL; }

// a byte into the zeroed words a member is built in
template <class W>
DFL_HD void dfl_put_byte(W &w, int at, uint32_t v) { w.shared((uint32_t)at >> 2, (v & 255u) << (8 * (at & 3))); }

// what stands around the deflate stream: the 18 bytes in front, CRC-32 and ISIZE behind.  ONE lane.
template <class W>
DFL_HD void dfl_put_frame(W &w, int member_bytes, uint32_t crc, int n)
{
    uint8_t h[DFL_HEAD];
    dfl_member_head(h, member_bytes);
    for (int i = 0; i < DFL_HEAD; i++) dfl_put_byte(w, i, h[i]);
    for (int i = 0; i < 4; i++) {
        dfl_put_byte(w, member_bytes - 8 + i, crc >> (8 * i));
        dfl_put_byte(w, member_bytes - 4 + i, (uint32_t)n >> (8 * i));
    }
}

// the five bytes in front of the data of a stored block of n bytes, BFINAL set.  ONE lane.
template <class W>
DFL_HD void dfl_put_stored_head(W &w, int n)
{
    dfl_put_byte(w, DFL_HEAD, 1);
    dfl_put_byte(w, DFL_HEAD + 1, (uint32_t)n); dfl_put_byte(w, DFL_HEAD + 2, (uint32_t)n >> 8);
    dfl_put_byte(w, DFL_HEAD + 3, ~(uint32_t)n); dfl_put_byte(w, DFL_HEAD + 4, ~(uint32_t)n >> 8);
}

// the empty member that ends a BGZF file
DFL_HD void dfl_eof_member(uint8_t out[28])
{
    dfl_member_head(out, 28);
    out[18] = 3; out[19] = 0;                     // an empty fixed-Huffman block, BFINAL set
    for (int i = 20; i < 28; i++) out[i] = 0;
}

// ---- CRC-32 -------------------------------------------------------------------------------------
constexpr uint32_t DFL_CRC_POLY = 0xEDB88320u;

DFL_HD uint32_t dfl_crc_entry(int i)
{
    uint32_t c = (uint32_t)i;
    for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ DFL_CRC_POLY : c >> 1;
    return c;
}

// the CRC-32 of n bytes, as zlib's crc32(0, b, n), by a table of the 256 dfl_crc_entry values
DFL_HD uint32_t dfl_crc(const uint32_t *table, const uint8_t *b, int n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 0; i < n; i++) c = table[(c ^ b[i]) & 255] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

// a(x) * b(x) mod P, polynomials over GF(2) in the CRC's reflected order (bit 31 is x^0)
DFL_HD uint32_t dfl_gf2_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1) ? (b >> 1) ^ DFL_CRC_POLY : b >> 1;
    }
    return p;
}

// x2n[k] = x^(2^k) mod P, k = 0..31
DFL_HD void dfl_crc_x2n(uint32_t x2n[32])
{
    uint32_t p = 0x40000000u;                     // x^1
    for (int k = 0; k < 32; k++) { x2n[k] = p; p = dfl_gf2_mul(p, p); }
}

// x^(8 * n_bytes) mod P
DFL_HD uint32_t dfl_crc_xpow8(const uint32_t x2n[32], uint32_t n_bytes)
{
    uint32_t p = 0x80000000u;                     // 1
    for (int k = 3; n_bytes; n_bytes >>= 1, k++)
        if (n_bytes & 1) p = dfl_gf2_mul(x2n[k & 31], p);
    return p;
}

// what a piece's CRC adds to the CRC of the whole, `behind` bytes following the piece: the whole's CRC is the XOR of these
// (zlib's crc32_combine, piece by piece)
DFL_HD uint32_t dfl_crc_shift(const uint32_t x2n[32], uint32_t crc, uint32_t behind)
{
    return behind ? dfl_gf2_mul(dfl_crc_xpow8(x2n, behind), crc) : crc;
}

}  // namespace ffq

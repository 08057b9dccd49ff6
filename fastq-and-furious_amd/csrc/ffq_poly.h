// ffq_poly.h -- poly-G / poly-X tail trimming by editing rows of the offset table (ffq_table_trim_poly).
//
// The rule (include/ffq.h states it as a loop): seq[0..n) = buf[pos2:pos3] is walked from its 3' end; per base b of the set S
// (one fixed base, or all four) the positions that are not b are counted, and the walk stops at the first position
// i >= min_len - 1 at which every base of S has more than allowed(i) = min(5, (i + 1) / 8) of them.  A walk that got to
// min_len positions cuts the read behind the deepest exact copy of the one base that was still passing: pos3 and pos5 move.
// Eligibility is the adapter trim's (ffq_rows.h: row_pos<true, false>, no '\n' in the sequence); any other row is copied
// unchanged and counted.  The quality line is never read.
//
// Shape: the row frame of ffq_rows.h, as ffq_trim.h uses it -- eight lanes per row; rows of more than POLY_LONG bases get a
// whole wave in the second launch.  The pass's own part is the walk, in chunks of G * B positions from the 3' end (B
// consecutive bytes per lane as unaligned dwords: trim_chunk of ffq_trim.h, walking backwards).  What a lane does with its bytes
// and what the group does with the reduced results is ffq_polywalk.h, which says how a chunk goes; here are the reductions:
//   * one RowGroup::incl_scan of the lanes' packed indicator sums -- all four bases in one register for the chunk of 64, in
//     two for the long rows' chunk of 1024;
//   * one max-reduction for the chunk's first stopping position, one move of the counts in front of it from the lane that
//     has them, and one max-reduction per base for the deepest exact hit in front of the stop -- only for bases that are
//     alive in some row of the wave: one with poly-G, and one from the second chunk on.
// Ordinary reads stop in the first chunk, so it is loaded together with the first pieces of the newline check; that check
// then covers whatever the walk did not read.  Every loop is uniform over the wave (`while (__any(act))`): a group without a
// row, with an ineligible, empty or short row, or done with its row, steps along idle.  No byte outside the row's own
// sequence range, itself checked against the buffer, is read.
#pragma once
#include "ffq_trim.h"
#include "ffq_polywalk.h"

namespace ffq {

constexpr int POLY_LONG = 4096;       // bases above which a row gets a wave of its own
constexpr int POLY_WG = 256;
constexpr int POLY_B = 8;             // bytes per lane and chunk of the short rows' kernel

// packed counts across a group: the prefix sum, and the value of one lane of the group (src: its place in it) in all of them
template <int G>
__device__ __forceinline__ uint32_t poly_scan(uint32_t x, int gl) { return (uint32_t)RowGroup<G>::incl_scan((int)x, gl); }
template <int G>
__device__ __forceinline__ uint64_t poly_scan(uint64_t x, int gl)
{
    return (uint64_t)poly_scan<G>((uint32_t)x, gl) | ((uint64_t)poly_scan<G>((uint32_t)(x >> 32), gl) << 32);
}

// (fields are below 2^(FB-1): a packed word is a non-negative int, and the maximum over `x or 0` is x)
template <int G>
__device__ __forceinline__ uint32_t poly_from(uint32_t x, int src, int gl, int gshift)
{
    if constexpr (G == 64) return (uint32_t)__shfl((int)x, src);
    else return (uint32_t)RowGroup<G>::maxall(gl == src ? (int)x : 0);
}
template <int G>
__device__ __forceinline__ uint64_t poly_from(uint64_t x, int src, int gl, int gshift)
{
    return (uint64_t)poly_from<G>((uint32_t)x, src, gl, gshift) | ((uint64_t)poly_from<G>((uint32_t)(x >> 32), src, gl, gshift) << 32);
}

// The walk of one row per group.  live: the group has an eligible row for this launch (uniform in the group).  first: the
// first chunk (trim_chunk<G, B, true> at w0 = 0), loaded by the caller.  newlen: the row's new length; nread: seq[n - nread .. n)
// went through the newline check here.
template <int G, int B>
__device__ __forceinline__ void poly_walk(const uint8_t *__restrict__ seq, int64_t n, bool live, int base, int min_len, int gl,
                                          int gshift, const int (&first)[B], int64_t &newlen, int64_t &nread, bool &nl)
{
    constexpr int C = G * B;
    typedef PolyOps<C> P;
    typedef typename P::T T;
    PolyState<C> s = {P::begin(base), -1, 0};
    newlen = n; nread = 0;
    bool act = live && n >= min_len;                    // (a shorter row cannot get to min_len positions)
    for (bool head = true; __any(act); head = false) {
        int qv[B];
        if (head) {
#pragma unroll
            for (int j = 0; j < B; j++) qv[j] = act ? first[j] : -1;
        } else
            trim_chunk<G, B, true>(seq, n, act, s.w0, gl, qv);
        const int64_t i0 = s.w0 + (int64_t)gl * B;        // this lane's first walk position
        const int avail = act ? (int)min(max(n - i0, (int64_t)0), (int64_t)B) : 0;
        int k[B];
        typename PolyHits<B>::T hits;
        nl |= poly_classify<B>(qv, k, hits);
        const T t = poly_lane_sum<C, B>(k, avail);
        const T start = s.mm + (poly_scan<G>(t, gl) - t);
        int stop_j;
        T at;
        poly_lane_walk<C, B>(k, avail, i0, min_len, start, stop_j, at);
        const int skey = RowGroup<G>::maxall(poly_stop_key<C, B>(gl, stop_j));
        at = poly_from<G>(at, act ? poly_end_lane<C, B>(skey, s.w0, n) : 0, gl, gshift);
        const int upto = poly_hit_upto<C, B>(skey, gl, avail);
        int g[4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            g[b] = 0;
            if (__any(act && P::field(s.mm, b) < POLY_DEAD)) g[b] = RowGroup<G>::maxall(poly_hit_key<B>(hits, b, upto, gl));
        }
        if (act) {
            nread = min(s.w0 + C, n);
            int64_t len;
            act = poly_chunk_end<C>(s, n, min_len, skey, at, g, &len);
            newlen = len;
        }
    }
}

// One row per group, as trim_row: have: this group has a row (uniform in the group); defer_long: rows above POLY_LONG are
// left to the second launch (returned).
template <int G, int B>
__device__ __forceinline__ bool poly_row(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                         const int64_t *__restrict__ table, int64_t *__restrict__ out, int64_t row, bool have,
                                         longlong2 r01, longlong2 r23, longlong2 r45, int base, int min_len, bool defer_long,
                                         int gl, int gshift, RowCounts &cnt)
{
    int64_t p2 = 0, p4 = 0, n = 0;
    const bool elig = have && row_pos<true, false>(nbytes, s, add, r23, r45, p2, p4, n);
    const bool is_long = defer_long && elig && n > POLY_LONG;
    const bool live = elig && !is_long && n > 0;
    const uint8_t *seq = d + (p2 - s);

    // everything a row whose walk ends in its first chunk needs, asked for at once: that chunk (the last C bases) and the first
    // G * 16 bytes of what lies in front of it
    constexpr int C = G * B;
    int qb[B];
    trim_chunk<G, B, true>(seq, n, live, 0, gl, qb);
    bool nl = false;
    if (live && (int64_t)gl * 16 < n - C) nl = rows_nl16(seq, (int64_t)gl * 16, n - C);
#pragma unroll
    for (int j = 0; j < B; j++) nl |= qb[j] == 10;      // (a row the walk does not take up is checked all the same)

    int64_t newlen = n, nread = 0;
    poly_walk<G, B>(seq, n, live, base, min_len, gl, gshift, qb, newlen, nread, nl);
    rows_scan_nl<G>(seq, (int64_t)G * 16, n - max(nread, (int64_t)C), live, gl, nl);
    const bool any_nl = group_any<G>(nl, gshift);

    // (pos + newlen: the row's own coordinates, whatever `add` is)
    row_edit_finish(table, out, row, gl, have, is_long, elig && !any_nl, r01, r23, r45, make_longlong2(r23.x, r23.x + newlen),
                    make_longlong2(r45.x, r45.x + newlen), n - newlen, cnt);
    return is_long;
}

__global__ __launch_bounds__(POLY_WG) void k_poly_rows(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                       const int64_t *table, int64_t n_rows, int base, int min_len, int64_t *out,
                                                       int64_t *__restrict__ long_list, RowsBlock *__restrict__ blk)
{
    constexpr int G = ROWS_G;
    const int lane = threadIdx.x & 63, gl = lane & (G - 1), gshift = lane & ~(G - 1);
    RowCounts cnt;
    constexpr int RPB = POLY_WG / G;
    const int64_t step = (int64_t)gridDim.x * RPB;
    longlong2 x01 = make_longlong2(0, 0), x23 = x01, x45 = x01;
    {
        const int64_t row = (int64_t)blockIdx.x * RPB + (threadIdx.x / G);
        if (row < n_rows) {
            const longlong2 *src = reinterpret_cast<const longlong2 *>(table + row * 6);
            x01 = src[0]; x23 = src[1]; x45 = src[2];
        }
    }
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < n_rows; r0 += step) {
        const int64_t row = r0 + (threadIdx.x / G);
        const longlong2 r01 = x01, r23 = x23, r45 = x45;
        if (row + step < n_rows) {
            const longlong2 *src = reinterpret_cast<const longlong2 *>(table + (row + step) * 6);
            x01 = src[0]; x23 = src[1]; x45 = src[2];
        }
        const bool is_long = poly_row<G, POLY_B>(d, nbytes, s, add, table, out, row, row < n_rows, r01, r23, r45, base, min_len, true, gl,
                                                 gshift, cnt);
        const int64_t at = long_list_append(is_long && gl == 0, lane, &blk->n_long);
        if (at >= 0) long_list[at] = row;
    }
    cnt.add_to<POLY_WG>(blk);
}

// the rows k_poly_rows left: sixteen bytes per lane and chunk
__global__ __launch_bounds__(POLY_WG) void k_poly_long(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                       const int64_t *table, int base, int min_len, int64_t *out,
                                                       const int64_t *__restrict__ long_list, RowsBlock *__restrict__ blk)
{
    const int lane = threadIdx.x & 63;
    RowCounts cnt;
    for (LongRows<POLY_WG, true> it((int64_t)blk->n_long, long_list, table); it.next();)
        poly_row<64, 16>(d, nbytes, s, add, table, out, it.row, it.have, it.r01, it.r23, it.r45, base, min_len, false, lane, 0, cnt);
    cnt.add_to<POLY_WG>(blk);
}

}  // namespace ffq

// ffq_render.h -- FASTQ text from (buffer, table): ffq_table_render_fastq.
//
// The reference's user guide keeps a table of positions "to avoid saving a FASTQ file after each filtering or
// read-trimming step" (/root/reference/doc/user-guide.rst:196-204); a pipeline still ends by saving one.  Row p renders as
//     "@" + buf[p0 + 1 : p1] + "\n" + buf[p2 : p3] + "\n+\n" + buf[p4 : p5] + "\n"
// -- the three slices entryfunc cuts (/root/reference/src/fastqandfurious.py:161-171) and six literal bytes; the '+' line
// is always bare.  A row is RENDERABLE if all six positions - add are >= 0, p0 + 1 <= p1, p2 <= p3, p4 <= p5 and every
// slice lies inside the buffer (a slice may end at its end; with a sentinel, coordinate 0 is the virtual '\n' and no
// slice with a byte in it may begin there); every other row -- FASTA rows (-1), rows that point outside -- renders as
// nothing and is counted.  Rows are independent: any order, repeated, overlapping.
//
// Shape.  Three launches behind one another:
//   k_render_sum    rendered bytes per block of 256 rows (and the number of renderable rows)
//   launch_scan     exclusive scan of those (ffq_scan.h: the machinery of the column gather)
//   k_render_rows   a workgroup per block of 256 rows: the prefix inside the block gives every row its place in the
//                   output (d_off), then a GROUP of eight lanes copies a row -- thirty-two rows at a time, neighbours in
//                   the output, so that a wave's stores fall into one run of lines
//   k_render_long   rows of more than RENDER_LONG output bytes were put on a list; each gets a whole wave
// The copy is ROW-centric and DESTINATION-aligned: a row's bytes in the output are cut into 16-byte chunks aligned on the
// output address, a lane builds a chunk in registers from up to three unaligned, non-temporal 16-byte loads (one per
// slice that has bytes under the chunk, positioned chunk-relative: load16_any of the column gather, which reads nothing
// outside the buffer) and the literals, and stores it with ONE aligned 16-byte store; only the first and the last chunk
// of a row, which it shares with its neighbours, are written in pieces (dwords and bytes).  RENDER_U chunks per lane are
// in flight.  No byte outside [out + off[i], out + off[i + 1]) is written for row i, and nothing at all if the total
// exceeds out_cap.
#pragma once
#include "ffq_kernels.h"
#include "ffq_rows.h"

namespace ffq {

constexpr int RENDER_WG = 256;
constexpr int RENDER_G = 8;           // lanes per row of the short rows' kernel
constexpr int RENDER_U = 4;           // chunks per lane in flight
constexpr int RENDER_LONG = 4096;     // output bytes above which a row gets a wave of its own
// (the prefix of the rows' lengths inside a block is wg_excl_scan<RENDER_WG, SCAN_ANY>, 64-bit throughout: a row that repeats
// most of a large buffer three times over is longer than 2^31)

// counters of a call: output bytes, rows rendered, rows on the long list
struct RenderBlock { unsigned long long total, rendered, n_long; };

// a renderable row: byte index in the buffer of its three slices and their lengths
struct RenderRow { int64_t hsrc, ssrc, qsrc, h, s, q; };

// rendered length of a row (0: not renderable) and where its slices are
__device__ __forceinline__ int64_t render_parse(longlong2 r01, longlong2 r23, longlong2 r45, int64_t nbytes, int s,
                                                int64_t add, RenderRow &R)
{
    const int64_t p0 = row_coord(r01.x, add), p1 = row_coord(r01.y, add), p2 = row_coord(r23.x, add), p3 = row_coord(r23.y, add);
    const int64_t p4 = row_coord(r45.x, add), p5 = row_coord(r45.y, add);
    const int64_t L = nbytes + s;
    bool ok = p0 >= 0 && p2 >= 0 && p4 >= 0 && p0 < p1 && p2 <= p3 && p4 <= p5 && p1 <= L && p3 <= L && p5 <= L;
    // all three lines are read, so none with a byte in it may begin at the virtual '\n' (ffq_rows.h: row_pos); the header
    // begins at p0 + 1 >= 1
    if (s && ((p3 > p2 && p2 < s) || (p5 > p4 && p4 < s))) ok = false;
    if (!ok) { R.hsrc = R.ssrc = R.qsrc = 0; R.h = R.s = R.q = 0; return 0; }
    R.hsrc = p0 + 1 - s; R.h = p1 - p0 - 1;
    R.ssrc = p2 - s; R.s = p3 - p2;
    R.qsrc = p4 - s; R.q = p5 - p4;
    return R.h + R.s + R.q + 6;
}

__device__ __forceinline__ int64_t render_row_len(const int64_t *__restrict__ table, int64_t row, int64_t n_rows,
                                                  int64_t nbytes, int s, int64_t add, RenderRow &R)
{
    if (row >= n_rows) { R.hsrc = R.ssrc = R.qsrc = 0; R.h = R.s = R.q = 0; return 0; }
    const longlong2 *src = reinterpret_cast<const longlong2 *>(table + row * 6);
    const longlong2 r01 = src[0], r23 = src[1], r45 = src[2];
    return render_parse(r01, r23, r45, nbytes, s, add, R);
}

// Workgroups stride over the blocks of 256 rows (one atomic per workgroup of the launch for the row count, not per block).
__global__ __launch_bounds__(RENDER_WG) void k_render_sum(int64_t nbytes, int s, int64_t add, const int64_t *__restrict__ table,
                                                          int64_t n_rows, int64_t nblk, long long *__restrict__ bsum,
                                                          RenderBlock *__restrict__ blk)
{
    unsigned int cnt = 0;
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
        const int64_t row = b * RENDER_WG + threadIdx.x;
        RenderRow R;
        const int64_t len = render_row_len(table, row, n_rows, nbytes, s, add, R);
        int64_t tot;
        (void)wg_excl_scan<RENDER_WG, SCAN_ANY>(len, tot);
        if (threadIdx.x == 0) bsum[b] = tot;
        cnt += (unsigned int)__popcll(__ballot(len > 0));
        __syncthreads();                                    // (the scan's LDS is written again by the next block of rows)
    }
    // (cnt is the WAVE's count, the same in all of its lanes: one lane hands it in)
    const unsigned int c[1] = {(threadIdx.x & 63) == 0 ? cnt : 0u};
    wg_counts_flush<RENDER_WG>(c, &blk->rendered);
}

// bytes [a, b) of x into y
__device__ __forceinline__ uint4 render_merge(uint4 y, uint4 x, int a, int b)
{
    const uint32_t m0 = lt_mask(b, 0) & ~lt_mask(a, 0), m1 = lt_mask(b, 1) & ~lt_mask(a, 1);
    const uint32_t m2 = lt_mask(b, 2) & ~lt_mask(a, 2), m3 = lt_mask(b, 3) & ~lt_mask(a, 3);
    return make_uint4((y.x & ~m0) | (x.x & m0), (y.y & ~m1) | (x.y & m1), (y.z & ~m2) | (x.z & m2), (y.w & ~m3) | (x.w & m3));
}

// literal byte v at chunk byte k, if the chunk has it
__device__ __forceinline__ uint4 render_put(uint4 y, int64_t k, uint32_t v)
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

// chunk bytes [a, b) that a span of xl bytes, whose first byte is chunk byte rel, covers
__device__ __forceinline__ void render_span(int64_t rel, int64_t xl, int &a, int &b)
{
    a = (int)min(max(rel, (int64_t)0), (int64_t)16);
    b = (int)min(max(rel + xl, (int64_t)0), (int64_t)16);
}

// bytes [kb, ke) of a chunk to its 16-byte aligned place o: whole dwords where it has them, bytes at the ends
__device__ __noinline__ void render_store_part(uint8_t *__restrict__ o, uint4 v, int kb, int ke)
{
    const uint32_t y[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const int lo = max(kb - 4 * w, 0), hi = min(ke - 4 * w, 4);
        if (lo >= hi) continue;
        if (lo == 0 && hi == 4) reinterpret_cast<uint32_t *>(o)[w] = y[w];
        else
            for (int t = lo; t < hi; t++) o[4 * w + t] = (uint8_t)(y[w] >> (8 * t));
    }
}

// One row by a group of G lanes (gl: this lane's place in it): `o` = where the row's first byte goes, len > 0 its length.
template <int G>
__device__ __forceinline__ void render_copy(const uint8_t *__restrict__ d, int64_t nbytes, const RenderRow &R, int64_t len,
                                            uint8_t *__restrict__ o, int gl)
{
    constexpr int U = RENDER_U;
    // chunk k covers row bytes [16 k - shift, +16) cut to [0, len)
    const int shift = (int)(reinterpret_cast<uintptr_t>(o) & 15);
    const int64_t nchunk = (len + shift + 15) >> 4;
    // row-relative places: '@' 0, header 1, '\n' o_s - 1, sequence o_s, "\n+\n" o_p, quality o_q, '\n' len - 1
    const int64_t o_s = 2 + R.h, o_p = o_s + R.s, o_q = o_p + 3;
    for (int64_t k0 = 0; k0 < nchunk; k0 += (int64_t)G * U) {
        uint4 xh[U], xs[U], xq[U];
        // every load of the lane's U chunks in flight together
#pragma unroll
        for (int j = 0; j < U; j++) {
            const int64_t k = k0 + (int64_t)j * G + gl;
            const int64_t clo = 16 * k - shift;
            xh[j] = xs[j] = xq[j] = make_uint4(0, 0, 0, 0);
            if (k >= nchunk) continue;
            int a, b;
            render_span(1 - clo, R.h, a, b);
            if (b > a) xh[j] = load16_any(d, nbytes, R.hsrc + (clo - 1));
            render_span(o_s - clo, R.s, a, b);
            if (b > a) xs[j] = load16_any(d, nbytes, R.ssrc + (clo - o_s));
            render_span(o_q - clo, R.q, a, b);
            if (b > a) xq[j] = load16_any(d, nbytes, R.qsrc + (clo - o_q));
        }
#pragma unroll
        for (int j = 0; j < U; j++) {
            const int64_t k = k0 + (int64_t)j * G + gl;
            const int64_t clo = 16 * k - shift;
            if (k >= nchunk) continue;
            uint4 y = make_uint4(0, 0, 0, 0);
            int a, b;
            render_span(1 - clo, R.h, a, b);
            y = render_merge(y, xh[j], a, b);
            render_span(o_s - clo, R.s, a, b);
            y = render_merge(y, xs[j], a, b);
            render_span(o_q - clo, R.q, a, b);
            y = render_merge(y, xq[j], a, b);
            y = render_put(y, 0 - clo, '@');
            y = render_put(y, o_s - 1 - clo, '\n');
            y = render_put(y, o_p - clo, '\n');
            y = render_put(y, o_p + 1 - clo, '+');
            y = render_put(y, o_p + 2 - clo, '\n');
            y = render_put(y, len - 1 - clo, '\n');
            const int kb = (int)max(-clo, (int64_t)0), ke = (int)min(len - clo, (int64_t)16);
            uint8_t *dst = o + clo;                           // 16-byte aligned; only [kb, ke) of it is the row's
            if (kb == 0 && ke == 16) *reinterpret_cast<uint4 *>(dst) = y;
            else render_store_part(dst, y, kb, ke);
        }
    }
}

// A workgroup per block of 256 rows.  total > out_cap: the offsets are written, the output is not touched.
__global__ __launch_bounds__(RENDER_WG) void k_render_rows(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                           const int64_t *__restrict__ table, int64_t n_rows,
                                                           const long long *__restrict__ bbase, const DevRes *__restrict__ res,
                                                           uint8_t *__restrict__ out, int64_t out_cap, int64_t *__restrict__ off,
                                                           int64_t *__restrict__ long_list, RenderBlock *__restrict__ blk)
{
    constexpr int G = RENDER_G, NG = RENDER_WG / G;
    __shared__ RenderRow s_row[RENDER_WG];
    __shared__ int64_t s_off[RENDER_WG], s_len[RENDER_WG];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * RENDER_WG;
    const int64_t total = res->n_qual_bytes;
    {
        RenderRow R;
        const int64_t len = render_row_len(table, r0 + tid, n_rows, nbytes, s, add, R);
        int64_t tot;
        const int64_t at = bbase[blockIdx.x] + wg_excl_scan<RENDER_WG, SCAN_ANY>(len, tot);
        s_row[tid] = R; s_off[tid] = at; s_len[tid] = len;
        if (off && r0 + tid < n_rows) off[r0 + tid] = at;
        if (blockIdx.x == 0 && tid == 0) {
            if (off) off[n_rows] = total;
            blk->total = (unsigned long long)total;
        }
    }
    __syncthreads();
    if (total > out_cap) return;
    const int g = tid / G, gl = tid & (G - 1), lane = tid & 63;
    // step i: group g has row i * NG + g of the block -- the thirty-two rows of a step are neighbours in the output
    for (int i = 0; i < G; i++) {
        const int r = i * NG + g;
        const int64_t len = s_len[r];
        const bool is_long = len > RENDER_LONG;
        if (len > 0 && !is_long) {
            const RenderRow R = s_row[r];
            render_copy<G>(d, nbytes, R, len, out + s_off[r], gl);
        }
        const int64_t e = long_list_append(is_long && gl == 0, lane, &blk->n_long);
        if (e >= 0) { long_list[2 * e] = r0 + r; long_list[2 * e + 1] = s_off[r]; }
    }
}

// the rows k_render_rows left: a wave per row ((row, place in the output) pairs of the list)
__global__ __launch_bounds__(RENDER_WG) void k_render_long(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                           const int64_t *__restrict__ table, int64_t n_rows,
                                                           uint8_t *__restrict__ out, const int64_t *__restrict__ long_list,
                                                           const RenderBlock *__restrict__ blk)
{
    constexpr int WPB = RENDER_WG / 64;
    const int lane = threadIdx.x & 63;
    const int64_t n_long = (int64_t)blk->n_long;
    for (int64_t j = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6); j < n_long; j += (int64_t)gridDim.x * WPB) {
        const int64_t row = long_list[2 * j], at = long_list[2 * j + 1];
        RenderRow R;
        const int64_t len = render_row_len(table, row, n_rows, nbytes, s, add, R);
        if (len > 0) render_copy<64>(d, nbytes, R, len, out + at, lane);
    }
}

}  // namespace ffq

// ffq_umi.h -- unique molecular identifiers: taken off the reads by editing rows (ffq_table_take_umi) and put into the names
// when the rows are rendered (ffq_table_render_fastq_umi).  include/ffq.h states the rule as a loop; what a lane does with its
// bytes is ffq_umiwalk.h.
//
// THE TAKE is a row-editing pass in the frame of ffq_rows.h: eight lanes per row, rows of more than UMI_LONG bases get a whole
// wave in the second launch.  Its own part is small: the newline look over BOTH lines (rows_scan_nl) and pos2 == pos1 + 1; the
// cut is arithmetic.  No byte outside the row's two checked lines is read.
//
// THE TAGGED RENDER keeps the three launches of ffq_render.h -- sum, scan (ffq_scan.h), rows and long rows -- as kernels of its
// own: k_render_sum / k_render_rows / k_render_long are not touched and compile as they did.  No side table: the take never moves
// pos1, so the tag of a row is found again at buf[pos1 + 1 : pos1 + 1 + len] of its SOURCE row (umi_carrier), whatever selects
// and compactions the row went through.  A source may be the rendered table itself or a table over another buffer (the other
// mate's), with its own `add` and sentinel: the kernels take three sides (UmiSide).
//   k_umi_render_sum    a thread per row: render_parse, then umi_carrier per source the location names (two table words and
//                       up to four 16-byte loads each); the length of a tagged row is the plain one + umi_ins_len
//   k_umi_render_rows   the same per-row parse for the offsets; then, per group of eight lanes and row, the header's first
//                       blank k (umi_first_blank: sixteen bytes per lane and step, a minimum over the group) and the copy
//   k_umi_render_long   a wave per row of more than RENDER_LONG output bytes: the same two steps, sixty-four lanes wide
// k is RECOMPUTED in the rows kernel, not kept in scratch between the launches: the sum kernel does not need it (the insert's
// length does not depend on where it goes), so keeping it would make that kernel walk headers it otherwise never reads and cost
// eight bytes per row written and read back; the group that recomputes it loads the header's bytes for the copy anyway.
// The copy is render_copy's, destination-aligned 16-byte chunks, with more pieces under a chunk: header head, the literal
// (delim, prefix, '_': from LDS), tag 1, tag 2, header tail, sequence, quality -- umi_layout says where they lie, umi_span what
// of a chunk they cover; every load is load16_any, which reads nothing outside its buffer.  A row that is not tagged goes
// through render_copy itself.  Every loop with a cross-lane move in it is uniform over the wave (`while (__any(act))`): a group
// without a row, or with a row that has no tag, steps along.
//
// A TRANSLATION UNIT OF ITS OWN.  This header is compiled by csrc/ffq_umi.hip alone, not by ffq_hip.hip: the tagged render shares
// render_copy, load16_any and their `__noinline__` helpers with ffq_render.h, and inside one translation unit the new callers
// changed the code the compiler made for k_render_sum / k_render_rows / k_render_long (registers around the helpers' calls).
// Built apart, the library's other kernels compile to what they compiled to without this file.  The host side (ffq_tables.h)
// reaches the kernels through the plain functions of ffq_umi_launch.h, whose types the kernels take as they are.
#pragma once
#include "ffq_umi_launch.h"
#include "ffq_render.h"
#include "ffq_umiwalk.h"

namespace ffq {

// (the boundary's types: a side -- buffer, bytes, sentinel, add, table, as PairSide of ffq_pair.h has them --, the rule, the counters)
typedef ::ffq_umi::Side UmiSide;
typedef ::ffq_umi::Arg UmiArg;
typedef ::ffq_umi::RenderCounts UmiRenderBlock;
static_assert(::ffq_umi::TAKE_WG == 256 && ::ffq_umi::RENDER_WG == RENDER_WG, "ffq_umi_launch.h");

constexpr int UMI_WG = 256;
constexpr int UMI_LONG = 4096;        // bases above which the take gives a row a wave of its own

// ---- the take ------------------------------------------------------------------------------------------------------------
// One row per group.  have: this group has a row (uniform in the group); defer_long: rows above UMI_LONG are left to the
// second launch (returned).
template <int G>
__device__ __forceinline__ bool umi_take_row(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                             const int64_t *__restrict__ table, int64_t *__restrict__ out, int64_t row, bool have,
                                             longlong2 r01, longlong2 r23, longlong2 r45, int len, int skip, bool defer_long, int gl,
                                             int gshift, RowCounts &cnt)
{
    int64_t p2 = 0, p4 = 0, n = 0;
    // both lines are read; the sequence line begins right behind the header's newline (a scanned, unwrapped record)
    const bool elig = have && row_pos<true, true>(nbytes, s, add, r23, r45, p2, p4, n) && (uint64_t)r23.x == (uint64_t)r01.y + 1u;
    const bool is_long = defer_long && elig && n > UMI_LONG;
    const bool live = elig && !is_long && n > 0;
    bool nl = false;
    rows_scan_nl<G>(d + (p2 - s), 0, n, live, gl, nl);
    rows_scan_nl<G>(d + (p4 - s), 0, n, live, gl, nl);
    const bool any_nl = group_any<G>(nl, gshift);
    const int64_t cut = umi_cut(n, len, skip);
    row_edit_finish(table, out, row, gl, have, is_long, elig && !any_nl, r01, r23, r45, make_longlong2(r23.x + cut, r23.y),
                    make_longlong2(r45.x + cut, r45.y), cut, cnt);
    return is_long;
}

__global__ __launch_bounds__(UMI_WG) void k_umi_take(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                     const int64_t *table, int64_t n_rows, int len, int skip, int64_t *out,
                                                     int64_t *__restrict__ long_list, RowsBlock *__restrict__ blk)
{
    constexpr int G = ROWS_G;
    const int lane = threadIdx.x & 63, gl = lane & (G - 1), gshift = lane & ~(G - 1);
    RowCounts cnt;
    constexpr int RPB = UMI_WG / G;
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
        const bool is_long = umi_take_row<G>(d, nbytes, s, add, table, out, row, row < n_rows, r01, r23, r45, len, skip, true, gl, gshift, cnt);
        const int64_t at = long_list_append(is_long && gl == 0, lane, &blk->n_long);
        if (at >= 0) long_list[at] = row;
    }
    cnt.add_to<UMI_WG>(blk);
}

// the rows k_umi_take left: a wave per row
__global__ __launch_bounds__(UMI_WG) void k_umi_take_long(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                          const int64_t *table, int len, int skip, int64_t *out,
                                                          const int64_t *__restrict__ long_list, RowsBlock *__restrict__ blk)
{
    const int lane = threadIdx.x & 63;
    RowCounts cnt;
    for (LongRows<UMI_WG, true> it((int64_t)blk->n_long, long_list, table); it.next();)
        umi_take_row<64>(d, nbytes, s, add, table, out, it.row, it.have, it.r01, it.r23, it.r45, len, skip, false, lane, 0, cnt);
    cnt.add_to<UMI_WG>(blk);
}

// ---- the tagged render ---------------------------------------------------------------------------------------------------
// (UmiRenderBlock: RenderBlock's counters and the rows that got a tag; UmiArg: the rule as the kernels take it, the literal --
// delim, prefix, '_' -- as five little-endian dwords: ffq_umi_launch.h)

// Row `row` of a source side carries a tag of `len` bytes: where the tag begins in S.d (>= 0); -1: it does not.
__device__ __forceinline__ int64_t umi_carrier(const UmiSide &S, int64_t row, int len)
{
    const int64_t c1 = row_coord(S.table[row * 6 + 1], S.add), c2 = row_coord(S.table[row * 6 + 2], S.add);
    if (!umi_carrier_pos(c1, c2, S.nbytes + S.s, len)) return -1;
    const int64_t a = c1 + 1 - S.s;                      // (>= 0 and a + len <= nbytes: umi_carrier_pos)
    bool nl = false;
    for (int t = 0; t < len; t += 16) {
        const uint4 x = load16_any(S.d, S.nbytes, a + t);
        nl |= umi_nl16(x.x, x.y, x.z, x.w, min(len - t, 16));
    }
    return nl ? -1 : a;
}

// rendered length of a row (0: not renderable), its slices, and -- tagged -- where the tags its source rows carry begin
__device__ __forceinline__ int64_t umi_row_len(const UmiSide &S0, const UmiSide &S1, const UmiSide &S2, const UmiArg &A, int64_t row,
                                               int64_t n_rows, RenderRow &R, int64_t &t1, int64_t &t2, bool &tagged)
{
    t1 = t2 = -1; tagged = false;
    const int64_t len = render_row_len(S0.table, row, n_rows, S0.nbytes, S0.s, S0.add, R);
    if (len == 0) return 0;
    bool ok = true;
    if (A.loc != UMI_READ2) { t1 = umi_carrier(S1, row, A.len); ok = t1 >= 0; }
    if (ok && A.loc != UMI_READ1) { t2 = umi_carrier(S2, row, A.len); ok = t2 >= 0; }
    tagged = ok;
    return len + (ok ? umi_ins_len(A.loc, A.len, A.prefix_len) : 0);
}

__global__ __launch_bounds__(RENDER_WG) void k_umi_render_sum(UmiSide S0, UmiSide S1, UmiSide S2, UmiArg A, int64_t n_rows, int64_t nblk,
                                                              long long *__restrict__ bsum, UmiRenderBlock *__restrict__ blk)
{
    unsigned int cnt = 0, tag = 0;
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
        const int64_t row = b * RENDER_WG + threadIdx.x;
        RenderRow R;
        int64_t t1, t2;
        bool tagged;
        const int64_t len = umi_row_len(S0, S1, S2, A, row, n_rows, R, t1, t2, tagged);
        int64_t tot;
        (void)wg_excl_scan<RENDER_WG, SCAN_ANY>(len, tot);
        if (threadIdx.x == 0) bsum[b] = tot;
        cnt += (unsigned int)__popcll(__ballot(len > 0));
        tag += (unsigned int)__popcll(__ballot(tagged));
        __syncthreads();                                    // (the scan's LDS is written again by the next block of rows)
    }
    // (the WAVE's counts, the same in all of its lanes: one lane hands them in)
    const bool first = (threadIdx.x & 63) == 0;
    const unsigned int c[2] = {first ? cnt : 0u, first ? tag : 0u};
    wg_counts_flush<RENDER_WG, 0, 2>(c, &blk->rendered);
}
static_assert(offsetof(UmiRenderBlock, tagged) == offsetof(UmiRenderBlock, rendered) + 16, "k_umi_render_sum: rendered, +2 words tagged");

// The header's first ' ' or '\t' (h if it has none), by a group of G lanes: sixteen bytes per lane and step.  live: the group has
// a row to look through (uniform in the group); every group of the wave steps along until the last one is done.
template <int G>
__device__ __forceinline__ int64_t umi_first_blank(const uint8_t *__restrict__ d, int64_t nbytes, int64_t hsrc, int64_t h, bool live, int gl)
{
    int64_t k = h;
    bool act = live;
    for (int64_t base = 0; __any(act); base += (int64_t)G * 16) {
        int key = G * 16;                                   // this lane's first blank as a place in the group's step
        const int64_t p = base + (int64_t)gl * 16;
        if (act && p < h) {
            const uint4 x = load16_any(d, nbytes, hsrc + p);
            const int f = umi_blank16(x.x, x.y, x.z, x.w, (int)min(h - p, (int64_t)16));
            if (f < 16) key = gl * 16 + f;
        }
        const int first = -RowGroup<G>::maxall(-key);
        if (act) {
            if (first < G * 16) { k = base + first; act = false; }
            else if (base + (int64_t)G * 16 >= h) act = false;
        }
    }
    return k;
}

// One TAGGED row by a group of G lanes, as render_copy: `o` = where the row's first byte goes, len its length (== the layout's).
template <int G>
__device__ __forceinline__ void umi_copy(const uint8_t *__restrict__ d, int64_t nbytes, const RenderRow &R, const uint8_t *__restrict__ d1,
                                         int64_t nb1, int64_t t1, const uint8_t *__restrict__ d2, int64_t nb2, int64_t t2, int64_t k,
                                         const UmiArg &A, const uint8_t *__restrict__ s_lit, int64_t len, uint8_t *__restrict__ o, int gl)
{
    constexpr int U = RENDER_U;
    const UmiLayout Y = umi_layout(R.h, k, R.s, R.q, A.loc, A.len, A.prefix_len);
    const int shift = (int)(reinterpret_cast<uintptr_t>(o) & 15);
    const int64_t nchunk = (len + shift + 15) >> 4;
    for (int64_t k0 = 0; k0 < nchunk; k0 += (int64_t)G * U) {
#pragma unroll
        for (int j = 0; j < U; j++) {
            const int64_t kc = k0 + (int64_t)j * G + gl;
            const int64_t clo = 16 * kc - shift;
            if (kc >= nchunk) continue;
            uint4 y = make_uint4(0, 0, 0, 0);
            int a, b;
            umi_span(1 - clo, k, a, b);
            if (b > a) y = render_merge(y, load16_any(d, nbytes, R.hsrc + (clo - 1)), a, b);
            umi_span(Y.o_t1 - clo, Y.t1_n, a, b);
            if (b > a) y = render_merge(y, load16_any(d1, nb1, t1 + (clo - Y.o_t1)), a, b);
            umi_span(Y.o_t2 - clo, Y.t2_n, a, b);
            if (b > a) y = render_merge(y, load16_any(d2, nb2, t2 + (clo - Y.o_t2)), a, b);
            umi_span(Y.o_tail - clo, Y.tail_n, a, b);
            if (b > a) y = render_merge(y, load16_any(d, nbytes, R.hsrc + k + (clo - Y.o_tail)), a, b);
            umi_span(Y.o_s - clo, R.s, a, b);
            if (b > a) y = render_merge(y, load16_any(d, nbytes, R.ssrc + (clo - Y.o_s)), a, b);
            umi_span(Y.o_q - clo, R.q, a, b);
            if (b > a) y = render_merge(y, load16_any(d, nbytes, R.qsrc + (clo - Y.o_q)), a, b);
            umi_span(Y.o_lit - clo, Y.lit_n, a, b);
            for (int t = a; t < b; t++) y = render_put(y, t, s_lit[t - (int)(Y.o_lit - clo)]);
            y = render_put(y, 0 - clo, '@');
            if (A.loc == UMI_PER_READ) y = render_put(y, Y.o_t2 - 1 - clo, '_');
            y = render_put(y, Y.o_s - 1 - clo, '\n');
            y = render_put(y, Y.o_p - clo, '\n');
            y = render_put(y, Y.o_p + 1 - clo, '+');
            y = render_put(y, Y.o_p + 2 - clo, '\n');
            y = render_put(y, len - 1 - clo, '\n');
            const int kb = (int)max(-clo, (int64_t)0), ke = (int)min(len - clo, (int64_t)16);
            uint8_t *dst = o + clo;                           // 16-byte aligned; only [kb, ke) of it is the row's
            if (kb == 0 && ke == 16) *reinterpret_cast<uint4 *>(dst) = y;
            else render_store_part(dst, y, kb, ke);
        }
    }
}

// the literal's bytes from the kernel's argument into LDS (the caller's barrier follows)
__device__ __forceinline__ void umi_lit_to_lds(const UmiArg &A, uint32_t *__restrict__ s_lit)
{
    if (threadIdx.x == 0) { s_lit[0] = A.lit[0]; s_lit[1] = A.lit[1]; s_lit[2] = A.lit[2]; s_lit[3] = A.lit[3]; s_lit[4] = A.lit[4]; }
}

// A workgroup per block of 256 rows.  total > out_cap: the offsets are written, the output is not touched.
__global__ __launch_bounds__(RENDER_WG) void k_umi_render_rows(UmiSide S0, UmiSide S1, UmiSide S2, UmiArg A, int64_t n_rows,
                                                               const long long *__restrict__ bbase, const DevRes *__restrict__ res,
                                                               uint8_t *__restrict__ out, int64_t out_cap, int64_t *__restrict__ off,
                                                               int64_t *__restrict__ long_list, UmiRenderBlock *__restrict__ blk)
{
    constexpr int G = RENDER_G, NG = RENDER_WG / G;
    __shared__ RenderRow s_row[RENDER_WG];
    __shared__ int64_t s_off[RENDER_WG], s_len[RENDER_WG], s_t1[RENDER_WG], s_t2[RENDER_WG];
    __shared__ uint8_t s_tag[RENDER_WG];
    __shared__ uint32_t s_lit[5];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * RENDER_WG;
    const int64_t total = res->n_qual_bytes;
    {
        RenderRow R;
        int64_t t1, t2;
        bool tagged;
        const int64_t len = umi_row_len(S0, S1, S2, A, r0 + tid, n_rows, R, t1, t2, tagged);
        int64_t tot;
        const int64_t at = bbase[blockIdx.x] + wg_excl_scan<RENDER_WG, SCAN_ANY>(len, tot);
        s_row[tid] = R; s_off[tid] = at; s_len[tid] = len; s_t1[tid] = t1; s_t2[tid] = t2; s_tag[tid] = tagged ? 1 : 0;
        if (off && r0 + tid < n_rows) off[r0 + tid] = at;
        if (blockIdx.x == 0 && tid == 0) {
            if (off) off[n_rows] = total;
            blk->total = (unsigned long long)total;
        }
        umi_lit_to_lds(A, s_lit);
    }
    __syncthreads();
    if (total > out_cap) return;
    const int g = tid / G, gl = tid & (G - 1), lane = tid & 63;
    // step i: group g has row i * NG + g of the block -- the thirty-two rows of a step are neighbours in the output
    for (int i = 0; i < G; i++) {
        const int r = i * NG + g;
        const int64_t len = s_len[r];
        const bool is_long = len > RENDER_LONG;
        const bool live = len > 0 && !is_long, tg = live && s_tag[r] != 0;
        const RenderRow R = s_row[r];
        const int64_t k = umi_first_blank<G>(S0.d, S0.nbytes, R.hsrc, R.h, tg, gl);
        if (live) {
            if (tg) umi_copy<G>(S0.d, S0.nbytes, R, S1.d, S1.nbytes, s_t1[r], S2.d, S2.nbytes, s_t2[r], k, A,
                                reinterpret_cast<const uint8_t *>(s_lit), len, out + s_off[r], gl);
            else render_copy<G>(S0.d, S0.nbytes, R, len, out + s_off[r], gl);
        }
        const int64_t e = long_list_append(is_long && gl == 0, lane, &blk->n_long);
        if (e >= 0) { long_list[2 * e] = r0 + r; long_list[2 * e + 1] = s_off[r]; }
    }
}

// the rows k_umi_render_rows left: a wave per row ((row, place in the output) pairs of the list)
__global__ __launch_bounds__(RENDER_WG) void k_umi_render_long(UmiSide S0, UmiSide S1, UmiSide S2, UmiArg A, int64_t n_rows,
                                                               uint8_t *__restrict__ out, const int64_t *__restrict__ long_list,
                                                               const UmiRenderBlock *__restrict__ blk)
{
    constexpr int WPB = RENDER_WG / 64;
    __shared__ uint32_t s_lit[5];
    umi_lit_to_lds(A, s_lit);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t n_long = (int64_t)blk->n_long;
    // (a wave's loop: its lanes have one row, so every step is the whole wave's)
    for (int64_t j = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6); j < n_long; j += (int64_t)gridDim.x * WPB) {
        const int64_t row = long_list[2 * j], at = long_list[2 * j + 1];
        RenderRow R;
        int64_t t1, t2;
        bool tagged;
        const int64_t len = umi_row_len(S0, S1, S2, A, row, n_rows, R, t1, t2, tagged);
        const int64_t k = umi_first_blank<64>(S0.d, S0.nbytes, R.hsrc, R.h, len > 0 && tagged, lane);
        if (len > 0) {
            if (tagged) umi_copy<64>(S0.d, S0.nbytes, R, S1.d, S1.nbytes, t1, S2.d, S2.nbytes, t2, k, A,
                                     reinterpret_cast<const uint8_t *>(s_lit), len, out + at, lane);
            else render_copy<64>(S0.d, S0.nbytes, R, len, out + at, lane);
        }
    }
}

}  // namespace ffq

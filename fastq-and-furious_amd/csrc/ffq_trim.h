// ffq_trim.h -- quality trimming by editing rows of the offset table (ffq_table_trim_quality).
//
// The reference's user guide names two uses of a table of positions (/root/reference/doc/user-guide.rst:196-204):
// deleting rows (ffq_table_select_seqlen) and MODIFYING them -- "trimming either end of the read could be done by
// ... modifying the values in a table of indices".  This is the second one, with the running-sum rule BWA and
// cutadapt use for -q.  For q[0..n) = buf[pos4:pos5], d(i) = cutoff - (q[i] - base):
//     5' end: walk i = 0 .. n-1, s += d(i); stop when s < 0; start = i + 1 at the FIRST maximum of s above 0
//     3' end: walk i = n-1 .. 0 with its own cutoff, independent of the 5' result; stop = i at the first maximum
//     start >= stop: the read is trimmed away (start = stop = 0)
// and the row becomes pos2 + start, pos2 + stop, pos4 + start, pos4 + stop.  A row is ELIGIBLE if its positions are
// (ffq_rows.h: row_pos) and no quality byte is '\n' (a wrapped record); any other row is copied unchanged and counted.
//
// Shape: the row frame of ffq_rows.h -- eight lanes per row; rows of more than TRIM_LONG quality bytes get a whole wave in
// the second launch, so that one long read does not hold back a wave of short ones.  The pass's own part is the walk.
// Either end is walked from the outside in, in chunks of G * B bytes (B consecutive bytes per lane, 8 or 16, as unaligned
// dwords: 64 bytes per short row and chunk); inside a chunk the lanes' sums of d are prefix-summed across the group, every
// lane steps through its B bytes, a ballot finds the first lane whose running sum went negative, and one max-reduction of
// (rise, position) the first maximum in front of it; (sum, best) are carried to the next chunk in 64 bits (a record of 2^31
// bytes of the lowest quality sums to 2^38), everything inside a chunk is 32-bit and relative to the carried sum.  An end is
// done when its sum has gone negative: on real reads that is the first chunk.  The eligibility rule needs every quality byte
// once, so the bytes between the two walks are then checked for '\n' 16 per lane -- for reads of a few hundred bases that is
// the same few 64-byte sectors the walks touch anyway.  No byte outside the row's own quality range, itself checked against
// the buffer, is read.
#pragma once
#include "ffq_rows.h"

namespace ffq {

constexpr int TRIM_LONG = 4096;       // quality bytes above which a row gets a wave of its own
constexpr int TRIM_WG = 256;
constexpr int TRIM_B = 8;             // bytes per lane and chunk of the short rows' kernel

// B bytes at a[0 .. B) as ints; only j in [jlo, jhi) are read, the others are -1
template <int B>
__device__ __forceinline__ void trim_load(const uint8_t *__restrict__ a, int jlo, int jhi, int (&qv)[B])
{
    if (jlo == 0 && jhi == B) {
#pragma unroll
        for (int w = 0; w < B / 4; w++) {
            const uint32_t x = *reinterpret_cast<const rows_u32u *>(a + 4 * w);
#pragma unroll
            for (int k = 0; k < 4; k++) qv[4 * w + k] = (int)((x >> (8 * k)) & 0xFFu);
        }
    } else {
#pragma unroll
        for (int j = 0; j < B; j++) qv[j] = (j >= jlo && j < jhi) ? (int)a[j] : -1;
    }
}

// This lane's B bytes of the chunk of walk positions [w0, w0 + G * B): walk position w is byte w of q[0 .. n) (front)
// or byte n - 1 - w (back); qv in ascending ADDRESS order, -1 where there is no byte (or the group is not active).
template <int G, int B, bool BACK>
__device__ __forceinline__ void trim_chunk(const uint8_t *__restrict__ q, int64_t n, bool act, int64_t w0, int gl, int (&qv)[B])
{
    const int64_t w = w0 + (int64_t)gl * B;           // this lane's first walk position
    const int avail = act ? (int)min(max(n - w, (int64_t)0), (int64_t)B) : 0;
    if (BACK) trim_load<B>(q + (n - w - B), B - avail, B, qv);
    else trim_load<B>(q + w, 0, avail, qv);
}

// One end of one row per group.  first: the end's first chunk (trim_chunk at w0 = 0), loaded by the caller together with
// the other end's so that a row whose walks end there -- nearly every one -- waits for memory once.
// cut = positions trimmed from this end, nread = positions [0, nread) were read, nl = one of them was '\n'.
// `live` is uniform inside a group; the loop is uniform over the wave (a finished group steps along with zeros).
template <int G, int B, bool BACK>
__device__ __forceinline__ void trim_walk(const uint8_t *__restrict__ q, int64_t n, bool live, int cutoff, int base,
                                          int gl, int gshift, const int (&first)[B], int64_t &cut, int64_t &nread, bool &nl)
{
    int64_t s = 0, best = 0, w0 = 0;
    cut = 0; nread = 0;
    bool act = live && n > 0;
    for (bool head = true; __any(act); head = false) {
        int qv[B];
        if (head) {
#pragma unroll
            for (int k = 0; k < B; k++) qv[k] = act ? first[k] : -1;
        } else
            trim_chunk<G, B, BACK>(q, n, act, w0, gl, qv);
        int d[B], t = 0;
#pragma unroll
        for (int k = 0; k < B; k++) {
            const int x = BACK ? qv[B - 1 - k] : qv[k];
            nl |= x == 10;
            d[k] = x < 0 ? 0 : cutoff + base - x;
            t += d[k];
        }
        const int incl = RowGroup<G>::incl_scan(t, gl);
        const int total = RowGroup<G>::sum(t);
        // relative to the carried sum s (>= 0 while the end is alive): dead when s + r < 0, a new maximum when s + r > best
        const int lim = (int)min(s, (int64_t)1 << 30);
        const int brel = (int)min(best - s, (int64_t)1 << 30);
        int r = incl - t, m = brel, mi = -1;
        bool ldead = false;
#pragma unroll
        for (int k = 0; k < B; k++) {
            r += d[k];
            if (!ldead) {
                if (r < -lim) ldead = true;
                else if (r > m) { m = r; mi = k; }
            }
        }
        const int fl = group_first<G>(__ballot(ldead), gshift);          // first lane that died; G: none
        // the first maximum in front of it: one max-reduction of (rise above best, C - 1 - position in the chunk) -- a
        // rise is below C * 382 < 2^19, so the key fits 32 bits; 0: no lane has a candidate
        constexpr int C = G * B, PB = C == 64 ? 6 : 10;
        static_assert(C == 64 || C == 1024, "the key of the first maximum is laid out for chunks of 64 or 1024 bytes");
        const bool cand = mi >= 0 && gl <= fl;
        const int gmax = RowGroup<G>::maxall(cand ? (((m - brel) << PB) | (C - 1 - (gl * B + mi))) : 0);
        if (act) {
            if (gmax > 0) { best = s + brel + (gmax >> PB); cut = w0 + (C - (gmax & (C - 1))); }
            s += total;
            w0 += (int64_t)G * B;
            nread = min(w0, n);
            act = fl == G && w0 < n;
        }
    }
}

// One row per group.  have: this group has a row (uniform in the group).  Returns through the references what lane 0
// of the group adds to the call's counters.  defer_long: rows above TRIM_LONG are left to the second launch (is_long).
template <int G, int B>
__device__ __forceinline__ bool trim_row(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                         const int64_t *__restrict__ table, int64_t *__restrict__ out, int64_t row,
                                         bool have, longlong2 r01, longlong2 r23, longlong2 r45, int base, int cf, int cb,
                                         bool defer_long, int gl, int gshift, RowCounts &cnt)
{
    bool is_long;
    int64_t p2 = 0, p4 = 0, n = 0;
    const bool elig = have && row_pos<false, true>(nbytes, s, add, r23, r45, p2, p4, n);
    is_long = defer_long && elig && n > TRIM_LONG;
    const bool live = elig && !is_long;
    const uint8_t *q = d + (p4 - s);

    // everything a row whose walks end in their first chunk needs, asked for at once: the first chunk of either end and
    // the next G * 16 bytes of what lies between them
    constexpr int C = G * B;
    int qf[B], qb[B];
    trim_chunk<G, B, false>(q, n, live && n > 0, 0, gl, qf);
    trim_chunk<G, B, true>(q, n, live && n > 0, 0, gl, qb);
    bool nl = false;
    if (live && C + (int64_t)gl * 16 < n - C) nl = rows_nl16(q, C + (int64_t)gl * 16, n - C);

    int64_t cutf = 0, cutb = 0, rf = 0, rb = 0;
    trim_walk<G, B, false>(q, n, live, cf, base, gl, gshift, qf, cutf, rf, nl);
    trim_walk<G, B, true>(q, n, live, cb, base, gl, gshift, qb, cutb, rb, nl);
    rows_scan_nl<G>(q, max(rf, (int64_t)(C + G * 16)), n - rb, live, gl, nl);
    const bool any_nl = group_first<G>(__ballot(nl), gshift) != G;

    int64_t start = cutf, stop = n - cutb;
    if (start >= stop) start = stop = 0;
    // (pos + start: the row's own coordinates, whatever `add` is)
    row_edit_finish(table, out, row, gl, have, is_long, elig && !any_nl, r01, r23, r45, make_longlong2(r23.x + start, r23.x + stop),
                    make_longlong2(r45.x + start, r45.x + stop), n - (stop - start), cnt);
    return is_long;
}

__global__ __launch_bounds__(TRIM_WG) void k_trim_rows(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                       const int64_t *table, int64_t n_rows, int base, int cf, int cb,
                                                       int64_t *out, int64_t *__restrict__ long_list,
                                                       RowsBlock *__restrict__ blk)
{
    constexpr int G = ROWS_G;
    const int lane = threadIdx.x & 63, gl = lane & (G - 1), gshift = lane & ~(G - 1);
    RowCounts cnt;
    constexpr int RPB = TRIM_WG / G;
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
        const bool is_long = trim_row<G, TRIM_B>(d, nbytes, s, add, table, out, row, row < n_rows, r01, r23, r45, base, cf, cb, true, gl,
                                                 gshift, cnt);
        const int64_t at = long_list_append(is_long && gl == 0, lane, &blk->n_long);
        if (at >= 0) long_list[at] = row;
    }
    cnt.add_to<TRIM_WG>(blk);
}

// the rows k_trim_rows left: sixteen bytes per lane and chunk
__global__ __launch_bounds__(TRIM_WG) void k_trim_long(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                       const int64_t *table, int base, int cf, int cb, int64_t *out,
                                                       const int64_t *__restrict__ long_list, RowsBlock *__restrict__ blk)
{
    const int lane = threadIdx.x & 63;
    RowCounts cnt;
    for (LongRows<TRIM_WG, true> it((int64_t)blk->n_long, long_list, table); it.next();)
        trim_row<64, 16>(d, nbytes, s, add, table, out, it.row, it.have, it.r01, it.r23, it.r45, base, cf, cb, false, lane, 0, cnt);
    cnt.add_to<TRIM_WG>(blk);
}

}  // namespace ffq

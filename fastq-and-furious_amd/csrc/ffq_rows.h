// ffq_rows.h -- the row frame of the passes over a device offset table: quality trim (ffq_trim.h), adapter trim
// (ffq_adapter.h), statistics (ffq_stats.h), content filter (ffq_filter.h), render (ffq_render.h).
//
// What the passes share:
//   the shape    workgroups stride over the table, a GROUP of ROWS_G = 8 lanes owns a row (WG / 8 rows per workgroup and step),
//                the next step's row is asked for before the current one is worked on; rows the pass calls long go onto a
//                list (long_list_append), and a second launch gives every listed row a whole wave (LongRows)
//   row_pos      a row's buffer coordinates and whether its positions make it eligible
//   row_edit_finish, RowCounts   what the two row-editing passes do with a row once they know its cut
//   wg_counts_flush, lds_hist_flush   how a pass's counts and LDS histograms leave: one set of atomics per workgroup
//   the small pieces: the unaligned dword, has_nl, wave_sum_u64, sums and maxima over a group, the newline looks
// Every loop over rows is uniform over the wave: every group of a wave takes a step as long as one of them has a row, `have`
// says whether this one does, and a group without a row -- or with a row that has nothing to do -- steps along.  What is done
// with a row may therefore use ballots, DPP moves and barriers; it must not leave a step for some lanes only.
// The strided walk of the four short-row kernels (k_trim_rows, k_adapter_rows, k_stats_rows, k_filter_rows) is NOT here: it stays written
// out in each of them.  Behind a shared function or iterator the compiler waited for the next row's prefetch before it asked for
// the current row's bytes, or spilled.
#pragma once
#include "ffq_dev.h"

namespace ffq {

constexpr int ROWS_G = 8;             // lanes per row of the short rows' kernels

typedef uint32_t rows_u32u __attribute__((aligned(1)));       // a dword at any address

// one of the four bytes of x is '\n'
__device__ __forceinline__ bool has_nl(uint32_t x)
{
    x ^= 0x0A0A0A0Au;
    return ((x - 0x01010101u) & ~x & 0x80808080u) != 0;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long x)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += (unsigned long long)__shfl_xor((long long)x, o);
    return x;
}

// ---- how a pass's counts leave ---------------------------------------------------------------------------------------------
// A lane's N counts c[] summed over the wave, over the workgroup's waves through LDS, and added to dst[] with one atomic per
// non-zero sum and WORKGROUP (device-wide atomics on a few addresses are served one at a time: DESIGN.md 4a, 4l).  Sum k goes
// to dst[k], or -- with an index list AT..., one entry per count -- to dst[AT[k]].
//   who calls it    every thread of the workgroup, once, at a point that is uniform over the workgroup: in front of it a
//                   kernel may return only with all of its threads (k_seqkey_long's `n_long == 0`)
//   what it costs   one barrier, and at most N atomics per workgroup; none for a sum of zero
// A lane's counters stay as narrow as they are in its loop, and T is their type (unsigned, 32 or 64 bits): a WAVE's sum crosses
// LDS as a T -- the lanes of a capped grid that count in 32 bits have waves that count far fewer than 2^32 --, the workgroup's
// sum has 64 bits.  Counters of both widths are widened in the array built for the call.  c[k] is a LANE's share: a value the
// whole wave already holds (a ballot's popcount) is handed in by one lane and as 0 by the others.  Hand in the counts there
// are and no zeros to fill gaps between destinations: a padded array costs a register and LDS.
template <int WG, int... AT, class T, int N>
__device__ __forceinline__ void wg_counts_flush(const T (&c)[N], unsigned long long *__restrict__ dst)
{
    static_assert(sizeof...(AT) == 0 || sizeof...(AT) == N, "one destination per count");
    __shared__ T s_cnt[WG / 64][N];
#pragma unroll
    for (int k = 0; k < N; k++) {
        const unsigned long long t = wave_sum_u64(c[k]);
        if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6][k] = (T)t;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < WG / 64; w++) t += s_cnt[w][threadIdx.x];
        [[maybe_unused]] int k = 0;
        int at = threadIdx.x;
        ((at = (int)threadIdx.x == k++ ? AT : at), ...);
        if (t) atomicAdd(&dst[at], t);
    }
}

// n 32-bit counters in LDS added to dst[0 .. n) with one 64-bit atomic per non-zero counter, and cleared if `clear`.  Every
// thread of the workgroup calls it; the barriers -- in front of it, and behind it before the counters are counted in again --
// are the caller's.
template <int WG>
__device__ __forceinline__ void lds_hist_flush(uint32_t *__restrict__ s, int n, unsigned long long *__restrict__ dst, bool clear = false)
{
    for (int i = threadIdx.x; i < n; i += WG) {
        const uint32_t x = s[i];
        if (clear) s[i] = 0;
        if (x) atomicAdd(&dst[i], (unsigned long long)x);
    }
}

// first lane of this lane's group whose bit is set in a wave ballot; G if none (gshift: the wave's lane of the group's first)
template <int G>
__device__ __forceinline__ int group_first(unsigned long long m, int gshift)
{
    if constexpr (G == 64) return m ? __builtin_ctzll(m) : 64;
    else {
        const uint32_t b = (uint32_t)(m >> gshift) & ((1u << G) - 1u);
        return b ? __builtin_ctz(b) : G;
    }
}

template <int G>
__device__ __forceinline__ bool group_any(bool x, int gshift) { return group_first<G>(__ballot(x), gshift) != G; }

// Sums and maxima across a group.  Eight lanes: DPP moves inside the 16-lane row (row_shr, quad_perm, row_half_mirror
// stay inside an aligned group of eight or are masked off by the lane's place in it) -- a VALU instruction each where a
// shuffle is an LDS round trip.  A whole wave: the library's DPP scan, xor shuffles.
template <int CTRL>
__device__ __forceinline__ int rows_dpp(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}

template <int G> struct RowGroup;

template <> struct RowGroup<8> {
    static __device__ __forceinline__ int incl_scan(int x, int gl)
    {
        x += rows_dpp<0x111>(x) & (gl >= 1 ? -1 : 0);       // row_shr:1
        x += rows_dpp<0x112>(x) & (gl >= 2 ? -1 : 0);       // row_shr:2
        x += rows_dpp<0x114>(x) & (gl >= 4 ? -1 : 0);       // row_shr:4
        return x;
    }
    static __device__ __forceinline__ int sum(int x)
    {
        x += rows_dpp<0xB1>(x);                             // quad_perm:[1,0,3,2]
        x += rows_dpp<0x4E>(x);                             // quad_perm:[2,3,0,1]
        x += rows_dpp<0x141>(x);                            // row_half_mirror: the other quad of the eight
        return x;
    }
    static __device__ __forceinline__ int maxall(int x)
    {
        x = max(x, rows_dpp<0xB1>(x));
        x = max(x, rows_dpp<0x4E>(x));
        x = max(x, rows_dpp<0x141>(x));
        return x;
    }
};

template <> struct RowGroup<64> {
    static __device__ __forceinline__ int incl_scan(int x, int) { return (int)wave_incl_scan((uint32_t)x); }
    static __device__ __forceinline__ int sum(int x)
    {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
        return x;
    }
    static __device__ __forceinline__ int maxall(int x)
    {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) x = max(x, __shfl_xor(x, o));
        return x;
    }
};

// '\n' among q[a .. min(a + 16, hi)), a < hi: sixteen bytes in one go; a piece cut short by hi is read as the sixteen
// bytes in front of hi instead (bytes of the same line: a newline there counts all the same)
__device__ __forceinline__ bool rows_nl16(const uint8_t *__restrict__ q, int64_t a, int64_t hi)
{
    bool nl = false;
    if (a + 16 > hi && hi < 16) {
        for (int64_t j = a; j < hi; j++) nl |= q[j] == 10;
        return nl;
    }
    const uint8_t *p = q + (a + 16 <= hi ? a : hi - 16);
#pragma unroll
    for (int k = 0; k < 4; k++) nl |= has_nl(*reinterpret_cast<const rows_u32u *>(p + 4 * k));
    return nl;
}

// '\n' among q[lo .. hi) (16 bytes per lane and step)
template <int G>
__device__ __forceinline__ void rows_scan_nl(const uint8_t *__restrict__ q, int64_t lo, int64_t hi, bool live, int gl, bool &nl)
{
    if (!live) return;
    for (int64_t w = lo + (int64_t)gl * 16; w < hi; w += (int64_t)G * 16) nl |= rows_nl16(q, w, hi);
}

// ---- a row's positions -----------------------------------------------------------------------------------------------------
// a table entry as a buffer coordinate (wrapping arithmetic: a row may hold anything)
__device__ __forceinline__ int64_t row_coord(long long pos, int64_t add) { return (int64_t)((uint64_t)pos - (uint64_t)add); }

// Coordinates of the sequence's and the quality's first byte (p2, p4), their common length n, and -- returned -- whether the
// positions make the row eligible: pos2..pos5 - add inside the buffer (s: it has a sentinel), in order, the two lines of one
// length.  Call it as `have && row_pos<..>(..)` with p2 = p4 = n = 0: a group without a row keeps the zeros.
//
// Coordinate 0 of a buffer with a sentinel is the virtual '\n': it is not in memory, so a pass may not READ it, and a line
// with bytes in it that begins there makes the row ineligible.  Only the lines a pass reads matter -- SEQ, QUAL say which:
// the quality trim reads the quality, the adapter trim the sequence, the statistics both.  (A line the pass does not read may
// begin at coordinate 0; an editing pass moves its ends like any other's.)
template <bool SEQ, bool QUAL>
__device__ __forceinline__ bool row_pos(int64_t nbytes, int s, int64_t add, longlong2 r23, longlong2 r45, int64_t &p2, int64_t &p4,
                                        int64_t &n)
{
    p2 = row_coord(r23.x, add);
    p4 = row_coord(r45.x, add);
    const int64_t p3 = row_coord(r23.y, add), p5 = row_coord(r45.y, add);
    const int64_t L = nbytes + s;
    n = p5 - p4;
    bool elig = p2 >= 0 && p4 >= 0 && p2 <= p3 && p4 <= p5 && p3 <= L && p5 <= L && p3 - p2 == n;
    if (elig && n > 0 && ((SEQ && p2 < s) || (QUAL && p4 < s))) elig = false;
    return elig;
}

// ---- the two launches ------------------------------------------------------------------------------------------------------
// The rows of a wave that are `mine` take their places on a list with one atomic on its counter; this lane's slot, -1 if
// it has none.  Every lane of the wave calls it.
__device__ __forceinline__ int64_t long_list_append(bool mine, int lane, unsigned long long *__restrict__ n_long)
{
    const unsigned long long lm = __ballot(mine);
    if (!lm) return -1;
    unsigned long long at = 0;
    if (lane == 0) at = atomicAdd(n_long, (unsigned long long)__popcll(lm));
    at = (unsigned long long)__shfl((long long)at, 0);
    return mine ? (int64_t)(at + __popcll(lm & ((1ull << lane) - 1ull))) : -1;
}

// The long rows' launch, a wave per entry of the list: `for (LongRows<WG, R01> it(n_long, long_list, table); it.next();)`.
// it.j: the wave's entry, it.row: its row; it.have: the entry exists and is not struck off (-1).  R01 false: the pass does
// not use pos0 / pos1, they are not loaded and it.r01 is zero.
template <int WG, bool R01>
struct LongRows {
    static constexpr int WPB = WG / 64;
    const int64_t *long_list, *table;
    int64_t n_long, j0, j, row;
    longlong2 r01, r23, r45;
    bool have;

    __device__ __forceinline__ LongRows(int64_t n_long_, const int64_t *long_list_, const int64_t *table_)
        : long_list(long_list_), table(table_), n_long(n_long_), j0((int64_t)blockIdx.x * WPB) {}
    __device__ __forceinline__ bool next()
    {
        if (j0 >= n_long) return false;
        j = j0 + (threadIdx.x >> 6);
        row = j < n_long ? long_list[j] : -1;
        have = row >= 0;
        r01 = r23 = r45 = make_longlong2(0, 0);
        if (have) {
            const longlong2 *src = reinterpret_cast<const longlong2 *>(table + row * 6);
            if constexpr (R01) r01 = src[0];
            r23 = src[1]; r45 = src[2];
        }
        j0 += (int64_t)gridDim.x * WPB;
        return true;
    }
};

// ---- what the row-editing passes share -------------------------------------------------------------------------------------
// counters of a call: rows changed, bases removed, rows skipped, rows on the long list
struct RowsBlock { unsigned long long changed, removed, skipped, n_long; };

// a lane's share of them
struct RowCounts {
    unsigned int changed = 0, skipped = 0;
    unsigned long long removed = 0;

    // every thread of the workgroup is here (wg_counts_flush)
    template <int WG>
    __device__ __forceinline__ void add_to(RowsBlock *__restrict__ blk) const
    {
        const unsigned long long c[3] = {changed, removed, skipped};
        wg_counts_flush<WG>(c, &blk->changed);
    }
};
static_assert(offsetof(RowsBlock, removed) == 8 && offsetof(RowsBlock, skipped) == 16, "RowCounts::add_to: changed, removed, skipped in a row");

// the 48 bytes of a row by the first three lanes of its group
__device__ __forceinline__ void row_store(int64_t *__restrict__ out, int64_t row, int gl, longlong2 a, longlong2 b, longlong2 c)
{
    longlong2 v = a;
    if (gl == 1) v = b;
    if (gl == 2) v = c;
    if (gl < 3) reinterpret_cast<longlong2 *>(out + row * 6)[gl] = v;
}

// The end of a row of an editing pass, by its group (gl: the lane's place in it).  Without a row, or with one left to the
// long rows' launch: nothing.  !ok (ineligible, or a newline was found): counted as skipped, the row as it was.  Otherwise
// the row with n23, n45, counted as changed if `removed` bases went.  The store rule: out of place every row is written, in
// place (out == table) only a changed one; the row's 48 bytes go out by the first three lanes of its group.
__device__ __forceinline__ void row_edit_finish(const int64_t *table, int64_t *__restrict__ out, int64_t row, int gl, bool have,
                                                bool is_long, bool ok, longlong2 r01, longlong2 r23, longlong2 r45,
                                                longlong2 n23, longlong2 n45, int64_t removed, RowCounts &cnt)
{
    if (!have || is_long) return;
    const bool ch = ok && removed != 0;
    if (gl == 0) {
        if (!ok) cnt.skipped++;
        if (ch) { cnt.changed++; cnt.removed += (unsigned long long)removed; }
    }
    if (!ok) { n23 = r23; n45 = r45; }
    if (ch || out != table) row_store(out, row, gl, r01, n23, n45);
}

}  // namespace ffq

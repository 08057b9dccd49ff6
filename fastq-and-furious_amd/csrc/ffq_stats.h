// ffq_stats.h -- per-cycle base and quality statistics of a read table, counted on the device (ffq_table_stats).
//
// What is counted, the layout of the words and the eligibility rule are stated in include/ffq.h.  Everything is an integer
// and every global update is an integer atomicAdd, so the result does not depend on the order rows arrive in.
//
// Shape (it differs from the trims' in two places, both said here).  Three launches on the context's stream:
//   k_stats_rows        the short rows' shape of ffq_rows.h, 64 rows per workgroup and step, 512 workgroups.  A row of up to STATS_TILE
//                       bases is held in REGISTERS: lane gl takes dwords gl, gl + 8, ... of the sequence and of the quality
//                       (five of either: every load of a row is in flight at once), the group looks for '\n' with one
//                       ballot -- eligibility has to be known before the first count --, and then counts out of the
//                       registers.  Longer rows go onto the list.
//   k_stats_long_check  a wave per listed row: walks the whole sequence and quality once for '\n' and for the per-read sums,
//                       counts the row's head and per-read histograms, and strikes an ineligible row off the list.
//   k_stats_long_count  a wave per listed row and CYCLE TILE (blockIdx.y): the per-cycle counts of cycles [y * STATS_TILE,
//                       (y + 1) * STATS_TILE) -- all C * 101 counters do not fit into LDS.  No byte at a cycle >= C is read.
//                       The first tile is counted here as well, so the short rows' kernel needs one tile only, and a row
//                       above STATS_TILE (not above a separate, larger threshold) is "long": at 153 bases a wave per row
//                       already has 39 lanes busy per step.
// Counters are 32-bit and workgroup-private in LDS: a cycle tile of STATS_TILE * (5 + 96) counters, the length histogram,
// the two per-read histograms.  They are flushed with one 64-bit atomicAdd per non-zero counter and workgroup (and round,
// below); the seven head counters are summed in registers and go out with one set of atomics per workgroup.  No global
// atomic per base, none per row.
//
// LDS addresses.  At a given cycle nearly every read has the same quality byte, so lanes that are on the same cycle at the
// same time serialise on one address.  Two things spread them: the lanes of a group are on cycles 4 apart (consecutive
// dwords), and the eight groups of a wave rotate the byte of the dword they start with (group g counts byte (j + g) & 3 in
// pass j), which leaves two groups per address where there were eight.  The quality counters of a cycle are STATS_QSTRIDE =
// 97 words apart in LDS, not 96: 96 is a multiple of the 32 banks, and all lanes of a wave would meet in one bank.
//
// Wrap.  A row adds at most 1 to any LDS counter (one class and one value per cycle, one bin per histogram), so a counter
// can wrap only after 2^32 rows of one workgroup.  Every kernel therefore works in rounds of at most STATS_ROUND steps of
// at most STATS_WG / STATS_G = 64 rows and flushes and clears its counters between rounds: STATS_ROUND * 64 = 2^26 < 2^32
// whatever n_rows and the table are (static_assert below).  The head sums are 64-bit, as are the words they are added to.
#pragma once
#include "ffq_rows.h"

namespace ffq {

constexpr int STATS_QBINS = 96, STATS_GCBINS = 101, STATS_HEAD = 8, STATS_MAX_CYCLES = 4096;
constexpr int STATS_TILE = 152;       // cycles per LDS tile; a row above it gets a wave of its own (151-base reads do not)
constexpr int STATS_WG = 512;
constexpr int STATS_G = ROWS_G;       // lanes per row of the short rows' kernel, a dword of either line each per step
constexpr int STATS_NS = (STATS_TILE + STATS_G * 4 - 1) / (STATS_G * 4);    // dwords per lane and line: 5
constexpr int STATS_QSTRIDE = 97;     // words between the quality counters of two cycles in LDS
constexpr int STATS_TILE_WORDS = STATS_TILE * (5 + STATS_QSTRIDE);
constexpr int64_t STATS_ROUND = (int64_t)1 << 20;     // steps between two flushes
static_assert((uint64_t)STATS_ROUND * (STATS_WG / STATS_G) < ((uint64_t)1 << 32),
              "a 32-bit LDS counter takes at most 1 per row: the rows of a round must stay below 2^32");
static_assert(STATS_NS * STATS_G * 4 >= STATS_TILE, "a short row fits the registers of its group");
static_assert((STATS_TILE_WORDS + STATS_TILE + 1 + STATS_QBINS + STATS_GCBINS) * 4 + (STATS_WG / 64) * 7 * 8 <= 65536,
              "k_stats_rows: the tile, the three histograms and the head sums are static LDS");

__host__ __device__ constexpr int64_t stats_words(int64_t C) { return 8 + C * 101 + (C + 1) + STATS_QBINS + STATS_GCBINS; }

typedef unsigned long long stats_u64;

// head sums of a lane: rows counted, rows skipped, bases, bases at cycles >= C, sum of v, GC bases, bases of class 4
struct StatsHead { stats_u64 v[7]; };

// bytes a[o .. min(o + 4, n)) as a dword, the missing ones 0; 0 <= o < n.  Reads inside a[0 .. n) only.
__device__ __forceinline__ uint32_t stats_ld(const uint8_t *__restrict__ a, int64_t o, int64_t n)
{
    if (o + 4 <= n) return *reinterpret_cast<const rows_u32u *>(a + o);
    if (n >= 4) return *reinterpret_cast<const rows_u32u *>(a + (n - 4)) >> (8 * (int)(o + 4 - n));
    uint32_t x = 0;
    for (int64_t j = o; j < n; j++) x |= (uint32_t)a[j] << (8 * (int)(j - o));
    return x;
}

// class of a base: A a / C c / G g / T t = 0..3, any other byte 4
__device__ __forceinline__ int stats_cls(uint32_t b)
{
    const uint32_t u = b & 0xDFu;
    return u == 0x41u ? 0 : u == 0x43u ? 1 : u == 0x47u ? 2 : u == 0x54u ? 3 : 4;
}

__device__ __forceinline__ int stats_qv(uint32_t b, int qbase)
{
    return min(max((int)b - qbase, 0), STATS_QBINS - 1);
}

// One byte pair at cycle t of the tile: the per-read sums, and -- in_tile: the cycle is below C and 0 <= t < STATS_TILE --
// the tile's two counters.
__device__ __forceinline__ void stats_count(uint32_t sb, uint32_t qb, int t, bool in_tile, int qbase,
                                            uint32_t *__restrict__ s_tile, int &sv, int &gc, int &nn)
{
    const int cls = stats_cls(sb), v = stats_qv(qb, qbase);
    sv += v;
    gc += (cls == 1 || cls == 2) ? 1 : 0;
    nn += cls == 4 ? 1 : 0;
    if (in_tile) {
        atomicAdd(&s_tile[t * 5 + cls], 1u);
        atomicAdd(&s_tile[STATS_TILE * 5 + t * STATS_QSTRIDE + v], 1u);
    }
}

// the counters of a cycle tile added to the block and cleared (every thread of the workgroup; barriers are the caller's)
__device__ __forceinline__ void stats_flush_tile(uint32_t *__restrict__ s_tile, int64_t tile_lo, int C, stats_u64 *__restrict__ out)
{
    for (int i = threadIdx.x; i < STATS_TILE * 5; i += STATS_WG) {
        const uint32_t x = s_tile[i];
        s_tile[i] = 0;
        const int64_t c = tile_lo + i / 5;
        if (x && c < C) atomicAdd(&out[8 + c * 5 + i % 5], (stats_u64)x);
    }
    for (int i = threadIdx.x; i < STATS_TILE * STATS_QSTRIDE; i += STATS_WG) {
        const uint32_t x = s_tile[STATS_TILE * 5 + i];
        s_tile[STATS_TILE * 5 + i] = 0;
        const int64_t c = tile_lo + i / STATS_QSTRIDE;
        const int v = i % STATS_QSTRIDE;
        if (x && c < C && v < STATS_QBINS) atomicAdd(&out[8 + (int64_t)C * 5 + c * STATS_QBINS + v], (stats_u64)x);
    }
}

// the three per-read histograms (n_len bins of the first) added to the block and cleared
__device__ __forceinline__ void stats_flush_reads(uint32_t *__restrict__ s_len, int n_len, uint32_t *__restrict__ s_rq,
                                                  uint32_t *__restrict__ s_gc, int C, stats_u64 *__restrict__ out)
{
    lds_hist_flush<STATS_WG>(s_len, n_len, out + 8 + (int64_t)C * 101, true);
    lds_hist_flush<STATS_WG>(s_rq, STATS_QBINS, out + 8 + (int64_t)C * 102 + 1, true);
    lds_hist_flush<STATS_WG>(s_gc, STATS_GCBINS, out + 8 + (int64_t)C * 102 + 1 + STATS_QBINS, true);
}

// once per step of the three kernels, by every thread of the workgroup: every STATS_ROUND steps the workgroup flushes its counters (Wrap, above)
struct StatsRound {
    int64_t in_round = 0;
    template <class Flush>
    __device__ __forceinline__ void step(Flush flush)
    {
        if (++in_round == STATS_ROUND) {
            in_round = 0;
            __syncthreads();
            flush();
            __syncthreads();
        }
    }
};

// every thread of the workgroup is here: the seven head sums to out[0 .. 7) (wg_counts_flush)
__device__ __forceinline__ void stats_add_head(stats_u64 *__restrict__ out, const StatsHead &h) { wg_counts_flush<STATS_WG>(h.v, out); }

// the per-read counts of one eligible row of n bases (one lane of its group or wave); T: wide enough for 100 * n
template <class T>
__device__ __forceinline__ void stats_read(StatsHead &h, int64_t n, int C, T sv, T gc, T nn,
                                           uint32_t *__restrict__ s_len, uint32_t *__restrict__ s_rq, uint32_t *__restrict__ s_gc)
{
    h.v[0]++;
    h.v[2] += (stats_u64)n;
    h.v[3] += (stats_u64)max(n - (int64_t)C, (int64_t)0);
    h.v[4] += sv; h.v[5] += gc; h.v[6] += nn;
    atomicAdd(&s_len[(int)min(n, (int64_t)C)], 1u);
    if (n > 0) {
        atomicAdd(&s_rq[(int)(sv / (T)n)], 1u);
        atomicAdd(&s_gc[(int)(((T)100 * gc) / (T)n)], 1u);
    }
}

// (four waves per SIMD asked for: two workgroups then fit a CU -- their LDS allows it -- at the price of 128 VGPRs and a
// spill of two dozen of them; one workgroup per CU with 157 VGPRs took 1.40 ms where this takes 1.03 on the table of DESIGN.md 4d)
// (the strided walk is written out, as in the two trims, without pos0 / pos1: ffq_rows.h says why)
__global__ __launch_bounds__(STATS_WG, 4) void k_stats_rows(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                         const int64_t *__restrict__ table, int64_t n_rows, int qbase, int C,
                                                         stats_u64 *__restrict__ out, int64_t *__restrict__ long_list,
                                                         RowsBlock *__restrict__ blk)
{
    constexpr int G = STATS_G;
    __shared__ uint32_t s_tile[STATS_TILE_WORDS];
    __shared__ uint32_t s_len[STATS_TILE + 1], s_rq[STATS_QBINS], s_gc[STATS_GCBINS];
    const int lane = threadIdx.x & 63, gl = lane & (G - 1), gshift = lane & ~(G - 1), rot = (lane / G) & 3;
    for (int i = threadIdx.x; i < STATS_TILE_WORDS; i += STATS_WG) s_tile[i] = 0;
    for (int i = threadIdx.x; i < STATS_TILE + 1; i += STATS_WG) s_len[i] = 0;
    if (threadIdx.x < STATS_QBINS) s_rq[threadIdx.x] = 0;
    if (threadIdx.x < STATS_GCBINS) s_gc[threadIdx.x] = 0;
    __syncthreads();

    StatsHead h;
#pragma unroll
    for (int k = 0; k < 7; k++) h.v[k] = 0;
    auto flush = [&] {
        stats_flush_tile(s_tile, 0, C, out);
        // (a row of this kernel has min(n, C) <= STATS_TILE; bins above C stay 0)
        stats_flush_reads(s_len, min(STATS_TILE, C) + 1, s_rq, s_gc, C, out);
    };
    StatsRound round;
    constexpr int RPB = STATS_WG / G;
    const int64_t step = (int64_t)gridDim.x * RPB;
    longlong2 x23 = make_longlong2(0, 0), x45 = x23;
    {
        const int64_t row = (int64_t)blockIdx.x * RPB + (threadIdx.x / G);
        if (row < n_rows) {
            const longlong2 *src = reinterpret_cast<const longlong2 *>(table + row * 6);
            x23 = src[1]; x45 = src[2];
        }
    }
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < n_rows; r0 += step) {
        const int64_t row = r0 + (threadIdx.x / G);
        const bool have = row < n_rows;
        const longlong2 r23 = x23, r45 = x45;
        if (row + step < n_rows) {
            const longlong2 *src = reinterpret_cast<const longlong2 *>(table + (row + step) * 6);
            x23 = src[1]; x45 = src[2];
        }
        int64_t p2 = 0, p4 = 0, n = 0;
        const bool elig = have && row_pos<true, true>(nbytes, s, add, r23, r45, p2, p4, n);
        const bool is_long = elig && n > STATS_TILE;
        const bool live = elig && !is_long;
        const uint8_t *sq = d + (p2 - s), *qq = d + (p4 - s);
        // the whole row into registers, every load asked for at once
        uint32_t xs[STATS_NS], xq[STATS_NS];
        bool nl = false;
#pragma unroll
        for (int k = 0; k < STATS_NS; k++) {
            const int o = (k * G + gl) * 4;
            xs[k] = 0; xq[k] = 0;
            if (live && o < n) { xs[k] = stats_ld(sq, o, n); xq[k] = stats_ld(qq, o, n); }
        }
#pragma unroll
        for (int k = 0; k < STATS_NS; k++) nl |= has_nl(xs[k]) || has_nl(xq[k]);
        const bool count = live && !group_any<G>(nl, gshift);
        int sv = 0, gc = 0, nn = 0;
#pragma unroll
        for (int k = 0; k < STATS_NS; k++) {
            const int o = (k * G + gl) * 4;
            const int cnt = count ? min(max((int)n - o, 0), 4) : 0;
#pragma unroll
            for (int jj = 0; jj < 4; jj++) {
                const int j = (jj + rot) & 3;
                // (o + j < n <= STATS_TILE: inside the tile)
                if (j < cnt) stats_count((xs[k] >> (8 * j)) & 0xFFu, (xq[k] >> (8 * j)) & 0xFFu, o + j, o + j < C, qbase, s_tile, sv, gc, nn);
            }
        }
        // (uniform over the wave: a group without a row sums zeros)
        sv = RowGroup<G>::sum(sv); gc = RowGroup<G>::sum(gc); nn = RowGroup<G>::sum(nn);
        if (gl == 0 && have && !is_long) {
            if (count) stats_read<uint32_t>(h, n, C, (uint32_t)sv, (uint32_t)gc, (uint32_t)nn, s_len, s_rq, s_gc);
            else h.v[1]++;
        }
        const int64_t at = long_list_append(is_long && gl == 0, lane, &blk->n_long);
        if (at >= 0) long_list[at] = row;
        round.step(flush);
    }
    __syncthreads();
    flush();
    stats_add_head(out, h);
}

// the rows k_stats_rows left: a wave per row walks both lines once -- '\n' anywhere makes the row ineligible (struck off
// the list: -1), any other row is counted in the head and in the per-read histograms
__global__ __launch_bounds__(STATS_WG) void k_stats_long_check(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                               const int64_t *__restrict__ table, int qbase, int C,
                                                               stats_u64 *__restrict__ out, int64_t *__restrict__ long_list,
                                                               const RowsBlock *__restrict__ blk)
{
    const int64_t n_long = (int64_t)blk->n_long;
    if (n_long == 0) return;
    __shared__ uint32_t s_len[STATS_MAX_CYCLES + 1], s_rq[STATS_QBINS], s_gc[STATS_GCBINS];
    for (int i = threadIdx.x; i < C + 1; i += STATS_WG) s_len[i] = 0;
    if (threadIdx.x < STATS_QBINS) s_rq[threadIdx.x] = 0;
    if (threadIdx.x < STATS_GCBINS) s_gc[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    StatsHead h;
#pragma unroll
    for (int k = 0; k < 7; k++) h.v[k] = 0;
    auto flush = [&] { stats_flush_reads(s_len, C + 1, s_rq, s_gc, C, out); };
    StatsRound round;
    for (LongRows<STATS_WG, false> it(n_long, long_list, table); it.next(); round.step(flush)) {
        if (!it.have) continue;                             // (uniform over the wave)
        int64_t p2, p4, n;
        const bool elig = row_pos<true, true>(nbytes, s, add, it.r23, it.r45, p2, p4, n);
        const uint8_t *sq = d + (p2 - s), *qq = d + (p4 - s);
        bool nl = false;
        stats_u64 sv = 0, gc = 0, nn = 0;
        if (elig) {
            for (int64_t o = (int64_t)lane * 4; o < n; o += 256) {
                const uint32_t a = stats_ld(sq, o, n), b = stats_ld(qq, o, n);
                nl |= has_nl(a) || has_nl(b);
                const int cnt = (int)min(n - o, (int64_t)4);
                int v1 = 0, g1 = 0, n1 = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (k < cnt) {
                        const int cls = stats_cls((a >> (8 * k)) & 0xFFu);
                        v1 += stats_qv((b >> (8 * k)) & 0xFFu, qbase);
                        g1 += (cls == 1 || cls == 2) ? 1 : 0;
                        n1 += cls == 4 ? 1 : 0;
                    }
                }
                sv += (stats_u64)v1; gc += (stats_u64)g1; nn += (stats_u64)n1;
            }
        }
        const bool bad = !elig || __ballot(nl) != 0;
        sv = wave_sum_u64(sv); gc = wave_sum_u64(gc); nn = wave_sum_u64(nn);
        if (lane == 0) {
            if (bad) { h.v[1]++; long_list[it.j] = -1; }
            else stats_read<stats_u64>(h, n, C, sv, gc, nn, s_len, s_rq, s_gc);
        }
    }
    __syncthreads();
    flush();
    stats_add_head(out, h);
}

// the per-cycle counts of the rows the check left on the list: a wave per row, cycle tile blockIdx.y
__global__ __launch_bounds__(STATS_WG) void k_stats_long_count(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                               const int64_t *__restrict__ table, int qbase, int C,
                                                               stats_u64 *__restrict__ out, const int64_t *__restrict__ long_list,
                                                               const RowsBlock *__restrict__ blk)
{
    const int64_t n_long = (int64_t)blk->n_long;
    if (n_long == 0) return;
    __shared__ uint32_t s_tile[STATS_TILE_WORDS];
    for (int i = threadIdx.x; i < STATS_TILE_WORDS; i += STATS_WG) s_tile[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t tile_lo = (int64_t)blockIdx.y * STATS_TILE;
    const int64_t tile_hi = min(tile_lo + STATS_TILE, (int64_t)C);
    auto flush = [&] { stats_flush_tile(s_tile, tile_lo, C, out); };
    StatsRound round;
    for (LongRows<STATS_WG, false> it(n_long, long_list, table); it.next(); round.step(flush)) {
        int64_t p2 = 0, p4 = 0, n = 0;
        if (!it.have || !row_pos<true, true>(nbytes, s, add, it.r23, it.r45, p2, p4, n)) continue;
        const uint8_t *sq = d + (p2 - s), *qq = d + (p4 - s);
        const int64_t hi = min(n, tile_hi);
        // (STATS_TILE is below 256: one dword per lane covers the tile)
        const int64_t o = tile_lo + (int64_t)lane * 4;
        if (o < hi) {
            // bytes behind hi but inside the row may be loaded with the dword; they are not counted
            const uint32_t a = stats_ld(sq, o, n), b = stats_ld(qq, o, n);
            const int cnt = (int)min(hi - o, (int64_t)4);
            int sv = 0, gc = 0, nn = 0;
#pragma unroll
            for (int k = 0; k < 4; k++)
                // (o + k < hi <= min(C, tile_lo + STATS_TILE))
                if (k < cnt) stats_count((a >> (8 * k)) & 0xFFu, (b >> (8 * k)) & 0xFFu, lane * 4 + k, true, qbase, s_tile, sv, gc, nn);
        }
    }
    __syncthreads();
    flush();
}
static_assert(STATS_TILE <= 256, "k_stats_long_count: a dword per lane covers a cycle tile");

}  // namespace ffq

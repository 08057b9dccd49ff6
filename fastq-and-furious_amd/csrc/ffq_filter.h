// ffq_filter.h -- rows of a read table kept or dropped for what is IN the read (ffq_table_select_reads): number of Ns, mean
// quality, share of unqualified bases, expected errors, complexity.  The rule, the order of its tests and what the eight
// counts mean are stated in include/ffq.h.  Everything is an integer; rows are independent.
//
// Shape: the two launches of ffq_rows.h that judge, and the compaction (ffq_compact.h) behind them.
//   k_filter_rows     the short rows' shape, 32 rows per workgroup and step.  The length test comes first and needs the row's
//                     positions only: a row that fails it has none of its bytes loaded.  A row of up to FILTER_TILE bases is
//                     held in registers the way k_stats_rows holds it (lane gl: dwords gl, gl + 8, ... of either line, every
//                     load in flight at once), the group looks for '\n' with one ballot -- eligibility has to be known
//                     before anything counts --, the five quantities are per-lane partial sums added over the group with DPP
//                     moves.  Longer rows go onto the list.
//   k_filter_long     a wave per listed row, 256 bytes of either line per step, 64-bit sums.
//   The compaction behind them is ffq_compact.h's, with "kept" read from the verdict bytes (KeepVerdict).
// Both judging kernels write ONE BYTE per row, the verdict: bits 0..2 the rule that dropped the row (0: kept), bit 7 "not
// judged by content".  The counts are summed in registers, over the wave, over the workgroup's waves through LDS, and go out
// with one set of atomics per workgroup.
//
// The pair seq[i] != seq[i + 1] crosses dwords and lanes.  The byte behind a lane's dword is the first byte of the next
// dword of the row, which another lane of the group holds in a register: lane gl + 1 in the same round (row_shl:1), or, for
// the group's last lane, lane 0 in the next round (row_shr:7).  Two DPP moves per round, no second load.  In the long rows'
// kernel the neighbour is the next lane of the wave (a shuffle), and the pair between the wave's last byte of a step and the
// first of the next is counted by lane 0 in that next step, from the dword lane 63 held.
//
// FFQ_EE_MICRO is read from LDS: the lanes of a wave look up 64 different qualities at once, which a constant (scalar) load
// would serve one lane at a time and a global load would send through the vector cache beside the row bytes; the 96 words
// are copied into LDS once per workgroup, and the quality values a file really holds (some forty of them) fall into
// different banks.
#pragma once
#include "ffq_rows.h"
#include "ffq_stats.h"

namespace ffq {

constexpr int FILTER_COUNTS = 8;
constexpr int FILTER_WG = 256;
constexpr int FILTER_G = ROWS_G;                                  // lanes per row, a dword of either line each per round
constexpr int FILTER_NS = 5;                                      // rounds: dwords per lane and line
constexpr int FILTER_TILE = FILTER_NS * FILTER_G * 4;             // 160: a row above it gets a wave of its own
constexpr uint32_t FILTER_REASON = 0x07u, FILTER_NOT_JUDGED = 0x80u;     // the verdict byte

// floor(1e6 * 10^(-v / 10) + 0.5), v = 0..95 (include/ffq.h)
#define FFQ_EE_MICRO_VALUES                                                                                              \
    1000000, 794328, 630957, 501187, 398107, 316228, 251189, 199526, 158489, 125893, 100000, 79433, 63096, 50119, 39811,  \
    31623, 25119, 19953, 15849, 12589, 10000, 7943, 6310, 5012, 3981, 3162, 2512, 1995, 1585, 1259, 1000, 794, 631, 501,  \
    398, 316, 251, 200, 158, 126, 100, 79, 63, 50, 40, 32, 25, 20, 16, 13, 10, 8, 6, 5, 4, 3, 3, 2, 2, 1, 1, 1, 1, 1,     \
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0
__device__ const uint32_t FILTER_EE_MICRO[STATS_QBINS] = {FFQ_EE_MICRO_VALUES};

// the content rules as the kernels take them (ffq_content_rules, checked)
struct FilterRules {
    int qual_base, max_n, min_mean_qual, qualified_qual, max_unqualified_pct, min_complexity_pct;
    long long max_ee_micro;
};

// counters of a call: the eight counts of include/ffq.h, rows on the long list
struct FilterBlock { unsigned long long cnt[FILTER_COUNTS], n_long; };

// Rules 2 to 6 on the five quantities of an eligible row of n bases; 0: kept.  (n is at most the buffer's size: the
// products, and ee <= 1e6 * n, stay inside 64 bits for any buffer a device holds.)
__device__ __forceinline__ uint32_t filter_verdict(const FilterRules &R, int64_t n, int64_t nN, int64_t sv, int64_t u, int64_t ee, int64_t d)
{
    if (R.max_n >= 0 && nN > (int64_t)R.max_n) return 2;
    if (R.min_mean_qual > 0 && sv < (int64_t)R.min_mean_qual * n) return 3;
    if (R.max_unqualified_pct >= 0 && 100 * u > (int64_t)R.max_unqualified_pct * n) return 4;
    if (R.max_ee_micro >= 0 && ee > (int64_t)R.max_ee_micro) return 5;
    if (R.min_complexity_pct > 0 && n >= 2 && 100 * d < (int64_t)R.min_complexity_pct * (n - 1)) return 6;
    return 0;
}

// a lane's share of the counts: one row's verdict byte added
struct FilterCounts {
    unsigned int c[FILTER_COUNTS] = {0, 0, 0, 0, 0, 0, 0, 0};

    __device__ __forceinline__ void add(uint32_t verdict)
    {
        const uint32_t r = verdict & FILTER_REASON;
#pragma unroll
        for (uint32_t k = 0; k < 7; k++) c[k] += r == k ? 1u : 0u;
        c[7] += (verdict & FILTER_NOT_JUDGED) ? 1u : 0u;
    }

    // every thread of the workgroup is here (wg_counts_flush; widened for it: handed in as 32-bit counts, k_filter_rows took
    // 97 VGPRs where it takes 96 -- four waves a SIMD where there are five)
    template <int WG>
    __device__ __forceinline__ void add_to(FilterBlock *__restrict__ blk) const
    {
        unsigned long long w[FILTER_COUNTS];
#pragma unroll
        for (int k = 0; k < FILTER_COUNTS; k++) w[k] = c[k];
        wg_counts_flush<WG>(w, blk->cnt);
    }
};

// the quantities of the cnt bytes of a sequence dword and a quality dword, and of the cntd pairs that begin in the
// sequence dword (y: the sequence one byte on)
__device__ __forceinline__ void filter_dword(uint32_t a, uint32_t y, uint32_t b, int cnt, int cntd, const FilterRules &R,
                                             const uint32_t *__restrict__ s_ee, int &nN, int &sv, int &u, int &ee, int &dd)
{
    const uint32_t z = a ^ y;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int v = stats_qv((b >> (8 * j)) & 0xFFu, R.qual_base);
        if (j < cnt) {
            nN += ((a >> (8 * j)) & 0xDFu) == 0x4Eu ? 1 : 0;
            sv += v;
            u += v < R.qualified_qual ? 1 : 0;
            ee += (int)s_ee[v];
        }
        if (j < cntd) dd += ((z >> (8 * j)) & 0xFFu) ? 1 : 0;
    }
}

// (the strided walk is written out, as in k_stats_rows, without pos0 / pos1: ffq_rows.h says why)
__global__ __launch_bounds__(FILTER_WG) void k_filter_rows(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                           const int64_t *__restrict__ table, int64_t n_rows, int64_t lo, int64_t hi,
                                                           FilterRules R, uint8_t *__restrict__ verdict,
                                                           int64_t *__restrict__ long_list, FilterBlock *__restrict__ blk)
{
    constexpr int G = FILTER_G;
    __shared__ uint32_t s_ee[STATS_QBINS];
    if (threadIdx.x < STATS_QBINS) s_ee[threadIdx.x] = FILTER_EE_MICRO[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, gl = lane & (G - 1), gshift = lane & ~(G - 1);
    FilterCounts cnt;
    constexpr int RPB = FILTER_WG / G;
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
        // rule 1, on the positions as they stand (ffq_table_select_seqlen's test)
        const int64_t len = (int64_t)((uint64_t)r23.y - (uint64_t)r23.x);
        const bool len_ok = have && len >= lo && len <= hi;
        int64_t p2 = 0, p4 = 0, n = 0;
        const bool pos_ok = have && row_pos<true, true>(nbytes, s, add, r23, r45, p2, p4, n);
        const bool is_long = len_ok && pos_ok && n > FILTER_TILE;
        const bool live = len_ok && pos_ok && !is_long;
        const uint8_t *sq = d + (p2 - s), *qq = d + (p4 - s);
        // the whole row into registers, every load asked for at once
        uint32_t xs[FILTER_NS], xq[FILTER_NS];
        bool nl = false;
#pragma unroll
        for (int k = 0; k < FILTER_NS; k++) {
            const int o = (k * G + gl) * 4;
            xs[k] = 0; xq[k] = 0;
            if (live && o < n) { xs[k] = stats_ld(sq, o, n); xq[k] = stats_ld(qq, o, n); }
        }
#pragma unroll
        for (int k = 0; k < FILTER_NS; k++) nl |= has_nl(xs[k]) || has_nl(xq[k]);
        const bool judged = live && !group_any<G>(nl, gshift);
        int nN = 0, sv = 0, u = 0, ee = 0, dd = 0;
#pragma unroll
        for (int k = 0; k < FILTER_NS; k++) {
            const int o = (k * G + gl) * 4;
            // the first byte of the row's next dword: lane gl + 1's of this round, or (last lane) lane 0's of the next
            const uint32_t same = (uint32_t)rows_dpp<0x101>((int)xs[k]);                                  // row_shl:1
            const uint32_t next = (uint32_t)rows_dpp<0x117>((int)xs[k + 1 < FILTER_NS ? k + 1 : k]);     // row_shr:7
            // (behind the last round's last dword there is no byte of a short row: c2 leaves that pair out)
            const uint32_t nb = gl == G - 1 ? next : same;
            const int c1 = judged ? min(max((int)n - o, 0), 4) : 0;
            const int c2 = judged ? min(max((int)n - 1 - o, 0), 4) : 0;
            filter_dword(xs[k], (xs[k] >> 8) | (nb << 24), xq[k], c1, c2, R, s_ee, nN, sv, u, ee, dd);
        }
        // (uniform over the wave: a group without a row sums zeros; ee <= 160 * 1e6 fits an int)
        nN = RowGroup<G>::sum(nN); sv = RowGroup<G>::sum(sv); u = RowGroup<G>::sum(u); ee = RowGroup<G>::sum(ee); dd = RowGroup<G>::sum(dd);
        if (gl == 0 && have && !is_long) {
            uint32_t v;
            if (!len_ok) v = 1u | (pos_ok ? 0u : FILTER_NOT_JUDGED);
            else if (!judged) v = FILTER_NOT_JUDGED;
            else v = filter_verdict(R, n, nN, sv, u, ee, dd);
            verdict[row] = (uint8_t)v;
            cnt.add(v);
        }
        const int64_t at = long_list_append(is_long && gl == 0, lane, &blk->n_long);
        if (at >= 0) long_list[at] = row;
    }
    cnt.add_to<FILTER_WG>(blk);
}
static_assert((int64_t)FILTER_TILE * 1000000 < ((int64_t)1 << 31), "k_filter_rows: a short row's sums are ints");

// the rows k_filter_rows left (they passed the length test and their positions are in order): a wave per row
__global__ __launch_bounds__(FILTER_WG) void k_filter_long(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                           const int64_t *__restrict__ table, FilterRules R,
                                                           uint8_t *__restrict__ verdict, const int64_t *__restrict__ long_list,
                                                           FilterBlock *__restrict__ blk)
{
    const int64_t n_long = (int64_t)blk->n_long;
    if (n_long == 0) return;
    __shared__ uint32_t s_ee[STATS_QBINS];
    if (threadIdx.x < STATS_QBINS) s_ee[threadIdx.x] = FILTER_EE_MICRO[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    FilterCounts cnt;
    for (LongRows<FILTER_WG, false> it(n_long, long_list, table); it.next();) {
        if (!it.have) continue;                             // (uniform over the wave)
        int64_t p2, p4, n;
        const bool elig = row_pos<true, true>(nbytes, s, add, it.r23, it.r45, p2, p4, n);
        const uint8_t *sq = d + (p2 - s), *qq = d + (p4 - s);
        bool nl = false;
        unsigned long long nN = 0, sv = 0, u = 0, ee = 0, dd = 0;
        uint32_t held = 0;                                  // the dword lane 63 held in the step before
        if (elig) {
            for (int64_t base = 0; base < n; base += 256) {        // (uniform over the wave: shuffles inside)
                const int64_t o = base + (int64_t)lane * 4;
                uint32_t a = 0, b = 0;
                if (o < n) { a = stats_ld(sq, o, n); b = stats_ld(qq, o, n); }
                nl |= has_nl(a) || has_nl(b);
                const uint32_t nb = (uint32_t)__shfl_down((int)a, 1);
                const int c1 = (int)min(max(n - o, (int64_t)0), (int64_t)4);
                // lane 63's last pair ends in the next step's first byte: lane 0 counts it there
                const int c2 = min((int)min(max(n - 1 - o, (int64_t)0), (int64_t)4), lane == 63 ? 3 : 4);
                int n1 = 0, v1 = 0, u1 = 0, e1 = 0, d1 = 0;
                filter_dword(a, (a >> 8) | (nb << 24), b, c1, c2, R, s_ee, n1, v1, u1, e1, d1);
                if (lane == 0 && base > 0) d1 += (held >> 24) != (a & 0xFFu) ? 1 : 0;
                held = (uint32_t)__shfl((int)a, 63);
                nN += (unsigned long long)n1; sv += (unsigned long long)v1; u += (unsigned long long)u1;
                ee += (unsigned long long)e1; dd += (unsigned long long)d1;
            }
        }
        const bool judged = elig && __ballot(nl) == 0;
        nN = wave_sum_u64(nN); sv = wave_sum_u64(sv); u = wave_sum_u64(u); ee = wave_sum_u64(ee); dd = wave_sum_u64(dd);
        if (lane == 0) {
            const uint32_t v = judged ? filter_verdict(R, n, (int64_t)nN, (int64_t)sv, (int64_t)u, (int64_t)ee, (int64_t)dd) : FILTER_NOT_JUDGED;
            verdict[it.row] = (uint8_t)v;
            cnt.add(v);
        }
    }
    cnt.add_to<FILTER_WG>(blk);
}

}  // namespace ffq

// ffq_overlap.h -- the overlap of the two mates of a pair: insert sizes, and adapters cut without naming them
// (ffq_table_pair_overlap; include/ffq.h states the rule).
//
// Shape: the row frame of ffq_rows.h -- a group of eight lanes per PAIR, workgroups striding over the pairs, the next pair's
// rows asked for ahead.  Per pair:
//   * both rows are checked as the adapter trim checks its row (row_pos, the sequence line); a pair with a mate above
//     OVL_MAX_LEN bases is not analysed and none of its bytes is read -- there is no long rows' launch;
//   * the lanes pack both mates into the group's LDS planes, sixteen bases per lane and step (ffq_overlapwalk.h: two bits per
//     base and a `bad` bit, mate 2 reversed and complemented as it is written), looking through the bytes for '\n' on the way
//     -- with at most 512 bases per mate the packing reads every byte of both sequences, so the newline check is complete;
//   * the candidates are taken in ROUNDS of eight in the rule's order, one per lane: ovl_count, words out of LDS, no byte
//     of the reads; one max-reduction over the group finds the first accepted candidate of the round and the group stops
//     at the first round that has one.
// The round loop is uniform over the wave, as the frame asks: a group without a pair, with a pair that is not analysed, or
// done with its pair steps along idle until every group of the wave is done.  The count of one candidate (ovl_count) holds
// no ballot, DPP move or barrier: its early exit may differ from lane to lane.
// Insert sizes go to a histogram in LDS (one per workgroup, 32-bit counters, added to the caller's with 64-bit atomics at the
// kernel's end: integer sums, the order does not matter); the six counts leave the way wg_counts_flush (ffq_rows.h) has it.
// Both are WRITTEN OUT at the kernel's end, not calls of lds_hist_flush and wg_counts_flush: with the calls the call measured
// 0.013 - 0.022 ms (0.5 - 0.7 %) above the parent's range, the loop's loads waited for a few instructions earlier.
#pragma once
#include "ffq_pair.h"
#include "ffq_overlapwalk.h"

namespace ffq {

constexpr int OVERLAP_WG = 256;
constexpr int OVERLAP_COUNTS = 6;
constexpr int OVERLAP_HIST = 2 * OVL_MAX_LEN + 1;

// analysed, with an overlap, changed, bases removed from mate 1, from mate 2, not analysed
struct OverlapBlock { unsigned long long cnt[OVERLAP_COUNTS]; };

struct OverlapRules { int min_overlap, max_diff, diff_permille, trim; };

// A mate's row out, by three lanes of the group (gl3: 0..2 for them): out of place the whole row -- pos0 / pos1 copied from
// the table --, in place (out == table) only pos2..pos5 of a changed row.
__device__ __forceinline__ void overlap_store(const int64_t *table, int64_t *__restrict__ out, int64_t pair, int gl3, bool changed,
                                              longlong2 n23, longlong2 n45)
{
    if (gl3 < 0 || gl3 > 2) return;
    longlong2 *dst = reinterpret_cast<longlong2 *>(out + pair * 6);
    longlong2 v;                                    // (selects, word by word: a choice of two structs goes through the stack)
    v.x = gl3 == 2 ? n45.x : n23.x;
    v.y = gl3 == 2 ? n45.y : n23.y;
    if (out != table) {
        if (gl3 == 0) v = *reinterpret_cast<const longlong2 *>(table + pair * 6);
        dst[gl3] = v;
    } else if (changed && gl3 > 0) {
        dst[gl3] = v;
    }
}

__global__ __launch_bounds__(OVERLAP_WG) void k_pair_overlap(PairSide A, PairSide B, int64_t n_pairs, const OverlapRules R,
                                                             int64_t *out1, int64_t *out2, int32_t *__restrict__ d_insert,
                                                             unsigned long long *__restrict__ hist, OverlapBlock *__restrict__ blk)
{
    constexpr int G = ROWS_G, RPB = OVERLAP_WG / G;
    // per group: mate 1's codes and bad bits, rb's codes and bad bits
    __shared__ uint32_t s_pl[RPB][4][OVL_PLANE];
    __shared__ uint32_t s_hist[OVERLAP_HIST];
    __shared__ unsigned long long s_cnt[OVERLAP_WG / 64][OVERLAP_COUNTS];
    const int lane = threadIdx.x & 63, gl = lane & (G - 1), gshift = lane & ~(G - 1);
    uint32_t *const ac = s_pl[threadIdx.x / G][0], *const ab = s_pl[threadIdx.x / G][1];
    uint32_t *const rc = s_pl[threadIdx.x / G][2], *const rbad = s_pl[threadIdx.x / G][3];
    if (gl < 4) { s_pl[threadIdx.x / G][gl][0] = 0; s_pl[threadIdx.x / G][gl][OVL_PLANE - 1] = 0; }
    if (hist)
        for (int i = threadIdx.x; i < OVERLAP_HIST; i += OVERLAP_WG) s_hist[i] = 0;
    __syncthreads();

    unsigned int c_an = 0, c_ov = 0, c_ch = 0, c_na = 0;
    unsigned long long c_r1 = 0, c_r2 = 0;
    const int64_t step = (int64_t)gridDim.x * RPB;
    const longlong2 zero = make_longlong2(0, 0);
    longlong2 xa23 = zero, xa45 = zero, xb23 = zero, xb45 = zero;
    {
        const int64_t pair = (int64_t)blockIdx.x * RPB + (threadIdx.x / G);
        if (pair < n_pairs) {
            const longlong2 *sa = reinterpret_cast<const longlong2 *>(A.table + pair * 6), *sb = reinterpret_cast<const longlong2 *>(B.table + pair * 6);
            xa23 = sa[1]; xa45 = sa[2]; xb23 = sb[1]; xb45 = sb[2];
        }
    }
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < n_pairs; r0 += step) {
        const int64_t pair = r0 + (threadIdx.x / G);
        const bool have = pair < n_pairs;
        const longlong2 a23 = xa23, a45 = xa45, b23 = xb23, b45 = xb45;
        if (pair + step < n_pairs) {
            const longlong2 *sa = reinterpret_cast<const longlong2 *>(A.table + (pair + step) * 6);
            const longlong2 *sb = reinterpret_cast<const longlong2 *>(B.table + (pair + step) * 6);
            xa23 = sa[1]; xa45 = sa[2]; xb23 = sb[1]; xb45 = sb[2];
        }
        int64_t pa2 = 0, pa4 = 0, na = 0, pb2 = 0, pb4 = 0, nb = 0;
        bool elig = have && row_pos<true, false>(A.nbytes, A.s, A.add, a23, a45, pa2, pa4, na);
        elig = elig && row_pos<true, false>(B.nbytes, B.s, B.add, b23, b45, pb2, pb4, nb);
        elig = elig && na <= OVL_MAX_LEN && nb <= OVL_MAX_LEN;
        const int n1 = elig ? (int)na : 0, n2 = elig ? (int)nb : 0;
        // (a line with bytes in it never begins at the sentinel's coordinate: row_pos)
        const uint8_t *sa = A.d + (elig ? pa2 - A.s : 0), *sb = B.d + (elig ? pb2 - B.s : 0);

        // ---- both mates into the planes; rb gets one word behind its last (all bad): a candidate's funnel shift takes it ----
        bool nl = false;
        const int nw1 = (n1 + 15) >> 4, nw2 = elig ? ovl_imin(((n2 + 15) >> 4) + 1, OVL_WORDS) : 0;
        for (int W = gl; W < nw1; W += G) {
            uint32_t x[4], c, m;
            ovl_pack_fwd(sa, n1, W, c, m, x);
            ac[W + 1] = c; ab[W + 1] = m;
            nl |= has_nl(x[0]) || has_nl(x[1]) || has_nl(x[2]) || has_nl(x[3]);
        }
        for (int W = gl; W < nw2; W += G) {
            uint32_t x[4], c, m;
            ovl_pack_rc(sb, n2, W, c, m, x);
            rc[W + 1] = c; rbad[W + 1] = m;
            nl |= has_nl(x[0]) || has_nl(x[1]) || has_nl(x[2]) || has_nl(x[3]);
        }
        wave_sync();
        const bool analysed = elig && !group_any<G>(nl, gshift);

        // ---- the candidates, eight per round in the rule's order ----
        const int ncand = analysed ? ovl_ncand(n1, n2, R.min_overlap) : 0;
        int found = -1, c0 = 0;
        bool act = ncand > 0;
        while (__any(act)) {                                       // (uniform over the wave: a DPP reduction inside)
            const int c = c0 + gl;
            int key = 0;
            if (act && c < ncand) {
                const int o = ovl_cand(c, n1, R.min_overlap);
                const int lo = ovl_imax(0, o), hi = ovl_imin(n1, n2 + o);
                const int limit = ovl_limit(hi - lo, R.max_diff, R.diff_permille);
                if (ovl_count(ac, ab, rc, rbad, o, lo, hi, limit) <= limit) key = G - gl;
            }
            const int gmax = RowGroup<G>::maxall(key);             // the round's first accepted candidate: G - its lane; 0: none
            if (act) {
                if (gmax > 0) { found = c0 + (G - gmax); act = false; }
                else { c0 += G; act = c0 < ncand; }
            }
        }
        wave_sync();                                               // (the planes are written again at the next step)

        // ---- what became of the pair ----
        const int o = found >= 0 ? ovl_cand(found, n1, R.min_overlap) : 0;
        const int insert = !analysed ? -2 : found < 0 ? -1 : n2 + o;
        int c1 = n1, c2 = n2;
        if (found >= 0 && o < 0 && R.trim) { c1 = ovl_imin(n1, insert); c2 = ovl_imin(n2, insert); }
        const bool ch1 = c1 != n1, ch2 = c2 != n2;
        if (have) {
            // (pos + c: the row's own coordinates, whatever `add` is)
            overlap_store(A.table, out1, pair, gl, ch1, ch1 ? make_longlong2(a23.x, a23.x + c1) : a23,
                          ch1 ? make_longlong2(a45.x, a45.x + c1) : a45);
            overlap_store(B.table, out2, pair, gl - 4, ch2, ch2 ? make_longlong2(b23.x, b23.x + c2) : b23,
                          ch2 ? make_longlong2(b45.x, b45.x + c2) : b45);
            if (gl == 3 && d_insert) d_insert[pair] = insert;
            if (gl == 7) {
                if (analysed) c_an++; else c_na++;
                if (found >= 0) { c_ov++; if (hist) atomicAdd(&s_hist[insert], 1u); }
                if (ch1 || ch2) c_ch++;
                c_r1 += (unsigned long long)(n1 - c1); c_r2 += (unsigned long long)(n2 - c2);
            }
        }
    }

    // the histogram, and the counts: wave, workgroup, one set of atomics
    __syncthreads();
    if (hist)
        for (int i = threadIdx.x; i < OVERLAP_HIST; i += OVERLAP_WG) {
            const uint32_t x = s_hist[i];
            if (x) atomicAdd(&hist[i], (unsigned long long)x);
        }
    const unsigned long long t_an = wave_sum_u64(c_an), t_ov = wave_sum_u64(c_ov), t_ch = wave_sum_u64(c_ch), t_r1 = wave_sum_u64(c_r1),
                             t_r2 = wave_sum_u64(c_r2), t_na = wave_sum_u64(c_na);
    if (lane == 0) {
        unsigned long long *w = s_cnt[threadIdx.x >> 6];
        w[0] = t_an; w[1] = t_ov; w[2] = t_ch; w[3] = t_r1; w[4] = t_r2; w[5] = t_na;
    }
    __syncthreads();
    if (threadIdx.x < OVERLAP_COUNTS) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < OVERLAP_WG / 64; w++) s += s_cnt[w][threadIdx.x];
        if (s) atomicAdd(&blk->cnt[threadIdx.x], s);
    }
}

}  // namespace ffq

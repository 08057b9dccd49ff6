// ffq_ends.h -- fixed trims and sliding-window quality cutting of both read ends by editing rows of the offset table
// (ffq_table_trim_ends).
//
// The rule (include/ffq.h states it in full): of q[0..n) = buf[pos4:pos5] the fixed trims leave [a, b); FRONT moves a to the
// first window of W values v = q - qual_base whose sum reaches quality * W, and on over that window's bases below the quality;
// RIGHT moves b to the first window from there whose sum does not reach it, behind the good bases at that window's head; TAIL
// moves b to the end of the last window that passes, and back over its bases below the quality.  pos2 / pos3 and pos4 / pos5
// move alike.  Eligibility is the quality trim's (ffq_rows.h: row_pos<false, true>, no '\n' in the whole quality line); any
// other row is copied unchanged and counted.  The sequence line is never read.
//
// Shape: the row frame of ffq_rows.h, as ffq_trim.h uses it -- eight lanes per row and chunks of 64 positions; rows of more
// than ENDS_LONG quality bytes get a whole wave and chunks of 1024 in the second launch.  The pass's own part is the walk,
// ffq_endswalk.h, which says how a chunk goes; here are the loads (trim_chunk of ffq_trim.h), the reductions and the words in
// LDS:
//   * one RowGroup::incl_scan and one sum of the lanes' sums of v per chunk; the lanes' prefix values go into the group's
//     2 * C words of LDS, B consecutive words per lane, where a window's sum is the difference of two of them at most 64 apart
//     (ENDS_WINDOW_MAX)
//   * one max-reduction per stage for the chunk's first window that passes (fails), and one for its "while" step, which goes by
//     the lanes' masks -- the second only when some row of the wave found its window
//   * FRONT and RIGHT are one forward walk over [a, b): RIGHT takes up the chunk FRONT ended in, with the same prefix values
//   * TAIL is the FRONT stage on what RIGHT left, walked backwards
// The first chunk of either walk is asked for at once; the backward one is used if the forward walk left the range as it was,
// as it does with a read that is good all through.  The eligibility rule needs every quality byte once: rows_scan_nl checks
// what the walks did not touch, the fixed trims' bytes among it.  Every loop is uniform over the wave (`while (__any(act))`).
// No byte outside the row's own quality range, itself checked against the buffer, is read.
#pragma once
#include "ffq_trim.h"
#include "ffq_endswalk.h"

namespace ffq {

constexpr int ENDS_LONG = 4096;       // quality bytes above which a row gets a wave of its own
constexpr int ENDS_WG = 256;
constexpr int ENDS_B = 8;             // bytes per lane and chunk of the short rows' kernel

// ffq_ends_rules as the kernels take them
struct EndsRules {
    int trim_front, trim_tail, keep_len, base;
    EndsStage front, right, tail;
};

// One walk of one row per group over the range q[0 .. L) (BACK: from its end).  live: the group has a range to walk (uniform
// in the group).  first: the walk's first chunk (trim_chunk at w0 = 0) if first_ok.  s: the walk's result; nread: walk
// positions [0, nread) went through the newline check here.
template <int G, int B, bool BACK>
__device__ __forceinline__ void ends_walk(const uint8_t *__restrict__ q, int64_t L, bool live, EndsStage pass, EndsStage fail, int base,
                                          uint32_t *words, int gl, const int (&first)[B], bool first_ok, EndsWalk &s,
                                          int64_t &nread, bool &nl)
{
    constexpr int C = G * B;
    ends_begin(s, live ? L : 0, pass, fail);
    nread = 0;
    bool act = s.stage != ENDS_DONE;
    uint32_t mp_prev = 0, mf_prev = 0;                  // the masks of the chunk in front
    for (bool head = true; __any(act); head = false) {
        const int64_t w0 = s.w0;
        const bool given = head && first_ok;
        int qv[B];
        trim_chunk<G, B, BACK>(q, L, act && !given, w0, gl, qv);
        if (given) {
#pragma unroll
            for (int j = 0; j < B; j++) qv[j] = act ? first[j] : -1;
        }
        int v[B];
        uint32_t p[B];
        const uint32_t t = ends_lane_vals<B>(qv, BACK, base, v, nl);
        const uint32_t mp = ends_lane_mask<B>(v, pass.quality), mf = ends_lane_mask<B>(v, fail.quality);
        const uint32_t incl = (uint32_t)RowGroup<G>::incl_scan((int)t, gl);
        const uint32_t total = (uint32_t)RowGroup<G>::sum((int)t);
        ends_lane_store<C, B>(words, gl, s.carry + (incl - t), v, p);
        wave_sync();                                    // the words are the group's to read
        bool judge_fail = act && s.stage == ENDS_FAIL;
        const bool in_pass = act && s.stage == ENDS_PASS;
        if (__any(in_pass)) {
            const int key = RowGroup<G>::maxall(in_pass ? ends_lane_judge<C, B>(words, w0, gl, p, s.W, s.T, s.elo, L, true) : 0);
            int fkey = 0;
            if (__any(key > 0))
                fkey = RowGroup<G>::maxall(key > 0 ? ends_lane_first<C, B>(ends_window_srel<C>(s, key), s.W, true, gl, mp, mp_prev) : 0);
            if (in_pass) judge_fail = ends_pass_end<C>(s, L, key, fkey, fail);
        }
        if (__any(judge_fail)) {
            const int key = RowGroup<G>::maxall(judge_fail ? ends_lane_judge<C, B>(words, w0, gl, p, s.W, s.T, s.elo, L, false) : 0);
            int fkey = 0;
            if (__any(key > 0))
                fkey = RowGroup<G>::maxall(key > 0 ? ends_lane_first<C, B>(ends_window_srel<C>(s, key), s.W, false, gl, mf, mf_prev) : 0);
            if (judge_fail) ends_fail_end<C>(s, L, key, fkey);
        }
        wave_sync();                                    // (the words are written behind these reads)
        ends_lane_keep<C, B>(words, gl, p);
        mp_prev = mp; mf_prev = mf;
        if (act) {
            nread = max(nread, min(w0 + C, L));
            act = ends_advance<C>(s, total);
        }
    }
}

// One row per group, as trim_row: have: this group has a row (uniform in the group); defer_long: rows above ENDS_LONG are
// left to the second launch (returned).  words: the group's 2 * G * B words of LDS.
template <int G, int B>
__device__ __forceinline__ bool ends_row(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                         const int64_t *__restrict__ table, int64_t *__restrict__ out, int64_t row, bool have,
                                         longlong2 r01, longlong2 r23, longlong2 r45, const EndsRules &R, bool defer_long,
                                         uint32_t *words, int gl, int gshift, RowCounts &cnt)
{
    int64_t p2 = 0, p4 = 0, n = 0;
    const bool elig = have && row_pos<false, true>(nbytes, s, add, r23, r45, p2, p4, n);
    const bool is_long = defer_long && elig && n > ENDS_LONG;
    const bool live = elig && !is_long;
    const uint8_t *q = d + (p4 - s);

    int64_t a = 0, b = 0;
    if (live) ends_fixed(n, R.trim_front, R.trim_tail, R.keep_len, a, b);

    // the first chunk of either walk, asked for at once
    const bool fwd_on = R.front.window > 0 || R.right.window > 0, tail_on = R.tail.window > 0;
    int qf[B], qb[B];
    trim_chunk<G, B, false>(q + a, b - a, live && fwd_on, 0, gl, qf);
    trim_chunk<G, B, true>(q + a, b - a, live && tail_on, 0, gl, qb);

    bool nl = false;
    int64_t rf = 0, rb = 0;
    EndsWalk f, t;
    ends_walk<G, B, false>(q + a, b - a, live, R.front, R.right, R.base, words, gl, qf, true, f, rf, nl);
    const int64_t a1 = a + f.a, b1 = a + f.b;
    const bool tlive = live && !f.zero && b1 > a1;
    ends_walk<G, B, true>(q + a1, b1 - a1, tlive, R.tail, EndsStage{0, 0}, R.base, words, gl, qb, a1 == a && b1 == b, t, rb, nl);
    int64_t start = a1, stop = b1 - t.a;                // (backwards, t.a positions went from the range's end)
    if (f.zero || t.zero || start >= stop) start = stop = 0;

    // what the walks did not read: in front of a, between them, behind b1
    const int64_t x = a + rf;
    rows_scan_nl<G>(q, 0, a, live, gl, nl);
    rows_scan_nl<G>(q, x, b1 - rb, live, gl, nl);
    rows_scan_nl<G>(q, max(x, b1), n, live, gl, nl);
    const bool any_nl = group_any<G>(nl, gshift);

    // (pos + start: the row's own coordinates, whatever `add` is)
    row_edit_finish(table, out, row, gl, have, is_long, elig && !any_nl, r01, r23, r45, make_longlong2(r23.x + start, r23.x + stop),
                    make_longlong2(r45.x + start, r45.x + stop), n - (stop - start), cnt);
    return is_long;
}

__global__ __launch_bounds__(ENDS_WG) void k_ends_rows(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                       const int64_t *table, int64_t n_rows, EndsRules R, int64_t *out,
                                                       int64_t *__restrict__ long_list, RowsBlock *__restrict__ blk)
{
    constexpr int G = ROWS_G;
    constexpr int RPB = ENDS_WG / G;
    __shared__ alignas(16) uint32_t s_words[RPB][2 * G * ENDS_B];
    const int lane = threadIdx.x & 63, gl = lane & (G - 1), gshift = lane & ~(G - 1);
    uint32_t *words = s_words[threadIdx.x / G];
    RowCounts cnt;
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
        const bool is_long = ends_row<G, ENDS_B>(d, nbytes, s, add, table, out, row, row < n_rows, r01, r23, r45, R, true, words, gl, gshift,
                                                 cnt);
        const int64_t at = long_list_append(is_long && gl == 0, lane, &blk->n_long);
        if (at >= 0) long_list[at] = row;
    }
    cnt.add_to<ENDS_WG>(blk);
}

// the rows k_ends_rows left: sixteen bytes per lane and chunk
__global__ __launch_bounds__(ENDS_WG, 2) void k_ends_long(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                       const int64_t *table, EndsRules R, int64_t *out,
                                                       const int64_t *__restrict__ long_list, RowsBlock *__restrict__ blk)
{
    __shared__ alignas(16) uint32_t s_words[ENDS_WG / 64][2 * 64 * 16];
    const int lane = threadIdx.x & 63;
    uint32_t *words = s_words[threadIdx.x >> 6];
    RowCounts cnt;
    for (LongRows<ENDS_WG, true> it((int64_t)blk->n_long, long_list, table); it.next();)
        ends_row<64, 16>(d, nbytes, s, add, table, out, it.row, it.have, it.r01, it.r23, it.r45, R, false, words, lane, 0, cnt);
    cnt.add_to<ENDS_WG>(blk);
}

}  // namespace ffq

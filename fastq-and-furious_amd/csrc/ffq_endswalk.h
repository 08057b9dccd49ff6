// ffq_endswalk.h -- what ONE LANE does with its bytes in the walks of the ends pass (csrc/ffq_ends.h, ffq_table_trim_ends;
// include/ffq.h states the rule), and what its group does with a chunk once the lanes' results are reduced.  Nothing here has a
// ballot or a DPP move in it: inline functions that compile for the host too.  The kernels call them, and
// tests/ends_walk_host.cpp drives the same functions on a CPU, a group lane by lane, against the rule's loop over bytes.
//
// A walk goes over a RANGE of the quality line, [lo, hi) of q, in CHUNKS of C = G * B walk positions, B consecutive ones per
// lane.  Positions are relative to the range: forwards position p is byte lo + p, backwards it is byte hi - 1 - p, so that the
// tail stage is the front stage on the range read backwards ("the last window that passes, then step back over its bad bases"
// is "the first window that passes, then step over its bad bases" from the other side).
//
// The prefix sums P(p) = v(0) + .. + v(p) are 32 bits and WRAP; a window's sum is P(e) - P(e - W) for the window that ENDS at
// e, exact as a difference because a window holds at most 64 values of magnitude below 256.  P(p) is 0 for p < 0.  The group
// keeps the prefix values of two chunks in 2 * C words, the chunk in front of the current one in [0, C) and the current one in
// [C, 2C): a window reaches at most 64 <= C positions back, into the chunk in front at the most, and every lane reads the B
// values it subtracts as B consecutive words.  A "while" step looks at one window's positions for the first value at or above
// (below) the stage's quality: that is one bit per position, which every lane keeps for its own positions of both chunks (a
// MASK per stage), so the step reads nothing back.
//
// A chunk, for its group:
//   1. every lane: ends_lane_vals (the values of its B bytes, their sum), ends_lane_mask for either stage's quality
//   2. the group:  an inclusive prefix sum of the lanes' sums; start = carried + (inclusive - own)
//   3. every lane: ends_lane_store (its prefix values into the current half and into registers); the words are then the group's
//      to read
//   4. PASS stage (front; tail on the backward range): every lane ends_lane_judge(pass), the group a maximum of the keys: the
//      first window that passes; every lane ends_lane_first(at or above the quality), a maximum: the "while" step;
//      ends_pass_end: the range's new start, and the FAIL stage entered if there is one -- on this very chunk, or on the one in
//      front of it again if the first window to judge ends there (it never ends further back; nothing in front of THAT chunk is
//      looked at then, as the range's new start lies inside it)
//   5. FAIL stage (right): the same with ends_lane_judge(fail), ends_lane_first(below the quality), ends_fail_end
//   6. every lane: ends_lane_keep (its prefix values into the half of the chunk in front), its masks kept; the group: ends_advance
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ENDS_HD __host__ __device__ __forceinline__
#else
#define ENDS_HD inline
#endif

namespace ffq {

constexpr int ENDS_WINDOW_MAX = 64;
constexpr int ENDS_QUALITY_LO = 1, ENDS_QUALITY_HI = 93;

struct EndsStage { int window, quality; };            // window 0: the stage is off

// qv: the lane's B bytes in ascending ADDRESS order, -1 where there is none; back: the walk goes backwards.  v: their values
// in WALK order (0 where there is no byte); nl: one of them is '\n'.  Returns the sum of v.
template <int B>
ENDS_HD uint32_t ends_lane_vals(const int (&qv)[B], bool back, int qual_base, int (&v)[B], bool &nl)
{
    uint32_t t = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < B; j++) {
        const int x = back ? qv[B - 1 - j] : qv[j];
        nl |= x == 10;
        v[j] = x < 0 ? 0 : x - qual_base;
        t += (uint32_t)v[j];
    }
    return t;
}

// bit j: the lane's position j has a value of q or more
template <int B>
ENDS_HD uint32_t ends_lane_mask(const int (&v)[B], int q)
{
    uint32_t m = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < B; j++) m |= (uint32_t)(v[j] >= q) << j;
    return m;
}

// the lane's prefix values from `start`, the prefix value in front of its first position: into p and the current half (words:
// 16-byte aligned; the lane's B words are 4 * B bytes apart from its neighbour's)
template <int C, int B>
ENDS_HD void ends_lane_store(uint32_t *words, int gl, uint32_t start, const int (&v)[B], uint32_t (&p)[B])
{
    uint32_t *dst = static_cast<uint32_t *>(__builtin_assume_aligned(words + C + gl * B, 16));
    uint32_t r = start;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < B; j++) {
        r += (uint32_t)v[j];
        p[j] = r;
        dst[j] = r;
    }
}

// ... and, when the chunk is done with, into the half of the chunk in front
template <int C, int B>
ENDS_HD void ends_lane_keep(uint32_t *words, int gl, const uint32_t (&p)[B])
{
    uint32_t *dst = static_cast<uint32_t *>(__builtin_assume_aligned(words + gl * B, 16));
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < B; j++) dst[j] = p[j];
}

// The lane's first position e = w0 + gl * B + j, elo <= e < L, at which the window of W (0 <= W <= 64) that ends there sums to
// T or more (pass) or to less (!pass): C - (its place in the chunk), what the group takes the maximum of; 0 if it has none.
template <int C, int B>
ENDS_HD int ends_lane_judge(const uint32_t *words, int64_t w0, int gl, const uint32_t (&p)[B], int W, int T, int64_t elo, int64_t L,
                            bool pass)
{
    static_assert(C >= ENDS_WINDOW_MAX, "a window reaches into the chunk in front at the most");
    const uint32_t *back = words + (C + gl * B - W);    // P(e - W) of the lane's first position, then of the next ones
    int key = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = B - 1; j >= 0; j--) {
        const int64_t e = w0 + gl * B + j;
        const int sum = (int)(p[j] - (e - W < 0 ? 0u : back[j]));
        if (e >= elo && e < L && (sum >= T) == pass) key = C - (gl * B + j);
    }
    return key;
}

// bits lo .. hi - 1 of m (either may lie outside 0 .. B)
template <int B>
ENDS_HD uint32_t ends_bits(uint32_t m, int lo, int hi)
{
    lo = lo < 0 ? 0 : lo;
    hi = hi > B ? B : hi;
    return hi <= lo ? 0u : m & (((1u << (hi - lo)) - 1u) << lo);
}

// The "while" step of a window of W that begins at chunk position srel (negative: in the chunk in front): the first of its
// positions whose value is at or above the stage's quality (ge) or below it (!ge), by the lane's masks of the current chunk
// and of the one in front.  ENDS_WINDOW_MAX - (the position's offset in the window), 0 if the lane has none.
template <int C, int B>
ENDS_HD int ends_lane_first(int srel, int W, bool ge, int gl, uint32_t cur, uint32_t prev)
{
    static_assert(B <= 16, "a mask's shifts");
    const uint32_t all = (1u << B) - 1u;
    // the lane's positions of the chunk in front are gl * B - C + j, those of the current one gl * B + j
    const int lo_prev = srel - (gl * B - C), lo_cur = srel - gl * B;
    const uint32_t mp = ends_bits<B>(ge ? prev : ~prev & all, lo_prev, lo_prev + W);
    const uint32_t mc = ends_bits<B>(ge ? cur : ~cur & all, lo_cur, lo_cur + W);
    if (mp) return ENDS_WINDOW_MAX - (__builtin_ctz(mp) - lo_prev);
    if (mc) return ENDS_WINDOW_MAX - (__builtin_ctz(mc) - lo_cur);
    return 0;
}

// what a group carries from chunk to chunk of one walk
struct EndsWalk {
    int stage;                        // ENDS_PASS, ENDS_FAIL or ENDS_DONE
    int W, T;                         // the stage's window on this range and its threshold, quality * W
    int64_t w0;                       // the chunk's first position
    int64_t elo;                      // the first position a window of the stage may end at
    int64_t a, b;                     // what is left of the range, [a, b)
    uint32_t carry, carry_prev;       // the prefix value in front of w0, and in front of w0 - C
    bool zero;                        // no window passed: the read goes to length 0
    bool again;                       // the chunk at w0 is walked once more (ends_pass_end), nothing is judged on it yet
};

constexpr int ENDS_PASS = 0, ENDS_FAIL = 1, ENDS_DONE = 2;

ENDS_HD void ends_enter(EndsWalk &s, int stage, EndsStage st, int64_t from, int64_t L)
{
    const int64_t left = L - from;
    s.stage = stage;
    s.W = (int)(left < st.window ? left : st.window);
    s.T = st.quality * s.W;
    s.elo = from + s.W - 1;
}

// a walk over a range of L positions: the PASS stage if it is on, then the FAIL stage if that is
ENDS_HD void ends_begin(EndsWalk &s, int64_t L, EndsStage pass, EndsStage fail)
{
    s = EndsWalk{ENDS_DONE, 0, 0, 0, 0, 0, L, 0u, 0u, false, false};
    if (L <= 0) return;
    if (pass.window > 0) ends_enter(s, ENDS_PASS, pass, 0, L);
    else if (fail.window > 0) ends_enter(s, ENDS_FAIL, fail, 0, L);
}

// where the window begins whose end the maximum `key` of ends_lane_judge names (key > 0), as a position of the chunk ...
template <int C>
ENDS_HD int ends_window_srel(const EndsWalk &s, int key) { return (C - key) - s.W + 1; }
// ... and of the range
template <int C>
ENDS_HD int64_t ends_window_start(const EndsWalk &s, int key) { return s.w0 + ends_window_srel<C>(s, key); }

// The end of a chunk's PASS stage.  key: the maximum of the lanes' judge keys, fkey: of their ends_lane_first keys for the
// window `key` names.  Returns whether the FAIL stage judges this same chunk.
template <int C>
ENDS_HD bool ends_pass_end(EndsWalk &s, int64_t L, int key, int fkey, EndsStage fail)
{
    if (s.stage != ENDS_PASS) return s.stage == ENDS_FAIL && !s.again;
    if (key > 0) {
        // (a window that passes holds a base at or above the quality: fkey > 0)
        s.a = ends_window_start<C>(s, key) + (fkey > 0 ? ENDS_WINDOW_MAX - fkey : s.W - 1);
        if (fail.window <= 0) { s.stage = ENDS_DONE; return false; }
        ends_enter(s, ENDS_FAIL, fail, s.a, L);
        if (s.elo >= s.w0) return true;
        // its first window ends in the chunk in front (s.a >= w0 - 63): that one once more, from the same prefix value
        s.w0 -= C; s.carry = s.carry_prev; s.again = true;
        return false;
    }
    if (s.w0 + C >= L) { s.zero = true; s.a = s.b = 0; s.stage = ENDS_DONE; }
    return false;
}

// the end of a chunk's FAIL stage, for a group that judged it
template <int C>
ENDS_HD void ends_fail_end(EndsWalk &s, int64_t L, int key, int fkey)
{
    if (key > 0) {
        // (a window that fails holds a base below the quality: fkey > 0; the good bases at its head stay)
        s.b = ends_window_start<C>(s, key) + (fkey > 0 ? ENDS_WINDOW_MAX - fkey : s.W);
        s.stage = ENDS_DONE;
    } else if (s.w0 + C >= L)
        s.stage = ENDS_DONE;
}

// on to the next chunk; total: the sum of the chunk's values.  Returns whether the walk goes on.
template <int C>
ENDS_HD bool ends_advance(EndsWalk &s, uint32_t total)
{
    if (s.again) { s.again = false; return true; }
    if (s.stage == ENDS_DONE) return false;
    s.carry_prev = s.carry; s.carry += total; s.w0 += C;
    return true;
}

// the fixed trims: [a, b) of a line of n
ENDS_HD void ends_fixed(int64_t n, int trim_front, int trim_tail, int keep_len, int64_t &a, int64_t &b)
{
    a = trim_front < n ? trim_front : n;
    b = n - (trim_tail < n - a ? trim_tail : n - a);
    if (keep_len > 0 && b - a > keep_len) b = a + keep_len;
}

}  // namespace ffq

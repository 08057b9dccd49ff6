// ffq_pairwalk.h -- the bookkeeping of the walk over two streams whose records are mates (ffq_pair, csrc/ffq_stream.h): plain
// host code without a device call, so that tests/pair_walk_host.cpp drives it on a CPU over scripted fill sizes.
//
// The fills of the two streams never hold the same number of records.  Each mate keeps its current fill and a WINDOW
// [lo, n) of that fill's rows that are not yet paired.  A round
//   1. advances every mate whose window is empty and whose stream has not ended (walk_wants; the caller scans the stream's
//      next fill and says what came: walk_filled),
//   2. takes m = min(rows left in 1, rows left in 2) (walk_take) -- the caller runs one table chain over the two slices
//      [lo, lo + m) --,
//   3. moves both windows by m and decides what the caller is told (walk_moved).
// A mate's fill stays where it is until its window is empty, so no row is processed twice and nothing is carried by hand.
// m == 0 happens in two ways only: a fill came without a complete record (a record longer than the chunk: the stream refills
// with more room), or one mate has ended and the other's next fill decides between a clean end and FFQ_END_ERR_PAIR_COUNT.
// Either way a mate advanced in that round, so rounds without progress do not repeat: walk_check says so.
//
// What a round reports, in this order:
//   a mate's own error (FFQ_END_ERR_FINAL_QUAL / _INCOMPLETE / _INVALID) in the round in which that mate's rows run out --
//       where ffq_stream_next reports it --, mate 1 before mate 2;
//   FFQ_END_OK when both mates are ended and empty;
//   FFQ_END_ERR_PAIR_COUNT when one mate is ended and empty and the other still holds a record (err_mate: the longer one,
//       err_row: the row of its fill that is its first unpaired record);
//   FFQ_END_REFILL otherwise.
#pragma once
#include <cstdint>

namespace ffq {

// (the values of include/ffq.h; ffq_stream.h checks them)
constexpr int WALK_END_OK = 0, WALK_END_REFILL = 1, WALK_END_ERR_PAIR_COUNT = 5, WALK_END_ERR_PAIR_NAMES = 6;

struct WalkMate {
    int64_t lo = 0, n = 0;              // rows [lo, n) of the current fill are not yet paired
    bool ended = false;                 // the stream has handed out its last fill
    int end_state = WALK_END_REFILL;    //   ... with this state (FFQ_END_OK, or its own FFQ_END_ERR_*)
    int64_t err_offset = -1;            //   ... and this offset
    int64_t fills = 0, rows = 0;        // totals: fills taken, rows paired

    int64_t left() const { return n - lo; }
    bool exhausted() const { return ended && left() == 0; }
};

struct WalkRound {
    int end_state = WALK_END_REFILL;
    int err_mate = 0;                   // 1 or 2 with an error state
    int64_t err_offset = -1;            // a mate's own error: the stream's offset; FFQ_END_ERR_PAIR_NAMES: the pair's global ordinal
    int64_t err_row = -1;               // FFQ_END_ERR_PAIR_COUNT: the row of err_mate's fill that holds its first unpaired record
};

struct PairWalk {
    WalkMate m[2];
    int64_t pairs = 0;                  // pairs handed to a chain so far: the global ordinal of the next round's first pair
    int64_t rounds = 0;
    bool done = false;                  // an end state other than FFQ_END_REFILL has been reported
    int advanced = 0;                   // bits: the mates that took a fill in the current round
};

// bit 0 / bit 1: that mate takes a new fill at the next round
inline int walk_wants(const PairWalk &w)
{
    if (w.done) return 0;
    int bits = 0;
    for (int k = 0; k < 2; k++)
        if (w.m[k].left() == 0 && !w.m[k].ended) bits |= 1 << k;
    return bits;
}

// the round begins (before the fills of walk_wants are taken)
inline void walk_begin(PairWalk &w) { w.advanced = 0; }

// mate k's stream handed out its next fill: n_rows records, the scan's end state and, with an error state, its offset
inline void walk_filled(PairWalk &w, int k, int64_t n_rows, int end_state, int64_t err_offset)
{
    WalkMate &m = w.m[k];
    m.lo = 0; m.n = n_rows;
    m.fills++;
    m.ended = end_state != WALK_END_REFILL;
    m.end_state = end_state;
    m.err_offset = m.ended && end_state != WALK_END_OK ? err_offset : -1;
    w.advanced |= 1 << k;
}

// pairs of this round
inline int64_t walk_take(const PairWalk &w)
{
    const int64_t a = w.m[0].left(), b = w.m[1].left();
    return a < b ? a : b;
}

// A round of m == 0 pairs is legitimate only if a mate took a fill in it (see above): what the caller asserts.
inline bool walk_check(const PairWalk &w, int64_t m)
{
    return m > 0 || w.advanced != 0 || (w.m[0].exhausted() && w.m[1].exhausted());
}

// the names check found pair `local` of this round different: nothing of the round is handed out
inline WalkRound walk_names_differ(PairWalk &w, int64_t local)
{
    WalkRound r;
    r.end_state = WALK_END_ERR_PAIR_NAMES;
    r.err_offset = w.pairs + local;
    w.done = true;
    w.rounds++;
    return r;
}

// the round's chain ran over m pairs: both windows move, and what the caller is told
inline WalkRound walk_moved(PairWalk &w, int64_t m)
{
    WalkRound r;
    for (int k = 0; k < 2; k++) { w.m[k].lo += m; w.m[k].rows += m; }
    w.pairs += m;
    w.rounds++;
    for (int k = 0; k < 2; k++)
        if (w.m[k].exhausted() && w.m[k].end_state != WALK_END_OK) {
            r.end_state = w.m[k].end_state; r.err_mate = k + 1; r.err_offset = w.m[k].err_offset;
            w.done = true;
            return r;
        }
    if (w.m[0].exhausted() && w.m[1].exhausted()) { r.end_state = WALK_END_OK; w.done = true; return r; }
    for (int k = 0; k < 2; k++)
        if (w.m[k].exhausted() && w.m[1 - k].left() > 0) {
            r.end_state = WALK_END_ERR_PAIR_COUNT; r.err_mate = 2 - k; r.err_row = w.m[1 - k].lo;
            w.done = true;
            return r;
        }
    return r;
}

}  // namespace ffq

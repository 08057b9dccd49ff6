// ffq_scanwalk.h -- the tier ladder of a buffer scan (ffq_scan_submit / ffq_scan_wait, csrc/ffq_hip.hip): which front a scan
// starts with, what follows each report the device publishes, and what the context remembers for its next scans.  Plain host
// code without a device call, so that tests/scan_walk_host.cpp drives it on a CPU over scripted reports.  ffq_hip.hip keeps
// the launches, the events and the host waits: it asks plan_front before a front, plan_lite where the general kernels start,
// and next_step after every report, and runs what they say.
//
// FRONTS (plan_front; the first that applies)
//   index only     FFQ_F_FORCE_SERIAL, FFQ_F_FORCE_RANKED, or the context remembers long records (ranked_skip)
//   single pass    decode + FFQ_F_SINGLE_PASS on a scan that may try the fast path, no index yet, offset < 16, an aligned
//                  quality buffer with room: segmented, or in place once the segments were refused (seg_refused, fz_in_place)
//                  -- unless the context holds it off (fused_skip)
//   fast path      four-line rows from the index; the DENSE row kernel if this buffer or the context met a dense tile
//   general        the group kernels (dense configuration: dense_cfg / dense_skip; lean kernel: plan_lite), with the fast
//                  path's kernels in front as a PROBE on the scan after fast4_skip has run out; WIDE (the index kernel also
//                  decodes in place) only on a scan that STARTS here with decode + FFQ_F_SINGLE_PASS, room and alignment
//
// STEPS (next_step: phase of the scan, report -> step)
//   FRONT    ERR_POOL                                 third time: fail; else grow the pool, index again, front again
//            ERR_INTERNAL                             fail
//            probe ran                                hint 1: forget fast4_remember; else fast4_skip = HOLD_OFF
//            fast path / single pass, no fallback     DONE path 3 / 6 (single pass: back-off reset, fz_in_place as it ran)
//            single pass refused by shape, with room  front again: the in-place pass, which builds the index itself
//            single pass refused otherwise            no_fused, fused_skip = back-off (15, 63, 255, 1023), index kept unless
//                                                     FZ_BAD_INDEX, front again
//            dense tile, not yet the DENSE kernel     dense4, dense4_remember, front again from the index
//            fast path refused otherwise              fast4_remember, fast4_skip = HOLD_OFF, GENERAL tier
//            general front                            as REPAIR below, round 0
//   GENERAL  ERR_INTERNAL: fail; else as REPAIR below, round 0
//   REPAIR   another pass while fallback, the first bad group moved, round < 16, no ERR_DSTAGE and none of: round >= 2 and
//            not irregular; a guess in eight wrong and long records; from round 4 an advance under round * ngroups / 64
//            (the first two only with the ranked tier available).  Then, in this order:
//            ERR_DSTAGE                               fifth time: fail; else grow the stage, front again from the index
//            fallback, irregular, not dense_cfg       dense_cfg, dense_skip = HOLD_OFF, front again
//            fallback or index-only, ranked available RANKED tier (only if sparse: the start came from ranked_skip)
//            fallback or index-only otherwise         WALK
//            else                                     DONE path 0 / 2
//   RANKED   too dense for a remembered start         forget ranked_skip and fast4_*, front again: the usual tiers
//            cannot run                               WALK
//            ran                                      DONE path 5, ranked_skip = HOLD_OFF unless forced
//   WALK     DONE path 1
//   Every DONE behind the group kernels: n_declined * 4 > ngroups sets lite_skip; decode + wide adds FFQ_PATH_IN_PLACE.
#pragma once
#include <algorithm>
#include <cstdint>

namespace ffq {

// (the values of ffq_dev.h, ffq_fused.h and include/ffq.h; ffq_hip.hip checks them)
constexpr uint32_t WALK_ERR_POOL = 1u, WALK_ERR_INTERNAL = 2u, WALK_ERR_DSTAGE = 4u;
constexpr int32_t WALK_FZ_BAD_SHAPE = 1, WALK_FZ_BAD_INDEX = 4;
constexpr int64_t WALK_TILE = 16384, WALK_SEG_STRIDE = 8704;
constexpr unsigned long long WALK_POOL_MIN = 64ull * WALK_TILE;
constexpr int WALK_PATH_IN_PLACE = 8, WALK_E_INTERNAL = -6;

// How long a verdict about a context's input holds: the scans that follow take the tier it chose without asking again.
constexpr int HOLD_OFF = 15;

// What a context remembers about its recent input: which tier its next scans start with.  ffq_ctx_forget resets all of it.
struct InputMemory {
    bool fast4_remember = false;         // the recent input was not plain four-line: scans start with the general kernels
    int fast4_skip = 0;                  //   ... and this many of them do so without asking again; the one after is a PROBE
                                         //   scan: general kernels as before, the fast path's kernels in front of them just
                                         //   to see whether they would have stood (DevRes::fast4_hint) -- no host round trip,
                                         //   no second front, whichever way it comes out
    int ranked_skip = 0;                 // scans left that go straight to the list-ranking tier (long records)
    int dense_skip = 0;                  // scans left that start with the dense configuration of the group kernels
    int lite_skip = 0;                   // scans left whose general path runs k_chain_wave over all groups (the lean kernel declined too many)
    bool dense4_remember = false;        // four-line input with dense tiles (reads of a dozen bases): the fast path starts with k_rows4<., true>
    int fused_skip = 0;                  // scans left that do not try the single pass (it failed: odd records) ...
    int fused_backoff = HOLD_OFF;        //   ... and the count after its next failure (grows 4 b + 3, up to 1023)
    bool fz_in_place = false;            // the last single pass that stood wrote in place (long lines): start with that one
};
inline void forget(InputMemory &mem) { mem = InputMemory{}; }

enum Phase { PH_FRONT, PH_GENERAL, PH_REPAIR, PH_RANKED, PH_WALK };    // whose report next_step reads next

// The deciding half of a scan's state (ffq_hip.hip adds the arguments, `active` and the completion number).
struct ScanWalk {
    // the caller's FFQ_F_* flags, read once at submit
    bool serial = false, decode = false, single_pass = false, force_ranked = false, force_general = false;
    bool poll_result = false, no_timing = false;
    int retries = 0;
    int repairs = 0;          // repair passes of the general kernels (reported with retries)
    bool dense_cfg = false, fast4_failed = false;
    bool probe4 = false;      // the front carries the fast path's kernels as a probe (see InputMemory::fast4_skip)
    bool untimed = false;     // FFQ_F_NO_TIMING: no marks around the index kernel, which may start beside the previous front's last kernel
    bool dense4 = false;      // the fast path's row kernel is the DENSE instantiation (it met a dense tile on this buffer, or the context remembers one)
    bool fused = false;       // the front is the single-pass index + decode kernel (ffq_fused.h)
    bool no_fused = false;    // ... which did not stand on this buffer: the two-pass kernels take it
    bool in_place = false;    // the single pass of this front writes in place (k_scan_ident) rather than segments (k_scan_seg)
    bool seg_refused = false; // the segmented single pass met a shape it cannot take (a long line): the in-place one is next
    bool wide = false;        // the index kernel of this scan also wrote EVERY byte decoded in place (k_scan_lines<.., WIDE>): the general
                              //   path's decode in one pass -- no tier of this scan runs a decode kernel, qoff[i] = pos4's offset in the buffer
    bool go_ranked = false;   // the front is the index kernel only: the list-ranking tier follows at the wait
    bool index_done = false;  // the line index of this buffer is built (a later tier re-uses it)
    bool lite_ran = false;    // the general front of this scan used the lean kernel
    int stage = 0;            // what the pending front consisted of: 1 fast four-line path, 2 general path
    int64_t ntiles = 0;
    int ngroups = 0;
    // the repair rounds: passes so far, the first bad group before the last pass and before the first
    int round = 0, prev_bad = -1, first_bad = 0;
    Phase phase = PH_FRONT;
    int path = 0;             // ffq_scan_result.path so far (0 general, 2 dense configuration, 5 ranked, 1 walk)
    int64_t n_bytes = 0, qual_cap = 0;       // of the call, as plan_front was told
};

struct Switches { bool no_fast4, no_wide, no_lite, no_ranked; };      // FFQ_NO_FAST4 / _WIDE / _LITE / _RANKED are set

struct CallFacts { int64_t offset, qual_cap, n_bytes; bool qual_aligned; };       // qual_aligned: d_qual is 16-byte aligned

enum Front { FRONT_FUSED, FRONT_FAST4, FRONT_GENERAL, FRONT_INDEX_ONLY };
struct FrontPlan {
    Front front = FRONT_GENERAL;
    bool in_place = false;    // FRONT_FUSED: k_scan_ident, TILE bytes per tile (else k_scan_seg, SG_STRIDE)
    bool dense4 = false;      // the row kernel (fast path or probe) is the DENSE instantiation
    bool probe4 = false;      // FRONT_GENERAL: the fast path's kernels in front
    bool wide = false;        // the index kernel decodes in place
    bool run_index = true;    // false: the index is there already
    bool untimed = false;     // no marks around the index kernel
    bool polled = false;      // the front ends in a publisher that writes a completion number: no end event
};

// What enqueue_front decides before its first launch.
inline FrontPlan plan_front(ScanWalk &st, InputMemory &mem, const CallFacts &f, const Switches &sw)
{
    FrontPlan p;
    st.phase = PH_FRONT;
    st.n_bytes = f.n_bytes; st.qual_cap = f.qual_cap;
    // the four-line fast path (ffq_rows4.h) is tried first unless it already failed on this buffer
    // (nor while the context remembers that its recent input was not four-line)
    if (mem.ranked_skip > 0 && !st.serial && !st.index_done) { mem.ranked_skip--; st.go_ranked = true; }
    if (st.force_ranked && !st.serial) st.go_ranked = true;
    st.probe4 = false;
    if (mem.fast4_remember && !st.fast4_failed) {
        st.fast4_failed = true;
        if (mem.fast4_skip > 0) mem.fast4_skip--;
        else st.probe4 = !st.serial && !st.go_ranked && !st.index_done;
    }
    if (mem.dense_skip > 0 && !st.dense_cfg && !st.index_done) { mem.dense_skip--; st.dense_cfg = true; }
    const bool try_fast4 = !st.serial && !st.go_ranked && !st.dense_cfg && !st.fast4_failed && !st.force_general && !sw.no_fast4;
    p.polled = st.poll_result && !st.decode;      // without the decode every front ends in a publisher: it can say "done" itself

    // ---- four-line input with the decode: index AND decoded stream in one pass over the bytes ---------
    // (two layouts, both "record i at d_qual + d_qoff[i]", include/ffq.h: SEGMENTED -- SG_STRIDE bytes of the caller's buffer
    // per tile, lines up to SG_EXT bytes behind a tile's end -- and IN PLACE -- TILE bytes per tile, lines of any length, a
    // few per cent slower on short reads (more bytes written); both write whole 16-byte pieces: an unaligned d_qual gets the
    // packed stream.  The segmented one first; once it has refused a buffer for its shape the in-place one, which the
    // context then remembers.)
    st.fused = false;
    st.in_place = (mem.fz_in_place || st.seg_refused) && f.qual_cap >= st.ntiles * WALK_TILE;
    if (st.decode && st.single_pass && try_fast4 && !st.index_done && !st.no_fused && f.offset < 16 &&
        (st.in_place || (!st.seg_refused && f.qual_cap >= st.ntiles * WALK_SEG_STRIDE)) && f.qual_aligned) {
        if (mem.fused_skip > 0) mem.fused_skip--;
        else st.fused = true;
    }
    if (st.fused) {
        p.front = FRONT_FUSED; p.in_place = st.in_place;
        st.stage = 1;
        return p;
    }
    // (FFQ_F_NO_TIMING with the polled completion: no stream marker anywhere in the front -- each is a barrier
    // packet with a few microseconds of idle GPU around it)
    st.untimed = st.no_timing && p.polled && !st.index_done;
    // The decode of records of ANY layout in one pass: a scan that starts on the general path (wrapped records: the context
    // remembers them; FFQ_F_FORCE_GENERAL; the ranking / one-wave tiers) with FFQ_F_SINGLE_PASS and FFQ_INPLACE_STRIDE bytes
    // of quality buffer per tile has its index kernel write EVERY byte decoded at the offset it has in the buffer: no tier of
    // the scan then runs a decode kernel -- qoff[i] = pos4's offset -- and the input is read once.  (The four-line fast path
    // has its own single passes, above; a scan that comes here from a refused fast path already has its index and takes the
    // packed decode, as before.)
    if (!st.index_done)
        st.wide = st.decode && st.single_pass && !try_fast4 && !sw.no_wide && f.qual_cap >= st.ntiles * WALK_TILE && f.qual_aligned;
    p.untimed = st.untimed; p.wide = st.wide; p.run_index = !st.index_done;
    if (try_fast4) {
        if (mem.dense4_remember) st.dense4 = true;
        p.front = FRONT_FAST4; p.dense4 = st.dense4;
        st.stage = 1;
    } else {
        p.front = (!st.serial && !st.go_ranked) ? FRONT_GENERAL : FRONT_INDEX_ONLY;
        p.probe4 = st.probe4; p.dense4 = st.probe4 && mem.dense4_remember;
        st.stage = 2;
    }
    return p;
}

// Whether the general kernels of this scan start with the lean kernel (ffq_lite.h).  A context whose recent input the lean
// kernel mostly declined -- tiles of more than LT_E lines that still fit the usual window: lines of 43-48 bytes -- runs
// k_chain_wave directly for a while: the list kernel is the slower way to run many groups.
inline bool plan_lite(ScanWalk &st, InputMemory &mem, const Switches &sw)
{
    bool lite = !st.dense_cfg && !sw.no_lite;
    if (lite && mem.lite_skip > 0) { mem.lite_skip--; lite = false; }
    st.lite_ran = lite;
    return lite;
}

// What the host reads back after a front or a tier: Ctl's error bits and pool_head, DevRes's verdicts, and how the ranked
// tier ended (RK_*; read in PH_RANKED only).
struct Report {
    uint32_t err = 0;
    unsigned long long pool_head = 0;
    int32_t fallback = 0, fast4_hint = 0, fused_bad = 0, fast4_dense = 0;
    int32_t bad_group = 0, bad_irregular = 0, n_bad = 0, n_declined = 0;
    int64_t approx_records = 0;
    int ranked = 0;
};

// The ranked tier's own verdict once the host knows its candidates: it cannot run (32-bit ranks), the buffer is too dense
// for a context that only REMEMBERS long records (more than one candidate per 512 bytes: back to the group kernels), or go on.
enum { RK_GO = 0, RK_CANNOT = 1, RK_DENSE = 2 };
inline int ranked_verdict(int64_t nc, int64_t n_bytes, bool only_if_sparse)
{
    if (nc >= 0x7FFFFFF0ll) return RK_CANNOT;
    if (only_if_sparse && nc * 512 > n_bytes) return RK_DENSE;
    return RK_GO;
}

// chunks the walked groups' stage gets after a scan asked for `asked` of them and it holds `dchunks` (STEP_GROW_STAGE; the
// host copies `asked` back on that step only)
inline int64_t stage_chunks(uint32_t asked, int32_t dchunks)
{
    return std::max<int64_t>((int64_t)asked + (asked >> 3) + 8, 2 * (int64_t)dchunks);
}

enum StepKind {
    STEP_DONE,          // the result stands: path, retries
    STEP_FRONT,         // the front again (plan_front decides which)
    STEP_GROW_POOL,     // the line-index pool to n entries, then the front again
    STEP_GROW_STAGE,    // the walked groups' stage to stage_chunks(), then the front again
    STEP_GENERAL,       // the general kernels behind a refused fast path
    STEP_REPAIR,        // a repair pass
    STEP_RANKED,        // the list-ranking tier (only_if_sparse)
    STEP_WALK,          // the one-wave walk
    STEP_FAIL           // code, text
};
struct Step {
    StepKind kind = STEP_DONE;
    bool front_counts = false;    // this report was a front's and it stood: its times go into the result
    int path = 0, retries = 0;
    unsigned long long n = 0;
    bool only_if_sparse = false;
    int code = 0;
    const char *text = nullptr;
};

namespace scanwalk {
inline Step step(StepKind k) { Step s; s.kind = k; return s; }
inline Step failed(const char *text) { Step s = step(STEP_FAIL); s.code = WALK_E_INTERNAL; s.text = text; return s; }
inline bool tiers(const ScanWalk &st) { return !st.serial && !st.go_ranked; }     // the group kernels ran: their fallbacks apply

inline Step done(ScanWalk &st, InputMemory &mem, const Report &r)
{
    if (tiers(st) && st.lite_ran && (int64_t)r.n_declined * 4 > (int64_t)st.ngroups) mem.lite_skip = HOLD_OFF;
    Step s = step(STEP_DONE);
    s.path = st.path | ((st.decode && st.wide) ? WALK_PATH_IN_PLACE : 0);
    s.retries = st.retries + st.repairs;
    return s;
}

// A guess the verification rejected is repaired, not escalated: the rejected groups are re-run from their predecessor's
// exit and everything is verified again.  Every round makes the first rejected group exact, so the first bad group moves
// forward; a round that does not move it (a group that does not fit the kernel at all) ends the repairs.  With list ranking
// behind them the passes only mend sporadic wrong guesses (two rounds); records that span whole groups correct one another a
// few groups per round, and list ranking is the tool for that.  (Groups that do not FIT -- bad_irregular, dense tiles -- are
// walked one repair pass after their predecessor: those passes go on.)
inline Step after_groups(ScanWalk &st, InputMemory &mem, const Report &r, const Switches &sw)
{
    if (tiers(st)) {
        if (st.round < 16 && r.fallback && r.bad_group > st.prev_bad && r.bad_group < st.ngroups && !(r.err & WALK_ERR_DSTAGE)) {
            bool stop = !sw.no_ranked && st.round >= 2 && !r.bad_irregular;
            // a guess in eight did not stand and the records are long (2.5 KB and more on average: wrapped reads from
            // ~1.2 kb): list ranking needs no guess and, at one wave per "\n@" match, costs less than two such passes there
            stop = stop || (!sw.no_ranked && !r.bad_irregular && (int64_t)r.n_bad * 8 > (int64_t)st.ngroups &&
                            r.approx_records * 2560 < st.n_bytes);
            stop = stop || (st.round >= 4 && !r.bad_irregular && r.bad_group - st.first_bad < st.round * std::max(st.ngroups / 64, 1));
            if (!stop) {
                st.prev_bad = r.bad_group;
                st.phase = PH_REPAIR;
                return step(STEP_REPAIR);
            }
        }
        // more groups were walked (dense regions, ffq_dense.h) than their stage has chunks for: size it for what was asked
        // and run the chain kernels again, from the index that is there
        if (r.err & WALK_ERR_DSTAGE) {
            if (st.retries >= 4) return failed("the walked groups' stage stays too small");
            st.retries++;
            st.index_done = true;
            st.fast4_failed = true;
            return step(STEP_GROW_STAGE);
        }
        // second tier: the same kernels with the LDS budget for short lines / short records (only a group that does not
        // FIT is helped by it; a guess that stays wrong is not); the next scans of this context start there
        if (r.fallback && !st.dense_cfg && r.bad_irregular) {
            st.dense_cfg = true;
            mem.dense_skip = HOLD_OFF;
            return step(STEP_FRONT);
        }
    }
    st.path = st.dense_cfg ? 2 : 0;
    bool walk = st.serial || (tiers(st) && r.fallback);
    if (!st.serial && !sw.no_ranked && (st.go_ranked || r.fallback)) {
        // the group kernels could not prove a chain (records long against a group): list ranking
        st.phase = PH_RANKED;
        Step s = step(STEP_RANKED);
        s.only_if_sparse = st.go_ranked && !st.force_ranked;
        return s;
    }
    if (st.go_ranked) walk = true;
    if (!walk) return done(st, mem, r);
    st.path = 1;
    st.phase = PH_WALK;
    return step(STEP_WALK);
}

inline Step first_round(ScanWalk &st, InputMemory &mem, const Report &r, const Switches &sw)
{
    st.round = 0; st.prev_bad = -1; st.first_bad = r.bad_group;
    return after_groups(st, mem, r, sw);
}

inline Step after_front(ScanWalk &st, InputMemory &mem, const Report &r, const Switches &sw)
{
    if (r.err & WALK_ERR_POOL) {
        // dense tiles did not fit the overflow pool: size it for what was asked and re-run
        if (st.retries >= 2) return failed("line-index pool overflow persists");
        st.retries++;
        st.index_done = false;
        Step s = step(STEP_GROW_POOL);
        s.n = std::max<unsigned long long>(r.pool_head + (r.pool_head >> 4), WALK_POOL_MIN);
        return s;
    }
    if (r.err & WALK_ERR_INTERNAL) return failed("chain kernel invariant failed");
    st.untimed = false;
    st.index_done = true;
    if (st.probe4) {
        // the probe's verdict: the next scan starts with the fast path again, or HOLD_OFF more do not ask
        st.probe4 = false;
        if (r.fast4_hint == 1) { mem.fast4_remember = false; mem.fast4_skip = 0; }
        else mem.fast4_skip = HOLD_OFF;
    }
    if (st.stage != 1) return first_round(st, mem, r, sw);
    if (!r.fallback) {
        Step s = step(STEP_DONE);
        s.path = st.fused ? 6 : 3; s.retries = st.retries;
        if (st.fused) { mem.fused_backoff = HOLD_OFF; mem.fz_in_place = st.in_place; }
        return s;
    }
    if (st.fused) {
        // the single pass did not stand (lines longer than a tile, a quality line that is not as long as its sequence line,
        // text in front of the first record, not four-line input at all ...)
        if (!st.in_place && !st.seg_refused && (r.fused_bad & WALK_FZ_BAD_SHAPE) && !(r.fused_bad & WALK_FZ_BAD_INDEX) &&
            st.qual_cap >= st.ntiles * WALK_TILE) {
            // a shape the segments cannot take (a line longer than SG_EXT behind a tile, no S P pair in a tile of a few
            // long lines) and the caller's buffer has room for the in-place layout: that pass next
            st.seg_refused = true;
            st.fused = false;
            st.index_done = false;          // (that pass builds the index itself)
            st.retries++;
            return step(STEP_FRONT);
        }
        // the two-pass kernels, from the index it built if that is whole
        mem.fz_in_place = false;
        st.no_fused = true;
        st.fused = false;
        mem.fused_skip = mem.fused_backoff;
        mem.fused_backoff = std::min(4 * mem.fused_backoff + 3, 1023);
        st.index_done = !(r.fused_bad & WALK_FZ_BAD_INDEX);
        st.retries++;
        return step(STEP_FRONT);
    }
    if (r.fast4_dense && !st.dense4 && !st.fused && !st.no_fused) {
        // the row kernel met a DENSE tile (lines under 16 bytes on average: reads of a dozen bases): its DENSE instantiation
        // takes those -- the same front again from the index that is there, and the context's next scans start with it
        st.dense4 = true;
        mem.dense4_remember = true;
        st.retries++;
        return step(STEP_FRONT);
    }
    // not plain four-line input: the general kernels, from the same line index.  The next scans of this context skip the
    // attempt (and the host round trip it costs here).
    st.fast4_failed = true;
    mem.fast4_remember = true;
    mem.fast4_skip = HOLD_OFF;
    st.phase = PH_GENERAL;
    return step(STEP_GENERAL);
}
}  // namespace scanwalk

// What scan_finish decides after each report: the report is the one of st.phase (a front's, or the tier's that the last
// step ran).
inline Step next_step(ScanWalk &st, InputMemory &mem, const Report &r, const Switches &sw)
{
    using namespace scanwalk;
    switch (st.phase) {
    case PH_FRONT: {
        Step s = after_front(st, mem, r, sw);
        s.front_counts = !(r.err & (WALK_ERR_POOL | WALK_ERR_INTERNAL));
        return s;
    }
    case PH_GENERAL:
        if (r.err & WALK_ERR_INTERNAL) return failed("chain kernel invariant failed");
        return first_round(st, mem, r, sw);
    case PH_REPAIR:
        st.repairs++;
        if (r.err & WALK_ERR_INTERNAL) return failed("chain kernel invariant failed");
        st.round++;
        return after_groups(st, mem, r, sw);
    case PH_RANKED:
        if (r.ranked == RK_DENSE) {
            // a context that remembers long records meets short ones again: the input has changed character, what is
            // remembered of it is void -- the usual tiers, from the line index that is there
            mem.ranked_skip = 0;
            mem.fast4_skip = 0;
            mem.fast4_remember = false;
            st.go_ranked = false;
            st.fast4_failed = false;
            return step(STEP_FRONT);
        }
        if (r.ranked == RK_CANNOT) {
            st.path = 1;
            st.phase = PH_WALK;
            return step(STEP_WALK);
        }
        st.path = 5;
        if (!st.force_ranked) mem.ranked_skip = HOLD_OFF;     // and the next scans of this context start there
        return done(st, mem, r);
    case PH_WALK:
        break;
    }
    return done(st, mem, r);
}

}  // namespace ffq

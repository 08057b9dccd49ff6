// The tier ladder of a buffer scan (csrc/ffq_scanwalk.h: plan_front, plan_lite, next_step, InputMemory), driven on the host
// over scripted reports.  The driver below does what enqueue_front / enqueue_general / scan_finish of csrc/ffq_hip.hip do with
// the device left out: plan_front at every front, plan_lite where the general kernels start, next_step after every report.
// Every expectation is written out here, none is computed from the header.
//
//   clang++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I <package>/csrc tests/scan_walk_host.cpp -o scan_walk_host
// Exit status 0 and "ok" on the last line, or 1 and a line per failure.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "ffq_scanwalk.h"

using namespace ffq;

static int g_fail = 0, g_checks = 0;
static const char *g_what = "";
#define CHECK(cond) do { g_checks++; if (!(cond)) { g_fail++; std::printf("FAIL %s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, g_what); } } while (0)

constexpr int64_t NTILES = 64, N_BYTES = 64 * 16384;                   // 1 MiB
constexpr int NGROUPS = 128;
constexpr int64_t ROOM_SEG = 64 * 8704, ROOM_IN_PLACE = 64 * 16384;      // quality buffers: segments only / the in-place layout too
constexpr uint32_t E_POOL = 1, E_INTERNAL = 2, E_DSTAGE = 4;

struct Ctx { InputMemory mem; Switches sw{false, false, false, false}; };
struct Call {
    bool serial = false, decode = false, single = false, f_ranked = false, f_general = false, poll = false, no_timing = false;
    int64_t offset = 0, qual_cap = 0;
    bool aligned = true;
};
struct Scan { ScanWalk st; FrontPlan p; CallFacts f{}; bool lite = false; int fronts = 0, lite_asked = 0; };

static void front(Ctx &c, Scan &s)
{
    s.p = plan_front(s.st, c.mem, s.f, c.sw);
    s.fronts++;
    if (s.p.front == FRONT_GENERAL) { s.lite = plan_lite(s.st, c.mem, c.sw); s.lite_asked++; }
}

static Scan submit(Ctx &c, const Call &k)
{
    Scan s;
    s.st.serial = k.serial; s.st.decode = k.decode; s.st.single_pass = k.single; s.st.force_ranked = k.f_ranked;
    s.st.force_general = k.f_general; s.st.poll_result = k.poll; s.st.no_timing = k.no_timing;
    s.st.ntiles = NTILES; s.st.ngroups = NGROUPS;
    s.f = CallFacts{k.offset, k.qual_cap, N_BYTES, k.aligned};
    front(c, s);
    return s;
}

static Step tell(Ctx &c, Scan &s, const Report &r)
{
    const Step t = next_step(s.st, c.mem, r, c.sw);
    if (t.kind == STEP_FRONT || t.kind == STEP_GROW_POOL || t.kind == STEP_GROW_STAGE) front(c, s);
    if (t.kind == STEP_GENERAL) { s.lite = plan_lite(s.st, c.mem, c.sw); s.lite_asked++; }
    return t;
}

static Report ok() { return Report{}; }
static Report fb(int bad_group = 0, int irregular = 0)
{
    Report r;
    r.fallback = 1; r.bad_group = bad_group; r.bad_irregular = irregular; r.n_bad = 1; r.approx_records = 4000;
    return r;
}
static Report err(uint32_t bits, unsigned long long pool_head = 0)
{
    Report r = fb(2);
    r.err = bits; r.pool_head = pool_head;
    return r;
}
static Report ranked(int how) { Report r = fb(2); r.ranked = how; return r; }
static bool is_done(const Step &t, int path, int retries) { return t.kind == STEP_DONE && t.path == path && t.retries == retries; }
static bool is_fail(const Step &t, const char *text) { return t.kind == STEP_FAIL && t.code == -6 && t.text && !std::strcmp(t.text, text); }
static bool fresh(const InputMemory &m)
{
    return !m.fast4_remember && m.fast4_skip == 0 && m.ranked_skip == 0 && m.dense_skip == 0 && m.lite_skip == 0 && !m.dense4_remember &&
           m.fused_skip == 0 && m.fused_backoff == 15 && !m.fz_in_place;
}

static void fresh_routes()
{
    g_what = "four-line input";
    CHECK(HOLD_OFF == 15);
    {
        Ctx c;
        Scan s = submit(c, Call{});
        CHECK(s.p.front == FRONT_FAST4 && !s.p.dense4 && !s.p.probe4 && !s.p.wide && s.p.run_index && !s.p.untimed && !s.p.polled);
        CHECK(s.lite_asked == 0);
        const Step t = tell(c, s, ok());
        CHECK(is_done(t, 3, 0) && t.front_counts);
        CHECK(fresh(c.mem));
    }
    g_what = "single pass";
    {
        Ctx c;
        c.mem.fused_backoff = 63;
        Call k; k.decode = true; k.single = true; k.qual_cap = ROOM_SEG;
        Scan s = submit(c, k);
        CHECK(s.p.front == FRONT_FUSED && !s.p.in_place && !s.p.polled);
        CHECK(is_done(tell(c, s, ok()), 6, 0));
        CHECK(c.mem.fused_backoff == 15 && !c.mem.fz_in_place);
        // a context that remembers the in-place pass starts with it where the buffer has the room ...
        c.mem.fz_in_place = true;
        k.qual_cap = ROOM_IN_PLACE;
        s = submit(c, k);
        CHECK(s.p.front == FRONT_FUSED && s.p.in_place);
        CHECK(is_done(tell(c, s, ok()), 6, 0) && c.mem.fz_in_place);
        // ... and with the segmented one where it has not, which it then remembers
        k.qual_cap = ROOM_SEG;
        s = submit(c, k);
        CHECK(s.p.front == FRONT_FUSED && !s.p.in_place);
        CHECK(is_done(tell(c, s, ok()), 6, 0) && !c.mem.fz_in_place);
        // not without alignment, room, or with text in front
        k.aligned = false;
        CHECK(submit(c, k).p.front == FRONT_FAST4);
        k.aligned = true; k.qual_cap = ROOM_SEG - 1;
        CHECK(submit(c, k).p.front == FRONT_FAST4);
        k.qual_cap = ROOM_SEG; k.offset = 16;
        CHECK(submit(c, k).p.front == FRONT_FAST4);
        k.offset = 15;
        CHECK(submit(c, k).p.front == FRONT_FUSED);
    }
    g_what = "dense tile";
    {
        Ctx c;
        Scan s = submit(c, Call{});
        Report r = fb(); r.fast4_dense = 1;
        Step t = tell(c, s, r);
        CHECK(t.kind == STEP_FRONT && t.front_counts);
        CHECK(s.p.front == FRONT_FAST4 && s.p.dense4 && !s.p.run_index);
        CHECK(c.mem.dense4_remember);
        CHECK(is_done(tell(c, s, ok()), 3, 1));
        s = submit(c, Call{});
        CHECK(s.p.front == FRONT_FAST4 && s.p.dense4 && s.p.run_index);
        // the DENSE kernel refused too: the general kernels
        r = fb(); r.fast4_dense = 1;
        CHECK(tell(c, s, r).kind == STEP_GENERAL);
    }
}

static void wrapped_and_probe()
{
    g_what = "wrapped input and the probe";
    Ctx c;
    Scan s = submit(c, Call{});
    Step t = tell(c, s, fb());
    CHECK(t.kind == STEP_GENERAL && t.front_counts);
    CHECK(c.mem.fast4_remember && c.mem.fast4_skip == 15);
    CHECK(s.lite && s.lite_asked == 1);
    t = tell(c, s, ok());
    CHECK(is_done(t, 0, 0) && !t.front_counts);
    for (int round = 0; round < 2; round++) {
        // 15 scans start general without asking, the 16th carries the probe
        for (int i = 1; i <= 15; i++) {
            s = submit(c, Call{});
            CHECK(s.p.front == FRONT_GENERAL && !s.p.probe4 && s.p.run_index && !s.p.wide);
            CHECK(c.mem.fast4_skip == 15 - i);
            CHECK(is_done(tell(c, s, ok()), 0, 0));
        }
        s = submit(c, Call{});
        CHECK(s.p.front == FRONT_GENERAL && s.p.probe4 && !s.p.dense4);
        CHECK(c.mem.fast4_skip == 0 && c.mem.fast4_remember);
        Report r = ok();
        r.fast4_hint = round == 0 ? 0 : 1;
        CHECK(is_done(tell(c, s, r), 0, 0));
        if (round == 0) CHECK(c.mem.fast4_remember && c.mem.fast4_skip == 15);      // anything but 1: hold off again
        else CHECK(!c.mem.fast4_remember && c.mem.fast4_skip == 0);
    }
    CHECK(fresh(c.mem));
    CHECK(submit(c, Call{}).p.front == FRONT_FAST4);
    // hint 2 is not 1
    c.mem.fast4_remember = true;
    s = submit(c, Call{});
    CHECK(s.p.probe4);
    Report r = ok(); r.fast4_hint = 2;
    tell(c, s, r);
    CHECK(c.mem.fast4_remember && c.mem.fast4_skip == 15);
    // the probe runs the row kernel the context remembers; no probe on a serial or ranked start
    c.mem.fast4_skip = 0; c.mem.dense4_remember = true;
    s = submit(c, Call{});
    CHECK(s.p.probe4 && s.p.dense4);
    Call k; k.serial = true;
    s = submit(c, k);
    CHECK(s.p.front == FRONT_INDEX_ONLY && !s.p.probe4 && !s.p.dense4);
    k = Call{}; k.f_ranked = true;
    CHECK(!submit(c, k).p.probe4);
}

static void dense_configuration()
{
    g_what = "dense configuration";
    Ctx c;
    Call k; k.f_general = true;
    Scan s = submit(c, k);
    CHECK(s.p.front == FRONT_GENERAL && s.lite);
    CHECK(tell(c, s, fb(3, 1)).kind == STEP_REPAIR);         // a group that does not fit is walked a pass later ...
    Step t = tell(c, s, fb(3, 1));                            // ... and stayed where it was: the dense configuration
    CHECK(t.kind == STEP_FRONT && !t.front_counts);
    CHECK(c.mem.dense_skip == 15);
    CHECK(s.p.front == FRONT_GENERAL && !s.p.run_index && !s.lite && s.st.dense_cfg);
    CHECK(c.mem.dense_skip == 15);                            // (not consumed by the scan that set it)
    CHECK(is_done(tell(c, s, ok()), 2, 1));
    s = submit(c, k);
    CHECK(s.st.dense_cfg && c.mem.dense_skip == 14 && !s.lite);
    CHECK(is_done(tell(c, s, ok()), 2, 0));
    // a plain scan of that context starts there too: no fast path
    s = submit(c, Call{});
    CHECK(s.p.front == FRONT_GENERAL && c.mem.dense_skip == 13);
    // consumed only with !dense_cfg && !index_done
    ScanWalk st; st.ntiles = NTILES; st.ngroups = NGROUPS; st.index_done = true;
    plan_front(st, c.mem, s.f, c.sw);
    CHECK(c.mem.dense_skip == 13 && !st.dense_cfg);
    st = ScanWalk{}; st.ntiles = NTILES; st.ngroups = NGROUPS; st.dense_cfg = true;
    plan_front(st, c.mem, s.f, c.sw);
    CHECK(c.mem.dense_skip == 13);
}

static void repair_rounds()
{
    Call k; k.f_general = true;
    g_what = "repairs: advancing, then round >= 2 and not irregular";
    {
        Ctx c;
        Scan s = submit(c, k);
        CHECK(tell(c, s, fb(2)).kind == STEP_REPAIR);
        CHECK(tell(c, s, fb(5)).kind == STEP_REPAIR);
        Step t = tell(c, s, fb(9));
        CHECK(t.kind == STEP_RANKED && !t.only_if_sparse);
        CHECK(is_done(tell(c, s, ranked(RK_GO)), 5, 2));
        CHECK(c.mem.ranked_skip == 15);
    }
    g_what = "repairs: a guess in eight wrong, long records";
    {
        Ctx c;
        Scan s = submit(c, k);
        Report r = fb(1); r.n_bad = 17; r.approx_records = 409;       // 136 > 128; 1047040 < 1048576
        CHECK(tell(c, s, r).kind == STEP_RANKED);
        s = submit(c, k);
        r.approx_records = 410;                                        // 1049600: the records are short
        CHECK(tell(c, s, r).kind == STEP_REPAIR);
        s = submit(c, k);
        r.approx_records = 409; r.n_bad = 16;                          // 128 > 128 is false
        CHECK(tell(c, s, r).kind == STEP_REPAIR);
        s = submit(c, k);
        r.n_bad = 17; r.bad_irregular = 1;
        CHECK(tell(c, s, r).kind == STEP_REPAIR);
    }
    g_what = "repairs: slow advance from round 4";
    {
        Ctx c;
        c.sw.no_ranked = true;                  // (with the ranked tier behind them the repairs end at round 2)
        Scan s = submit(c, k);
        CHECK(tell(c, s, fb(0)).kind == STEP_REPAIR);
        CHECK(tell(c, s, fb(2)).kind == STEP_REPAIR);
        CHECK(tell(c, s, fb(4)).kind == STEP_REPAIR);
        CHECK(tell(c, s, fb(6)).kind == STEP_REPAIR);
        CHECK(tell(c, s, fb(7)).kind == STEP_WALK);           // round 4: 7 - 0 < 4 * (128 / 64)
        CHECK(is_done(tell(c, s, fb(7)), 1, 4));
        s = submit(c, k);
        for (int g : {0, 2, 4, 6}) CHECK(tell(c, s, fb(g)).kind == STEP_REPAIR);
        CHECK(tell(c, s, fb(8)).kind == STEP_REPAIR);         // 8 - 0 < 8 is false
        CHECK(tell(c, s, fb(9)).kind == STEP_WALK);           // round 5: 9 < 10
    }
    g_what = "repairs: no movement";
    {
        Ctx c;
        Scan s = submit(c, k);
        CHECK(tell(c, s, fb(3)).kind == STEP_REPAIR);
        CHECK(tell(c, s, fb(3)).kind == STEP_RANKED);
        s = submit(c, k);
        CHECK(tell(c, s, fb(NGROUPS)).kind == STEP_RANKED);   // no group to repair
        s = submit(c, k);
        CHECK(tell(c, s, fb(3)).kind == STEP_REPAIR);
        CHECK(is_done(tell(c, s, ok()), 0, 1));               // mended
    }
    g_what = "repairs: the cap of 16";
    {
        Ctx c;
        c.mem.dense_skip = 1;
        Scan s = submit(c, k);
        int passes = 0;
        Step t;
        for (int g = 0; g < 40; g++) {
            t = tell(c, s, fb(g, 1));
            if (t.kind != STEP_REPAIR) break;
            passes++;
        }
        CHECK(passes == 16 && t.kind == STEP_RANKED);
        CHECK(is_done(tell(c, s, ranked(RK_GO)), 5, 16));
    }
    g_what = "repairs: ERR_DSTAGE ends them";
    {
        Ctx c;
        Scan s = submit(c, k);
        CHECK(tell(c, s, fb(2)).kind == STEP_REPAIR);
        Step t = tell(c, s, err(E_DSTAGE));
        CHECK(t.kind == STEP_GROW_STAGE && !t.front_counts);
        CHECK(s.p.front == FRONT_GENERAL && !s.p.run_index && s.st.retries == 1 && s.st.repairs == 1);
        CHECK(is_done(tell(c, s, ok()), 0, 2));
    }
    g_what = "ERR_INTERNAL behind a tier";
    {
        Ctx c;
        Scan s = submit(c, k);
        CHECK(tell(c, s, fb(2)).kind == STEP_REPAIR);
        CHECK(is_fail(tell(c, s, err(E_INTERNAL)), "chain kernel invariant failed"));
        s = submit(c, Call{});
        CHECK(tell(c, s, fb()).kind == STEP_GENERAL);
        CHECK(is_fail(tell(c, s, err(E_INTERNAL)), "chain kernel invariant failed"));
    }
}

static void ranked_tier()
{
    g_what = "ranked: the verdict";
    CHECK(ranked_verdict(0x7FFFFFF0ll, (int64_t)1 << 50, false) == RK_CANNOT);
    CHECK(ranked_verdict(0x7FFFFFEFll, (int64_t)1 << 50, true) == RK_GO);
    CHECK(ranked_verdict(2049, N_BYTES, true) == RK_DENSE);
    CHECK(ranked_verdict(2048, N_BYTES, true) == RK_GO);
    CHECK(ranked_verdict(2049, N_BYTES, false) == RK_GO);
    CHECK(RK_GO == 0 && RK_CANNOT == 1 && RK_DENSE == 2);
    g_what = "ranked: a remembered start meets short records";
    {
        Ctx c;
        c.mem.ranked_skip = 15; c.mem.fast4_remember = true; c.mem.fast4_skip = 7;
        Scan s = submit(c, Call{});
        CHECK(s.p.front == FRONT_INDEX_ONLY && c.mem.ranked_skip == 14 && c.mem.fast4_skip == 6 && s.lite_asked == 0);
        Step t = tell(c, s, ok());
        CHECK(t.kind == STEP_RANKED && t.only_if_sparse && t.front_counts);
        t = tell(c, s, ranked(RK_DENSE));
        CHECK(t.kind == STEP_FRONT && !t.front_counts);
        CHECK(fresh(c.mem));
        CHECK(s.p.front == FRONT_FAST4 && !s.p.run_index);
        CHECK(is_done(tell(c, s, ok()), 3, 0));
    }
    g_what = "ranked: cannot run";
    {
        Ctx c;
        c.mem.ranked_skip = 2;
        Scan s = submit(c, Call{});
        CHECK(tell(c, s, ok()).kind == STEP_RANKED);
        CHECK(tell(c, s, ranked(RK_CANNOT)).kind == STEP_WALK);
        CHECK(is_done(tell(c, s, ok()), 1, 0));
        CHECK(c.mem.ranked_skip == 1);
    }
    g_what = "ranked: success";
    {
        Ctx c;
        c.mem.ranked_skip = 1;
        Scan s = submit(c, Call{});
        CHECK(c.mem.ranked_skip == 0);
        CHECK(tell(c, s, ok()).kind == STEP_RANKED);
        CHECK(is_done(tell(c, s, ranked(RK_GO)), 5, 0));
        CHECK(c.mem.ranked_skip == 15);
        Ctx d;
        Call k; k.f_ranked = true;
        s = submit(d, k);
        CHECK(s.p.front == FRONT_INDEX_ONLY);
        Step t = tell(d, s, ok());
        CHECK(t.kind == STEP_RANKED && !t.only_if_sparse);
        CHECK(is_done(tell(d, s, ranked(RK_GO)), 5, 0));
        CHECK(fresh(d.mem));
        // FFQ_NO_RANKED: an index-only start goes to the walk
        d.sw.no_ranked = true;
        s = submit(d, k);
        CHECK(tell(d, s, ok()).kind == STEP_WALK);
        CHECK(is_done(tell(d, s, ok()), 1, 0));
    }
}

static void other_starts()
{
    g_what = "FFQ_F_FORCE_SERIAL";
    Ctx c;
    c.mem.ranked_skip = 3;
    Call k; k.serial = true;
    Scan s = submit(c, k);
    CHECK(s.p.front == FRONT_INDEX_ONLY && s.p.run_index && c.mem.ranked_skip == 3 && s.lite_asked == 0);
    Step t = tell(c, s, ok());
    CHECK(t.kind == STEP_WALK && t.front_counts);
    CHECK(is_done(tell(c, s, ok()), 1, 0));
    g_what = "FFQ_F_FORCE_GENERAL";
    Ctx d;
    k = Call{}; k.f_general = true;
    s = submit(d, k);
    CHECK(s.p.front == FRONT_GENERAL && !s.p.probe4 && s.lite);
    CHECK(is_done(tell(d, s, ok()), 0, 0));
    CHECK(fresh(d.mem));
    g_what = "FFQ_NO_FAST4";
    d.sw.no_fast4 = true;
    s = submit(d, Call{});
    CHECK(s.p.front == FRONT_GENERAL);
    d.sw.no_fast4 = false;
    CHECK(submit(d, Call{}).p.front == FRONT_FAST4);
    g_what = "FFQ_F_POLL_RESULT | FFQ_F_NO_TIMING";
    k = Call{}; k.poll = true; k.no_timing = true;
    s = submit(d, k);
    CHECK(s.p.polled && s.p.untimed);
    Report r = fb(); r.fast4_dense = 1;
    CHECK(tell(d, s, r).kind == STEP_FRONT);
    CHECK(s.p.polled && !s.p.untimed);                        // (the index is there: nothing to leave unmarked)
    k.decode = true; k.qual_cap = ROOM_SEG;
    s = submit(d, k);
    CHECK(!s.p.polled && !s.p.untimed);
    k = Call{}; k.poll = true;
    s = submit(d, k);
    CHECK(s.p.polled && !s.p.untimed);
}

static void limits()
{
    g_what = "pool overflow";
    {
        Ctx c;
        Scan s = submit(c, Call{});
        Step t = tell(c, s, err(E_POOL, 2000000));
        CHECK(t.kind == STEP_GROW_POOL && t.n == 2125000 && !t.front_counts);
        CHECK(s.p.run_index && s.st.retries == 1);
        t = tell(c, s, err(E_POOL | E_DSTAGE, 100));
        CHECK(t.kind == STEP_GROW_POOL && t.n == 1048576);
        CHECK(is_fail(tell(c, s, err(E_POOL, 100)), "line-index pool overflow persists"));
        // a counter is consumed again when the front is planned again without an index
        Ctx d;
        d.mem.ranked_skip = 5;
        s = submit(d, Call{});
        CHECK(d.mem.ranked_skip == 4);
        CHECK(tell(d, s, err(E_POOL, 100)).kind == STEP_GROW_POOL);
        CHECK(d.mem.ranked_skip == 3);
    }
    g_what = "stage too short";
    {
        Ctx c;
        Call k; k.f_general = true;
        Scan s = submit(c, k);
        for (int i = 1; i <= 4; i++) {
            Step t = tell(c, s, err(E_DSTAGE));
            CHECK(t.kind == STEP_GROW_STAGE && t.front_counts);
            CHECK(s.st.retries == i && !s.p.run_index && s.fronts == i + 1);
        }
        CHECK(is_fail(tell(c, s, err(E_DSTAGE)), "the walked groups' stage stays too small"));
        CHECK(stage_chunks(100, 64) == 128);
        CHECK(stage_chunks(1000, 64) == 1133);
        CHECK(stage_chunks(0xFFFFFFFFu, 64) == 4831838214ll);
        // a refused fast path that walked too many groups does not try the fast path again
        Ctx d;
        s = submit(d, Call{});
        CHECK(tell(d, s, fb()).kind == STEP_GENERAL);
        CHECK(tell(d, s, err(E_DSTAGE)).kind == STEP_GROW_STAGE);
        CHECK(s.p.front == FRONT_GENERAL && !s.p.probe4 && !s.p.run_index);
    }
    g_what = "ERR_INTERNAL";
    {
        Ctx c;
        Scan s = submit(c, Call{});
        Step t = tell(c, s, err(E_INTERNAL));
        CHECK(is_fail(t, "chain kernel invariant failed") && !t.front_counts);
        CHECK(fresh(c.mem));
    }
}

static void single_pass_refused()
{
    Call k; k.decode = true; k.single = true;
    Report shape = fb(); shape.fused_bad = 1;
    Report index = fb(); index.fused_bad = 1 | 4;
    g_what = "single pass refused by shape, with room";
    {
        Ctx c;
        k.qual_cap = ROOM_IN_PLACE;
        Scan s = submit(c, k);
        CHECK(s.p.front == FRONT_FUSED && !s.p.in_place);
        Step t = tell(c, s, shape);
        CHECK(t.kind == STEP_FRONT && t.front_counts);
        CHECK(s.p.front == FRONT_FUSED && s.p.in_place && !s.st.index_done);
        CHECK(c.mem.fused_skip == 0 && c.mem.fused_backoff == 15);
        CHECK(is_done(tell(c, s, ok()), 6, 1));
        CHECK(c.mem.fz_in_place);
        // the in-place pass refused as well: the two-pass kernels
        s = submit(c, k);
        CHECK(s.p.in_place);
        CHECK(tell(c, s, shape).kind == STEP_FRONT);
        CHECK(s.p.front == FRONT_FAST4 && !s.p.run_index && !c.mem.fz_in_place && c.mem.fused_skip == 15);
    }
    g_what = "single pass refused without room";
    {
        Ctx c;
        k.qual_cap = ROOM_IN_PLACE - 1;
        Scan s = submit(c, k);
        CHECK(tell(c, s, shape).kind == STEP_FRONT);
        CHECK(s.st.no_fused && c.mem.fused_skip == 15 && c.mem.fused_backoff == 63);
        CHECK(s.p.front == FRONT_FAST4 && !s.p.run_index && !s.p.polled);       // the index kept
        // a single pass that was refused does not try the dense row kernel
        Report r = fb(); r.fast4_dense = 1;
        CHECK(tell(c, s, r).kind == STEP_GENERAL);
        CHECK(!c.mem.dense4_remember);
        CHECK(is_done(tell(c, s, ok()), 0, 1));
    }
    g_what = "single pass refused by FZ_BAD_INDEX";
    {
        Ctx c;
        k.qual_cap = ROOM_IN_PLACE;
        Scan s = submit(c, k);
        CHECK(tell(c, s, index).kind == STEP_FRONT);
        CHECK(s.st.no_fused && !s.st.seg_refused && c.mem.fused_skip == 15);
        CHECK(s.p.front == FRONT_FAST4 && s.p.run_index);                         // the index rebuilt
        CHECK(is_done(tell(c, s, ok()), 3, 1));
    }
    g_what = "the back-off";
    {
        Ctx c;
        k.qual_cap = ROOM_SEG;
        const int gaps[5] = {15, 63, 255, 1023, 1023};
        const int backoff[5] = {63, 255, 1023, 1023, 1023};
        for (int i = 0; i < 5; i++) {
            Scan s = submit(c, k);
            CHECK(s.p.front == FRONT_FUSED);
            tell(c, s, shape);
            CHECK(c.mem.fused_skip == gaps[i] && c.mem.fused_backoff == backoff[i]);
            tell(c, s, ok());
            int held = 0;
            while (held < 5000) {
                s = submit(c, k);
                if (s.p.front != FRONT_FAST4) break;
                tell(c, s, ok());
                held++;
            }
            CHECK(held == gaps[i]);
        }
        Scan s = submit(c, k);                    // an attempt that stands resets the back-off
        CHECK(s.p.front == FRONT_FUSED);
        CHECK(is_done(tell(c, s, ok()), 6, 0) && c.mem.fused_backoff == 15);
    }
}

static void wide()
{
    g_what = "wide";
    Ctx c;
    Call k; k.f_general = true; k.decode = true; k.single = true; k.qual_cap = ROOM_IN_PLACE;
    Scan s = submit(c, k);
    CHECK(s.p.front == FRONT_GENERAL && s.p.wide);
    // kept across a re-entry with the index done, whatever the switch says by then
    c.sw.no_wide = true;
    CHECK(tell(c, s, err(E_DSTAGE)).kind == STEP_GROW_STAGE);
    CHECK(s.p.wide && !s.p.run_index);
    CHECK(is_done(tell(c, s, ok()), 8, 1));
    s = submit(c, k);
    CHECK(!s.p.wide);
    CHECK(is_done(tell(c, s, ok()), 0, 0));
    c.sw.no_wide = false;
    k.aligned = false;
    CHECK(!submit(c, k).p.wide);
    k.aligned = true; k.qual_cap = ROOM_IN_PLACE - 1;
    CHECK(!submit(c, k).p.wide);
    k.qual_cap = ROOM_IN_PLACE; k.single = false;
    CHECK(!submit(c, k).p.wide);
    k.single = true; k.decode = false;
    CHECK(!submit(c, k).p.wide);
    // a scan that may try the fast path has the single pass, not this; refused there, it has its index and the packed decode
    k = Call{}; k.decode = true; k.single = true; k.qual_cap = ROOM_IN_PLACE; k.aligned = false;
    s = submit(c, k);
    CHECK(s.p.front == FRONT_FAST4 && !s.p.wide);
    CHECK(tell(c, s, fb()).kind == STEP_GENERAL);
    CHECK(!s.st.wide);
    CHECK(is_done(tell(c, s, ok()), 0, 0));
    // the ranked, walked and dense routes of a wide scan carry the bit as well
    k = Call{}; k.serial = true; k.decode = true; k.single = true; k.qual_cap = ROOM_IN_PLACE;
    s = submit(c, k);
    CHECK(s.p.front == FRONT_INDEX_ONLY && s.p.wide);
    CHECK(tell(c, s, ok()).kind == STEP_WALK);
    CHECK(is_done(tell(c, s, ok()), 9, 0));
    k.serial = false; k.f_ranked = true;
    s = submit(c, k);
    CHECK(s.p.wide);
    CHECK(tell(c, s, ok()).kind == STEP_RANKED);
    CHECK(is_done(tell(c, s, ranked(RK_GO)), 13, 0));
}

static void lean_kernel()
{
    g_what = "lean kernel";
    Ctx c;
    Call k; k.f_general = true;
    Scan s = submit(c, k);
    Report r = ok(); r.n_declined = 32;                       // 128 > 128 is false
    CHECK(s.lite && is_done(tell(c, s, r), 0, 0) && c.mem.lite_skip == 0);
    s = submit(c, k);
    r.n_declined = 33;
    CHECK(is_done(tell(c, s, r), 0, 0) && c.mem.lite_skip == 15);
    s = submit(c, k);
    CHECK(!s.lite && c.mem.lite_skip == 14);
    CHECK(is_done(tell(c, s, r), 0, 0) && c.mem.lite_skip == 14);       // (the lean kernel did not run: nothing to learn)
    // consumed only where the lean kernel would have run: not by a fast-path scan, not by the dense configuration
    s = submit(c, Call{});
    CHECK(is_done(tell(c, s, ok()), 3, 0) && c.mem.lite_skip == 14 && s.lite_asked == 0);
    c.mem.dense_skip = 1;
    s = submit(c, k);
    CHECK(!s.lite && s.lite_asked == 1 && c.mem.lite_skip == 14);
    tell(c, s, ok());
    c.sw.no_lite = true;
    s = submit(c, k);
    CHECK(!s.lite && c.mem.lite_skip == 14);
    c.sw.no_lite = false;
    // ... and again by a general front that is enqueued a second time
    s = submit(c, k);
    CHECK(c.mem.lite_skip == 13);
    CHECK(tell(c, s, err(E_DSTAGE)).kind == STEP_GROW_STAGE);
    CHECK(c.mem.lite_skip == 12 && !s.lite);
    // set behind the ranked tier and the walk too, from the report that is there then
    Ctx d;
    s = submit(d, k);
    CHECK(tell(d, s, fb(NGROUPS)).kind == STEP_RANKED);
    Report q = ranked(RK_GO); q.n_declined = 40;
    CHECK(is_done(tell(d, s, q), 5, 0) && d.mem.lite_skip == 15 && d.mem.ranked_skip == 15);
}

static void forget_all()
{
    g_what = "forget";
    InputMemory m;
    m.fast4_remember = true; m.fast4_skip = 3; m.ranked_skip = 4; m.dense_skip = 5; m.lite_skip = 6; m.dense4_remember = true;
    m.fused_skip = 7; m.fused_backoff = 1023; m.fz_in_place = true;
    CHECK(!fresh(m));
    forget(m);
    CHECK(fresh(m));
}

int main()
{
    fresh_routes();
    wrapped_and_probe();
    dense_configuration();
    repair_rounds();
    ranked_tier();
    other_starts();
    limits();
    single_pass_refused();
    wide();
    lean_kernel();
    forget_all();
    std::printf("%d checks, %d failures\n", g_checks, g_fail);
    if (g_fail) return 1;
    std::printf("ok\n");
    return 0;
}

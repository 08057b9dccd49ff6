// The loop of the byte-range shards (csrc/ffq_shard_proto.h: sh_settle), driven on the host for ONE rank: the gather hook
// replays hand-made word tables, every other hook writes down that it was called and with what.  Checked: the sequence of
// hook calls and the verdict.  Every expectation is written out here, none is computed from the header.
//
//   clang++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I <package>/csrc tests/shard_settle_host.cpp -o shard_settle_host
// Exit status 0 and "ok" on the last line, or 1 and a line per failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ffq_shard_proto.h"

using namespace ffq;

static int g_fail = 0, g_checks = 0;
static const char *g_what = "";
#define CHECK(cond) do { g_checks++; if (!(cond)) { g_fail++; std::printf("FAIL %s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, g_what); } } while (0)

constexpr int64_t U = -2, NONE = -1;                 // SH_UNKNOWN, SH_NONE, written out
constexpr int64_t E_INTERNAL = -6, NOT_READY = 101, TABLE_FULL = 100, QUAL_FULL = 102, ERR_INCOMPLETE = 3;

struct Words { int64_t exit, first, n, want, had, err, byte, search; };
typedef std::vector<Words> Table;                    // one gather: a row of words per rank

struct Scripted {
    std::vector<Table> tables;                       // what the gathers hand back, in order
    ShView v;
    int rank = 1;
    int mine = 0;                                    // my local failure
    bool refuses = false;
    std::string fail_hook;                           // the hook that fails, with fail_code
    int fail_code = 0;
    // what was seen
    std::string log;
    size_t next = 0;
    int looks = 0, last_rounds = -1, last_regathers = -1;
    std::vector<int64_t> flat;
    int64_t published[SH_WORDS] = {0};

    int fails(const char *hook) const { return fail_hook == hook ? fail_code : 0; }
    int gather(const int64_t **A)
    {
        log += "gather ";
        if (fails("gather")) return fail_code;
        if (next >= tables.size()) { log += "(script ended) "; return -99; }
        flat.clear();
        for (const Words &w : tables[next]) { const int64_t a[SH_WORDS] = {w.exit, w.first, w.n, w.want, w.had, w.err, w.byte, w.search}; flat.insert(flat.end(), a, a + SH_WORDS); }
        next++;
        *A = flat.data();
        return 0;
    }
    const ShView &view() const { return v; }
    int local_failure() const { return mine; }
    void look(const ShRound &, const int64_t *, int rounds, int regathers) { looks++; last_rounds = rounds; last_regathers = regathers; }
    int not_ready(int64_t start)
    {
        log += "not_ready(" + std::to_string(start) + ") ";
        return refuses ? SH_REFUSED : fails("not_ready");
    }
    int grow(const ShRound &d, const int64_t *A)
    {
        log += std::string("grow(") + (d.i_grow ? "me" : "other") + ") ";
        if (d.i_grow) v = sh_make_view(v.lo, v.hi, v.total, v.origin, v.tail, A[(size_t)rank * SH_WORDS + 3]);      // (as a driver does: my view is the larger one)
        return fails("grow");
    }
    int rescan(int64_t start) { log += "rescan(" + std::to_string(start) + ") "; return fails("rescan"); }
    int publish(const int64_t *w)
    {
        if (!w) { log += "stand "; return fails("publish"); }
        memcpy(published, w, sizeof published);
        log += "publish(exit " + std::to_string(w[0]) + " first " + std::to_string(w[1]) + " err " + std::to_string(w[5]) + " search " + std::to_string(w[7]) + ") ";
        return fails("publish");
    }
};

// three ranks over [0, 3000), I am rank 1: [1000, 2000) with 100 bytes of run-in and of look-ahead
static const std::vector<int64_t> B3 = {0, 1000, 2000, 3000};
static Scripted me() { Scripted r; r.v = sh_make_view(1000, 2000, 3000, 0, 100, 100); return r; }
static ShVerdict settle(Scripted &r) { return sh_settle(r, 3, 1, B3); }

// every edge proven: exit[r] == first[r + 1]
static const Table SETTLED = {{1010, 0, 10, 0, 100, 0, 0, 900}, {2020, 1010, 9, 0, 100, 0, 0, 1900}, {NONE, 2020, 8, 0, 0, 0, 0, 2900}};

static Table with(Table t, int r, Words w) { t[(size_t)r] = w; return t; }

static void settled_at_once()
{
    g_what = "settled at once";
    Scripted r = me();
    r.tables = {SETTLED};
    const ShVerdict v = settle(r);
    CHECK(v.kind == ShVerdict::SETTLED && v.ok() && v.rounds == 0 && v.regathers == 0 && v.err_state == 0);
    CHECK(r.log == "gather " && r.looks == 1 && r.last_rounds == 0 && r.last_regathers == 0);
}

static void stream_errors()
{
    g_what = "stream error";
    Scripted r = me();
    r.tables = {with(SETTLED, 2, {NONE, 2020, 8, 0, 0, ERR_INCOMPLETE, 2777, 2700})};       // the failing rank owns rows: its own byte
    ShVerdict v = settle(r);
    CHECK(v.kind == ShVerdict::STREAM_ERROR && v.ok() && v.err_state == 3 && v.err_byte == 2777 && r.log == "gather ");
    // it owns none, nor does rank 1: the byte is the search start of rank 0's exit
    r = me();
    r.tables = {{{2100, 0, 30, 0, 100, 0, 0, 777}, {2100, 2100, 0, 0, 100, 0, 0, 1500}, {NONE, 2100, 0, 0, 0, ERR_INCOMPLETE, 2600, 2500}}};
    v = settle(r);
    CHECK(v.kind == ShVerdict::STREAM_ERROR && v.err_state == 3 && v.err_byte == 777 && r.log == "gather ");
    // the nearest rank to the left that owns a row is rank 1
    r = me();
    r.tables = {{{1010, 0, 10, 0, 100, 0, 0, 900}, {2100, 1010, 5, 0, 100, 0, 0, 1888}, {NONE, 2100, 0, 0, 0, ERR_INCOMPLETE, 2600, 2500}}};
    v = settle(r);
    CHECK(v.kind == ShVerdict::STREAM_ERROR && v.err_byte == 1888);
    // a failure of my own goes first
    r = me();
    r.mine = -4;
    r.tables = {with(SETTLED, 2, {NONE, 2020, 8, 0, 0, ERR_INCOMPLETE, 2777, 2700})};
    v = settle(r);
    CHECK(v.kind == ShVerdict::MINE && v.code == -4 && !v.ok());
}

static void full_and_internal()
{
    g_what = "table full";
    Scripted r = me();
    r.tables = {with(SETTLED, 2, {U, U, 0, 0, 0, TABLE_FULL, 12345, 0})};
    ShVerdict v = settle(r);
    CHECK(v.kind == ShVerdict::TABLE_FULL && v.who == 2 && v.need == 12345 && !v.ok() && r.log == "gather ");
    g_what = "quality buffer full";
    r = me();
    r.tables = {with(SETTLED, 0, {U, U, 0, 0, 100, QUAL_FULL, 999, 0})};
    v = settle(r);
    CHECK(v.kind == ShVerdict::QUAL_FULL && v.who == 0 && v.need == 999 && r.log == "gather ");
    g_what = "internal: a peer's";
    r = me();
    r.tables = {with(SETTLED, 0, {U, U, 0, 0, 100, E_INTERNAL, 0, 0})};
    v = settle(r);
    CHECK(v.kind == ShVerdict::INTERNAL && v.who == 0 && !strcmp(v.what, "unexpected end state of its scan") && v.code == 0 && r.log == "gather ");
    g_what = "internal: nobody can move";
    r = me();
    r.tables = {with(SETTLED, 1, {U, 1010, 9, 0, 100, 0, 0, 1900})};
    v = settle(r);
    CHECK(v.kind == ShVerdict::INTERNAL && v.who == 1 && !strcmp(v.what, "has no exit and nobody can move"));
    g_what = "internal: mine";
    r = me();
    r.mine = -2;
    r.tables = {with(SETTLED, 1, {U, U, 0, 0, 100, E_INTERNAL, 0, 0})};
    v = settle(r);
    CHECK(v.kind == ShVerdict::MINE && v.code == -2 && r.log == "gather ");       // (my code, not "rank 1 failed")
    // THE RECONCILIATION: a lower rank's table is full in the round of my failure -- TABLE_FULL, on me as on everybody
    g_what = "table full in the round of my failure";
    r = me();
    r.mine = -2;
    r.tables = {with(with(SETTLED, 1, {U, U, 0, 0, 100, E_INTERNAL, 0, 0}), 0, {U, U, 0, 0, 100, TABLE_FULL, 4321, 0})};
    v = settle(r);
    CHECK(v.kind == ShVerdict::TABLE_FULL && v.who == 0 && v.need == 4321);
    r = me();
    r.mine = -2;
    r.tables = {with(with(SETTLED, 1, {U, U, 0, 0, 100, E_INTERNAL, 0, 0}), 0, {U, U, 0, 0, 100, QUAL_FULL, 77, 0})};
    v = settle(r);
    CHECK(v.kind == ShVerdict::QUAL_FULL && v.who == 0 && v.need == 77);
    // (one look names the LOWEST rank that has anything to say: a higher rank's full table behind my failure is not seen)
    r = me();
    r.mine = -2;
    r.tables = {with(with(SETTLED, 1, {U, U, 0, 0, 100, E_INTERNAL, 0, 0}), 2, {U, U, 0, 0, 0, TABLE_FULL, 77, 0})};
    v = settle(r);
    CHECK(v.kind == ShVerdict::MINE && v.code == -2);
}

static void not_ready()
{
    const Table NR = with(SETTLED, 2, {U, U, 0, 0, 0, NOT_READY, 0, 0});
    g_what = "not ready: four times, then settled";
    Scripted r = me();
    r.tables = {NR, NR, NR, NR, SETTLED};
    ShVerdict v = settle(r);
    CHECK(v.kind == ShVerdict::SETTLED && v.regathers == 4 && v.rounds == 0);
    CHECK(r.log == "gather not_ready(-1) gather not_ready(-1) gather not_ready(-1) gather not_ready(-1) gather ");
    CHECK(r.looks == 5 && r.last_regathers == 4);
    g_what = "not ready: the fifth is the verdict";
    r = me();
    r.tables = {NR, NR, NR, NR, NR, SETTLED};
    v = settle(r);
    CHECK(v.kind == ShVerdict::NOT_READY && v.regathers == 5 && !v.ok());
    CHECK(r.log == "gather not_ready(-1) gather not_ready(-1) gather not_ready(-1) gather not_ready(-1) gather ");
    g_what = "not ready with a failure of my own";
    r = me();
    r.mine = -4;
    r.tables = {with(SETTLED, 1, {U, U, 0, 0, 100, NOT_READY, 0, 0}), with(SETTLED, 1, {U, U, 0, 0, 100, E_INTERNAL, 0, 0})};
    v = settle(r);
    CHECK(v.kind == ShVerdict::MINE && v.code == -4 && v.regathers == 1);
    CHECK(r.log == "gather publish(exit -2 first -2 err -6 search 0) gather ");         // failed words, made on the host
    CHECK(r.published[2] == 0 && r.published[3] == 0 && r.published[4] == 100 && r.published[6] == 0);
    g_what = "not ready on a rank that refuses";
    r = me();
    r.refuses = true;
    r.tables = {NR, SETTLED};
    v = settle(r);
    CHECK(v.kind == ShVerdict::INTERNAL && v.who == -1 && !strcmp(v.what, "") && r.log == "gather not_ready(-1) ");
}

static void repairs()
{
    g_what = "repair: I grow";
    Scripted r = me();
    r.tables = {with(SETTLED, 1, {U, 1010, 9, 4096, 100, 0, 0, 1900}), SETTLED};
    ShVerdict v = settle(r);
    CHECK(v.kind == ShVerdict::SETTLED && v.rounds == 1 && v.regathers == 0);
    CHECK(r.log == "gather grow(me) rescan(-1) gather " && r.v.head == 4096 && r.last_rounds == 1);      // (the rescan: from the old start)
    g_what = "repair: somebody else grows";
    r = me();
    r.tables = {with(SETTLED, 0, {U, 0, 10, 4096, 100, 0, 0, 900}), SETTLED};
    v = settle(r);
    CHECK(v.kind == ShVerdict::SETTLED && v.rounds == 1 && r.log == "gather grow(other) stand gather ");
    g_what = "repair: I am forced";
    r = me();
    r.tables = {with(SETTLED, 0, {1050, 0, 10, 0, 100, 0, 0, 990}), SETTLED};
    v = settle(r);
    CHECK(v.kind == ShVerdict::SETTLED && v.rounds == 1 && r.log == "gather rescan(990) gather ");
    g_what = "repair: somebody else is forced";
    r = me();
    r.tables = {with(SETTLED, 2, {NONE, 2030, 8, 0, 0, 0, 0, 2900}), SETTLED};
    v = settle(r);
    CHECK(v.kind == ShVerdict::SETTLED && v.rounds == 1 && r.log == "gather stand gather ");
    g_what = "repair: passed over, the chain ends before my range";
    r = me();
    // (then the script has me grow: the rescan starts where the passed-over words moved `start` to)
    r.tables = {with(SETTLED, 0, {NONE, 0, 10, 0, 100, 0, 0, 950}), with(SETTLED, 1, {U, 1010, 9, 4096, 100, 0, 0, 1900}), SETTLED};
    v = settle(r);
    CHECK(v.kind == ShVerdict::SETTLED && v.rounds == 2);
    CHECK(r.log == "gather publish(exit -1 first -1 err 0 search 950) gather grow(me) rescan(950) gather ");
    CHECK(r.published[2] == 0 && r.published[3] == 0 && r.published[4] == 100);
    g_what = "repair: passed over, the chain passes my whole range";
    r = me();
    r.tables = {with(SETTLED, 0, {2500, 0, 10, 0, 100, 0, 0, 960}), SETTLED};
    v = settle(r);
    CHECK(v.kind == ShVerdict::SETTLED && v.rounds == 1 && r.log == "gather publish(exit 2500 first 2500 err 0 search 960) gather ");
    g_what = "repair: an exit AT my right edge passes me over, one in front of it does not";
    r = me();
    r.tables = {with(SETTLED, 0, {2000, 0, 10, 0, 100, 0, 0, 960}), SETTLED};
    v = settle(r);
    CHECK(r.log == "gather publish(exit 2000 first 2000 err 0 search 960) gather ");
    r = me();
    r.tables = {with(SETTLED, 0, {1999, 0, 10, 0, 100, 0, 0, 960}), SETTLED};
    v = settle(r);
    CHECK(r.log == "gather rescan(960) gather ");
    g_what = "repair: grow and force in one round";
    r = me();
    r.tables = {with(with(SETTLED, 0, {1050, 0, 10, 0, 100, 0, 0, 990}), 1, {U, 1010, 9, 4096, 100, 0, 0, 1900}), SETTLED};
    v = settle(r);
    CHECK(v.kind == ShVerdict::SETTLED && v.rounds == 1 && r.log == "gather grow(me) rescan(990) gather ");
    g_what = "repair: grow and passed over in one round";
    r = me();
    r.tables = {with(with(SETTLED, 0, {NONE, 0, 10, 0, 100, 0, 0, 950}), 2, {U, 2020, 8, 512, 0, 0, 0, 2900}), SETTLED};
    v = settle(r);
    CHECK(r.log == "gather grow(other) publish(exit -1 first -1 err 0 search 950) gather ");
}

static void round_limit()
{
    for (int W : {1, 8}) {
        g_what = W == 1 ? "round limit, W = 1" : "round limit, W = 8";
        const int limit = 2 * W + 48;                            // 50 and 64
        CHECK(limit == (W == 1 ? 50 : 64));
        std::vector<int64_t> B;
        for (int r = 0; r <= W; r++) B.push_back(1000 * r);
        // rank 0 wants more look-ahead round after round; everybody else's words are settled (nobody owns a row)
        Table repair, settled;
        for (int r = 0; r < W; r++) {
            const int64_t ex = r + 1 < W ? 5 : NONE;
            settled.push_back({ex, r ? 5 : 0, r ? 0 : 1, 0, 10, 0, 0, 0});
            repair.push_back({r ? ex : U, r ? 5 : 0, r ? 0 : 1, r ? 0 : 64, 10, 0, 0, 0});
        }
        if (W == 1) repair[0] = {U, 0, 1, 64, 10, 0, 0, 0};
        for (int extra = 0; extra < 2; extra++) {
            Scripted r;
            r.rank = 0;
            r.v = sh_make_view(0, 1000, 1000 * W, 0, 0, W == 1 ? 0 : 10);
            // (W == 1: a view that ends the stream cannot ask in earnest; the table says so all the same)
            r.tables.assign((size_t)(limit + extra), repair);
            r.tables.push_back(settled);
            const ShVerdict v = sh_settle(r, W, 0, B);
            if (!extra) CHECK(v.kind == ShVerdict::SETTLED && v.rounds == limit && r.next == (size_t)limit + 1);
            else CHECK(v.kind == ShVerdict::UNSETTLED && v.rounds == limit + 1 && !v.ok() && r.next == (size_t)limit + 1);
            // (the round over the limit ends at the look: no grow, no rescan for it)
            size_t rescans = 0;
            for (size_t at = r.log.find("rescan("); at != std::string::npos; at = r.log.find("rescan(", at + 1)) rescans++;
            CHECK(rescans == (size_t)limit);
        }
    }
}

static void failing_hooks()
{
    g_what = "a hook that fails";
    const Table NR = with(SETTLED, 2, {U, U, 0, 0, 0, NOT_READY, 0, 0});
    const Table I_GROW = with(SETTLED, 1, {U, 1010, 9, 4096, 100, 0, 0, 1900});
    const Table OTHER_GROWS = with(SETTLED, 0, {U, 0, 10, 4096, 100, 0, 0, 900});
    const Table PASSED = with(SETTLED, 0, {NONE, 0, 10, 0, 100, 0, 0, 950});
    struct Case { const char *hook; Table first; const char *log; } cases[] = {
        {"gather", SETTLED, "gather "},
        {"not_ready", NR, "gather not_ready(-1) "},
        {"grow", I_GROW, "gather grow(me) "},
        {"rescan", I_GROW, "gather grow(me) rescan(-1) "},
        {"publish", OTHER_GROWS, "gather grow(other) stand "},
        {"publish", PASSED, "gather publish(exit -1 first -1 err 0 search 950) "},
    };
    for (const Case &k : cases) {
        Scripted r = me();
        r.fail_hook = k.hook; r.fail_code = -7;
        r.tables = {k.first, SETTLED};
        const ShVerdict v = settle(r);
        CHECK(v.kind == ShVerdict::HOOK && v.code == -7 && !v.ok());
        CHECK(r.log == k.log);
    }
    // ... also where the words are my own failure's
    Scripted r = me();
    r.mine = -4; r.fail_hook = "publish"; r.fail_code = -2;
    r.tables = {with(SETTLED, 1, {U, U, 0, 0, 100, NOT_READY, 0, 0}), SETTLED};
    const ShVerdict v = settle(r);
    CHECK(v.kind == ShVerdict::HOOK && v.code == -2 && r.log == "gather publish(exit -2 first -2 err -6 search 0) ");
}

static void own_block()
{
    g_what = "own block";
    int64_t blk[SH_BLOCK];
    for (int i = 0; i < SH_BLOCK; i++) blk[i] = 100 + i;
    sh_owns_no_rows(blk);
    for (int i = 0; i < SH_BLOCK; i++) CHECK(blk[i] == ((i == 8 || i == 9 || i == 10) ? 0 : 100 + i));
    CHECK(SH_WORDS == 8 && SH_BLOCK == 16 && SH_ROW_LO == 8 && SH_ROW_HI == 9 && SH_ROWS == 10);
}

int main()
{
    settled_at_once();
    stream_errors();
    full_and_internal();
    not_ready();
    repairs();
    round_limit();
    failing_hooks();
    own_block();
    std::printf("%d checks, %d failures\n", g_checks, g_fail);
    if (g_fail) return 1;
    std::printf("ok\n");
    return 0;
}

// The bookkeeping of the walk over two streams whose records are mates (csrc/ffq_pairwalk.h: windows, which mate advances,
// the end-state decision, the ordinal of a name error), driven on the host over scripted fill sizes.  A "stream" here is a
// list of fills, each a vector of the global ordinals of its records; the driver does what ffq_pair_next does with the
// device left out: it takes the fills walk_wants names, reads rows [lo, lo + m) of both current fills THROUGH the vectors (a
// window that leaves its fill is an out-of-bounds read AddressSanitizer reports), and checks that record i of mate 1 meets
// record i of mate 2, every record once, and that the end is the scripted one.
//
//   clang++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I <package>/csrc tests/pair_walk_host.cpp -o pair_walk_host
// Exit status 0 and "ok" on the last line, or 1 and a line per failure.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "ffq_pairwalk.h"

using namespace ffq;

static int g_fail = 0, g_checks = 0;
#define CHECK(cond) do { g_checks++; if (!(cond)) { g_fail++; std::printf("FAIL %s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, g_what); } } while (0)
static const char *g_what = "";

constexpr int END_ERR_INCOMPLETE = 3, END_ERR_FINAL_QUAL = 2;

// a scripted stream: the sizes of its fills and the state its last fill ends with
struct Script { std::vector<int64_t> fills; int end_state = WALK_END_OK; int64_t err_offset = -1; };

struct Expect { int end_state; int err_mate; int64_t pairs; int64_t err_value; };       // err_value: err_row's global ordinal, the stream's
                                                                                         // offset, or the pair's ordinal

static Script fills_of(int64_t total, std::vector<int64_t> pattern, int end_state = WALK_END_OK, int64_t err_offset = -1)
{
    Script s;
    s.end_state = end_state; s.err_offset = err_offset;
    size_t k = 0;
    while (total > 0) {
        const int64_t n = pattern[k++ % pattern.size()] < total ? pattern[(k - 1) % pattern.size()] : total;
        s.fills.push_back(n);
        total -= n;
    }
    if (s.fills.empty()) s.fills.push_back(0);           // an empty file: one fill without a record
    return s;
}

// names_differ_at >= 0: the names check finds that global pair different
static void drive(const char *what, const Script &a, const Script &b, Expect want, int64_t names_differ_at = -1)
{
    g_what = what;
    const Script *sc[2] = {&a, &b};
    PairWalk w;
    size_t next_fill[2] = {0, 0};
    int64_t next_row[2] = {0, 0};                          // global ordinal of the next fill's first record
    std::unique_ptr<std::vector<int64_t>> cur[2];          // the current fill: freed when the mate takes its next one
    int64_t seen_pairs = 0, limit = 0;
    for (auto *s : sc) limit += (int64_t)s->fills.size();
    limit = 2 * limit + 4;
    WalkRound r;
    for (;;) {
        CHECK(w.rounds <= limit);
        if (w.rounds > limit) return;
        walk_begin(w);
        const int wants = walk_wants(w);
        for (int k = 0; k < 2; k++) {
            if (!(wants & (1 << k))) continue;
            CHECK(w.m[k].left() == 0 && !w.m[k].ended);
            CHECK(next_fill[k] < sc[k]->fills.size());
            if (next_fill[k] >= sc[k]->fills.size()) return;
            const int64_t n = sc[k]->fills[next_fill[k]++];
            cur[k].reset(new std::vector<int64_t>((size_t)n));
            for (int64_t i = 0; i < n; i++) (*cur[k])[(size_t)i] = next_row[k] + i;
            next_row[k] += n;
            const bool last = next_fill[k] == sc[k]->fills.size();
            walk_filled(w, k, n, last ? sc[k]->end_state : WALK_END_REFILL, sc[k]->err_offset);
        }
        const int64_t m = walk_take(w);
        CHECK(walk_check(w, m));
        if (!walk_check(w, m)) return;
        if (names_differ_at >= 0 && names_differ_at >= w.pairs && names_differ_at < w.pairs + m) {
            r = walk_names_differ(w, names_differ_at - w.pairs);
            break;
        }
        for (int64_t i = 0; i < m; i++) {
            // (through the vectors' own data: an index outside the fill is a heap overflow)
            const int64_t r1 = cur[0]->data()[w.m[0].lo + i], r2 = cur[1]->data()[w.m[1].lo + i];
            CHECK(r1 == seen_pairs && r2 == seen_pairs);
            seen_pairs++;
        }
        r = walk_moved(w, m);
        CHECK(w.pairs == seen_pairs);
        if (r.end_state != WALK_END_REFILL) break;
        CHECK(!w.done);
    }
    CHECK(w.done && walk_wants(w) == 0);
    CHECK(r.end_state == want.end_state);
    CHECK(r.err_mate == want.err_mate);
    CHECK(seen_pairs == want.pairs);
    if (r.end_state == WALK_END_ERR_PAIR_COUNT) {
        CHECK(r.err_row >= 0 && r.err_row < (int64_t)cur[r.err_mate - 1]->size());
        if (r.err_row >= 0 && r.err_row < (int64_t)cur[r.err_mate - 1]->size()) CHECK((*cur[r.err_mate - 1])[(size_t)r.err_row] == want.err_value);
    } else if (r.end_state != WALK_END_OK) {
        CHECK(r.err_offset == want.err_value);
    }
}

int main()
{
    // equal totals
    drive("one mate always ahead", fills_of(1000, {100}), fills_of(1000, {7}), {WALK_END_OK, 0, 1000, -1});
    drive("the other one ahead", fills_of(1000, {3}), fills_of(1000, {250}), {WALK_END_OK, 0, 1000, -1});
    drive("alternating", fills_of(600, {3, 50}), fills_of(600, {50, 3}), {WALK_END_OK, 0, 600, -1});
    drive("the same fills", fills_of(90, {30}), fills_of(90, {30}), {WALK_END_OK, 0, 90, -1});
    drive("fills without a record", fills_of(40, {10, 0, 0, 5}), fills_of(40, {0, 13}), {WALK_END_OK, 0, 40, -1});
    drive("one fill each", fills_of(5, {5}), fills_of(5, {5}), {WALK_END_OK, 0, 5, -1});
    drive("empty files", fills_of(0, {1}), fills_of(0, {1}), {WALK_END_OK, 0, 0, -1});
    {
        Script a = fills_of(12, {4}), b = fills_of(12, {6});
        a.fills.push_back(0); b.fills.push_back(0); b.fills.push_back(0);      // the end comes with fills of their own
        drive("the end in a fill without a record", a, b, {WALK_END_OK, 0, 12, -1});
    }
    // unequal totals: a mate that ends with rows left, or whose next fill brings them
    drive("mate 1 one record long", fills_of(101, {10}), fills_of(100, {7}), {WALK_END_ERR_PAIR_COUNT, 1, 100, 100});
    drive("mate 2 one record long", fills_of(100, {10}), fills_of(101, {7}), {WALK_END_ERR_PAIR_COUNT, 2, 100, 100});
    drive("mate 2 long, in a fill of its own", fills_of(100, {10}), fills_of(130, {100}), {WALK_END_ERR_PAIR_COUNT, 2, 100, 100});
    drive("mate 1 much longer", fills_of(500, {64}), fills_of(20, {20}), {WALK_END_ERR_PAIR_COUNT, 1, 20, 20});
    drive("mate 1 empty", fills_of(0, {1}), fills_of(3, {2}), {WALK_END_ERR_PAIR_COUNT, 2, 0, 0});
    {
        Script a = fills_of(30, {10}), b = fills_of(30, {15});
        b.fills.push_back(0); b.fills.push_back(2);                             // two more records behind a fill without one
        drive("the longer mate's rows come late", a, b, {WALK_END_ERR_PAIR_COUNT, 2, 30, 30});
    }
    // a mate's own error: in the round in which its rows run out, before anything else
    drive("mate 2 malformed in the middle", fills_of(100, {10}), fills_of(55, {7}, END_ERR_INCOMPLETE, 4711), {END_ERR_INCOMPLETE, 2, 55, 4711});
    drive("mate 1 malformed at once", fills_of(0, {1}, END_ERR_INCOMPLETE, 0), fills_of(9, {4}), {END_ERR_INCOMPLETE, 1, 0, 0});
    drive("both malformed at the same record", fills_of(20, {8}, END_ERR_FINAL_QUAL, 5), fills_of(20, {20}, END_ERR_INCOMPLETE, 6),
          {END_ERR_FINAL_QUAL, 1, 20, 5});
    drive("mate 1 malformed behind more records than mate 2 has", fills_of(50, {50}, END_ERR_INCOMPLETE, 9), fills_of(20, {5}),
          {WALK_END_ERR_PAIR_COUNT, 1, 20, 20});
    drive("mate 1 ends, mate 2 malformed later", fills_of(20, {5}), fills_of(50, {10}, END_ERR_INCOMPLETE, 9),
          {WALK_END_ERR_PAIR_COUNT, 2, 20, 20});
    // names: the global ordinal of the pair, nothing of its round counted
    drive("names differ in the first round", fills_of(100, {10}), fills_of(100, {7}), {WALK_END_ERR_PAIR_NAMES, 0, 0, 3}, 3);
    drive("names differ later", fills_of(100, {10}), fills_of(100, {7}), {WALK_END_ERR_PAIR_NAMES, 0, 63, 64}, 64);
    drive("names differ in the last pair", fills_of(100, {33}), fills_of(100, {100}), {WALK_END_ERR_PAIR_NAMES, 0, 99, 99}, 99);

    std::printf("%d checks, %d failures\n", g_checks, g_fail);
    if (g_fail) return 1;
    std::printf("ok\n");
    return 0;
}

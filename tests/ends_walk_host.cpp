// The lane and chunk work of the ends pass (csrc/ffq_endswalk.h: the functions k_ends_rows and k_ends_long themselves call),
// driven on the host against the rule's loop over bytes (include/ffq.h, ffq_table_trim_ends).  A group is emulated lane by
// lane: every lane takes the values of its bytes, the prefix sum and the maxima that the kernel takes with DPP moves are plain
// loops here, the words that the kernel keeps in LDS are an array, and ends_pass_end / ends_fail_end / ends_advance move the state
// on -- in both shapes, eight lanes of eight bytes (chunks of 64) and sixty-four lanes of sixteen (chunks of 1024).  Every
// quality line lives in a heap block of exactly its length, so a load that leaves the line is an out-of-bounds read
// AddressSanitizer reports.
//
//   clang++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I <package>/csrc tests/ends_walk_host.cpp -o ends_walk_host
// Exit status 0 and "ok" on the last line, or 1 and a line per failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "ffq_endswalk.h"

using namespace ffq;

static int g_fail = 0;
static long g_checks = 0;
static long g_again = 0, g_same = 0, g_zero = 0;          // walks whose right stage took up the chunk in front, the same chunk; reads that went away
#define CHECK(cond, ...) do { g_checks++; if (!(cond)) { if (g_fail++ < 20) { std::printf("FAIL %s:%d: %s  [", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("]\n"); } } } while (0)

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17;
    return (uint32_t)(g_seed >> 24);
}

struct Rules {
    int trim_front, trim_tail, keep_len, base;
    EndsStage front, right, tail;
};

// ---- the rule over bytes (include/ffq.h) ----
static int64_t wsum(const std::vector<int> &v, int64_t i, int W)
{
    int64_t s = 0;
    for (int k = 0; k < W; k++) s += v[(size_t)(i + k)];
    return s;
}

static void loop_cut(const uint8_t *q, int64_t n, const Rules &r, int64_t *oa, int64_t *ob)
{
    std::vector<int> v((size_t)n);
    for (int64_t i = 0; i < n; i++) v[(size_t)i] = (int)q[i] - r.base;
    int64_t a = r.trim_front < n ? r.trim_front : n;
    int64_t b = n - (r.trim_tail < n - a ? r.trim_tail : n - a);
    if (r.keep_len > 0 && b - a > r.keep_len) b = a + r.keep_len;
    *oa = *ob = 0;
    if (r.front.window > 0 && b > a) {
        const int W = (int)(r.front.window < b - a ? r.front.window : b - a);
        int64_t s = -1;
        for (int64_t i = a; i <= b - W; i++)
            if (wsum(v, i, W) >= (int64_t)r.front.quality * W) { s = i; break; }
        if (s < 0) return;
        a = s;
        while (v[(size_t)a] < r.front.quality) a++;
    }
    if (r.right.window > 0 && b > a) {
        const int W = (int)(r.right.window < b - a ? r.right.window : b - a);
        int64_t s = -1;
        for (int64_t i = a; i <= b - W; i++)
            if (wsum(v, i, W) < (int64_t)r.right.quality * W) { s = i; break; }
        if (s >= 0) {
            int64_t b2 = s;
            while (b2 < s + W && v[(size_t)b2] >= r.right.quality) b2++;
            b = b2;
        }
    }
    if (r.tail.window > 0 && b > a) {
        const int W = (int)(r.tail.window < b - a ? r.tail.window : b - a);
        int64_t e = -1;
        for (int64_t j = a + W; j <= b; j++)
            if (wsum(v, j - W, W) >= (int64_t)r.tail.quality * W) e = j;
        if (e < 0) return;
        b = e;
        while (v[(size_t)(b - 1)] < r.tail.quality) b--;
    }
    if (a < b) { *oa = a; *ob = b; }
}

// ---- a group of G lanes with B bytes each, lane by lane ----
// One walk over q[0 .. L) (back: from its end), as ends_walk of csrc/ffq_ends.h goes.  *chunks: the chunks it took.
template <int G, int B>
static void group_walk(const uint8_t *q, int64_t L, bool back, EndsStage pass, EndsStage fail, int base, EndsWalk &s, bool *saw_nl, int *chunks)
{
    constexpr int C = G * B;
    alignas(16) static uint32_t words[2 * C];
    for (int i = 0; i < 2 * C; i++) words[i] = 0xDEADBEEFu + (uint32_t)i;          // (what another row left there)
    uint32_t mp[G], mf[G], mp_prev[G], mf_prev[G];
    for (int gl = 0; gl < G; gl++) mp_prev[gl] = mf_prev[gl] = rnd();             // (and masks that mean nothing)
    ends_begin(s, L, pass, fail);
    bool act = s.stage != ENDS_DONE;
    *chunks = 0;
    while (act) {
        ++*chunks;
        const int64_t w0 = s.w0;
        static int v[G][B];
        static uint32_t p[G][B];
        uint32_t t[G], run = 0;
        for (int gl = 0; gl < G; gl++) {
            const int64_t w = w0 + (int64_t)gl * B, left = L - w;
            const int avail = (int)(left < 0 ? 0 : left < B ? left : B);
            int qv[B];                                  // ascending addresses, -1 where the range has no byte
            for (int j = 0; j < B; j++) {
                if (back) qv[j] = j >= B - avail ? (int)q[L - w - B + j] : -1;
                else qv[j] = j < avail ? (int)q[w + j] : -1;
            }
            bool nl = false;
            t[gl] = ends_lane_vals<B>(qv, back, base, v[gl], nl);
            mp[gl] = ends_lane_mask<B>(v[gl], pass.quality); mf[gl] = ends_lane_mask<B>(v[gl], fail.quality);
            *saw_nl |= nl;
        }
        for (int gl = 0; gl < G; gl++) {                // start = carried + the exclusive prefix
            ends_lane_store<C, B>(words, gl, s.carry + run, v[gl], p[gl]);
            run += t[gl];
        }
        bool judge_fail = s.stage == ENDS_FAIL;
        if (s.stage == ENDS_PASS) {
            int key = 0, fkey = 0;
            for (int gl = 0; gl < G; gl++) {
                const int k = ends_lane_judge<C, B>(words, w0, gl, p[gl], s.W, s.T, s.elo, L, true);
                if (k > key) key = k;
            }
            if (key > 0)
                for (int gl = 0; gl < G; gl++) {
                    const int k = ends_lane_first<C, B>(ends_window_srel<C>(s, key), s.W, true, gl, mp[gl], mp_prev[gl] & ((1u << B) - 1u));
                    if (k > fkey) fkey = k;
                }
            CHECK(key == 0 || fkey > 0, "a window that passes holds a good base");
            judge_fail = ends_pass_end<C>(s, L, key, fkey, fail);
            g_again += s.again; g_same += judge_fail; g_zero += s.zero;
        }
        if (judge_fail) {
            int key = 0, fkey = 0;
            for (int gl = 0; gl < G; gl++) {
                const int k = ends_lane_judge<C, B>(words, w0, gl, p[gl], s.W, s.T, s.elo, L, false);
                if (k > key) key = k;
            }
            if (key > 0)
                for (int gl = 0; gl < G; gl++) {
                    const int k = ends_lane_first<C, B>(ends_window_srel<C>(s, key), s.W, false, gl, mf[gl], mf_prev[gl] & ((1u << B) - 1u));
                    if (k > fkey) fkey = k;
                }
            CHECK(key == 0 || fkey > 0, "a window that fails holds a bad base");
            ends_fail_end<C>(s, L, key, fkey);
        }
        for (int gl = 0; gl < G; gl++) {
            ends_lane_keep<C, B>(words, gl, p[gl]);
            mp_prev[gl] = mp[gl]; mf_prev[gl] = mf[gl];
        }
        act = ends_advance<C>(s, run);
    }
}

template <int G, int B>
static void group_cut(const uint8_t *q, int64_t n, const Rules &r, int64_t *oa, int64_t *ob, int *chunks)
{
    int64_t a, b;
    ends_fixed(n, r.trim_front, r.trim_tail, r.keep_len, a, b);
    EndsWalk f, t;
    bool nl = false;
    int cf = 0, cb = 0;
    group_walk<G, B>(q + a, b - a, false, r.front, r.right, r.base, f, &nl, &cf);
    const int64_t a1 = a + f.a, b1 = a + f.b;
    const bool tlive = !f.zero && b1 > a1;
    group_walk<G, B>(q + a1, tlive ? b1 - a1 : 0, true, r.tail, EndsStage{0, 0}, r.base, t, &nl, &cb);
    int64_t start = a1, stop = b1 - t.a;
    if (f.zero || t.zero || start >= stop) start = stop = 0;
    *oa = start; *ob = stop;
    *chunks = cf + cb;
}

static void one(const std::vector<uint8_t> &line, const Rules &r, const char *what)
{
    const int64_t n = (int64_t)line.size();
    std::unique_ptr<uint8_t[]> block(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(block.get(), line.data(), (size_t)n);
    int64_t wa, wb, a8, b8, a64, b64;
    int c8 = 0, c64 = 0;
    loop_cut(block.get(), n, r, &wa, &wb);
    group_cut<8, 8>(block.get(), n, r, &a8, &b8, &c8);
    group_cut<64, 16>(block.get(), n, r, &a64, &b64, &c64);
    CHECK(a8 == wa && b8 == wb, "%s: n %lld windows %d/%d %d/%d %d/%d fixed %d %d %d: chunks of 64 give (%lld, %lld), the loop (%lld, %lld)", what,
          (long long)n, r.front.window, r.front.quality, r.right.window, r.right.quality, r.tail.window, r.tail.quality, r.trim_front,
          r.trim_tail, r.keep_len, (long long)a8, (long long)b8, (long long)wa, (long long)wb);
    CHECK(a64 == wa && b64 == wb, "%s: n %lld windows %d/%d %d/%d %d/%d fixed %d %d %d: chunks of 1024 give (%lld, %lld), the loop (%lld, %lld)", what,
          (long long)n, r.front.window, r.front.quality, r.right.window, r.right.quality, r.tail.window, r.tail.quality, r.trim_front,
          r.trim_tail, r.keep_len, (long long)a64, (long long)b64, (long long)wa, (long long)wb);
    // (every chunk once per walk, and one of the forward walk once more at the most)
    CHECK(c8 <= 2 * (n / 64 + 1) + 1 && c64 <= 2 * (n / 1024 + 1) + 1, "%s: %d and %d chunks for %lld bytes", what, c8, c64, (long long)n);
}

static Rules rules(EndsStage f, EndsStage r, EndsStage t, int tf = 0, int tt = 0, int keep = 0) { return Rules{tf, tt, keep, 33, f, r, t}; }

static std::vector<uint8_t> hand_line(const char *text)
{
    std::vector<uint8_t> v;
    for (const char *c = text; *c; c++) v.push_back((uint8_t)(*c == 'u' ? 33 + 30 : 33 + 2));     // the issue's notation: u = Q30, 2 = Q2
    return v;
}

static const EndsStage OFF = {0, 0}, WQ = {4, 20};

int main()
{
    // the issue's hand values
    struct { const char *line; Rules r; int64_t a, b; } hand[] = {
        {"uuuuuuuu", rules(WQ, WQ, WQ), 0, 8}, {"22uuuuuu", rules(WQ, OFF, OFF), 2, 8}, {"2u2uuuuu", rules(WQ, OFF, OFF), 1, 8},
        {"uuuuu2u222", rules(OFF, WQ, OFF), 0, 5}, {"uuuuu2u222", rules(OFF, OFF, WQ), 0, 7}, {"uuuu2222uuuu", rules(OFF, WQ, OFF), 0, 4},
        {"uuuu2222uuuu", rules(OFF, OFF, WQ), 0, 12}, {"uuuuuu222", rules(OFF, WQ, OFF), 0, 6}, {"2222", rules(WQ, OFF, OFF), 0, 0},
        {"2222", rules(OFF, WQ, OFF), 0, 0}, {"u2", rules(WQ, OFF, OFF), 0, 0}, {"u2", rules(OFF, WQ, OFF), 0, 1}, {"u2", rules(OFF, OFF, WQ), 0, 0},
        {"u22", rules(OFF, OFF, WQ), 0, 0}, {"uuuuuuuuuu", rules(OFF, OFF, OFF, 3, 2, 4), 3, 7}, {"uuu", rules(OFF, OFF, OFF, 5, 2), 0, 0},
        {"2uuu2uuuu", rules(EndsStage{1, 20}, EndsStage{1, 20}, OFF, 1), 1, 4}, {"", rules(WQ, OFF, OFF, 1), 0, 0},
    };
    for (const auto &h : hand) {
        const std::vector<uint8_t> v = hand_line(h.line);
        int64_t a, b;
        loop_cut(v.data(), (int64_t)v.size(), h.r, &a, &b);
        CHECK(a == h.a && b == h.b, "the loop on %s: (%lld, %lld)", h.line, (long long)a, (long long)b);
        one(v, h.r, "hand");
    }

    // the single failing (or passing) window at every position: 0..140, and around 1024
    static const int WINDOWS[] = {1, 2, 3, 4, 7, 8, 9, 31, 32, 33, 63, 64};
    std::vector<int> places;
    for (int o = 0; o <= 140; o++) places.push_back(o);
    for (int o = 1024 - 70; o <= 1024 + 70; o++) places.push_back(o);
    for (int W : WINDOWS)
        for (int o : places) {
            const int n = o + W + (int)(rnd() % 90);
            const EndsStage st = {W, 20};
            for (int kind = 0; kind < 4; kind++) {
                // 0: bad up to o, good behind; 1: good up to o, bad behind; 2: all bad but W good at o; 3: all good but W bad at o
                std::vector<uint8_t> v((size_t)n);
                for (int i = 0; i < n; i++) {
                    const bool in = i >= o && i < o + W;
                    const bool good = kind == 0 ? i >= o : kind == 1 ? i < o : kind == 2 ? in : !in;
                    v[(size_t)i] = (uint8_t)(33 + (good ? 30 + rnd() % 11 : rnd() % 9));
                }
                one(v, rules(st, OFF, OFF), "placed, front");
                one(v, rules(OFF, st, OFF), "placed, right");
                one(v, rules(OFF, OFF, st), "placed, tail");
                one(v, rules(st, st, st), "placed, all three");
                one(v, rules(st, EndsStage{WINDOWS[rnd() % 12], 25}, EndsStage{WINDOWS[rnd() % 12], 15}, (int)(rnd() % 4), (int)(rnd() % 4)), "placed, mixed windows");
            }
        }

    // front ends in one chunk and right's first window in the one in front of it: wide front window, narrow right window
    for (int o = 60; o <= 200; o++)
        for (int wr : {1, 2, 5, 30}) {
            std::vector<uint8_t> v(300, (uint8_t)(33 + 2));
            for (int i = o; i < o + 40; i++) v[(size_t)i] = (uint8_t)(33 + 41);      // a window of 64 passes from o - 24 on
            v[(size_t)o + 7] = (uint8_t)(33 + 3);
            one(v, rules(EndsStage{64, 20}, EndsStage{wr, 20}, OFF), "right takes up the chunk in front");
            one(v, rules(EndsStage{64, 20}, EndsStage{wr, 20}, EndsStage{3, 20}), "right takes up the chunk in front, tail");
        }

    // seeded lines up to 5000 bytes: flat, decaying, bad heads, dips, all bad; any windows, any fixed trims
    for (int it = 0; it < 3000; it++) {
        const int n = (int)(rnd() % (it % 4 == 0 ? 5001u : it % 4 == 1 ? 1300u : 230u));
        std::vector<uint8_t> v((size_t)n);
        const int kind = (int)(rnd() % 6);
        const int head = n ? (int)(rnd() % (uint32_t)n) : 0;
        for (int i = 0; i < n; i++) {
            int x = 30 + (int)(rnd() % 11);
            if (kind == 1 && i >= head) x = 36 - (int)(34.0 * (i - head) / (n - head)) + (int)(rnd() % 9) - 4;
            if (kind == 2 && i < head % 41) x = 2 + (int)(rnd() % 9);
            if (kind == 3) x = (int)(rnd() % 16);
            if (kind == 4 && rnd() % 23 == 0) x = 2;
            if (kind == 5) x = (int)(rnd() % 42);
            v[(size_t)i] = (uint8_t)(33 + (x < 0 ? 0 : x));
        }
        const auto stage = [&]() { return rnd() % 4 == 0 ? OFF : EndsStage{rnd() % 3 ? WINDOWS[rnd() % 12] : 1 + (int)(rnd() % 64), 1 + (int)(rnd() % (rnd() % 5 ? 40u : 93u))}; };
        Rules r = rules(stage(), stage(), stage(), rnd() % 3 ? 0 : (int)(rnd() % 40), rnd() % 3 ? 0 : (int)(rnd() % 40), rnd() % 3 ? 0 : (int)(rnd() % 300));
        if (it % 50 == 0) r.base = 64;                  // (values go negative)
        one(v, r, "seeded");
    }
    // lines of one value at the chunk edges
    for (int n : {0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2048, 4096, 4097, 5000})
        for (int x : {2, 20, 40}) {
            std::vector<uint8_t> v((size_t)n, (uint8_t)(33 + x));
            one(v, rules(WQ, WQ, WQ), "flat");
            one(v, rules(EndsStage{64, 20}, EndsStage{64, 20}, EndsStage{64, 20}), "flat, window 64");
            one(v, rules(OFF, OFF, OFF, 5, 3, 100), "flat, fixed");
        }

    CHECK(g_again > 500 && g_same > 500 && g_zero > 500, "every way through a chunk is taken: %ld %ld %ld", g_again, g_same, g_zero);
    std::printf("%ld checks, %d failures\n", g_checks, g_fail);
    if (g_fail) return 1;
    std::printf("ok\n");
    return 0;
}

// The arithmetic of duplicate removal (csrc/ffq_dedupwalk.h: the functions the kernels of csrc/ffq_dedup.h themselves call),
// driven on the host against a loop over bytes: the key of a sequence at every length 0..70 and every start alignment 0..15
// inside a padded array whose guard bytes differ between two runs -- a key that depends on a byte outside the read shows --,
// and again in a heap block of exactly the read's length, so that a load that leaves the sequence is an out-of-bounds read
// AddressSanitizer reports; seeded lengths up to 5000; the terms added in another order; key 0 -> 1; the pair key and its NONE
// rule; the home slot and the growth rule.
//
//   clang++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I <package>/csrc tests/dedup_key_host.cpp -o dedup_key_host
// Exit status 0 and "ok" on the last line, or 1 and a line per failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "ffq_dedupwalk.h"

using namespace ffq;

static int g_fail = 0;
static long g_checks = 0;
#define CHECK(cond, ...) do { g_checks++; if (!(cond)) { if (g_fail++ < 20) { std::printf("FAIL %s:%d: %s  [", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("]\n"); } } } while (0)

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17;
    return (uint32_t)(g_seed >> 24);
}

// ---- the rule over bytes (include/ffq.h) ----
static uint64_t sm(uint64_t z)
{
    z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27; z *= 0x94d049bb133111ebull;
    z ^= z >> 31;
    return z;
}
static uint64_t loop_key(const std::vector<uint8_t> &s)
{
    const int64_t n = (int64_t)s.size();
    uint64_t sum = 0;
    for (int64_t k = 0; 4 * k < n; k++) {
        uint64_t w = 0;
        for (int j = 0; j < 4; j++) {
            const int64_t i = 4 * k + j;
            w |= (uint64_t)(i < n ? s[(size_t)i] : 0) << (8 * j);
        }
        sum += sm(((uint64_t)(k + 1) << 32) | w);
    }
    const uint64_t key = sm(sum + (uint64_t)n * 0x9e3779b97f4a7c15ull);
    return key ? key : 1;
}

// the key as a kernel puts it together: the words in a scattered order (lanes, rounds)
static uint64_t scattered_key(const uint8_t *seq, int64_t n)
{
    const int64_t words = (n + 3) / 4;
    uint64_t sum = 0;
    for (int64_t lane = 7; lane >= 0; lane--)
        for (int64_t w = lane; w < words; w += 8) sum += dedup_term(w, dedup_word(seq, 4 * w, n));
    return dedup_finish(sum, n);
}

static std::vector<uint8_t> random_read(int64_t n)
{
    std::vector<uint8_t> s((size_t)n);
    for (auto &b : s) {
        const uint32_t r = rnd();
        b = (r & 31) == 0 ? (uint8_t)(r >> 8) : (uint8_t)"ACGTN"[(r >> 5) % 5];     // (any byte now and then: 0, '\n', 0xFF)
    }
    return s;
}

static void check_read(const std::vector<uint8_t> &s)
{
    const int64_t n = (int64_t)s.size();
    const uint64_t want = loop_key(s);
    CHECK(want != DEDUP_KEY_NONE, "n=%lld", (long long)n);
    // every alignment, two different guards
    for (int a = 0; a < 16; a++) {
        for (int g = 0; g < 2; g++) {
            alignas(16) uint8_t pad[16 + 16 + 5008 + 32];
            std::memset(pad, g ? 0xA5 : 0x0A, sizeof pad);
            uint8_t *p = pad + 16 + a;
            if (n) std::memcpy(p, s.data(), (size_t)n);
            CHECK(dedup_seq_key(p, n) == want, "n=%lld a=%d g=%d", (long long)n, a, g);
            CHECK(scattered_key(p, n) == want, "scattered n=%lld a=%d g=%d", (long long)n, a, g);
        }
    }
    // a block of exactly n bytes
    std::unique_ptr<uint8_t[]> heap(new uint8_t[(size_t)(n ? n : 1)]);
    if (n) std::memcpy(heap.get(), s.data(), (size_t)n);
    CHECK(dedup_seq_key(heap.get(), n) == want, "heap n=%lld", (long long)n);
    CHECK(scattered_key(heap.get(), n) == want, "heap scattered n=%lld", (long long)n);
}

int main()
{
    // sm against the constants of the rule, on a known value (splitmix64's first output for seed 0 is sm(golden))
    CHECK(dedup_sm(0x9e3779b97f4a7c15ull) == 0xe220a8397b1dcdafull, "%llx", (unsigned long long)dedup_sm(0x9e3779b97f4a7c15ull));
    CHECK(dedup_sm(0) == 0, "sm(0)");
    for (int i = 0; i < 1000; i++) {
        const uint64_t z = ((uint64_t)rnd() << 40) ^ ((uint64_t)rnd() << 20) ^ rnd();
        CHECK(dedup_sm(z) == sm(z), "%llx", (unsigned long long)z);
    }
    for (int64_t n = 0; n <= 70; n++)
        for (int rep = 0; rep < 3; rep++) check_read(random_read(n));
    for (int i = 0; i < 60; i++) check_read(random_read(71 + rnd() % 4930));
    // neighbours differ: a swap of two words, a zero byte behind the end, poly-A of every length
    {
        std::vector<uint8_t> s = random_read(64), t = s;
        for (int j = 0; j < 4; j++) std::swap(t[(size_t)j], t[(size_t)(8 + j)]);
        if (s != t) CHECK(loop_key(s) != loop_key(t) && dedup_seq_key(t.data(), 64) == loop_key(t), "word swap");
        std::vector<uint8_t> a(5, 'A'), b = a;
        b.push_back(0);
        CHECK(dedup_seq_key(a.data(), 5) != dedup_seq_key(b.data(), 6), "zero padding");
        std::vector<uint64_t> seen;
        std::vector<uint8_t> poly(600, 'A');
        for (int64_t n = 0; n < 600; n++) seen.push_back(dedup_seq_key(poly.data(), n));
        for (size_t i = 0; i < seen.size(); i++)
            for (size_t j = i + 1; j < seen.size(); j++) CHECK(seen[i] != seen[j], "poly-A %zu %zu", i, j);
    }
    // a key of 0 becomes 1: sm is a bijection with sm(0) == 0, so the sum that mixes to 0 is -n * the constant
    CHECK(dedup_finish(0, 0) == 1, "finish(0, 0)");
    for (int64_t n = 1; n < 50; n++) {
        CHECK(dedup_finish((uint64_t)0 - (uint64_t)n * DEDUP_LEN_MUL, n) == 1, "n=%lld", (long long)n);
        CHECK(dedup_finish(1 - (uint64_t)n * DEDUP_LEN_MUL, n) == sm(1), "n=%lld", (long long)n);
    }
    CHECK(dedup_seq_key(nullptr, 0) == 1, "the empty read");
    // the pair key
    {
        const uint64_t k1 = 0x123456789abcdef1ull, k2 = 0xfedcba9876543211ull;
        CHECK(dedup_pair_key(k1, k2) == sm(sm(k1) + k2), "pair");
        CHECK(dedup_pair_key(k1, k2) != dedup_pair_key(k2, k1) && dedup_pair_key(k1, k1) != dedup_pair_key(k1, k2) &&
              dedup_pair_key(k1, k1) != dedup_pair_key(k2, k1), "ordered");
        CHECK(dedup_pair_key(DEDUP_KEY_NONE, k2) == DEDUP_KEY_NONE && dedup_pair_key(k1, DEDUP_KEY_NONE) == DEDUP_KEY_NONE &&
              dedup_pair_key(DEDUP_KEY_NONE, DEDUP_KEY_NONE) == DEDUP_KEY_NONE, "NONE");
        // sm(k1) + k2 == 0 mixes to 0: the pair key is 1
        CHECK(dedup_pair_key(k1, (uint64_t)0 - sm(k1)) == 1, "pair key 0 -> 1");
    }
    // the home slot and the growth rule
    for (int64_t slots = 1024; slots <= ((int64_t)1 << 40); slots <<= 3) {
        for (int i = 0; i < 50; i++) {
            const uint64_t key = ((uint64_t)rnd() << 40) ^ ((uint64_t)rnd() << 20) ^ rnd();
            const int64_t h = dedup_home(key, slots);
            CHECK(h >= 0 && h < slots && (uint64_t)h == key % (uint64_t)slots, "home");
        }
        CHECK(dedup_home((uint64_t)slots - 1, slots) == slots - 1 && dedup_home((uint64_t)slots, slots) == 0, "home at the edge");
    }
    {
        struct { int64_t slots, distinct, n, want; } ladder[] = {
            {0, 0, 0, 1024}, {0, 512, 0, 1024}, {0, 513, 0, 2048}, {0, 1000000, 0, 2097152}, {1024, 0, 512, 1024}, {1024, 0, 513, 2048},
            {1024, 500, 12, 1024}, {1024, 500, 13, 2048}, {1024, 0, 4096, 8192}, {8192, 4096, 4096, 16384}, {16384, 8192, 4096, 32768},
            {32768, 12288, 4096, 32768}, {32768, 12288, 4097, 65536}, {2048, 3, 0, 2048}, {1 << 20, 1, 1, 1 << 20},
            {1024, 0, 65536, 131072}, {4096, 2048, 1, 8192},
        };
        for (const auto &c : ladder) {
            const int64_t got = dedup_slots_for(c.slots, c.distinct, c.n);
            CHECK(got == c.want, "slots_for(%lld, %lld, %lld) = %lld, want %lld", (long long)c.slots, (long long)c.distinct, (long long)c.n,
                  (long long)got, (long long)c.want);
            CHECK((got & (got - 1)) == 0 && got >= 1024 && got >= c.slots && 2 * (c.distinct + c.n) <= got, "invariants");
        }
    }
    std::printf("%ld checks, %d failures\n", g_checks, g_fail);
    if (g_fail) return 1;
    std::printf("ok\n");
    return 0;
}

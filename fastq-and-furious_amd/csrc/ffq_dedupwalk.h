// ffq_dedupwalk.h -- the arithmetic of duplicate removal (csrc/ffq_dedup.h, ffq_table_seq_keys, ffq_dedup_select;
// include/ffq.h states the rule): the 64-bit key of a sequence, the key of a pair, a key's home slot in the set's table and
// the rule by which that table grows.  Inline functions that compile for the host too: the kernels call them, ffq_seq_key_host
// is dedup_seq_key, and tests/dedup_key_host.cpp drives the same functions on a CPU against a loop over bytes.
//
// The key is a SUM of one term per four bytes, mixed once more with the length: the terms may be added in any order -- by
// the lanes of a group, by the steps of a wave -- and the result is bit-identical.  A word's place in the sequence is part
// of its term (k + 1 in the upper half), so that swapping two words changes the sum; the length is part of the final mix, so
// that a sequence and the same sequence with zero bytes behind it differ.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DDP_HD __host__ __device__ __forceinline__
#else
#define DDP_HD inline
#endif

namespace ffq {

constexpr uint64_t DEDUP_KEY_NONE = 0;                       // FFQ_KEY_NONE: the row has no key
constexpr uint64_t DEDUP_LEN_MUL = 0x9e3779b97f4a7c15ull;
constexpr uint64_t DEDUP_NO_FIRST = ~(uint64_t)0;            // `first` of an empty slot
constexpr int64_t DEDUP_MIN_SLOTS = 1024;

typedef uint32_t dedup_u32u __attribute__((aligned(1)));     // a dword at any address

// the splitmix64 finaliser (ffq_synth_* use the same)
DDP_HD uint64_t dedup_sm(uint64_t z)
{
    z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27; z *= 0x94d049bb133111ebull;
    z ^= z >> 31;
    return z;
}

// the term of word k (bytes seq[4 k .. 4 k + 4), little-endian)
DDP_HD uint64_t dedup_term(int64_t k, uint32_t w) { return dedup_sm(((uint64_t)(k + 1) << 32) | (uint64_t)w); }

// The word at byte o of seq[0 .. n), o < n: four bytes little-endian, a byte behind the end taken as 0.  No byte outside
// seq[0 .. n) is read: a word cut short by the end is the four bytes in FRONT of the end shifted down, or -- a sequence of
// fewer than four bytes -- put together byte by byte.
DDP_HD uint32_t dedup_word(const uint8_t *seq, int64_t o, int64_t n)
{
    if (o + 4 <= n) return *reinterpret_cast<const dedup_u32u *>(seq + o);
    if (n >= 4) return *reinterpret_cast<const dedup_u32u *>(seq + (n - 4)) >> (8 * (int)(o + 4 - n));
    uint32_t x = 0;
    for (int64_t j = o; j < n; j++) x |= (uint32_t)seq[j] << (8 * (int)(j - o));
    return x;
}

// the sum of the terms and the length mixed into the key; never DEDUP_KEY_NONE
DDP_HD uint64_t dedup_finish(uint64_t sum, int64_t n)
{
    const uint64_t k = dedup_sm(sum + (uint64_t)n * DEDUP_LEN_MUL);
    return k ? k : 1;
}

// the rule from end to end, one word after the other
DDP_HD uint64_t dedup_seq_key(const uint8_t *seq, int64_t n)
{
    uint64_t sum = 0;
    for (int64_t o = 0; o < n; o += 4) sum += dedup_term(o >> 2, dedup_word(seq, o, n));
    return dedup_finish(sum, n);
}

// the key of a pair: ordered (k1, k2 and k2, k1 differ); no key if either mate has none
DDP_HD uint64_t dedup_pair_key(uint64_t k1, uint64_t k2)
{
    if (k1 == DEDUP_KEY_NONE || k2 == DEDUP_KEY_NONE) return DEDUP_KEY_NONE;
    const uint64_t k = dedup_sm(dedup_sm(k1) + k2);
    return k ? k : 1;
}

// where a key's probe begins; slots is a power of two
DDP_HD int64_t dedup_home(uint64_t key, int64_t slots) { return (int64_t)(key & (uint64_t)(slots - 1)); }

// The slots the table must have before a call of n rows is entered into a set of `distinct` keys in `slots` slots: as it is
// while 2 (distinct + n) <= slots, else the smallest power of two >= 2 (distinct + n), and never below DEDUP_MIN_SLOTS.  A call
// adds at most n keys, so the load stays <= 1/2 and an insert always meets an empty slot.
DDP_HD int64_t dedup_slots_for(int64_t slots, int64_t distinct, int64_t n)
{
    const int64_t need = 2 * (distinct + n);
    if (slots >= DEDUP_MIN_SLOTS && need <= slots) return slots;
    int64_t s = slots > DEDUP_MIN_SLOTS ? slots : DEDUP_MIN_SLOTS;
    while (s < need) s <<= 1;
    return s;
}

}  // namespace ffq

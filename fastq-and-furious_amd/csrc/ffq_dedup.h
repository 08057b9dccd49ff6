// ffq_dedup.h -- duplicate reads and pairs dropped, the first copy in file order kept (ffq_table_seq_keys, ffq_dedup_select).
// include/ffq.h states the rule; the arithmetic is csrc/ffq_dedupwalk.h.  Two halves that never meet:
//
// THE KEY PASS reads the buffer and writes one 64-bit key per row, in the row frame of ffq_rows.h.
//   k_seqkey_rows     the short rows' shape, 32 rows per workgroup and step, the next step's row asked for first.  A row of up
//                     to SEQKEY_TILE bases is held in registers (lane gl: dwords gl, gl + 8, ... of the sequence, every load in
//                     flight at once; the quality line is never read), the group looks for '\n' with one ballot, every lane
//                     turns its dwords into terms, and the group's sum is a 64-bit add of two 32-bit halves moved by DPP.
//                     Longer rows go onto the list.
//   k_seqkey_long     a wave per listed row, 256 bytes per step, the wave's sum by shuffles.
//   The terms are added in whatever order the lanes hold them: the sum is commutative (ffq_dedupwalk.h).
//
// THE SET works on keys only.  An open-addressing table of 16-byte slots {key, first}, linear probing with wrap-around, an
// empty slot has key 0 and first = ~0.  Its load never exceeds 1/2: the host grows it BEFORE a call is launched
// (dedup_slots_for), from what it knows without asking the device.
//   k_dedup_clear     every slot empty
//   (insert and resolve stride over the rows, DEDUP_GRID_ROWS workgroups at most, and count in registers: dedup_flush)
//   k_dedup_insert    row i of the call (global ordinal g = g0 + i): its key, a pair's two combined; the probe claims an
//                     empty slot with a 64-bit atomicCAS on `key` or finds its key, then atomicMin(first, g)
//   k_dedup_resolve   a SEPARATE launch -- the kernel boundary is what orders it behind every insert: the slot is found again,
//                     the row is kept iff first == g; one verdict byte per row (0 kept, 1 duplicate: the length filter's
//                     count and scan take it from there), the call's counts
//   (the compaction of ffq_compact.h follows on that byte: the rows of one or two tables, or of none, and the ordinals
//                     through d_ord go to their places)
//   k_dedup_rehash    every occupied slot of the old table entered, with its `first`, into the new one
// NO LOOP ON THE DEVICE IS UNBOUNDED: a probe that has visited `slots` slots gives up and sets the block's error word, which
// the host turns into FFQ_E_INTERNAL -- a table corrupted by a bug must not make a kernel spin.
// The atomics are device scope, relaxed: nothing but the slot itself is published through them.
#pragma once
#include "ffq_rows.h"
#include "ffq_pair.h"
#include "ffq_dedupwalk.h"

namespace ffq {

constexpr int SEQKEY_WG = 256;
constexpr int SEQKEY_G = ROWS_G;                                  // lanes per row, a dword each per round
constexpr int SEQKEY_NS = 5;                                      // rounds
constexpr int SEQKEY_TILE = SEQKEY_NS * SEQKEY_G * 4;             // 160: a row above it gets a wave of its own
constexpr int DEDUP_COUNTS = 6;

// a 64-bit sum over the eight lanes of a group: both halves moved by DPP (RowGroup<8>::sum's three moves), added with carry
template <int CTRL>
__device__ __forceinline__ unsigned long long seqkey_dpp64(unsigned long long x)
{
    const uint32_t lo = (uint32_t)rows_dpp<CTRL>((int)(uint32_t)x), hi = (uint32_t)rows_dpp<CTRL>((int)(uint32_t)(x >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long seqkey_group_sum(unsigned long long x)
{
    x += seqkey_dpp64<0xB1>(x);                                   // quad_perm:[1,0,3,2]
    x += seqkey_dpp64<0x4E>(x);                                   // quad_perm:[2,3,0,1]
    x += seqkey_dpp64<0x141>(x);                                  // row_half_mirror
    return x;
}

// (the strided walk is written out, as in k_filter_rows, without pos0 / pos1: ffq_rows.h says why.  The counters are the row
// passes' own block: `changed` counts the keyed rows, `skipped` the rows without a key.)
__global__ __launch_bounds__(SEQKEY_WG) void k_seqkey_rows(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                           const int64_t *__restrict__ table, int64_t n_rows,
                                                           unsigned long long *__restrict__ keys, int64_t *__restrict__ long_list,
                                                           RowsBlock *__restrict__ blk)
{
    constexpr int G = SEQKEY_G;
    const int lane = threadIdx.x & 63, gl = lane & (G - 1), gshift = lane & ~(G - 1);
    RowCounts cnt;
    constexpr int RPB = SEQKEY_WG / G;
    const int64_t step = (int64_t)gridDim.x * RPB;
    longlong2 x23 = make_longlong2(0, 0), x45 = x23;
    {
        const int64_t row = (int64_t)blockIdx.x * RPB + (threadIdx.x / G);
        if (row < n_rows) {
            const longlong2 *src = reinterpret_cast<const longlong2 *>(table + row * 6);
            x23 = src[1]; x45 = src[2];
        }
    }
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < n_rows; r0 += step) {
        const int64_t row = r0 + (threadIdx.x / G);
        const bool have = row < n_rows;
        const longlong2 r23 = x23, r45 = x45;
        if (row + step < n_rows) {
            const longlong2 *src = reinterpret_cast<const longlong2 *>(table + (row + step) * 6);
            x23 = src[1]; x45 = src[2];
        }
        int64_t p2 = 0, p4 = 0, n = 0;
        const bool pos_ok = have && row_pos<true, false>(nbytes, s, add, r23, r45, p2, p4, n);
        const bool is_long = pos_ok && n > SEQKEY_TILE;
        const bool live = pos_ok && !is_long;
        const uint8_t *sq = d + (p2 - s);
        // the whole sequence into registers, every load asked for at once
        uint32_t xs[SEQKEY_NS];
        bool nl = false;
#pragma unroll
        for (int k = 0; k < SEQKEY_NS; k++) {
            const int o = (k * G + gl) * 4;
            xs[k] = 0;
            if (live && o < n) xs[k] = dedup_word(sq, o, n);
        }
#pragma unroll
        for (int k = 0; k < SEQKEY_NS; k++) nl |= has_nl(xs[k]);
        const bool keyed = live && !group_any<G>(nl, gshift);
        unsigned long long sum = 0;
#pragma unroll
        for (int k = 0; k < SEQKEY_NS; k++) {
            const int w = k * G + gl;
            if (live && w * 4 < n) sum += dedup_term(w, xs[k]);
        }
        // (uniform over the wave: a group without a row sums zeros)
        sum = seqkey_group_sum(sum);
        if (gl == 0 && have && !is_long) {
            keys[row] = keyed ? dedup_finish(sum, n) : DEDUP_KEY_NONE;
            if (keyed) cnt.changed++; else cnt.skipped++;
        }
        const int64_t at = long_list_append(is_long && gl == 0, lane, &blk->n_long);
        if (at >= 0) long_list[at] = row;
    }
    cnt.add_to<SEQKEY_WG>(blk);
}

// the rows k_seqkey_rows left (their positions are in order): a wave per row
__global__ __launch_bounds__(SEQKEY_WG) void k_seqkey_long(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                           const int64_t *__restrict__ table, unsigned long long *__restrict__ keys,
                                                           const int64_t *__restrict__ long_list, RowsBlock *__restrict__ blk)
{
    const int64_t n_long = (int64_t)blk->n_long;
    if (n_long == 0) return;
    const int lane = threadIdx.x & 63;
    RowCounts cnt;
    for (LongRows<SEQKEY_WG, false> it(n_long, long_list, table); it.next();) {
        if (!it.have) continue;                             // (uniform over the wave)
        int64_t p2, p4, n;
        const bool elig = row_pos<true, false>(nbytes, s, add, it.r23, it.r45, p2, p4, n);
        const uint8_t *sq = d + (p2 - s);
        bool nl = false;
        unsigned long long sum = 0;
        if (elig) {
            for (int64_t base = 0; base < n; base += 256) {
                const int64_t o = base + (int64_t)lane * 4;
                if (o < n) {
                    const uint32_t a = dedup_word(sq, o, n);
                    nl |= has_nl(a);
                    sum += dedup_term(o >> 2, a);
                }
            }
        }
        const bool keyed = elig && __ballot(nl) == 0;
        sum = wave_sum_u64(sum);
        if (lane == 0) {
            keys[it.row] = keyed ? dedup_finish(sum, n) : DEDUP_KEY_NONE;
            if (keyed) cnt.changed++; else cnt.skipped++;
        }
    }
    cnt.add_to<SEQKEY_WG>(blk);
}

// ---- the set --------------------------------------------------------------------------------------------------------------
struct DedupSlot { unsigned long long key, first; };
static_assert(sizeof(DedupSlot) == 16, "a slot is 16 bytes");

// counters of a call: rows kept, duplicates, rows without a key, keys entered, the error word
struct DedupBlock { unsigned long long kept, dups, nokey, added, err; };
constexpr int DEDUP_WG = 256;

// A workgroup's share of the counters, and whether one of its probes gave up (`bit` of the error word).  Every thread of the
// workgroup is here: the four counts leave by wg_counts_flush, one set of atomics per WORKGROUP.  The launches stride over the
// rows for this: with an atomic per wave on the same three addresses -- 52 000 waves for the 3.3 M rows of a GiB --
// k_dedup_resolve took 0.64 - 1.24 ms, the counters served one at a time.  `lost` is an OR, not a sum: a flag
// per wave, read behind the flush's barrier, and one atomic per workgroup that lost a probe.
__device__ __forceinline__ void dedup_flush(unsigned int kept, unsigned int dups, unsigned int nokey, unsigned int added, bool lost,
                                            unsigned long long bit, DedupBlock *__restrict__ blk)
{
    __shared__ bool s_lost[DEDUP_WG / 64];
    const unsigned long long ml = __ballot(lost);
    if ((threadIdx.x & 63) == 0) s_lost[threadIdx.x >> 6] = ml != 0;
    const unsigned int c[4] = {kept, dups, nokey, added};
    wg_counts_flush<DEDUP_WG>(c, &blk->kept);
    if (threadIdx.x == 0) {
        bool any = false;
#pragma unroll
        for (int w = 0; w < DEDUP_WG / 64; w++) any |= s_lost[w];
        if (any) atomicOr(&blk->err, bit);
    }
}
static_assert(offsetof(DedupBlock, dups) == 8 && offsetof(DedupBlock, nokey) == 16 && offsetof(DedupBlock, added) == 24, "dedup_flush: the four counts in a row");

__global__ __launch_bounds__(256) void k_dedup_clear(DedupSlot *__restrict__ tab, int64_t slots)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < slots; i += (int64_t)gridDim.x * 256)
        tab[i] = DedupSlot{DEDUP_KEY_NONE, DEDUP_NO_FIRST};
}

// the key of row i of a call: d_keys*[j], j = ord ? ord[i] : i
__device__ __forceinline__ unsigned long long dedup_row_key(const unsigned long long *__restrict__ k1, const unsigned long long *__restrict__ k2,
                                                            const int64_t *__restrict__ ord, int64_t i, int64_t &j)
{
    j = ord ? ord[i] : i;
    const unsigned long long a = k1[j];
    return k2 ? dedup_pair_key(a, k2[j]) : a;
}

// The slot of `key` (not DEDUP_KEY_NONE), claimed if the key is not in the table (CLAIM) or looked for only; -1: the probe
// visited every slot, or -- looking only -- met an empty one.  *claimed: this call entered the key.
template <bool CLAIM>
__device__ __forceinline__ int64_t dedup_probe(DedupSlot *__restrict__ tab, int64_t slots, unsigned long long key, bool *claimed)
{
    int64_t h = dedup_home(key, slots);
    for (int64_t visited = 0; visited < slots; visited++) {
        unsigned long long cur = __hip_atomic_load(&tab[h].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == DEDUP_KEY_NONE) {
            if (!CLAIM) return -1;
            cur = atomicCAS(&tab[h].key, (unsigned long long)DEDUP_KEY_NONE, key);
            if (cur == DEDUP_KEY_NONE) { if (claimed) *claimed = true; return h; }
        }
        if (cur == key) return h;
        h = (h + 1) & (slots - 1);
    }
    return -1;
}

__global__ __launch_bounds__(DEDUP_WG) void k_dedup_insert(DedupSlot *__restrict__ tab, int64_t slots, const unsigned long long *__restrict__ k1,
                                                      const unsigned long long *__restrict__ k2, const int64_t *__restrict__ ord, int64_t n,
                                                      unsigned long long g0, DedupBlock *__restrict__ blk)
{
    unsigned int added = 0;
    bool lost = false;
    for (int64_t i = (int64_t)blockIdx.x * DEDUP_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * DEDUP_WG) {
        int64_t j;
        const unsigned long long key = dedup_row_key(k1, k2, ord, i, j);
        if (key == DEDUP_KEY_NONE) continue;
        bool claimed = false;
        const int64_t h = dedup_probe<true>(tab, slots, key, &claimed);
        if (h >= 0) atomicMin(&tab[h].first, g0 + (unsigned long long)i);
        else lost = true;
        added += claimed ? 1u : 0u;
    }
    dedup_flush(0, 0, 0, added, lost, 1ull, blk);
}

__global__ __launch_bounds__(DEDUP_WG) void k_dedup_resolve(DedupSlot *__restrict__ tab, int64_t slots, const unsigned long long *__restrict__ k1,
                                                       const unsigned long long *__restrict__ k2, const int64_t *__restrict__ ord, int64_t n,
                                                       unsigned long long g0, int drop, uint8_t *__restrict__ verdict,
                                                       DedupBlock *__restrict__ blk)
{
    unsigned int n_kept = 0, n_dup = 0, n_nokey = 0;
    bool lost = false;
    for (int64_t i = (int64_t)blockIdx.x * DEDUP_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * DEDUP_WG) {
        int64_t j;
        const unsigned long long key = dedup_row_key(k1, k2, ord, i, j);
        bool dup = false;
        if (key == DEDUP_KEY_NONE) { n_kept++; n_nokey++; }
        else {
            const int64_t h = dedup_probe<false>(tab, slots, key, nullptr);
            if (h < 0) lost = true;
            else if (tab[h].first == g0 + (unsigned long long)i) n_kept++;
            else { dup = true; n_dup++; }
        }
        verdict[i] = (uint8_t)(dup && drop ? 1 : 0);
    }
    dedup_flush(n_kept, n_dup, n_nokey, 0, lost, 2ull, blk);
}

// every key of the old table is in it once: the claim always meets an empty slot of the larger table, or the probe gives up
__global__ __launch_bounds__(256) void k_dedup_rehash(const DedupSlot *__restrict__ old_tab, int64_t old_slots, DedupSlot *__restrict__ tab,
                                                      int64_t slots, DedupBlock *__restrict__ blk)
{
    bool lost = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < old_slots; i += (int64_t)gridDim.x * 256) {
        const DedupSlot e = old_tab[i];
        if (e.key == DEDUP_KEY_NONE) continue;
        const int64_t h = dedup_probe<true>(tab, slots, e.key, nullptr);
        if (h >= 0) atomicMin(&tab[h].first, e.first);
        else lost = true;
    }
    if (lost) atomicOr(&blk->err, 4ull);
}

}  // namespace ffq

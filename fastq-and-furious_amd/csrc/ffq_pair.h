// ffq_pair.h -- two read tables whose rows are mates (paired-end files): the pairs kept or dropped together
// (ffq_table_select_pairs) and the check that the mates really are mates (ffq_table_pair_names).  include/ffq.h states both
// rules.
//
// ffq_table_select_pairs: every mate is judged on its own by the launches of ffq_filter.h (k_filter_rows, k_filter_long) into
// its own verdict bytes; a mate without content rules gets them from k_pair_len, which looks at the row's positions only.  Then
//   k_pair_count     blocks of 256 pairs: the two verdict bytes combined under the mode, the kept pairs per block for the scan,
//                    and the call's five pair counts -- summed over everything a workgroup strides over, one set of atomics each
//   and the compaction of ffq_compact.h behind its scan: the 48-byte rows of BOTH tables and the ordinal copied to the pair's
//   place, "kept" said by KeepPair -- the predicate k_pair_count takes apart for its counts
// ffq_table_pair_names:
//   k_pair_names     in the row frame of ffq_rows.h, a group of 8 lanes per pair: 32 bytes of either header per round as
//                    unaligned dwords, the delimiter found with a byte-mask test, the first differing byte with an xor; the
//                    round loop is uniform over the wave (every group steps as long as one group of the wave has bytes left)
#pragma once
#include "ffq_compact.h"

namespace ffq {

constexpr int PAIR_ANY = 0, PAIR_BOTH = 1, PAIR_FIRST = 2;
constexpr int PAIR_COUNTS = 5;
constexpr int PAIR_NAMES_WG = 256;

// counters of a call: pairs kept, dropped, only mate 1 failed, only mate 2 failed, both failed
struct PairBlock { unsigned long long cnt[PAIR_COUNTS]; };

// counters of a names call: equal, different, not compared, ordinal of the first different pair (initialised to n_pairs)
struct PairNamesBlock { unsigned long long equal, different, not_compared, first; };

// ---- a mate without content rules: the verdict of the length test, from the positions alone --------------------------------
__global__ __launch_bounds__(256) void k_pair_len(const int64_t *__restrict__ table, int64_t n, int64_t lo, int64_t hi,
                                                  uint8_t *__restrict__ verdict, FilterBlock *__restrict__ blk)
{
    const KeepLen keep = {table, lo, hi};
    FilterCounts cnt;
    for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < n; i0 += (int64_t)gridDim.x * 256) {
        const int64_t i = i0 + threadIdx.x;
        if (i < n) {
            const uint32_t v = keep(i, n) ? 0u : 1u;
            verdict[i] = (uint8_t)v;
            cnt.add(v);
        }
    }
    cnt.add_to<256>(blk);
}

// Is pair i kept?  failed(): the mates' verdicts name a reason (v2 == nullptr: mate 2 is not judged); dropped(): what the mode
// makes of the two.
struct KeepPair {
    const uint8_t *v1, *v2; int mode;
    __device__ __forceinline__ void failed(int64_t i, int64_t n, bool &f1, bool &f2) const
    {
        f1 = i < n && (v1[i] & FILTER_REASON) != 0;
        f2 = i < n && v2 != nullptr && (v2[i] & FILTER_REASON) != 0;
    }
    __device__ __forceinline__ bool dropped(bool f1, bool f2) const
    {
        return mode == PAIR_ANY ? (f1 || f2) : mode == PAIR_BOTH ? (f1 && f2) : f1;
    }
    __device__ __forceinline__ bool operator()(int64_t i, int64_t n) const
    {
        bool f1, f2;
        failed(i, n, f1, f2);
        return i < n && !dropped(f1, f2);
    }
};

// (a workgroup strides over the blocks of 256 pairs: the kept pairs of every block go to the scan, the five counts are summed
// in registers and leave with one set of atomics per WORKGROUP -- with a set per block of 256, 13 000 of them for the 3.3 M
// pairs of a GiB, the call took 1.40 ms where it takes 1.08: DESIGN.md 4h)
__global__ __launch_bounds__(256) void k_pair_count(KeepPair keep, int64_t n, int64_t nblk, unsigned int *__restrict__ bcnt,
                                                    PairBlock *__restrict__ blk)
{
    unsigned int c[PAIR_COUNTS] = {0, 0, 0, 0, 0};
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {         // (uniform over the workgroup: a barrier inside)
        const int64_t i = b * 256 + threadIdx.x;
        bool f1, f2;
        keep.failed(i, n, f1, f2);
        const bool have = i < n, drop = keep.dropped(f1, f2);
        const int kept = __syncthreads_count(have && !drop ? 1 : 0);
        if (threadIdx.x == 0) bcnt[b] = (unsigned int)kept;
        c[0] += have && !drop ? 1u : 0u;
        c[1] += have && drop ? 1u : 0u;
        c[2] += f1 && !f2 ? 1u : 0u;
        c[3] += f2 && !f1 ? 1u : 0u;
        c[4] += f1 && f2 ? 1u : 0u;
    }
    wg_counts_flush<256>(c, blk->cnt);
}

// ---- names -------------------------------------------------------------------------------------------------------------------
// one mate's buffer and table as the kernel takes them
struct PairSide { const uint8_t *d; int64_t nbytes; int s; int64_t add; const int64_t *table; };

// The header slice of a row, buf[pos0 + 1 : pos1]: where it begins in memory and its length; false: the row is not compared
// (pos0 - add < 0, pos0 + 1 > pos1, or the slice leaves the buffer).  The slice begins at coordinate pos0 + 1 >= 1: the
// sentinel's coordinate 0 is never part of it.
__device__ __forceinline__ bool pair_header(const PairSide &S, longlong2 r01, const uint8_t *&h, int64_t &n)
{
    const int64_t p0 = row_coord(r01.x, S.add), p1 = row_coord(r01.y, S.add);
    const bool ok = p0 >= 0 && p0 < p1 && p1 <= S.nbytes + S.s;
    h = S.d + (ok ? p0 + 1 - S.s : 0);
    n = ok ? p1 - p0 - 1 : 0;
    return ok;
}

// The geometry of a pair that has an insert size, for the passes that walk the mates' overlap (ffq_correct.h, ffq_merge.h).
// True: both rows are eligible with both of their lines read (row_pos), neither has more than max_len bases, ins >= 0 and
// mate 2 lies at o = ins - n2 with -n2 < o < n1.  P (CorPair, MrgPair) gets where the four lines begin in memory, n1, n2 and o
// -- zeros if the pair fails.  Positions and ranges only: no byte of the reads is looked at.
template <class Pair>
__device__ __forceinline__ bool pair_geometry(const PairSide &A, const PairSide &B, longlong2 a23, longlong2 a45, longlong2 b23, longlong2 b45,
                                              int32_t ins, int max_len, Pair &P)
{
    int64_t pa2 = 0, pa4 = 0, na = 0, pb2 = 0, pb4 = 0, nb = 0;
    bool ok = row_pos<true, true>(A.nbytes, A.s, A.add, a23, a45, pa2, pa4, na);
    ok = ok && row_pos<true, true>(B.nbytes, B.s, B.add, b23, b45, pb2, pb4, nb);
    ok = ok && na <= max_len && nb <= max_len && ins >= 0;
    const int64_t o = (int64_t)ins - nb;
    ok = ok && -nb < o && o < na;
    P.asrc = P.qasrc = P.bsrc = P.qbsrc = 0; P.n1 = P.n2 = P.o = 0;
    if (!ok) return false;
    P.asrc = pa2 - A.s; P.qasrc = pa4 - A.s; P.bsrc = pb2 - B.s; P.qbsrc = pb4 - B.s;
    P.n1 = (int32_t)na; P.n2 = (int32_t)nb; P.o = (int32_t)o;
    return true;
}

// place (0..3) of the first byte of x that is 0x20 or 0x09; 4: none.  (The zero-byte test may flag a byte ABOVE a true hit,
// never one below it: the lowest flag is exact.)
__device__ __forceinline__ int pair_first_delim(uint32_t x)
{
    const uint32_t a = x ^ 0x20202020u, b = x ^ 0x09090909u;
    const uint32_t m = (((a - 0x01010101u) & ~a) | ((b - 0x01010101u) & ~b)) & 0x80808080u;
    return m ? (__builtin_ctz(m) >> 3) : 4;
}

// an id without its "/1" or "/2": the length that is compared
__device__ __forceinline__ int64_t pair_id_len(const uint8_t *__restrict__ h, int64_t e)
{
    if (e >= 2 && h[e - 2] == (uint8_t)'/' && (h[e - 1] == (uint8_t)'1' || h[e - 1] == (uint8_t)'2')) return e - 2;
    return e;
}

__global__ __launch_bounds__(PAIR_NAMES_WG) void k_pair_names(PairSide A, PairSide B, int64_t n_pairs, PairNamesBlock *__restrict__ blk)
{
    constexpr int G = ROWS_G, RPB = PAIR_NAMES_WG / G;
    const int lane = threadIdx.x & 63, gl = lane & (G - 1);
    unsigned int c_eq = 0, c_df = 0, c_nc = 0;
    unsigned long long first = (unsigned long long)n_pairs;
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < n_pairs; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t pair = r0 + (threadIdx.x / G);
        const bool have = pair < n_pairs;
        longlong2 a01 = make_longlong2(0, 0), b01 = a01;
        if (have) {
            a01 = *reinterpret_cast<const longlong2 *>(A.table + pair * 6);
            b01 = *reinterpret_cast<const longlong2 *>(B.table + pair * 6);
        }
        const uint8_t *ha = A.d, *hb = B.d;
        int64_t na = 0, nb = 0;
        const bool oka = have && pair_header(A, a01, ha, na), okb = have && pair_header(B, b01, hb, nb);
        const bool cmp = oka && okb;
        // ea, eb: where the ids end (the first delimiter, or the header's end); fd: the first byte in which the headers differ
        int64_t ea = -1, eb = -1, fd = -1;
        for (int64_t base = 0;; base += G * 4) {
            const bool more_a = cmp && ea < 0 && base < na, more_b = cmp && eb < 0 && base < nb;
            if (cmp && ea < 0 && !more_a) ea = na;
            if (cmp && eb < 0 && !more_b) eb = nb;
            // (uniform over the wave: every group steps as long as one of them has bytes to look at; a finished group idles)
            if (__ballot(more_a || more_b) == 0) break;
            const int64_t o = base + gl * 4;
            uint32_t xa = 0, xb = 0;
            if ((more_a || more_b) && o < na) xa = stats_ld(ha, o, na);
            if ((more_a || more_b) && o < nb) xb = stats_ld(hb, o, nb);
            // a byte behind a slice's end reads as 0: not a delimiter, and only bytes in front of both ids' ends are compared
            const int da = more_a && o < na ? pair_first_delim(xa) : 4, db = more_b && o < nb ? pair_first_delim(xb) : 4;
            const int pa = da < 4 && o + da < na ? gl * 4 + da : G * 4, pb = db < 4 && o + db < nb ? gl * 4 + db : G * 4;
            const uint32_t z = xa ^ xb;
            const int pz = (more_a || more_b) && z ? gl * 4 + (__builtin_ctz(z) >> 3) : G * 4;
            const int ma = -RowGroup<G>::maxall(-pa), mb = -RowGroup<G>::maxall(-pb), mz = -RowGroup<G>::maxall(-pz);
            if (more_a && ma < G * 4) ea = base + ma;
            if (more_b && mb < G * 4) eb = base + mb;
            if (fd < 0 && mz < G * 4) fd = base + mz;
        }
        if (gl == 0 && have) {
            if (!cmp) c_nc++;
            else {
                const int64_t la = pair_id_len(ha, ea), lb = pair_id_len(hb, eb);
                const bool equal = la == lb && (fd < 0 || fd >= la);
                if (equal) c_eq++;
                else { c_df++; first = min(first, (unsigned long long)pair); }
            }
        }
    }
    // the three counts leave by wg_counts_flush; `first` is a MINIMUM: over the wave here, over the waves behind the flush's
    // barrier, and one atomic per workgroup that has a different pair
    __shared__ unsigned long long s_first[PAIR_NAMES_WG / 64];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) first = min(first, (unsigned long long)__shfl_xor((long long)first, o));
    if (lane == 0) s_first[threadIdx.x >> 6] = first;
    const unsigned int c[3] = {c_eq, c_df, c_nc};
    wg_counts_flush<PAIR_NAMES_WG>(c, &blk->equal);
    if (threadIdx.x == 0) {
        unsigned long long f = s_first[0];
#pragma unroll
        for (int w = 1; w < PAIR_NAMES_WG / 64; w++) f = min(f, s_first[w]);
        if (f < (unsigned long long)n_pairs) atomicMin(&blk->first, f);
    }
}
static_assert(offsetof(PairNamesBlock, different) == 8 && offsetof(PairNamesBlock, not_compared) == 16, "k_pair_names: the three counts in a row");

}  // namespace ffq

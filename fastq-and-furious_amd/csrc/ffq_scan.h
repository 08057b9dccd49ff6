// ffq_scan.h -- the prefix sum over a workgroup, once, and the scan of an array built from it.
//
// The primitives (every table pass that gives its rows a place in an output calls one of them):
//   wave_incl_scan_bits<BITS>   inclusive scan inside the wave of values whose WIDTH the caller states
//   wg_excl_scan<WG, BITS>      this thread's exclusive prefix over the workgroup, and the workgroup's sum
//   wg_sum<WG>                  the sum alone
//   wg_rank<WG>                 the ballot form: how many keeping threads stand in front of this one
// The scan family, three kernels and their driver's thresholds (launch_scan is in ffq_hip.hip):
//   k_scan_one<T, Total>        exclusive scan of an array by ONE workgroup; in place, or u32 counts -> int64 offsets
//   k_scan_blksum<T>, k_scan_blkapply<T>   the two outer levels for long arrays, a workgroup per SCAN_BLK values
// What is NOT here: the scans inside the buffer scan's own kernels (k_sbscan, k_rows4, k_qscan4, k_expand and the chain
// kernels, ffq_fused.h, ffq_lite.h, ffq_dense.h, ffq_ranked.h).  They carry more than a sum through their waves and are
// tuned where they stand.
#pragma once
#include "ffq_chain.h"

namespace ffq {

// ---- inside the wave -------------------------------------------------------------------------------------------------------
// Inclusive scan of x over the 64 lanes of the wave, for values 0 <= x < 2^BITS.  The DPP scan of ffq_dev.h
// (wave_incl_scan) adds in 32 bits, so it is exact as long as the last lane's sum fits them: 64 lanes times 2^H must fit 32
// bits, H <= 26.
//   BITS <= 26   one DPP scan
//   BITS <= 52   two of them, over the low H = ceil(BITS / 2) bits and over the rest (each half below 2^26)
//   wider        the ladder of six __shfl_up steps in T's own width: exact for any value, modulo 2^(bits of T)
// BITS is a promise of the caller's about its values, not a conversion: a value at or above 2^BITS gives a wrong sum.
constexpr int SCAN_ANY = 64;          // BITS of a caller that promises nothing

template <int BITS, class T>
__device__ __forceinline__ T wave_incl_scan_bits(T x)
{
    static_assert(BITS >= 1 && BITS <= SCAN_ANY, "width of the values");
    if constexpr (BITS <= 26) {
        return (T)wave_incl_scan((uint32_t)x);
    } else if constexpr (BITS <= 52) {
        static_assert(sizeof(T) == 8, "a sum of 64 such values needs 64 bits");
        constexpr int H = (BITS + 1) / 2;
        const uint32_t lo = wave_incl_scan((uint32_t)x & ((1u << H) - 1u)), hi = wave_incl_scan((uint32_t)(x >> H));
        return (T)(((unsigned long long)hi << H) + lo);
    } else {
        const int lane = threadIdx.x & 63;
        T incl = x;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const T y = __shfl_up(incl, d);
            if (lane >= d) incl += y;
        }
        return incl;
    }
}

// ---- over the workgroup ----------------------------------------------------------------------------------------------------
// The sum of x over the threads in front of this one in a workgroup of WG threads, and `total`, the sum over all of them
// (the same in every thread).  Values as wave_incl_scan_bits<BITS> wants them; the waves' totals and `total` are T's.
//   who calls it    every thread of the workgroup, at a point that is uniform over it
//   what it costs   one barrier and WG / 64 words of LDS: s_w, the caller's -- or, in the form without it, the function's own
//   what the caller owes   a barrier between this call's return and whatever writes s_w next: a second call in a loop
//                   (k_render_sum), or the caller's own use of the words it handed in
// A caller that never looks at `total` pays nothing for it.
template <int WG, int BITS, class T>
__device__ __forceinline__ T wg_excl_scan(T x, T &total, T *s_w)
{
    static_assert(WG % 64 == 0 && WG <= 1024, "whole waves");
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const T incl = wave_incl_scan_bits<BITS>(x);
    if (lane == 63) s_w[wid] = incl;
    __syncthreads();
    T wpre = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < WG / 64; q++) {
        const T t = s_w[q];
        if (q < wid) wpre += t;
        tot += t;
    }
    total = tot;
    return wpre + incl - x;
}

template <int WG, int BITS, class T>
__device__ __forceinline__ T wg_excl_scan(T x, T &total)
{
    __shared__ T s_w[WG / 64];
    return wg_excl_scan<WG, BITS>(x, total, s_w);
}

// The sum of x over the workgroup, in every thread.  Callers, cost and debt as for wg_excl_scan (the LDS is its own).
template <int WG>
__device__ __forceinline__ long long wg_sum(long long x)
{
    __shared__ long long s_w[WG / 64];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    long long tot = 0;
#pragma unroll
    for (int q = 0; q < WG / 64; q++) tot += s_w[q];
    return tot;
}

// How many threads with a lower number in the workgroup of WG keep theirs: the value means something to the keeping ones
// only.  In two halves, so that a kernel whose next step has a barrier of its own (k_merge_rows: its byte scan) spends no
// second one: wg_rank_put leaves the wave's count in s_w[wave] and returns the wave's ballot, wg_rank_get -- BEHIND a
// barrier -- makes the rank of them.  wg_rank is the two around a barrier, on LDS of its own.
//   who calls it    every thread of the workgroup, at a point that is uniform over it (put and wg_rank; get may be left to
//                   the keeping threads)
//   what it costs   WG / 64 words of LDS; wg_rank one barrier
//   what the caller owes   a barrier before s_w is written again
template <int WG>
__device__ __forceinline__ unsigned long long wg_rank_put(bool keep, uint32_t *s_w)
{
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    return m;
}

template <int WG>
__device__ __forceinline__ uint32_t wg_rank_get(unsigned long long m, const uint32_t *s_w)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t wpre = 0;
#pragma unroll
    for (int q = 0; q < WG / 64; q++)
        if (q < wid) wpre += s_w[q];
    return wpre + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

template <int WG>
__device__ __forceinline__ uint32_t wg_rank(bool keep)
{
    __shared__ uint32_t s_w[WG / 64];
    const unsigned long long m = wg_rank_put<WG>(keep, s_w);
    __syncthreads();
    return wg_rank_get<WG>(m, s_w);
}

// ---- the scan of an array --------------------------------------------------------------------------------------------------
// Exclusive scan of nv values v[] of type T -- unsigned 32-bit counts, or int64 -- into the int64 out[]: out[i] = the values
// in front of i; out may be v itself (T = long long: in place).  Arrays are hipMalloc'ed scratch of the context, so a
// thread's run of values starts on a 16-byte boundary and goes in and out in 16-byte pieces; no kernel here defends against
// another alignment.  One workgroup up to SCAN_ONE_U32 / SCAN_ONE_I64 values, above that two levels: k_scan_blksum, a
// workgroup per SCAN_BLK values, their sums; k_scan_one over the sums, in place (it also writes the total); k_scan_blkapply,
// the scan inside each block on top of its base.  Three launches of a few microseconds: the one workgroup took 132 us for
// the 262 144 per-tile counts of a 4 GiB buffer -- eight rounds, every lane reading its own 256 bytes.
constexpr int SCAN_ONE_WG = 1024;                             // threads of k_scan_one
constexpr int SCAN_PER = 32;                                  // consecutive values a thread of it owns
constexpr int SCAN_ROUND = SCAN_ONE_WG * SCAN_PER;            // values per barrier round: 32 768
constexpr int64_t SCAN_ONE_U32 = SCAN_ROUND;                  // one workgroup up to here, counts: one round
constexpr int64_t SCAN_ONE_I64 = 2 * SCAN_ROUND;              // ... int64 values: two
constexpr int SCAN_BLK_WG = 256, SCAN_BLK_PER = 8;
constexpr int SCAN_BLK = SCAN_BLK_WG * SCAN_BLK_PER;          // values per workgroup of the outer levels: 2048

template <class T>
constexpr int64_t scan_one_max() { return sizeof(T) == 4 ? SCAN_ONE_U32 : SCAN_ONE_I64; }

// where k_scan_one leaves the total: a word ...
struct ScanToWord {
    long long *p;
    __device__ __forceinline__ void operator()(long long t) const { *p = t; }
};
// ... or a result block, as k_decode_stream, k_col_offsets and the render kernels read it (n_records = n_rows,
// n_qual_bytes = the total)
struct ScanToRes {
    DevRes *res; int64_t n_rows;
    __device__ __forceinline__ void operator()(long long t) const { res->n_records = n_rows; res->n_qual_bytes = t; res->fallback = 0; }
};

// values [b0, b0 + N) of v, zero past nv, into x; their sum
template <class T, int N>
__device__ __forceinline__ long long scan_load(const T *v, int64_t nv, int64_t b0, T (&x)[N])
{
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "u32 counts or int64 values");
    constexpr int V = 16 / (int)sizeof(T);                    // values per 16-byte load (b0 is a multiple of N, N of V)
    static_assert(N % V == 0, "whole 16-byte pieces");
    if (b0 + N <= nv) {
#pragma unroll
        for (int k = 0; k < N / V; k++) {
            if constexpr (V == 4) {
                const uint4 t = *reinterpret_cast<const uint4 *>(v + b0 + 4 * k);
                x[4 * k] = t.x; x[4 * k + 1] = t.y; x[4 * k + 2] = t.z; x[4 * k + 3] = t.w;
            } else {
                const longlong2 t = *reinterpret_cast<const longlong2 *>(v + b0 + 2 * k);
                x[2 * k] = t.x; x[2 * k + 1] = t.y;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; k++) x[k] = (b0 + k < nv) ? v[b0 + k] : (T)0;
    }
    long long s = 0;
#pragma unroll
    for (int k = 0; k < N; k++) s += (long long)x[k];
    return s;
}

// out[b0 + k] = run + x[0] + ... + x[k - 1] for the k inside the array
template <class T, int N>
__device__ __forceinline__ void scan_store(long long *out, int64_t nv, int64_t b0, long long run, const T (&x)[N])
{
    if (b0 + N <= nv) {
#pragma unroll
        for (int k = 0; k < N / 2; k++) {
            longlong2 o;
            o.x = run; run += (long long)x[2 * k];
            o.y = run; run += (long long)x[2 * k + 1];
            *reinterpret_cast<longlong2 *>(out + b0 + 2 * k) = o;
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; k++) { if (b0 + k < nv) out[b0 + k] = run; run += (long long)x[k]; }
    }
}

// One workgroup.  A thread owns SCAN_PER = 32 CONSECUTIVE values (eight or sixteen 16-byte loads in flight, a sum in
// registers), the 1024 thread sums are scanned once per round of 32 768 values, and the thread writes its 32 results: one
// barrier round per 32 768 values.  (A round per 1024 values took 65 us for the 65 536 tiles of a GiB, 1 us each; the
// Hillis-Steele version before that twenty barriers per 1024 values: 483 us for the 262 144 tiles of 4 GiB -- a fifth of the
// list-ranking tier's time --, 200 us for the row blocks of a 10 GiB table.)
// Thread sums of counts stay below 2^37 (32 values of 32 bits): the wave scan in two halves of 24 bits; int64 values take
// the ladder.
// The step through LDS is wg_excl_scan<SCAN_ONE_WG, BITS> WRITTEN OUT, the one place: the kernel lives at the 128 VGPRs its
// 1024 threads leave it (114 for counts, 118 in place), and with the same arithmetic behind the function's name the
// compiler orders the sixteen LDS reads otherwise and spills 15 to 23 dwords.  A change to wg_excl_scan is
// made here too.
template <class T, class Total>
__global__ __launch_bounds__(SCAN_ONE_WG) void k_scan_one(const T *v, int64_t nv, long long *out, Total total)
{
    constexpr int BITS = sizeof(T) == 4 ? 48 : SCAN_ANY;
    __shared__ long long s_w[SCAN_ONE_WG / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    long long carry = 0;
    for (int64_t c0 = 0; c0 < nv; c0 += SCAN_ROUND) {
        const int64_t b0 = c0 + (int64_t)tid * SCAN_PER;
        T x[SCAN_PER];
        const long long mine = scan_load(v, nv, b0, x);
        const long long incl = wave_incl_scan_bits<BITS>(mine);
        if (lane == 63) s_w[wid] = incl;
        __syncthreads();
        long long wpre = 0, tot = 0;
#pragma unroll
        for (int q = 0; q < SCAN_ONE_WG / 64; q++) {
            const long long t = s_w[q];
            if (q < wid) wpre += t;
            tot += t;
        }
        scan_store(out, nv, b0, carry + wpre + incl - mine, x);
        __syncthreads();                                      // (s_w is written again by the next round)
        carry += tot;
    }
    if (tid == 0) total(carry);
}

template <class T>
__global__ __launch_bounds__(SCAN_BLK_WG) void k_scan_blksum(const T *__restrict__ v, int64_t nv, long long *__restrict__ bs)
{
    T x[SCAN_BLK_PER];
    const long long s = scan_load(v, nv, (int64_t)blockIdx.x * SCAN_BLK + (int64_t)threadIdx.x * SCAN_BLK_PER, x);
    const long long tot = wg_sum<SCAN_BLK_WG>(s);
    if (threadIdx.x == 0) bs[blockIdx.x] = tot;
}

// bs: the blocks' bases (the scanned sums)
template <class T>
__global__ __launch_bounds__(SCAN_BLK_WG) void k_scan_blkapply(const T *v, int64_t nv, const long long *__restrict__ bs, long long *out)
{
    const int64_t b0 = (int64_t)blockIdx.x * SCAN_BLK + (int64_t)threadIdx.x * SCAN_BLK_PER;
    const long long base = bs[blockIdx.x];
    T x[SCAN_BLK_PER];
    const long long mine = scan_load(v, nv, b0, x);
    long long tot;
    const long long run = base + wg_excl_scan<SCAN_BLK_WG, SCAN_ANY>(mine, tot);
    scan_store(out, nv, b0, run, x);
}

}  // namespace ffq

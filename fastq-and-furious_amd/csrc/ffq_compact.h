// ffq_compact.h -- stable compaction of table rows, once: every table call that keeps some rows and drops the rest
// (ffq_table_select_seqlen[_idx], ffq_table_select_reads, ffq_table_select_pairs, ffq_dedup_select) does the same three steps
//   k_compact_count<Keep>     one row per thread: kept rows per block of 256 into bcnt
//   launch_scan               exclusive scan of those counts, their total (ffq_scan.h, ffq_hip.hip)
//   k_compact_scatter<Keep, NT, ORD>   rank inside the workgroup by ballots (wg_rank); the 48-byte rows of NT tables (0, 1 or 2) and the
//                             row's ordinal (ORD: through `ord`) copied to the rank.  The host picks the instantiation by
//                             the pointers it was given: a kernel that tested them itself was 1 % slower than the
//                             one-table kernel it replaced
// and differs only in what "kept" means.  That is a Keep: a small struct passed to the kernels by value, with
//   __device__ bool operator()(int64_t i, int64_t n) const          is row i of n kept?  (false for i >= n)
// KeepLen and KeepVerdict are here, KeepPair is beside the pair counts that share its pieces (ffq_pair.h).  k_pair_count is a
// count kernel of its own that writes the same bcnt.  The host side -- compact_reserve, compact_enqueue, compact_scatter -- is
// with the table calls (ffq_tables.h).
#pragma once
#include "ffq_filter.h"
#include "ffq_scan.h"

namespace ffq {

// row i of `table` to row r of `out`: three 16-byte loads in flight, three stores
__device__ __forceinline__ void row_copy48(const int64_t *__restrict__ table, int64_t i, int64_t *__restrict__ out, int64_t r)
{
    const longlong2 *src = reinterpret_cast<const longlong2 *>(table + i * 6);
    longlong2 *dst = reinterpret_cast<longlong2 *>(out + r * 6);
    const longlong2 a = src[0], b = src[1], c = src[2];
    dst[0] = a; dst[1] = b; dst[2] = c;
}

// min_len <= pos3 - pos2 <= max_len, read from the table (push-down of the length filter of
// the reference's doc/user-guide.rst:153-180): no verdict array
struct KeepLen {
    const int64_t *table; int64_t lo, hi;
    __device__ __forceinline__ bool operator()(int64_t i, int64_t n) const
    {
        if (i >= n) return false;
        const longlong2 p = *reinterpret_cast<const longlong2 *>(table + i * 6 + 2);      // pos2, pos3
        const int64_t ln = p.y - p.x;
        return ln >= lo && ln <= hi;
    }
};

// the verdict byte of a judging pass (ffq_filter.h, ffq_dedup.h) names no reason
struct KeepVerdict {
    const uint8_t *v;
    __device__ __forceinline__ bool operator()(int64_t i, int64_t n) const { return i < n && (v[i] & FILTER_REASON) == 0; }
};

template <class Keep>
__global__ __launch_bounds__(256) void k_compact_count(Keep keep, int64_t n, unsigned int *__restrict__ bcnt)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = __syncthreads_count(keep(i, n) ? 1 : 0);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = (unsigned int)c;
}

// The rows of t1 (NT >= 1) and t2 (NT == 2).  idx_out (optional): the ordinal of every kept row -- ord[i] with ORD, else i --
// what a host that must hand back one item per ORIGINAL row (None for a dropped one, the reference's
// doc/user-guide.rst:166-170) puts the kept ones back by
template <class Keep, int NT, bool ORD>
__global__ __launch_bounds__(256) void k_compact_scatter(Keep keep, int64_t n, const long long *__restrict__ bbase,
                                                         const int64_t *__restrict__ t1, const int64_t *__restrict__ t2,
                                                         const int64_t *__restrict__ ord, int64_t *__restrict__ out1,
                                                         int64_t *__restrict__ out2, int64_t *__restrict__ idx_out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool kept = keep(i, n);
    const uint32_t rank = wg_rank<256>(kept);
    if (!kept) return;
    const int64_t r = bbase[blockIdx.x] + rank;
    if (NT >= 1) row_copy48(t1, i, out1, r);
    if (NT == 2) row_copy48(t2, i, out2, r);
    if (idx_out) idx_out[r] = ORD ? ord[i] : i;
}

}  // namespace ffq

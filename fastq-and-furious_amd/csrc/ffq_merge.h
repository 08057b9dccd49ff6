// ffq_merge.h -- the two mates of a pair merged into one read, rendered as FASTQ text: ffq_table_pair_merge (include/ffq.h
// states the rule; the byte work is csrc/ffq_mergewalk.h).
//
// Shape: the render pass's three steps (ffq_render.h).
//   k_merge_sum     per block of 256 pairs, from the rows' positions and the pair's insert size alone: the bytes of merged
//                   text and the number of pairs that are NOT merged; the call's counts [0], [3], [4] on the way
//   the two scans   launch_scan (ffq_scan.h) over the bytes and over the unmerged pairs
//   k_merge_rows    a workgroup per block of 256 pairs.  A thread per pair first: the pair is parsed again, the prefix inside
//                   the block gives a merged pair its place in the text (d_off) and an unmerged pair its place in the rest
//                   tables, where the thread copies both rows (96 bytes) and the ordinal.  Then a GROUP of eight lanes per
//                   merged pair, thirty-two pairs at a time, neighbours in the output: the text is cut into 16-byte chunks
//                   aligned on the OUTPUT address, a lane builds a chunk in registers (mrg_chunk_load / mrg_chunk_build:
//                   up to seven unaligned 16-byte loads, mate 2's at the mirrored address, reversed and complemented in
//                   registers, the choice a per-byte compare) and stores it with ONE aligned 16-byte store; only the first
//                   and the last chunk of a record are written in pieces.  MERGE_U chunks per lane are in flight.
// No byte outside [d_text + off[k], d_text + off[k + 1]) is written for pair k, and none at all if the total exceeds text_cap
// (the loads are still made then: counts[5] needs the qualities).  No loop of the copy holds a ballot, a DPP move or a
// barrier; the loop over the eight steps is uniform, and a group whose pair is not merged steps along idle.
// A merged record is at most 6 + 2 * 1023 bytes beside its header, so there is no long rows' launch: a header of many KiB is
// walked by its group of eight, sixteen chunks a round.
// Nothing is staged in LDS but the parsed pairs (64 bytes each) and their places: 20.5 KiB per workgroup of four waves.
#pragma once
#include "ffq_pair.h"
#include "ffq_render.h"
#include "ffq_mergewalk.h"

namespace ffq {

constexpr int MERGE_WG = 256;
constexpr int MERGE_G = 8;            // lanes per merged pair
constexpr int MERGE_U = 2;            // chunks per lane in flight (seven loads each at most)
constexpr int MERGE_COUNTS = 6;

// pairs merged, not merged, bytes of text, bases of the merged reads, positions inside overlaps, of those taken from mate 2
struct MergeBlock { unsigned long long cnt[MERGE_COUNTS]; };

// Text length of pair (rows a.., b.., insert size ins); 0: the pair is not merged.  Positions and ranges only.
__device__ __forceinline__ int64_t merge_parse(const PairSide &A, const PairSide &B, longlong2 a01, longlong2 a23, longlong2 a45,
                                               longlong2 b23, longlong2 b45, int32_t ins, MrgPair &P)
{
    // the pair's geometry (ffq_pair.h), and mate 1's header
    const bool geo = pair_geometry(A, B, a23, a45, b23, b45, ins, MRG_MAX_LEN, P);
    const int64_t p0 = row_coord(a01.x, A.add), p1 = row_coord(a01.y, A.add);
    P.hsrc = 0; P.h = 0; P.L = 0;
    if (!geo || !(p0 >= 0 && p0 < p1 && p1 <= A.nbytes + A.s)) {
        P.asrc = P.qasrc = P.bsrc = P.qbsrc = 0; P.n1 = P.n2 = P.o = 0;
        return 0;
    }
    P.hsrc = p0 + 1 - A.s; P.h = p1 - p0 - 1;
    P.L = mrg_L(P.n1, P.n2, P.o);
    return mrg_len(P);
}

// pair k's rows and insert size (the thread has a pair: k < n_pairs)
struct MergeIn { longlong2 a01, a23, a45, b01, b23, b45; int64_t j; int32_t ins; };

__device__ __forceinline__ void merge_fetch(const PairSide &A, const PairSide &B, int64_t k, const int32_t *__restrict__ d_insert,
                                            const int64_t *__restrict__ d_ord, MergeIn &I)
{
    const longlong2 *sa = reinterpret_cast<const longlong2 *>(A.table + k * 6), *sb = reinterpret_cast<const longlong2 *>(B.table + k * 6);
    I.a01 = sa[0]; I.a23 = sa[1]; I.a45 = sa[2];
    I.b01 = sb[0]; I.b23 = sb[1]; I.b45 = sb[2];
    I.j = d_ord ? d_ord[k] : k;
    I.ins = d_insert[I.j];
}

// Workgroups stride over the blocks of 256 pairs; the three sums leave with one set of atomics per workgroup of the launch
// (wg_counts_flush, to the call's counts [0], [3], [4]).
__global__ __launch_bounds__(MERGE_WG) void k_merge_sum(PairSide A, PairSide B, int64_t n_pairs, int64_t nblk,
                                                        const int32_t *__restrict__ d_insert, const int64_t *__restrict__ d_ord,
                                                        long long *__restrict__ bsum, unsigned int *__restrict__ brest,
                                                        MergeBlock *__restrict__ blk)
{
    unsigned long long c_m = 0, c_b = 0, c_o = 0;
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {             // (uniform over the workgroup: barriers inside)
        const int64_t k = b * MERGE_WG + threadIdx.x;
        const bool have = k < n_pairs;
        int64_t len = 0;
        if (have) {
            MergeIn I;
            MrgPair P;
            merge_fetch(A, B, k, d_insert, d_ord, I);
            len = merge_parse(A, B, I.a01, I.a23, I.a45, I.b23, I.b45, I.ins, P);
            if (len > 0) { c_m++; c_b += (unsigned long long)P.L; c_o += (unsigned long long)mrg_overlap(P.n1, P.n2, P.o); }
        }
        int64_t tot;
        (void)wg_excl_scan<MERGE_WG, SCAN_ANY>(len, tot);
        const int rest = __syncthreads_count(have && len == 0 ? 1 : 0);  // (and the scan's LDS may be written again)
        if (threadIdx.x == 0) { bsum[b] = tot; brest[b] = (unsigned int)rest; }
    }
    const unsigned long long c[3] = {c_m, c_b, c_o};
    wg_counts_flush<MERGE_WG, 0, 3, 4>(c, blk->cnt);
}

// One merged pair by a group of G lanes (gl: this lane's place in it): `o` = where its first byte goes, len > 0 its length.
// store false: nothing is written.  Returns the lane's share of the overlap's positions taken from mate 2.
template <int G>
__device__ __forceinline__ unsigned int merge_copy(const uint8_t *__restrict__ d1, int64_t nb1, const uint8_t *__restrict__ d2, int64_t nb2,
                                                   const MrgPair &P, int64_t len, uint8_t *__restrict__ o, int gl, bool store)
{
    constexpr int U = MERGE_U;
    // chunk k covers text bytes [16 k - shift, +16) cut to [0, len)
    const int shift = (int)(reinterpret_cast<uintptr_t>(o) & 15);
    const int64_t nchunk = (len + shift + 15) >> 4;
    unsigned int taken = 0;
    for (int64_t k0 = 0; k0 < nchunk; k0 += (int64_t)G * U) {
        MrgLoads X[U];
        // every load of the lane's U chunks in flight together
#pragma unroll
        for (int j = 0; j < U; j++) {
            const int64_t k = k0 + (int64_t)j * G + gl;
            if (k < nchunk) mrg_chunk_load(d1, nb1, d2, nb2, P, 16 * k - shift, X[j]);
        }
#pragma unroll
        for (int j = 0; j < U; j++) {
            const int64_t k = k0 + (int64_t)j * G + gl;
            const int64_t clo = 16 * k - shift;
            if (k >= nchunk) continue;
            Mrg16 y;
            taken += (unsigned int)mrg_chunk_build(P, clo, X[j], y);
            if (!store) continue;
            const int kb = (int)max(-clo, (int64_t)0), ke = (int)min(len - clo, (int64_t)16);
            uint8_t *dst = o + clo;                           // 16-byte aligned; only [kb, ke) of it is the record's
            const uint4 v = make_uint4(y.x, y.y, y.z, y.w);
            if (kb == 0 && ke == 16) *reinterpret_cast<uint4 *>(dst) = v;
            else render_store_part(dst, v, kb, ke);
        }
    }
    return taken;
}

// A workgroup per block of 256 pairs.  total > text_cap: the offsets and the rest tables are written, the text is not touched.
__global__ __launch_bounds__(MERGE_WG) void k_merge_rows(PairSide A, PairSide B, int64_t n_pairs, const int32_t *__restrict__ d_insert,
                                                         const int64_t *__restrict__ d_ord, const long long *__restrict__ tbase,
                                                         const DevRes *__restrict__ res, const long long *__restrict__ rbase,
                                                         uint8_t *__restrict__ out, int64_t out_cap, int64_t *__restrict__ off,
                                                         int64_t *__restrict__ rest1, int64_t *__restrict__ rest2,
                                                         int64_t *__restrict__ rest_ord, MergeBlock *__restrict__ blk)
{
    constexpr int G = MERGE_G, NG = MERGE_WG / G;
    __shared__ MrgPair s_pair[MERGE_WG];
    __shared__ int64_t s_off[MERGE_WG], s_len[MERGE_WG];
    __shared__ uint32_t s_w[MERGE_WG / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t r0 = (int64_t)blockIdx.x * MERGE_WG, k = r0 + tid;
    const int64_t total = res->n_qual_bytes;
    {
        const bool have = k < n_pairs;
        MergeIn I;
        MrgPair P;
        int64_t len = 0;
        P.hsrc = P.asrc = P.qasrc = P.bsrc = P.qbsrc = 0; P.h = 0; P.n1 = P.n2 = P.o = P.L = 0;
        if (have) {
            merge_fetch(A, B, k, d_insert, d_ord, I);
            len = merge_parse(A, B, I.a01, I.a23, I.a45, I.b23, I.b45, I.ins, P);
        }
        const bool unm = have && len == 0;
        const unsigned long long m = wg_rank_put<MERGE_WG>(unm, s_w);
        int64_t tot;
        const int64_t at = tbase[blockIdx.x] + wg_excl_scan<MERGE_WG, SCAN_ANY>(len, tot);    // (a barrier inside: s_w is there behind it)
        s_pair[tid] = P; s_off[tid] = at; s_len[tid] = len;
        if (off && have) off[k] = at;
        if (blockIdx.x == 0 && tid == 0) {
            if (off) off[n_pairs] = total;
            blk->cnt[2] = (unsigned long long)total;
        }
        if (unm) {
            const int64_t r = rbase[blockIdx.x] + wg_rank_get<MERGE_WG>(m, s_w);
            longlong2 *da = reinterpret_cast<longlong2 *>(rest1 + r * 6), *db = reinterpret_cast<longlong2 *>(rest2 + r * 6);
            da[0] = I.a01; da[1] = I.a23; da[2] = I.a45;
            db[0] = I.b01; db[1] = I.b23; db[2] = I.b45;
            if (rest_ord) rest_ord[r] = I.j;
        }
    }
    __syncthreads();
    const bool store = total <= out_cap;
    const int g = tid / G, gl = tid & (G - 1);
    unsigned int taken = 0;
    // step i: group g has pair i * NG + g of the block -- the thirty-two pairs of a step are neighbours in the output
#pragma unroll 1
    for (int i = 0; i < G; i++) {
        const int r = i * NG + g;
        const int64_t len = s_len[r];
        if (len > 0) {
            const MrgPair P = s_pair[r];
            taken += merge_copy<G>(A.d, A.nbytes, B.d, B.nbytes, P, len, out + s_off[r], gl, store);
        }
    }
    const unsigned long long t = wave_sum_u64(taken);
    if (lane == 0 && t) atomicAdd(&blk->cnt[5], t);
}

}  // namespace ffq

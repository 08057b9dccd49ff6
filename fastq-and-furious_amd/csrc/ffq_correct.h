// ffq_correct.h -- mismatched bases inside the overlap of a pair's mates corrected by the surer mate: ffq_table_pair_correct
// (include/ffq.h states the rule; the byte work is csrc/ffq_correctwalk.h).
//
// Shape: the row frame of ffq_rows.h -- a group of eight lanes per PAIR, workgroups striding over the pairs, the next pair's
// rows and insert size asked for ahead.  Per pair:
//   * both rows are checked as the merge checks them (row_pos, both lines), the lengths against COR_MAX_LEN, the insert size
//     against the rows as they stand: a pair that fails is counted as not looked at and none of its bytes is read;
//   * the overlap is cut into chunks of sixteen positions, chunk c to lane c % 8, CORRECT_U chunks of a lane in flight: four
//     16-byte loads each, bounded by the LINE they read (cor_chunk_load), judged in registers (cor_chunk_build);
//   * THE STORE RULE: a lane writes only the corrected bytes, one byte store each -- base and quality of the mate that loses.
//     It never writes a loaded chunk back: sixteen bytes around a position reach into the other lines of the record and into
//     the neighbouring records, which other groups may be editing at the same time.  A pair has an insert size only if its
//     mismatches are few (max_diff), so stores are rare; the common pair, whose overlap agrees, costs its loads and nothing else.
//   * the chunks of a pair are distinct positions of both mates, so no lane reads a byte another lane of its group writes; rows
//     of DIFFERENT pairs must not share bytes -- the call's contract, unlike every other table pass.
// The loop over a lane's chunks holds no ballot, DPP move or barrier: its trip count differs from lane to lane.  Behind it the
// group sums its corrections with DPP moves (uniform again).  No pair above 512 bases is touched: there is no long rows' launch.
// The matrix goes to counters in LDS (32 bit, one set per workgroup) and leaves with one set of 64-bit atomics per workgroup
// (lds_hist_flush); the six counts leave by wg_counts_flush (ffq_rows.h).
#pragma once
#include "ffq_pair.h"
#include "ffq_correctwalk.h"

namespace ffq {

constexpr int CORRECT_WG = 256;
constexpr int CORRECT_U = 2;          // chunks per lane in flight (four loads each)
constexpr int CORRECT_COUNTS = 6;
constexpr int CORRECT_MATRIX = 20;    // (class before 0..4) * 4 + class after 0..3

// pairs looked at, pairs with a correction, bases corrected in mate 1, in mate 2, mismatch positions, pairs not looked at
struct CorrectBlock { unsigned long long cnt[CORRECT_COUNTS]; unsigned long long matrix[CORRECT_MATRIX]; };

struct CorrectRules { uint32_t G, B; };           // the threshold BYTES: qual_base + good_quality, qual_base + bad_quality

// Is pair (rows a.., b.., insert size ins) looked at?  The pair's geometry (ffq_pair.h) and nothing else.
__device__ __forceinline__ bool correct_parse(const PairSide &A, const PairSide &B, longlong2 a23, longlong2 a45, longlong2 b23, longlong2 b45,
                                              int32_t ins, CorPair &P)
{
    return pair_geometry(A, B, a23, a45, b23, b45, ins, MRG_MAX_LEN, P);
}

// w1 / w2: the two buffers again (A.d, B.d), writable
__global__ __launch_bounds__(CORRECT_WG) void k_pair_correct(PairSide A, PairSide B, uint8_t *w1, uint8_t *w2, int64_t n_pairs,
                                                             const int32_t *__restrict__ d_insert, const CorrectRules R, int want_matrix,
                                                             CorrectBlock *__restrict__ blk)
{
    constexpr int G = ROWS_G, RPB = CORRECT_WG / G, U = CORRECT_U;
    __shared__ uint32_t s_mat[CORRECT_MATRIX];
    const int lane = threadIdx.x & 63, gl = lane & (G - 1);
    if (threadIdx.x < CORRECT_MATRIX) s_mat[threadIdx.x] = 0;
    __syncthreads();

    unsigned int c_look = 0, c_pairs = 0, c_f1 = 0, c_f2 = 0, c_not = 0;
    unsigned long long c_mm = 0;
    const int64_t step = (int64_t)gridDim.x * RPB;
    const longlong2 zero = make_longlong2(0, 0);
    longlong2 xa23 = zero, xa45 = zero, xb23 = zero, xb45 = zero;
    int32_t xins = -1;
    {
        const int64_t pair = (int64_t)blockIdx.x * RPB + (threadIdx.x / G);
        if (pair < n_pairs) {
            const longlong2 *sa = reinterpret_cast<const longlong2 *>(A.table + pair * 6), *sb = reinterpret_cast<const longlong2 *>(B.table + pair * 6);
            xa23 = sa[1]; xa45 = sa[2]; xb23 = sb[1]; xb45 = sb[2];
            xins = d_insert[pair];
        }
    }
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < n_pairs; r0 += step) {
        const int64_t pair = r0 + (threadIdx.x / G);
        const bool have = pair < n_pairs;
        const longlong2 a23 = xa23, a45 = xa45, b23 = xb23, b45 = xb45;
        const int32_t ins = xins;
        if (pair + step < n_pairs) {
            const longlong2 *sa = reinterpret_cast<const longlong2 *>(A.table + (pair + step) * 6);
            const longlong2 *sb = reinterpret_cast<const longlong2 *>(B.table + (pair + step) * 6);
            xa23 = sa[1]; xa45 = sa[2]; xb23 = sb[1]; xb45 = sb[2];
            xins = d_insert[pair + step];
        }
        CorPair P;
        const bool look = have && correct_parse(A, B, a23, a45, b23, b45, ins, P);
        const int nchunk = look ? cor_nchunk(P) : 0, lo = cor_lo(P);

        // ---- the lane's chunks: gl, gl + 8, ...; U of them in flight (no ballot, DPP move or barrier in here) ----
        unsigned int f1 = 0, f2 = 0;
        for (int c0 = gl; c0 < nchunk; c0 += G * U) {
            CorLoads X[U];
#pragma unroll
            for (int j = 0; j < U; j++)
                if (c0 + j * G < nchunk) cor_chunk_load(A.d, B.d, P, c0 + j * G, X[j]);
#pragma unroll
            for (int j = 0; j < U; j++) {
                const int c = c0 + j * G;
                if (c >= nchunk) continue;
                CorChunk Y;
                cor_chunk_build(P, c, X[j], R.G, R.B, Y);
                c_mm += (unsigned long long)Y.mism;
                const int p0 = lo + 16 * c;
                // the store rule: the corrected bytes, one by one, and nothing beside them
                for (uint32_t m = cor_bits16(Y.fix1); m; m &= m - 1) {
                    const int i = __builtin_ctz(m);
                    const uint8_t nb = cor_byte(Y.na, i);
                    w1[P.asrc + p0 + i] = nb;
                    w1[P.qasrc + p0 + i] = cor_byte(Y.nqa, i);
                    if (want_matrix) atomicAdd(&s_mat[cor_cls(cor_byte(X[j].a, i)) * 4 + cor_cls(nb)], 1u);
                    f1++;
                }
                for (uint32_t m = cor_bits16(Y.fix2); m; m &= m - 1) {
                    const int i = __builtin_ctz(m), bi = cor_bi(P, p0 + i);
                    const uint8_t nb = cor_byte(Y.nb, i);
                    w2[P.bsrc + bi] = nb;
                    w2[P.qbsrc + bi] = cor_byte(Y.nqb, i);
                    // (byte i in position order is byte 15 - i of mate 2's load)
                    if (want_matrix) atomicAdd(&s_mat[cor_cls(cor_byte(X[j].b, 15 - i)) * 4 + cor_cls(nb)], 1u);
                    f2++;
                }
            }
        }
        const int fixed = RowGroup<G>::sum((int)(f1 + f2));
        c_f1 += f1; c_f2 += f2;
        if (have && gl == 0) {
            if (look) c_look++; else c_not++;
            if (fixed > 0) c_pairs++;
        }
    }

    // the matrix (lds_hist_flush), and the counts (wg_counts_flush)
    __syncthreads();
    if (want_matrix) lds_hist_flush<CORRECT_WG>(s_mat, CORRECT_MATRIX, blk->matrix);
    const unsigned long long c[CORRECT_COUNTS] = {c_look, c_pairs, c_f1, c_f2, c_mm, c_not};
    wg_counts_flush<CORRECT_WG>(c, blk->cnt);
}

}  // namespace ffq

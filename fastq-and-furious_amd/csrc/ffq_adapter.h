// ffq_adapter.h -- 3' adapter trimming by editing rows of the offset table (ffq_table_trim_adapter).
//
// The rule (include/ffq.h states it as a loop): for seq[0..n) = buf[pos2:pos3] and the adapter ad[0..m), the LEFTMOST
// position p in [0, n - min_overlap] at which the first ov = min(m, n - p) adapter bytes differ from seq[p .. p + ov) in
// at most ov * err_permille / 1000 places ('N' in the adapter matches anything) becomes the read's new end: pos3 = pos2 + p,
// pos5 = pos4 + p.  Mismatches only, no indels.  Eligibility is ffq_table_trim_quality's, with the newline looked for in the
// SEQUENCE; any other row is copied unchanged and counted.
//
// Shape: the row frame of ffq_rows.h -- eight lanes per row; rows of more than ADAPTER_LONG bases get a whole wave in the second
// launch.  The pass's own part is the match.  Candidates are taken in CHUNKS of G * 8 ascending positions, eight consecutive
// ones per lane:
//   * the chunk's bytes seq[p0 .. p0 + G * 8 + 64) -- its candidates and the 63 bytes behind the last of them -- are staged
//     once into the group's LDS window, sixteen bytes per lane (unaligned dword loads; a piece the read's end cuts short
//     byte by byte, zeros behind it), and looked through for '\n' on the way;
//   * a lane takes the dwords of its own eight candidates out of the window (its first byte is dword-aligned there), and for
//     candidate k and adapter dword w byte-aligns two of them (v_alignbyte), XORs the adapter dword, ANDs the wildcard mask
//     (0x00 for 'N' and behind the adapter) and the overlap mask (behind the read's end), and counts the non-zero bytes; the
//     adapter and its mask are a kernel argument passed by value -- scalar registers, indexed by constants in the unrolled loop;
//   * a candidate is dropped when its mismatches exceed what ITS overlap allows, and the loop over the adapter's dwords ends
//     as soon as no lane of the wave has a live candidate (on random bases: after the second dword);
//   * one max-reduction of (chunk size - position) over the group finds the leftmost hit; the group stops at the first chunk
//     that has one.
// Every loop is uniform over the wave, as the frame asks: a group with an empty or ineligible row, or done with its row, steps
// along with nothing to do until every group of the wave is done.  What the chunks did not read (the read behind a hit) is
// then looked through for '\n' sixteen bytes per lane.  No byte outside the row's own sequence range, itself checked against
// the buffer, is read.
#pragma once
#include "ffq_rows.h"

namespace ffq {

constexpr int ADAPTER_LONG = 2048;    // bases above which a row gets a wave of its own
constexpr int ADAPTER_WG = 256;
constexpr int ADAPTER_MAX = 64;       // longest adapter
constexpr int ADAPTER_K = 8;          // consecutive candidates per lane and chunk

// the adapter as the kernels take it, by value: its bytes and, per byte, 0xFF where it has to match (0x00: 'N', or behind the end)
struct AdapterArg { uint32_t a[ADAPTER_MAX / 4]; uint32_t k[ADAPTER_MAX / 4]; };

template <int G> struct AdapterShape {
    static constexpr int CH = G * ADAPTER_K;          // candidates per chunk
    static constexpr int WIN = CH + ADAPTER_MAX;      // bytes of the window
    static_assert(WIN <= G * 16 && WIN % 16 == 0, "sixteen bytes per lane fill the window");
};

// number of non-zero bytes of x (exact, no carry between bytes)
__device__ __forceinline__ int adapter_nzbytes(uint32_t x)
{
    return __popc((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u);
}

// seq[a .. a + 16) into x, zeros from seq[n] on (a >= 0); nl: one of the bytes read is '\n'
__device__ __forceinline__ void adapter_load16(const uint8_t *__restrict__ seq, int64_t a, int64_t n, uint32_t (&x)[4], bool &nl)
{
    x[0] = x[1] = x[2] = x[3] = 0;
    if (a + 16 <= n) {
#pragma unroll
        for (int w = 0; w < 4; w++) x[w] = *reinterpret_cast<const rows_u32u *>(seq + a + 4 * w);
    } else {
        const int have = (int)max(n - a, (int64_t)0);
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (j < have) x[j >> 2] |= (uint32_t)seq[a + j] << (8 * (j & 3));
        if (have <= 0) return;
        // (zeros behind the end are no newlines)
    }
#pragma unroll
    for (int w = 0; w < 4; w++) nl |= has_nl(x[w]);
}

// The cut of one row per group: the leftmost qualifying position, n if there is none.  live: the group has an eligible row
// to match (uniform in the group).  win: the group's WIN bytes of LDS.  nread: seq[0 .. nread) went through the newline check.
template <int G>
__device__ __forceinline__ void adapter_match(const uint8_t *__restrict__ seq, int64_t n, bool live, const AdapterArg &ad, int m,
                                              int err, int min_overlap, int gl, uint32_t *__restrict__ win, int64_t &cut,
                                              int64_t &nread, bool &nl)
{
    constexpr int CH = AdapterShape<G>::CH, WIN = AdapterShape<G>::WIN, K = ADAPTER_K;
    constexpr int NR = (K - 1 + ADAPTER_MAX - 1) / 4 + 1;       // dwords a lane's eight candidates can touch: 18 (K = 8)
    static_assert(K % 4 == 0 && (G - 1) * K + NR * 4 <= WIN, "a lane's dwords lie inside the window");
    const int64_t ncand = n - min_overlap + 1;                  // candidates are 0 .. ncand - 1
    const int nd = min(NR, (K - 1 + m - 1) / 4 + 2);            // dwords a lane needs for this adapter (uniform)
    cut = n; nread = 0;
    int64_t p0 = 0;
    bool act = live && ncand > 0;
    while (__any(act)) {
        // ---- stage seq[p0 .. p0 + WIN) ----
        if (gl * 16 < WIN) {
            uint32_t x[4] = {0, 0, 0, 0};
            if (act) adapter_load16(seq, p0 + gl * 16, n, x, nl);
            *reinterpret_cast<uint4 *>(win + gl * 4) = make_uint4(x[0], x[1], x[2], x[3]);
        }
        wave_sync();
        uint32_t r[NR];
#pragma unroll
        for (int i = 0; i < NR; i++) r[i] = i < nd ? win[gl * (K / 4) + i] : 0u;
        // ---- this lane's candidates p0 + gl * K + k, ascending; its first hit ----
        int key = 0;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int64_t p = p0 + gl * K + k;
            const bool valid = act && p < ncand;
            const int ov = (int)min((int64_t)m, n - p);         // (>= min_overlap where valid)
            const int allowed = valid ? (ov * err) / 1000 : -1;
            int mm = 0;
            bool go = true;                                     // uniform: some lane's candidate is alive
#pragma unroll
            for (int w = 0; w < ADAPTER_MAX / 4; w++) {
                if (go && 4 * w < m) {
                    const uint32_t x = __builtin_amdgcn_alignbyte(r[(k >> 2) + w + 1], r[(k >> 2) + w], k & 3);
                    const int vc = ov - 4 * w;                  // bytes of this dword inside the overlap
                    const uint32_t bm = vc >= 4 ? 0xFFFFFFFFu : vc <= 0 ? 0u : (1u << (8 * vc)) - 1u;
                    mm += adapter_nzbytes((x ^ ad.a[w]) & ad.k[w] & bm);
                    go = __any(mm <= allowed) != 0;
                }
            }
            if (mm <= allowed && key == 0) key = CH - (gl * K + k);
        }
        const int gmax = RowGroup<G>::maxall(key);             // the leftmost hit of the chunk: CH - its position; 0: none
        if (act) {
            nread = min(p0 + WIN, n);
            if (gmax > 0) { cut = p0 + (CH - gmax); act = false; }
            else { p0 += CH; act = p0 < ncand; }
        }
    }
}

// One row per group.  have: this group has a row (uniform in the group).  defer_long: rows above ADAPTER_LONG are left to the
// second launch; returns whether this is one.
template <int G>
__device__ __forceinline__ bool adapter_row(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add, const int64_t *table,
                                            int64_t *out, int64_t row, bool have, longlong2 r01, longlong2 r23, longlong2 r45,
                                            const AdapterArg &ad, int m, int err, int min_overlap, bool defer_long, int gl,
                                            int gshift, uint32_t *__restrict__ win, RowCounts &cnt)
{
    int64_t p2 = 0, p4 = 0, n = 0;
    const bool elig = have && row_pos<true, false>(nbytes, s, add, r23, r45, p2, p4, n);
    const bool is_long = defer_long && elig && n > ADAPTER_LONG;
    const bool live = elig && !is_long && n > 0;
    const uint8_t *seq = d + (p2 - s);

    int64_t cut = n, nread = 0;
    bool nl = false;
    adapter_match<G>(seq, n, live, ad, m, err, min_overlap, gl, win, cut, nread, nl);
    rows_scan_nl<G>(seq, nread, n, live, gl, nl);
    const bool any_nl = group_any<G>(nl, gshift);

    // (pos + cut: the row's own coordinates, whatever `add` is)
    row_edit_finish(table, out, row, gl, have, is_long, elig && !any_nl, r01, r23, r45, make_longlong2(r23.x, r23.x + cut),
                    make_longlong2(r45.x, r45.x + cut), n - cut, cnt);
    return is_long;
}

__global__ __launch_bounds__(ADAPTER_WG) void k_adapter_rows(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                             const int64_t *table, int64_t n_rows, const AdapterArg ad, int m,
                                                             int err, int min_overlap, int64_t *out,
                                                             int64_t *__restrict__ long_list, RowsBlock *__restrict__ blk)
{
    constexpr int G = ROWS_G;
    __shared__ __attribute__((aligned(16))) uint32_t s_win[ADAPTER_WG / G][AdapterShape<G>::WIN / 4];
    const int lane = threadIdx.x & 63, gl = lane & (G - 1), gshift = lane & ~(G - 1);
    uint32_t *win = s_win[threadIdx.x / G];
    RowCounts cnt;
    constexpr int RPB = ADAPTER_WG / G;
    const int64_t step = (int64_t)gridDim.x * RPB;
    longlong2 x01 = make_longlong2(0, 0), x23 = x01, x45 = x01;
    {
        const int64_t row = (int64_t)blockIdx.x * RPB + (threadIdx.x / G);
        if (row < n_rows) {
            const longlong2 *src = reinterpret_cast<const longlong2 *>(table + row * 6);
            x01 = src[0]; x23 = src[1]; x45 = src[2];
        }
    }
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < n_rows; r0 += step) {
        const int64_t row = r0 + (threadIdx.x / G);
        const longlong2 r01 = x01, r23 = x23, r45 = x45;
        if (row + step < n_rows) {
            const longlong2 *src = reinterpret_cast<const longlong2 *>(table + (row + step) * 6);
            x01 = src[0]; x23 = src[1]; x45 = src[2];
        }
        const bool is_long = adapter_row<G>(d, nbytes, s, add, table, out, row, row < n_rows, r01, r23, r45, ad, m, err, min_overlap, true,
                                            gl, gshift, win, cnt);
        const int64_t at = long_list_append(is_long && gl == 0, lane, &blk->n_long);
        if (at >= 0) long_list[at] = row;
    }
    cnt.add_to<ADAPTER_WG>(blk);
}

// the rows k_adapter_rows left: 512 candidates per chunk
__global__ __launch_bounds__(ADAPTER_WG) void k_adapter_long(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                             const int64_t *table, const AdapterArg ad, int m, int err,
                                                             int min_overlap, int64_t *out, const int64_t *__restrict__ long_list,
                                                             RowsBlock *__restrict__ blk)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_win[ADAPTER_WG / 64][AdapterShape<64>::WIN / 4];
    const int lane = threadIdx.x & 63;
    uint32_t *win = s_win[threadIdx.x >> 6];
    RowCounts cnt;
    for (LongRows<ADAPTER_WG, true> it((int64_t)blk->n_long, long_list, table); it.next();)
        adapter_row<64>(d, nbytes, s, add, table, out, it.row, it.have, it.r01, it.r23, it.r45, ad, m, err, min_overlap, false, lane, 0, win,
                        cnt);
    cnt.add_to<ADAPTER_WG>(blk);
}

}  // namespace ffq

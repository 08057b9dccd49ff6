// ffq_trim.h -- quality trimming by editing rows of the offset table (ffq_table_trim_quality).
//
// The reference's user guide names two uses of a table of positions (/root/reference/doc/user-guide.rst:196-204):
// deleting rows (ffq_table_select_seqlen) and MODIFYING them -- "trimming either end of the read could be done by
// ... modifying the values in a table of indices".  This is the second one, with the running-sum rule BWA and
// cutadapt use for -q.  For q[0..n) = buf[pos4:pos5], d(i) = cutoff - (q[i] - base):
//     5' end: walk i = 0 .. n-1, s += d(i); stop when s < 0; start = i + 1 at the FIRST maximum of s above 0
//     3' end: walk i = n-1 .. 0 with its own cutoff, independent of the 5' result; stop = i at the first maximum
//     start >= stop: the read is trimmed away (start = stop = 0)
// and the row becomes pos2 + start, pos2 + stop, pos4 + start, pos4 + stop.  A row is ELIGIBLE if pos2..pos5 - add
// are inside the buffer, pos3 - pos2 == pos5 - pos4 >= 0 and no quality byte is '\n' (a wrapped record); any other
// row is copied unchanged and counted.
//
// Shape.  A GROUP of G lanes owns a row (G = 8: eight rows per wave, thirty-two per workgroup; rows of more than
// TRIM_LONG quality bytes go onto a list and a second launch gives each a whole wave, G = 64, so that one long read
// does not hold back a wave of short ones).  Either end is walked from the outside in, in chunks of G * B bytes
// (B consecutive bytes per lane, 8 or 16, as unaligned dwords: 64 bytes per short row and chunk); inside a chunk the lanes' sums of d are
// prefix-summed across the group, every lane steps through its B bytes, a ballot finds the first lane whose running
// sum went negative, and one max-reduction of (rise, position) the first maximum in front of it; (sum, best) are carried to the
// next chunk in 64 bits (a record of 2^31 bytes of the lowest quality sums to 2^38), everything inside a chunk is
// 32-bit and relative to the carried sum.  An end is done when its sum has gone negative: on real reads that is the
// first chunk.  The eligibility rule needs every quality byte once, so the bytes between the two walks are then
// checked for '\n' 16 per lane -- for reads of a few hundred bases that is the same few 64-byte sectors the walks
// touch anyway.  No byte outside the row's own quality range, itself checked against the buffer, is read.
#pragma once
#include "ffq_dev.h"

namespace ffq {

constexpr int TRIM_LONG = 4096;       // quality bytes above which a row gets a wave of its own
constexpr int TRIM_WG = 256;
constexpr int TRIM_G = 8, TRIM_B = 8; // lanes per row and bytes per lane and chunk of the short rows' kernel

// counters of a call: rows changed, bases removed, rows skipped, rows on the long list
struct TrimBlock { unsigned long long changed, removed, skipped, n_long; };

typedef uint32_t trim_u32u __attribute__((aligned(1)));

// B bytes at a[0 .. B) as ints; only j in [jlo, jhi) are read, the others are -1
template <int B>
__device__ __forceinline__ void trim_load(const uint8_t *__restrict__ a, int jlo, int jhi, int (&qv)[B])
{
    if (jlo == 0 && jhi == B) {
#pragma unroll
        for (int w = 0; w < B / 4; w++) {
            const uint32_t x = *reinterpret_cast<const trim_u32u *>(a + 4 * w);
#pragma unroll
            for (int k = 0; k < 4; k++) qv[4 * w + k] = (int)((x >> (8 * k)) & 0xFFu);
        }
    } else {
#pragma unroll
        for (int j = 0; j < B; j++) qv[j] = (j >= jlo && j < jhi) ? (int)a[j] : -1;
    }
}

// first lane of this lane's group whose bit is set in a wave ballot; G if none
template <int G>
__device__ __forceinline__ int trim_first(unsigned long long m, int gshift)
{
    if constexpr (G == 64) return m ? __builtin_ctzll(m) : 64;
    else {
        const uint32_t b = (uint32_t)(m >> gshift) & ((1u << G) - 1u);
        return b ? __builtin_ctz(b) : G;
    }
}

// Sums and maxima across a group.  Eight lanes: DPP moves inside the 16-lane row (row_shr, quad_perm, row_half_mirror
// stay inside an aligned group of eight or are masked off by the lane's place in it) -- a VALU instruction each where a
// shuffle is an LDS round trip.  A whole wave: the library's DPP scan, xor shuffles.
template <int CTRL>
__device__ __forceinline__ int trim_dpp(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}

template <int G> struct TrimGroup;

template <> struct TrimGroup<8> {
    static __device__ __forceinline__ int incl_scan(int x, int gl)
    {
        x += trim_dpp<0x111>(x) & (gl >= 1 ? -1 : 0);       // row_shr:1
        x += trim_dpp<0x112>(x) & (gl >= 2 ? -1 : 0);       // row_shr:2
        x += trim_dpp<0x114>(x) & (gl >= 4 ? -1 : 0);       // row_shr:4
        return x;
    }
    static __device__ __forceinline__ int sum(int x)
    {
        x += trim_dpp<0xB1>(x);                             // quad_perm:[1,0,3,2]
        x += trim_dpp<0x4E>(x);                             // quad_perm:[2,3,0,1]
        x += trim_dpp<0x141>(x);                            // row_half_mirror: the other quad of the eight
        return x;
    }
    static __device__ __forceinline__ int maxall(int x)
    {
        x = max(x, trim_dpp<0xB1>(x));
        x = max(x, trim_dpp<0x4E>(x));
        x = max(x, trim_dpp<0x141>(x));
        return x;
    }
};

template <> struct TrimGroup<64> {
    static __device__ __forceinline__ int incl_scan(int x, int) { return (int)wave_incl_scan((uint32_t)x); }
    static __device__ __forceinline__ int sum(int x)
    {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
        return x;
    }
    static __device__ __forceinline__ int maxall(int x)
    {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) x = max(x, __shfl_xor(x, o));
        return x;
    }
};

// This lane's B bytes of the chunk of walk positions [w0, w0 + G * B): walk position w is byte w of q[0 .. n) (front)
// or byte n - 1 - w (back); qv in ascending ADDRESS order, -1 where there is no byte (or the group is not active).
template <int G, int B, bool BACK>
__device__ __forceinline__ void trim_chunk(const uint8_t *__restrict__ q, int64_t n, bool act, int64_t w0, int gl, int (&qv)[B])
{
    const int64_t w = w0 + (int64_t)gl * B;           // this lane's first walk position
    const int avail = act ? (int)min(max(n - w, (int64_t)0), (int64_t)B) : 0;
    if (BACK) trim_load<B>(q + (n - w - B), B - avail, B, qv);
    else trim_load<B>(q + w, 0, avail, qv);
}

// One end of one row per group.  first: the end's first chunk (trim_chunk at w0 = 0), loaded by the caller together with
// the other end's so that a row whose walks end there -- nearly every one -- waits for memory once.
// cut = positions trimmed from this end, nread = positions [0, nread) were read, nl = one of them was '\n'.
// `live` is uniform inside a group; the loop is uniform over the wave (a finished group steps along with zeros).
template <int G, int B, bool BACK>
__device__ __forceinline__ void trim_walk(const uint8_t *__restrict__ q, int64_t n, bool live, int cutoff, int base,
                                          int gl, int gshift, const int (&first)[B], int64_t &cut, int64_t &nread, bool &nl)
{
    int64_t s = 0, best = 0, w0 = 0;
    cut = 0; nread = 0;
    bool act = live && n > 0;
    for (bool head = true; __any(act); head = false) {
        int qv[B];
        if (head) {
#pragma unroll
            for (int k = 0; k < B; k++) qv[k] = act ? first[k] : -1;
        } else
            trim_chunk<G, B, BACK>(q, n, act, w0, gl, qv);
        int d[B], t = 0;
#pragma unroll
        for (int k = 0; k < B; k++) {
            const int x = BACK ? qv[B - 1 - k] : qv[k];
            nl |= x == 10;
            d[k] = x < 0 ? 0 : cutoff + base - x;
            t += d[k];
        }
        const int incl = TrimGroup<G>::incl_scan(t, gl);
        const int total = TrimGroup<G>::sum(t);
        // relative to the carried sum s (>= 0 while the end is alive): dead when s + r < 0, a new maximum when s + r > best
        const int lim = (int)min(s, (int64_t)1 << 30);
        const int brel = (int)min(best - s, (int64_t)1 << 30);
        int r = incl - t, m = brel, mi = -1;
        bool ldead = false;
#pragma unroll
        for (int k = 0; k < B; k++) {
            r += d[k];
            if (!ldead) {
                if (r < -lim) ldead = true;
                else if (r > m) { m = r; mi = k; }
            }
        }
        const int fl = trim_first<G>(__ballot(ldead), gshift);          // first lane that died; G: none
        // the first maximum in front of it: one max-reduction of (rise above best, C - 1 - position in the chunk) -- a
        // rise is below C * 382 < 2^19, so the key fits 32 bits; 0: no lane has a candidate
        constexpr int C = G * B, PB = C == 64 ? 6 : 10;
        static_assert(C == 64 || C == 1024, "the key of the first maximum is laid out for chunks of 64 or 1024 bytes");
        const bool cand = mi >= 0 && gl <= fl;
        const int gmax = TrimGroup<G>::maxall(cand ? (((m - brel) << PB) | (C - 1 - (gl * B + mi))) : 0);
        if (act) {
            if (gmax > 0) { best = s + brel + (gmax >> PB); cut = w0 + (C - (gmax & (C - 1))); }
            s += total;
            w0 += (int64_t)G * B;
            nread = min(w0, n);
            act = fl == G && w0 < n;
        }
    }
}

// '\n' among q[a .. min(a + 16, hi)), a < hi: sixteen bytes in one go; a piece cut short by hi is read as the sixteen
// bytes in front of hi instead (bytes of the same quality string: a newline there counts all the same)
__device__ __forceinline__ bool trim_nl16(const uint8_t *__restrict__ q, int64_t a, int64_t hi)
{
    bool nl = false;
    if (a + 16 > hi && hi < 16) {
        for (int64_t j = a; j < hi; j++) nl |= q[j] == 10;
        return nl;
    }
    const uint8_t *p = q + (a + 16 <= hi ? a : hi - 16);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t x = *reinterpret_cast<const trim_u32u *>(p + 4 * k) ^ 0x0A0A0A0Au;
        nl |= ((x - 0x01010101u) & ~x & 0x80808080u) != 0;
    }
    return nl;
}

// '\n' among q[lo .. hi) (16 bytes per lane and step)
template <int G>
__device__ __forceinline__ void trim_scan_nl(const uint8_t *__restrict__ q, int64_t lo, int64_t hi, bool live, int gl, bool &nl)
{
    if (!live) return;
    for (int64_t w = lo + (int64_t)gl * 16; w < hi; w += (int64_t)G * 16) nl |= trim_nl16(q, w, hi);
}

// the 48 bytes of a row by the first three lanes of its group
__device__ __forceinline__ void trim_store_row(int64_t *__restrict__ out, int64_t row, int gl, longlong2 a, longlong2 b,
                                               longlong2 c)
{
    longlong2 v = a;
    if (gl == 1) v = b;
    if (gl == 2) v = c;
    if (gl < 3) reinterpret_cast<longlong2 *>(out + row * 6)[gl] = v;
}

// One row per group.  have: this group has a row (uniform in the group).  Returns through the references what lane 0
// of the group adds to the call's counters.  defer_long: rows above TRIM_LONG are left to the second launch (is_long).
template <int G, int B>
__device__ __forceinline__ void trim_row(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                         const int64_t *__restrict__ table, int64_t *__restrict__ out, int64_t row,
                                         bool have, longlong2 r01, longlong2 r23, longlong2 r45, int base, int cf, int cb,
                                         bool defer_long, int gl, int gshift, bool &is_long, unsigned int &changed,
                                         unsigned long long &removed, unsigned int &skipped)
{
    // buffer coordinates (wrapping arithmetic: a row may hold anything)
    const int64_t p2 = (int64_t)((uint64_t)r23.x - (uint64_t)add), p3 = (int64_t)((uint64_t)r23.y - (uint64_t)add);
    const int64_t p4 = (int64_t)((uint64_t)r45.x - (uint64_t)add), p5 = (int64_t)((uint64_t)r45.y - (uint64_t)add);
    const int64_t L = nbytes + s;
    const int64_t n = p5 - p4;
    bool elig = have && p2 >= 0 && p4 >= 0 && p2 <= p3 && p4 <= p5 && p3 <= L && p5 <= L && p3 - p2 == n;
    // coordinate 0 of a buffer with a sentinel is the virtual '\n'
    if (elig && n > 0 && p4 < s) elig = false;
    is_long = defer_long && elig && n > TRIM_LONG;
    const bool live = elig && !is_long;
    const uint8_t *q = d + (p4 - s);

    // everything a row whose walks end in their first chunk needs, asked for at once: the first chunk of either end and
    // the next G * 16 bytes of what lies between them
    constexpr int C = G * B;
    int qf[B], qb[B];
    trim_chunk<G, B, false>(q, n, live && n > 0, 0, gl, qf);
    trim_chunk<G, B, true>(q, n, live && n > 0, 0, gl, qb);
    bool nl = false;
    if (live && C + (int64_t)gl * 16 < n - C) nl = trim_nl16(q, C + (int64_t)gl * 16, n - C);

    int64_t cutf = 0, cutb = 0, rf = 0, rb = 0;
    trim_walk<G, B, false>(q, n, live, cf, base, gl, gshift, qf, cutf, rf, nl);
    trim_walk<G, B, true>(q, n, live, cb, base, gl, gshift, qb, cutb, rb, nl);
    trim_scan_nl<G>(q, max(rf, (int64_t)(C + G * 16)), n - rb, live, gl, nl);
    const bool any_nl = trim_first<G>(__ballot(nl), gshift) != G;

    if (!have || is_long) return;
    if (!elig || any_nl) {
        if (gl == 0) skipped++;
        if (out != table) trim_store_row(out, row, gl, r01, r23, r45);
        return;
    }
    int64_t start = cutf, stop = n - cutb;
    if (start >= stop) start = stop = 0;
    const bool ch = start != 0 || stop != n;
    if (gl == 0 && ch) { changed++; removed += (unsigned long long)(n - (stop - start)); }
    if (ch || out != table) {
        // (pos + start: the row's own coordinates, whatever `add` is)
        const longlong2 n23 = make_longlong2(r23.x + start, r23.x + stop), n45 = make_longlong2(r45.x + start, r45.x + stop);
        trim_store_row(out, row, gl, r01, n23, n45);
    }
}

__device__ __forceinline__ void trim_add_counters(TrimBlock *__restrict__ blk, unsigned int changed,
                                                  unsigned long long removed, unsigned int skipped)
{
    // every thread of the workgroup is here: sums over the wave, over the workgroup's waves through LDS, and one set of
    // atomics per workgroup (device-wide atomics on three addresses are served one at a time)
    __shared__ unsigned long long s_cnt[TRIM_WG / 64][3];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        changed += __shfl_xor(changed, o);
        skipped += __shfl_xor(skipped, o);
        removed += (unsigned long long)__shfl_xor((long long)removed, o);
    }
    if ((threadIdx.x & 63) == 0) {
        s_cnt[threadIdx.x >> 6][0] = changed; s_cnt[threadIdx.x >> 6][1] = removed; s_cnt[threadIdx.x >> 6][2] = skipped;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long c = 0, r = 0, k = 0;
#pragma unroll
        for (int w = 0; w < TRIM_WG / 64; w++) { c += s_cnt[w][0]; r += s_cnt[w][1]; k += s_cnt[w][2]; }
        if (c) atomicAdd(&blk->changed, c);
        if (r) atomicAdd(&blk->removed, r);
        if (k) atomicAdd(&blk->skipped, k);
    }
}

// thirty-two rows per workgroup and step, eight lanes and 64-byte chunks each; workgroups stride over the table (the
// counters cost three atomics per workgroup of the launch, not per row) and ask for their next rows before they work on these
__global__ __launch_bounds__(TRIM_WG) void k_trim_rows(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                       const int64_t *table, int64_t n_rows, int base, int cf, int cb,
                                                       int64_t *out, int64_t *__restrict__ long_list,
                                                       TrimBlock *__restrict__ blk)
{
    constexpr int G = TRIM_G, RPB = TRIM_WG / G;
    const int lane = threadIdx.x & 63, gl = lane & (G - 1), gshift = lane & ~(G - 1);
    unsigned int changed = 0, skipped = 0;
    unsigned long long removed = 0;
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
        bool is_long = false;
        trim_row<G, TRIM_B>(d, nbytes, s, add, table, out, row, row < n_rows, r01, r23, r45, base, cf, cb, true, gl, gshift,
                            is_long, changed, removed, skipped);
        // the long rows of the wave take their places on the list with one atomic
        const unsigned long long lm = __ballot(is_long && gl == 0);
        if (lm) {
            unsigned long long at = 0;
            if (lane == 0) at = atomicAdd(&blk->n_long, (unsigned long long)__popcll(lm));
            at = (unsigned long long)__shfl((long long)at, 0);
            if (is_long && gl == 0) long_list[at + __popcll(lm & ((1ull << lane) - 1ull))] = row;
        }
    }
    trim_add_counters(blk, changed, removed, skipped);
}

// the rows k_trim_rows left: a wave per row, sixteen bytes per lane and chunk
__global__ __launch_bounds__(TRIM_WG) void k_trim_long(const uint8_t *__restrict__ d, int64_t nbytes, int s, int64_t add,
                                                       const int64_t *table, int base, int cf, int cb, int64_t *out,
                                                       const int64_t *__restrict__ long_list, TrimBlock *__restrict__ blk)
{
    constexpr int WPB = TRIM_WG / 64;
    const int lane = threadIdx.x & 63;
    const int64_t n_long = (int64_t)blk->n_long;
    unsigned int changed = 0, skipped = 0;
    unsigned long long removed = 0;
    for (int64_t j0 = (int64_t)blockIdx.x * WPB; j0 < n_long; j0 += (int64_t)gridDim.x * WPB) {
        const int64_t j = j0 + (threadIdx.x >> 6);
        const bool have = j < n_long;
        const int64_t row = have ? long_list[j] : 0;
        longlong2 r01 = make_longlong2(0, 0), r23 = r01, r45 = r01;
        if (have) {
            const longlong2 *src = reinterpret_cast<const longlong2 *>(table + row * 6);
            r01 = src[0]; r23 = src[1]; r45 = src[2];
        }
        bool is_long = false;
        trim_row<64, 16>(d, nbytes, s, add, table, out, row, have, r01, r23, r45, base, cf, cb, false, lane, 0, is_long, changed,
                         removed, skipped);
    }
    trim_add_counters(blk, changed, removed, skipped);
}

}  // namespace ffq

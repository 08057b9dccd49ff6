// ffq_deflate.h -- BGZF members deflated on the GPU: ffq_deflate_bgzf (include/ffq.h states the container, the bound and the
// match rule; ffq_tables.h has the launch sequence).
//
// d_src[0, n) is cut into blocks of DFL_BLOCK = 65280 bytes, what bgzip puts into a member, and every block becomes one gzip
// member: one BTYPE=2 block under two Huffman codes built from the block's own counts, or one stored block where that
// would be longer.  Members do not depend on one another, so a WORKGROUP TAKES A BLOCK, under a capped persistent grid.
//   k_deflate_members  a workgroup of 256 lanes per block: everything ffq_deflatewalk.h lists, in one kernel, the member
//                      built in LDS and copied into the block's own 64 KiB slot of the scratch; its size
//   launch_scan        exclusive scan of the sizes (ffq_scan.h)
//   k_deflate_pack     a workgroup per member: slot -> d_out, destination-aligned words; nothing if the total exceeds out_cap
// The pack costs the compressed bytes once more, and spares the blocks any knowledge of one another.
//
// LDS of k_deflate_members, one workgroup per CU:
//     the block's bytes                                   65280 + 16
//     the hash table, 2^14 entries of 32 bits             65536   (a maximum per entry needs a whole word: 1 + position)
//       ... and behind the walk the member's words        (the same 65536: a member is at most 65280 + 31 bytes)
//     counts, sorted symbols, work, codes, lengths of
//     the three alphabets; CRC table; x^(2^k); scan        ~6.6 KiB
//   about 137.5 of the 160 KiB a workgroup of gfx950 may declare.  What does NOT fit beside these is a record per position:
//   the candidate distances, then the lanes' tokens in their place (ffq_deflatewalk.h: dfl_walk), are 65280 words of global
//   scratch that belong to the WORKGROUP, not the block -- DEFLATE_GRID of them, whatever the input's size.
// The block's bytes stay 65280: the table is what the budget squeezes (2^14 entries where zlib's level 1 has 2^15), and
// halving the block to widen it would double the members' fixed cost.
//
// Determinism: lookups of a round see the inserts of earlier rounds only (a barrier on each side), an entry is a maximum,
// the counts are sums, the CRC an XOR, and a lane's bit offset a prefix sum: the same input gives the same bytes.
#pragma once
#include "ffq_deflatewalk.h"
#include "ffq_kernels.h"

namespace ffq {

constexpr int DEFLATE_GRID = 256;             // workgroups of k_deflate_members at most: one per CU (its LDS admits no second)
constexpr int DEFLATE_COUNTS = 4;             // FFQ_DEFLATE_COUNTS
constexpr int DFL_PAD = 320;                  // entries of the literal/length arrays (286 used), 32 for the other two

// counters of a call: members stored, the bytes of all members (written by the pack)
struct DeflateBlock { unsigned long long stored, total; };

struct DeflateLds {
    uint32_t lfreq[DFL_PAD], dfreq[32], cfreq[32];
    int32_t lwork[DFL_PAD], dwork[32], cwork[32];
    uint16_t lsorted[DFL_PAD], dsorted[32], csorted[32];
    uint16_t lcode[DFL_PAD], dcode[32], ccode[32];
    uint8_t llen[DFL_PAD], dlen[32], clen[32];
    uint32_t crc_tab[256], x2n[32];
    uint32_t wsum[DFL_LANES / 64];
    uint32_t crc;
    DflPlan pl;
};

// the member's words in LDS (DflBits, dfl_put_byte)
struct DeflateWords {
    uint32_t *w;
    __device__ __forceinline__ void plain(uint32_t i, uint32_t v) { w[i] = v; }
    __device__ __forceinline__ void shared(uint32_t i, uint32_t v) { atomicOr(&w[i], v); }
};

// slots: DFL_BLOCK words per workgroup; members: DFL_SLOT bytes per block; sizes: a word per block
__global__ __launch_bounds__(DFL_LANES) void k_deflate_members(const uint8_t *__restrict__ src, int64_t n_bytes, int64_t n_blocks,
                                                                uint32_t *__restrict__ slots, uint8_t *__restrict__ members,
                                                                long long *__restrict__ sizes, DeflateBlock *blk)
{
    __shared__ uint32_t s_blk[(DFL_BLOCK + 16) / 4];
    __shared__ uint32_t s_tab[DFL_SLOT / 4];
    __shared__ DeflateLds s;
    static_assert((1 << DFL_HASH_BITS) <= DFL_SLOT / 4 && DFL_ROUND % DFL_LANES == 0, "the table's words, a round's positions");
    const int tid = threadIdx.x;
    uint8_t *const b = reinterpret_cast<uint8_t *>(s_blk);
    uint32_t *const slot = slots + (size_t)blockIdx.x * DFL_BLOCK;
    s.crc_tab[tid] = dfl_crc_entry(tid);
    if (tid == 0) dfl_crc_x2n(s.x2n);
    for (int64_t bi = blockIdx.x; bi < n_blocks; bi += gridDim.x) {
        __syncthreads();                                   // (the block before is out of LDS)
        const int64_t base = bi * DFL_BLOCK;
        const int n = (int)(n_bytes - base < DFL_BLOCK ? n_bytes - base : DFL_BLOCK);
        const uint8_t *g = src + base;
        // ---- the block's bytes, a cleared table, cleared counts ----
        if ((reinterpret_cast<uintptr_t>(g) & 3) == 0) {
            const uint32_t *g4 = reinterpret_cast<const uint32_t *>(g);
            for (int i = tid; i < n / 4; i += DFL_LANES) s_blk[i] = __builtin_nontemporal_load(g4 + i);
            if (tid < (n & 3)) b[(n & ~3) + tid] = g[(n & ~3) + tid];
        } else {
            for (int i = tid; i < n; i += DFL_LANES) b[i] = g[i];
        }
        for (int i = tid; i < (1 << DFL_HASH_BITS); i += DFL_LANES) s_tab[i] = 0;
        for (int i = tid; i < DFL_PAD; i += DFL_LANES) s.lfreq[i] = i == DFL_EOB ? 1u : 0u;
        if (tid < 32) s.dfreq[tid] = s.cfreq[tid] = 0;
        if (tid == 0) s.crc = 0;
        __syncthreads();
        // ---- 1. candidates, in rounds: look up, barrier, enter, barrier ----
        for (int r0 = 0; r0 < n; r0 += DFL_ROUND) {
            uint32_t h[DFL_ROUND / DFL_LANES];
#pragma unroll
            for (int k = 0; k < DFL_ROUND / DFL_LANES; k++) {
                const int p = r0 + k * DFL_LANES + tid;
                h[k] = 0xFFFFFFFFu;
                if (p + 4 <= n) {
                    h[k] = dfl_hash(dfl_load4(b, p));
                    slot[p] = dfl_candidate(p, s_tab[h[k]]);
                } else if (p < n) {
                    slot[p] = 0;
                }
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < DFL_ROUND / DFL_LANES; k++)
                if (h[k] != 0xFFFFFFFFu) atomicMax(&s_tab[h[k]], (uint32_t)(r0 + k * DFL_LANES + tid) + 1u);
            __syncthreads();                               // (and the slots are the workgroup's to read: written and read on one CU)
        }
        // ---- 2. the walk; 3. counts; the lane's CRC ----
        const int nseg = (n + DFL_SEG - 1) / DFL_SEG;
        const int begin = tid * DFL_SEG, end = begin + DFL_SEG < n ? begin + DFL_SEG : n;
        int ntok = 0;
        if (tid < nseg) {
            ntok = dfl_walk(b, begin, end, slot);
            for (int k = 0; k < ntok; k++) {
                int ls, ds;
                dfl_token_syms(slot[begin + k], ls, ds);
                atomicAdd(&s.lfreq[ls], 1u);
                if (ds >= 0) atomicAdd(&s.dfreq[ds], 1u);
            }
            atomicXor(&s.crc, dfl_crc_shift(s.x2n, dfl_crc(s.crc_tab, b + begin, end - begin), (uint32_t)(n - end)));
        }
        __syncthreads();
        // ---- code lengths and codes: ranks by every lane, then a lane per alphabet ----
        dfl_rank_lane(s.lfreq, DFL_NLIT, tid, DFL_LANES, s.lsorted, s.lwork, s.llen);
        dfl_rank_lane(s.dfreq, DFL_NDIST, tid, DFL_LANES, s.dsorted, s.dwork, s.dlen);
        __syncthreads();
        if (tid == 0) {
            dfl_lengths(s.lfreq, DFL_NLIT, DFL_LIT_BITS, true, s.lsorted, s.lwork, s.llen);
            dfl_codes(s.llen, DFL_NLIT, s.lcode);
        }
        if (tid == 64) {
            dfl_lengths(s.dfreq, DFL_NDIST, DFL_LIT_BITS, false, s.dsorted, s.dwork, s.dlen);
            dfl_codes(s.dlen, DFL_NDIST, s.dcode);
        }
        __syncthreads();
        // ---- 4. the header's own code ----
        if (tid == 0) dfl_header_counts(s.llen, s.dlen, s.pl);
        __syncthreads();
        {
            const int hlit = s.pl.hlit, hdist = s.pl.hdist;
            for (int i = tid; i < hlit + hdist; i += DFL_LANES) atomicAdd(&s.cfreq[i < hlit ? s.llen[i] : s.dlen[i - hlit]], 1u);
        }
        __syncthreads();
        dfl_rank_lane(s.cfreq, DFL_NCL, tid, DFL_LANES, s.csorted, s.cwork, s.clen);
        __syncthreads();
        if (tid == 0) {
            dfl_lengths(s.cfreq, DFL_NCL, DFL_CL_BITS, true, s.csorted, s.cwork, s.clen);
            dfl_codes(s.clen, DFL_NCL, s.ccode);
            dfl_header_plan(s.cfreq, s.clen, s.pl);
        }
        __syncthreads();
        // ---- 5. sizes ----
        uint32_t bits = 0;
        if (tid < nseg) {
            for (int k = 0; k < ntok; k++) bits += (uint32_t)dfl_token_bits(slot[begin + k], s.llen, s.dlen);
            if (tid == nseg - 1) bits += s.llen[DFL_EOB];
        }
        uint32_t body_bits;
        // (the words are handed in: the kernel has no LDS to spare; the barriers around this step are its own)
        const uint32_t at = wg_excl_scan<DFL_LANES, SCAN_ANY>(bits, body_bits, s.wsum);
        const int head_bits = s.pl.head_bits;
        const int64_t stream_bits = (int64_t)head_bits + body_bits;
        const bool stored = dfl_stored(stream_bits, n);
        const int member_bytes = dfl_member_bytes(stored ? n + DFL_STORED_HEAD : (int)((stream_bits + 7) / 8));
        const int member_words = (member_bytes + 3) / 4;   // (at most DFL_SLOT / 4: a member is at most n + DFL_OVERHEAD bytes)
        for (int i = tid; i < member_words; i += DFL_LANES) s_tab[i] = 0;
        __syncthreads();
        // ---- 6. the member, in the words the table had ----
        DeflateWords w{s_tab};
        if (stored) {
            if (tid == 0) dfl_put_stored_head(w, n);
            for (int i = tid; i < n; i += DFL_LANES) dfl_put_byte(w, DFL_HEAD + DFL_STORED_HEAD + i, b[i]);
        } else {
            if (tid == 0) {
                DflBits<DeflateWords> o(w, 8 * DFL_HEAD);
                dfl_put_header(o, s.pl, s.llen, s.dlen, s.ccode, s.clen);
                o.finish();
            }
            if (tid < nseg) {
                DflBits<DeflateWords> o(w, (int64_t)(8 * DFL_HEAD + head_bits) + at);
                for (int k = 0; k < ntok; k++) dfl_put_token(o, slot[begin + k], s.lcode, s.llen, s.dcode, s.dlen);
                if (tid == nseg - 1) o.put(s.lcode[DFL_EOB], s.llen[DFL_EOB]);
                o.finish();
            }
        }
        if (tid == DFL_LANES - 1) dfl_put_frame(w, member_bytes, s.crc, n);
        __syncthreads();
        uint32_t *dst = reinterpret_cast<uint32_t *>(members + bi * DFL_SLOT);
        for (int i = tid; i < member_words; i += DFL_LANES) dst[i] = s_tab[i];
        if (tid == 0) {
            sizes[bi] = member_bytes;
            if (stored) atomicAdd(&blk->stored, 1ull);
        }
    }
}

// off: the scanned sizes; res->n_qual_bytes: their total.  A workgroup per member, striding.  d_off: NULL, or n_blocks + 1 words.
__global__ __launch_bounds__(256) void k_deflate_pack(const uint8_t *__restrict__ members, const long long *__restrict__ off,
                                                       int64_t n_blocks, const DevRes *__restrict__ res, uint8_t *__restrict__ out,
                                                       int64_t out_cap, int64_t *__restrict__ d_off, DeflateBlock *blk)
{
    const int64_t total = res->n_qual_bytes;
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && tid == 0) blk->total = (unsigned long long)total;
    for (int64_t m = blockIdx.x; m < n_blocks; m += gridDim.x) {
        const int64_t o = off[m];
        const int size = (int)((m + 1 < n_blocks ? off[m + 1] : total) - o);
        if (d_off && tid == 0) {
            d_off[m] = o;
            if (m == n_blocks - 1) d_off[n_blocks] = total;
        }
        if (total > out_cap) continue;
        const uint8_t *sb = members + m * DFL_SLOT;
        const uint32_t *sw = reinterpret_cast<const uint32_t *>(sb);
        uint8_t *dst = out + o;
        int head = (int)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3);
        if (head > size) head = size;
        const int nw = (size - head) / 4, tail = size - head - 4 * nw;
        if (tid < head) dst[tid] = sb[tid];
        if (tid < tail) dst[head + 4 * nw + tid] = sb[head + 4 * nw + tid];
        uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head);
        const int sh = 8 * head;                           // (the slot is word-aligned: every source word is shifted alike)
        for (int i = tid; i < nw; i += 256) {
            // bytes head + 4i .. head + 4i + 3 of the slot: inside words i and i + 1, and i + 1 <= (size - 1) / 4 when head > 0
            const uint32_t w0 = sw[i];
            dw[i] = sh ? (w0 >> sh) | (sw[i + 1] << (32 - sh)) : w0;
        }
    }
}

}  // namespace ffq

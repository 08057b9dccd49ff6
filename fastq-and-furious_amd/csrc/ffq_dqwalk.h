// ffq_dqwalk.h -- the integer control flow of k_decode_stream's window walk (csrc/ffq_kernels.h), as inline functions
// that compile for the host too: the kernel calls them, and tests/dq_windows_host.cpp drives the same walk on a CPU over
// offset arrays no scan would produce in a test's time (thousands of empty records in a row).
//
// The output stream is cut into blocks of DQ_BLK bytes (one workgroup each) and those into 16-byte chunks aligned on the
// DESTINATION address: with shiftA = (address of the block's first byte) & 15, chunk k covers the block-relative bytes
// [16 k - shiftA, +16) cut to [0, oe).  A workgroup walks its block in WINDOWS: (offset, source) of the records
// rbase .. rbase + nrec go to LDS, and the window writes every chunk that lies wholly below cend = the offset of record
// rbase + nrec -- every record with a byte under such a chunk is cached.
//
// Termination.  The state is (rbase, done, want); chunks [0, done) are written.  One turn of the loop ends in one of
// three ways:
//   (a) the window covers a whole chunk: klim > done, and done := klim;
//   (b) it covers none and was sized from the mean length: the same base again at full size (want := -1);
//   (c) it covers none at full size -- more than DQ_REC - 2 EMPTY records lie under chunk `done`, no window of DQ_REC - 1
//       consecutive records reaches from the record under its first byte to the one under its last --: that one chunk is
//       written byte by byte from global memory (a search over qoff per byte), done := done + 1, and the next base is
//       searched in global memory, which skips the empty records however many there are.
// (b) is followed by (a) or (c), so `done` grows at least every second turn: at most 2 nchunk turns per block.
// Before (c) existed, (b) followed (b) for ever.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DQ_HD __host__ __device__ __forceinline__
#else
#define DQ_HD inline
#endif

namespace ffq {

constexpr int DQ_SHIFT = 16;
constexpr int DQ_BLK = 1 << DQ_SHIFT;             // output bytes per workgroup
constexpr int DQ_REC = 1024;                      // records cached in LDS per window (DQ_REC - 1, and the end of the last)

// Directory of the decoded-quality stream: qdir[b] = the record whose decoded bytes cover
// stream offset b << DQ_SHIFT.  Record r with bytes [q, q + len) owns every such boundary
// inside its range, so each entry below the stream's end has exactly one writer.
DQ_HD void qdir_mark(int64_t *__restrict__ qdir, int64_t qdir_cap, int64_t q, int64_t len, int64_t r)
{
    for (int64_t b = (q + (1 << DQ_SHIFT) - 1) >> DQ_SHIFT; (b << DQ_SHIFT) < q + len && b < qdir_cap; b++)
        qdir[b] = r;
}

DQ_HD int dq_imin(int a, int b) { return a < b ? a : b; }
DQ_HD int dq_imax(int a, int b) { return a > b ? a : b; }

// mean component length: what a window is sized from
DQ_HD int dq_mean(int64_t qtotal, int64_t n)
{
    const int64_t m = qtotal / n;
    return (int)(m < 1 ? 1 : (m > ((int64_t)1 << 20) ? (int64_t)1 << 20 : m));
}

// chunks of a block of oe bytes; a destination that is not 16-byte aligned has one more (partial) chunk at the end
DQ_HD int dq_nchunk(int oe, int shiftA) { return (oe + shiftA + 15) >> 4; }

// first block-relative byte of chunk k (clo < 0: the chunk begins in front of the block)
DQ_HD int dq_clo(int k, int shiftA) { return 16 * k - shiftA; }

// stream offset of a record relative to the block, as the window caches it
DQ_HD int32_t dq_rel(int64_t qraw, int64_t ob)
{
    const int64_t q = qraw - ob;
    return (int32_t)(q < -0x7FFFFFFF ? (int64_t)-0x7FFFFFFF : (q > 0x7FFFFFFF ? (int64_t)0x7FFFFFFF : q));
}

// records the next window asks for: sized from the mean length; want < 0 asks for the full size
DQ_HD int dq_window_want(int want, int done, int oe, int shiftA, int mean)
{
    const int rem = oe - dq_imax(dq_clo(done, shiftA), 0);
    return (want < 0) ? DQ_REC - 1 : dq_imin(DQ_REC - 1, rem / mean + rem / (8 * mean) + 8);
}

DQ_HD int dq_window_nrec(int want, int64_t n, int64_t rbase)
{
    const int64_t left = n - rbase;               // >= 1
    return (int)((int64_t)want < left ? (int64_t)want : left);
}

// chunks [done, klim) are the window's: those wholly below cend -- all of them if the window reaches the end of the table
// or of the block
DQ_HD int dq_klim(int64_t rbase, int nrec, int64_t n, int cend, int oe, int shiftA, int nchunk)
{
    return (rbase + nrec == n || cend >= oe) ? nchunk : dq_imin(nchunk, (cend + shiftA) >> 4);
}

// largest cached index i in [a, b] with s_q[i] <= v (s_q[a] <= v)
template <class SQ>
DQ_HD int dq_search(SQ s_q, int a, int b, int v)
{
    while (b > a) {
        const int m = (a + b + 1) >> 1;
        if (s_q[m] <= v) a = m; else b = m - 1;
    }
    return a;
}

// the cached record under byte vlo of a chunk of the window: largest index a with s_q[a] <= vlo (it is below nrec);
// equal-length records make the interpolated guess exact
template <class SQ>
DQ_HD int dq_chunk_record(SQ s_q, int nrec, int vlo, float inv_mean)
{
    int a = 0, b = nrec - 1;
    const int g = dq_imin(dq_imax((int)((float)(vlo - s_q[0]) * inv_mean), 0), nrec - 1);
    if (s_q[g] <= vlo) { a = g; if (s_q[g + 1] > vlo) b = g; } else b = g - 1;
    return dq_search(s_q, a, b, vlo);
}

// largest record r in [lo, hi] with qoff[r] <= x (qoff[lo] <= x; qoff does not decrease): with qoff[hi + 1] > x it is
// the record that holds stream byte x, and no empty record
DQ_HD int64_t dq_find_record(const int64_t *__restrict__ qoff, int64_t lo, int64_t hi, int64_t x)
{
    while (hi > lo) {
        const int64_t m = lo + ((hi - lo + 1) >> 1);
        if (qoff[m] <= x) lo = m; else hi = m - 1;
    }
    return lo;
}

struct DqWalk {
    int64_t rbase;                                // first record of the window
    int done;                                     // chunks [0, done) are written
    int want;                                     // 0: size the window from the mean; -1: full size
};

constexpr int DQ_NEXT_WINDOW = 0, DQ_NEXT_SLOW = 1;

// After a window that did not finish the block (klim < nchunk).  DQ_NEXT_WINDOW: go on with the window the state
// describes.  DQ_NEXT_SLOW: not even a full window covers chunk `done` -- the caller writes it from global memory and
// calls dq_after_slow.  Reads s_q: call it before the cache is rewritten.
template <class SQ>
DQ_HD int dq_next(DqWalk &w, SQ s_q, int nrec, int klim, int shiftA)
{
    if (klim > w.done) {
        // the next window starts at the record under the first byte of chunk klim (> 0 and < cend)
        w.rbase += dq_search(s_q, 0, nrec - 1, dq_clo(klim, shiftA));
        w.done = klim;
        w.want = 0;
        return DQ_NEXT_WINDOW;
    }
    if (w.want >= 0) { w.want = -1; return DQ_NEXT_WINDOW; }      // no whole chunk covered: full-size window, same base
    return DQ_NEXT_SLOW;
}

// chunk `done` was written from global memory: true if it was the block's last; otherwise the next window starts at the
// record under the first byte of the next chunk, found in qoff itself
DQ_HD bool dq_after_slow(DqWalk &w, const int64_t *__restrict__ qoff, int64_t n, int64_t ob, int shiftA, int nchunk)
{
    w.done += 1;
    w.want = 0;
    if (w.done >= nchunk) return true;
    w.rbase = dq_find_record(qoff, w.rbase, n - 1, ob + dq_clo(w.done, shiftA));
    return false;
}

}  // namespace ffq

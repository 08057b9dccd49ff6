// ffq_umi_launch.h -- the boundary between the library's two translation units: ffq_hip.hip (everything else; the host side of the
// UMI calls is in ffq_tables.h) and ffq_umi.hip (the kernels of ffq_umi.h, which says why they are built apart).  Plain types and
// plain functions: no kernel and no template crosses it, and the counter blocks and the scan's result go over as untyped device
// pointers.  The grids are the caller's; a function enqueues its launches on `st` and returns.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ffq_umi {

constexpr int TAKE_WG = 256, RENDER_WG = 256;             // threads of a workgroup of the take's and of the render's kernels

// a buffer and a table over it, as the kernels take them (PairSide of ffq_pair.h)
struct Side { const uint8_t *d; int64_t nbytes; int s; int64_t add; const int64_t *table; };
// the rule: FFQ_UMI_* location, bases of the tag, bytes of the prefix; the literal (delim, prefix, '_') as five little-endian dwords
struct Arg { int loc, len, prefix_len; uint32_t lit[5]; };
// counters of a render call: RenderBlock's (output bytes, rows rendered, rows on the long list) and the rows that got a tag
struct RenderCounts { unsigned long long total, rendered, n_long, tagged; };

// k_umi_take and k_umi_take_long; d_rows_blk: the call's RowsBlock on the device
void launch_take(hipStream_t st, unsigned grid_short, unsigned grid_long, const uint8_t *d_buf, int64_t n_bytes, int s, int64_t add,
                 const int64_t *d_table, int64_t n_rows, int len, int skip, int64_t *d_out, int64_t *d_long_list, void *d_rows_blk);
// k_umi_render_sum: the rendered bytes of every block of RENDER_WG rows into d_bsum
void launch_render_sum(hipStream_t st, unsigned grid, const Side &rows, const Side &src1, const Side &src2, const Arg &arg, int64_t n_rows,
                       int64_t nblk, long long *d_bsum, RenderCounts *d_blk);
// k_umi_render_rows and k_umi_render_long, behind the scan of d_bsum into d_bbase; d_res: the scan's DevRes (its total)
void launch_render_rows(hipStream_t st, unsigned grid_rows, unsigned grid_long, const Side &rows, const Side &src1, const Side &src2,
                        const Arg &arg, int64_t n_rows, const long long *d_bbase, const void *d_res, uint8_t *d_out, int64_t out_cap,
                        int64_t *d_off, int64_t *d_long_list, RenderCounts *d_blk);

}  // namespace ffq_umi

// ffq_umi.hip -- the second translation unit of libffq_hip.so: the kernels of csrc/ffq_umi.h (the UMI take and the tagged render)
// and the plain functions that launch them (csrc/ffq_umi_launch.h).  ffq_umi.h says why they are not part of ffq_hip.hip: built in
// there, they changed the code of the plain render's kernels.
//
// The device headers come in through an unnamed namespace: everything they define has internal linkage here, so no symbol of
// this file meets one of ffq_hip.hip, on the host or in the code object.  The kernel templates of those headers, which this file
// never launches, are not instantiated; their plain kernels (ffq_kernels.h, ffq_render.h, ...) are emitted once more, dead -- about
// 0.3 MB of the library.  The system headers they include are included first, outside.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ffq_umi_launch.h"

namespace {
#include "ffq_umi.h"
}

namespace ffq_umi {

void launch_take(hipStream_t st, unsigned grid_short, unsigned grid_long, const uint8_t *d_buf, int64_t n_bytes, int s, int64_t add,
                 const int64_t *d_table, int64_t n_rows, int len, int skip, int64_t *d_out, int64_t *d_long_list, void *d_rows_blk)
{
    ffq::RowsBlock *blk = static_cast<ffq::RowsBlock *>(d_rows_blk);
    hipLaunchKernelGGL(ffq::k_umi_take, dim3(grid_short), dim3(ffq::UMI_WG), 0, st, d_buf, n_bytes, s, add, d_table, n_rows, len, skip, d_out,
                       d_long_list, blk);
    hipLaunchKernelGGL(ffq::k_umi_take_long, dim3(grid_long), dim3(ffq::UMI_WG), 0, st, d_buf, n_bytes, s, add, d_table, len, skip, d_out,
                       (const int64_t *)d_long_list, blk);
}

void launch_render_sum(hipStream_t st, unsigned grid, const Side &rows, const Side &src1, const Side &src2, const Arg &arg, int64_t n_rows,
                       int64_t nblk, long long *d_bsum, RenderCounts *d_blk)
{
    hipLaunchKernelGGL(ffq::k_umi_render_sum, dim3(grid), dim3(ffq::RENDER_WG), 0, st, rows, src1, src2, arg, n_rows, nblk, d_bsum, d_blk);
}

void launch_render_rows(hipStream_t st, unsigned grid_rows, unsigned grid_long, const Side &rows, const Side &src1, const Side &src2,
                        const Arg &arg, int64_t n_rows, const long long *d_bbase, const void *d_res, uint8_t *d_out, int64_t out_cap,
                        int64_t *d_off, int64_t *d_long_list, RenderCounts *d_blk)
{
    hipLaunchKernelGGL(ffq::k_umi_render_rows, dim3(grid_rows), dim3(ffq::RENDER_WG), 0, st, rows, src1, src2, arg, n_rows, d_bbase,
                       static_cast<const ffq::DevRes *>(d_res), d_out, out_cap, d_off, d_long_list, d_blk);
    // the rows it left (above RENDER_LONG output bytes; their number is known on the device only): a wave each
    hipLaunchKernelGGL(ffq::k_umi_render_long, dim3(grid_long), dim3(ffq::RENDER_WG), 0, st, rows, src1, src2, arg, n_rows, d_out,
                       (const int64_t *)d_long_list, (const RenderCounts *)d_blk);
}

}  // namespace ffq_umi

/*
 * voxproj_cluster.h -- label sums over a feature table in libvoxproj.so: the per-label sum of rows that a Lloyd iteration,
 * mask pooling and class prototypes share, and the row norms a cosine metric needs (the reference clusters on the CPU with
 * sklearn.cluster.KMeans on the raw rows: script/debug_checks_scripts/voxel_cluster_to_ply.py).  Same library, same vp_
 * prefix, same error codes and vp_last_error(); VP_ABI_VERSION does not change, a caller detects these functions by symbol.
 * voxproj.h, voxproj_ext.h, voxproj_mesh.h and voxproj_grid.h stay as they are.
 */
#ifndef VOXPROJ_CLUSTER_H
#define VOXPROJ_CLUSTER_H

#include "voxproj.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Rows: `rows` points at n_rows rows of C channels, binary16 when rows_f16 = 1 and float32 when 0, channel stride 1, row
 * stride `stride` ELEMENTS (>= C).  1 <= C <= 4096, 0 <= n_rows < 2^31.  16-byte loads are used where C is a multiple of
 * the 8 (binary16) or 4 (float32) channels they hold and the base and the row stride are multiples of 16 bytes; element
 * loads otherwise.  The results do not depend on which.
 *
 * vp_row_inv_norms: inv[r] = (float)(1 / max(sqrt(sum_c (double)x[r,c]^2), 1e-12)), the sum in float64 (every order of it is
 * within an ulp of float32 after the rounding).  A row that is all zeros gets 0 and is counted in status[0]; a row with a
 * non-finite element gets 0 and is counted in status[1].  inv f32 [n_rows], status i32 [2] (zeroed by the call, then counted
 * with integer adds).  One wavefront per row, four rows per wavefront where a quarter of one covers a row.
 *
 * vp_label_sums, the contract (tests/label_sums_reference.py states it in NumPy; sums and counts equal that twin's byte for
 * byte):
 *
 *   a[r,c]      = fl32( fl32(x[r,c]) * s_r )                   one rounding; binary16 -> f32 is exact; s_r = row_scale[r], or
 *                                                              1 when row_scale is NULL
 *   part(k, p)  = the rows of label k in ascending row index, positions [p R, min((p + 1) R, n_k))
 *   partial     = (((+0 + a[r0,c]) + a[r1,c]) + a[r2,c]) + ... float32, in that order, the product never contracted into
 *                                                              the sum
 *   sums[k,c]   = fl32( +0 + the float64 sum of the label's partials in ascending p )
 *   R           = part_rows, or max(256, ceil(n_rows / 32768)) when part_rows = 0
 *
 * A channel never crosses lanes: a row's channels are spread over the wavefront, 16 bytes per lane, and a lane only ever
 * adds to its own accumulators.  labels i32 [n_rows]: a row with label < 0 is ignored and counted in status[0], a row with
 * label >= K is left out as well and counted in status[1] (status i32 [2], zeroed by the call).  sums f32 [K, C] and
 * counts i32 [K] are written whole: a label without rows gets a zero row and count 0.  1 <= K <= 65536.
 *
 * The stages, all on `stream` and inside `workspace`: keys (the label, or K for a row left out) and a stable
 * rocprim::radix_sort_pairs of (key, row index) over the bits K needs; each label's run by binary search and its number of
 * parts; an exclusive scan that gives every part its slot; a fixed grid of one wavefront per part (at most
 * n_rows / R + min(K, n_rows) of them) that finds its (k, p) in the scanned table, streams its rows four at a time and
 * writes one partial row; one wavefront per label and 64 channels that adds the label's partials in order.  No float
 * atomics, no scratch memory, no allocation, no host synchronisation; the results are bit-identical from run to run.
 *
 * vp_label_sums_workspace_bytes(n_rows, K, C) is the size for part_rows = 0 (0 for arguments out of range, or when the
 * device cannot be asked for the sort's scratch size).  The partial rows are the workspace's last section, so a part_rows
 * below the default R needs (min(n_rows, n_rows / part_rows + min(K, n_rows)) - min(n_rows, n_rows / R + min(K, n_rows)))
 * * C * 4 bytes more, rounded up to 256.
 *
 * VP_EINVAL / VP_EWORKSPACE, decided on the host before any launch: a NULL array the call reads or writes (row_scale may be
 * NULL; rows, labels and inv only when n_rows = 0), rows_f16 that is neither 0 nor 1, n_rows, C, K outside their ranges,
 * stride < C, part_rows < 0, a workspace that is NULL, not 256-byte aligned or too small.
 */
int vp_row_inv_norms(const void *rows, int rows_f16, int64_t n_rows, int C, int64_t stride, float *inv, int32_t *status,
                     void *stream);
size_t vp_label_sums_workspace_bytes(int64_t n_rows, int K, int C);
int vp_label_sums(const void *rows, int rows_f16, int64_t n_rows, int C, int64_t stride, const int32_t *labels,
                  const float *row_scale, int K, int64_t part_rows, float *sums, int32_t *counts, int32_t *status,
                  void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VOXPROJ_CLUSTER_H */

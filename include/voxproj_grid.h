/*
 * voxproj_grid.h -- stage 2 of the pipeline in libvoxproj.so: the sparse voxel grid of a Gaussian cloud (the reference builds
 * it on the CPU, script/minkowski_voxel_grid_from_ply_advanced.py: cKDTree.query_ball_point in Python loops, np.unique and a
 * per-voxel mask loop).  Same library, same vp_ prefix, same error codes and vp_last_error(); VP_ABI_VERSION does not change,
 * a caller detects these functions by symbol.  voxproj.h, voxproj_ext.h and voxproj_mesh.h stay as they are.
 */
#ifndef VOXPROJ_GRID_H
#define VOXPROJ_GRID_H

#include "voxproj.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The contract (tests/voxel_grid_reference.py states it in NumPy; the GPU results equal that twin's value for value).
 *
 *   Columns        as stored in the ply: x y z f32, opacity (the logit), scale_0..2 (the logs), nx ny nz when present,
 *                  f_dc_0..2.  Colour of a Gaussian: uint8(clip(f_dc_c, 0, 1) * 255) in float32, truncating.
 *   Spikiness      scales below 1e-6 become 1e-6; a Gaussian is kept when max / min < spikiness_threshold, in float32.
 *   Opacity rank   N_keep = max(1, int(N (1 - opacity_threshold))) largest opacities; ties at the cut go to the lowest index.
 *   Ball statistics (vp_ball_count), per query i over the current point set:
 *                  d2 = (dx dx + dy dy) + dz dz in float64 on the float64-converted fp32 differences q - p, no contraction;
 *                  a point is within the ball iff d2 <= r r, r = radius or (double)radii[i]; the query itself counts when it
 *                  is a point of the set, boundary points count.  With normals (unit, n / (|n| + 1e-8) formed by the caller
 *                  in float32): dot = (nx mx + ny my) + nz mz in float64, `consistent` counts the points within the ball
 *                  whose dot > min_dot.  Outputs count i32 [M], consistent i32 [M].
 *   Filters        in the reference's order, the point set bucketed again from the survivors before each:
 *                  normal consistency (only with normals and normal_consistency < 1): keep iff count >= min_neighbors and
 *                  consistent >= min_neighbors at radius normal_consistency_eps; density: keep iff count >
 *                  density_min_neighbors at radius density_eps, or, adaptive, at the per-point radius
 *                  clip(|mean of the three scale columns|, eps / 2, 2 eps), mean and clip in float32.
 *   Voxelisation   (vp_voxel_grid) min_corner = the float32 minimum of the kept points per axis;
 *                  idx = floor((p - min_corner) / (float)voxel_size) in float32, correctly rounded; the unique cells in
 *                  lexicographic (x, y, z) order; centre = (float)((double)idx voxel_size + (double)min_corner);
 *                  colour per channel = (uint8)(float)((double)(sum of the colours) / (double)count): the sum is an integer,
 *                  so the result does not depend on the order of the points.
 *
 * vp_ball_count takes the point set bucketed on a uniform grid exactly as vp_knn_points takes it: pts_sorted f32 [N,3] in
 * cell order, perm i32 [N] (sorted row t is the caller's point perm[t]), cell_start i32 [nx ny nz + 1], the grid's origin (3
 * doubles in HOST memory), cell size and dims.  queries f32 [M,3] in any order (cell order is fastest: the lanes of a
 * wavefront then walk the same cells).  radii f32 [M] or NULL (then `radius` holds for every query; with radii it is not
 * used).  point_normals f32 [N,3] in the CALLER's order (read through perm) and query_normals f32 [M,3]: both or neither;
 * `consistent` is written only with normals and may be NULL without.  Every cell whose box can touch the ball is visited
 * (the box is padded by a cell, so no rounding of the cell arithmetic can lose a point) and every candidate takes the
 * exact test; any cell size is correct, one no smaller than the largest radius keeps the box at 3 x 3 x 3 cells.  A query or
 * radius that is NaN counts nothing.
 *
 * vp_voxel_grid: points f32 [N,3], colors u8 [N,3], keep u8 [N] or NULL (all kept).  Outputs, each with room for N rows,
 * rows [0, V) written: centers f32 [.,3], voxel_colors u8 [.,3], counts i32 [.], voxel_index i32 [.,3]; point_voxel i32 [N]
 * (-1 for a point not kept); n_voxels i32 [1], min_corner f32 [3] (+inf when nothing is kept) and status i32 [1] on the
 * device (status may be NULL).  The cell key holds 21 bits per axis: when a cell index is above 2^21 - 1 or a kept point is
 * not finite, *status = 1, *n_voxels = 0 and nothing else is written; otherwise *status = 0.  The stages: a min reduction,
 * keys, a stable rocprim::radix_sort_pairs of (key, point index), run heads and their scan, one pass per voxel and one per
 * point, all inside `workspace`.
 *
 * Both calls: no float atomics, integer results bit-identical from run to run, no allocation, no host synchronisation,
 * asynchronous on `stream`.  N = 0 and M = 0 are valid.  VP_EINVAL / VP_EWORKSPACE, decided on the host before any launch: a
 * NULL array the call reads or writes, counts outside [0, 2^31 - 1], a bad grid, a radius (without radii) that is negative
 * or not finite, a min_dot that is NaN, normals for only one side, voxel_size <= 0 or not finite, a workspace that is NULL,
 * not 256-byte aligned or smaller than vp_voxel_grid_workspace_bytes(N) (0 for N out of range).
 */
int vp_ball_count(const float *pts_sorted, const int32_t *perm, const int32_t *cell_start, const double *grid_origin3,
                  double cell_size, int nx, int ny, int nz, const float *queries, int64_t M, double radius, const float *radii,
                  const float *point_normals, const float *query_normals, double min_dot, int32_t *count,
                  int32_t *consistent, void *stream);
size_t vp_voxel_grid_workspace_bytes(int64_t N);
int vp_voxel_grid(const float *points, const uint8_t *colors, const uint8_t *keep, int64_t N, double voxel_size,
                  float *centers, uint8_t *voxel_colors, int32_t *counts, int32_t *voxel_index, int32_t *point_voxel,
                  int32_t *n_voxels, float *min_corner, int32_t *status, void *workspace, size_t workspace_bytes,
                  void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VOXPROJ_GRID_H */

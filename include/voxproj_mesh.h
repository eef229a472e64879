/*
 * voxproj_mesh.h -- the triangle-mesh rasterizer of libvoxproj.so: ground-truth label maps, face-id maps and depth maps of
 * an annotated mesh through one pinhole camera (the reference renders them off-screen with Open3D,
 * debug_checks_scripts/render_scannetpp.py; its depth counterpart is generate_pseudo_depth_maps.py).  Same library, same vp_
 * prefix, same error codes and vp_last_error(); VP_ABI_VERSION does not change, a caller detects these functions by symbol.
 * voxproj.h and voxproj_ext.h stay as they are.
 */
#ifndef VOXPROJ_MESH_H
#define VOXPROJ_MESH_H

#include "voxproj.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The contract (tests/mesh_reference.py states it in NumPy; the GPU maps equal that twin's bit for bit).  The camera and the
 * pixel centres are the splatter's (vp_splat_project): viewmat is the world-to-camera matrix, f32 [4,4] row-major in HOST
 * memory, pixel (j, i) samples the image point (j + 0.5, i + 0.5).  All float arithmetic is float64 on the fp32 inputs,
 * without contraction, with correctly rounded division, in the order written.
 *
 *   Camera space   c[k] = ((R[k][0] x + R[k][1] y) + R[k][2] z) + t[k] per vertex.
 *   Near clip      a vertex is inside when c.z >= near.  A face without an inside vertex is skipped.  Otherwise the polygon
 *                  v0 v1 v2 is clipped (Sutherland-Hodgman: per edge a -> b, a is kept when inside, and a crossing adds the
 *                  point q = s + tt (e - s), tt = (near - s.z) / (e.z - s.z), q.z = near, always from the inside end s to the
 *                  outside end e, so two faces that share the edge get the same point).  The 3 or 4 points p0.. are fanned
 *                  into the sub-triangles (p0 p1 p2) and (p0 p2 p3) of the same face.
 *   Snap           X = floor((fx (x / z) + cx) 256 + 0.5), Y likewise: 1/256 pixel units.  A face with a snapped coordinate
 *                  that is not finite or beyond +-2^29 is dropped whole.
 *   Coverage       area = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) in int64: 0 skips the sub-triangle, a negative one swaps
 *                  its last two points (both sides of a face are drawn).  With P = (256 j + 128, 256 i + 128) and, per edge
 *                  a -> b, (dx, dy) = b - a and E = dx (P.y - a.y) - dy (P.x - a.x) in int64, the sample is covered when
 *                  every edge has E > 0, or E == 0 and (dy < 0, or dy == 0 and dx > 0): of two faces on opposite sides of a
 *                  shared edge exactly one takes a sample on it.
 *   Depth          from the unclipped face: n = (c1 - c0) x (c2 - c0), d = (n.x c0.x + n.y c0.y) + n.z c0.z,
 *                  den = (n.x ((j + 0.5 - cx) / fx) + n.y ((i + 0.5 - cy) / fy)) + n.z, z = d / den; a NaN drops the sample,
 *                  else z is clamped to [min c.z, max c.z] of the three vertices and kept when near <= z <= far;
 *                  depth = (float)z.
 *   Winner         the smallest fp32 depth; ties go to the lowest face index.
 *   Outputs        face_ids i32 [H,W] (-1 where nothing is drawn), depth f32 [H,W] (0 there), labels u8 [H,W] (255 there).
 *                  The label of a face is the majority of its three vertex labels, the smallest when all three differ.
 *   Dropped faces  a vertex index outside [0, n_verts) (no vertex is read through it), a non-finite vertex, a snapped
 *                  coordinate beyond the guard band: counters i32 [3] on the device, in that order, each += its count
 *                  (not reset by the call; may be NULL).
 *
 * vp_mesh_project sets up every face once into `workspace` (records, 16 x 16 tile boxes, the scan of the tile counts) and
 * leaves the number of (tile, face) pairs in the workspace and, when not NULL, in the device int64 *n_isect.
 * vp_mesh_rasterize, on the workspace vp_mesh_project filled with the same n_faces, W and H: emits the pairs in face order,
 * sorts them stably by tile (rocprim::radix_sort_pairs), finds the tile runs and runs one 256-thread workgroup per tile, one
 * pixel per thread.  `capacity` sizes the sort: when the pair count exceeds it, no output is written and *status (device
 * i32, may be NULL) is set to 1.  Each of face_ids, depth, labels may be NULL; labels needs vertex_labels (u8 [n_verts]) and
 * the faces array (i32 [n_faces,3]) of the projection.
 *
 * Both calls: no atomics, bit-identical from run to run, no allocation, no host synchronisation, asynchronous on `stream`.
 * n_faces = 0 is valid and fills the outputs with "nothing drawn".  VP_EINVAL / VP_EWORKSPACE, decided on the host before
 * any launch: counts outside [0, 2^31 - 1], W or H outside [1, 32768], a NULL array the call reads, labels without
 * vertex_labels or faces (n_faces > 0), a NULL or non-finite viewmat, fx or fy <= 0, near <= 0, far <= near, a workspace
 * that is NULL, not 256-byte aligned or smaller than vp_mesh_workspace_bytes(n_faces, W, H, capacity) (0 for arguments out of range;
 * vp_mesh_project needs the size at capacity 0, which the larger layouts keep in place).
 */
size_t vp_mesh_workspace_bytes(int64_t n_faces, int W, int H, int64_t capacity);
int vp_mesh_project(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *viewmat,
                    float fx, float fy, float cx, float cy, int W, int H, float near_plane, float far_plane,
                    int64_t *n_isect, int32_t *counters, void *workspace, size_t workspace_bytes, void *stream);
int vp_mesh_rasterize(const uint8_t *vertex_labels, const int32_t *faces, int64_t n_faces, int W, int H, int64_t capacity,
                      int32_t *face_ids, float *depth, uint8_t *labels, int32_t *status, void *workspace,
                      size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VOXPROJ_MESH_H */

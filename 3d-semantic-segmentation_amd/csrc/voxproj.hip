// voxproj.hip -- MI355X (gfx950) 2D -> sparse-voxel feature projector: C-ABI and launch plumbing (kernels in vp_*.h).
//
// Replaces the device path of the reference's project_features_cuda extension
// (cuda_project_image_to_sparse_voxel/project_image_cuda_kernel.cu:24-92,140-334,374-459) with a
// two-phase design written for CDNA4:
//
//   phase 1  k_first_hit   one lane per (pixel, view): the reference's ray-march replayed in the
//                          exact fp32 operation order of oracle/projector_oracle.c (no FMA
//                          contraction, IEEE divide/sqrt, t += inc) -> first-hit voxel ID image and a
//                          per-call integer hit histogram.  Pixel -> voxel assignment is bit-exact.
//   phase 2  k_gather      one 64-lane wavefront per voxel: project the voxel's cube into every
//                          view (lane = view, world->camera table from k_worklist's trailing workgroups), scan the small pixel box in the ID
//                          image for pixels that first-hit THIS voxel ("occlusion test"), and stream
//                          their C-wide feature rows from HBM with 16-byte-per-lane coalesced loads,
//                          accumulating in registers in (view, y, x) order; one non-atomic
//                          read-modify-write of the output row; hit count by ballot/popcount.
//                          The box is only a search hint: the per-call histogram of phase 1 is the
//                          ground truth, and a voxel whose box scan finds fewer pixels than phase 1
//                          counted is rescanned over the whole image.  A voxel above the call's split
//                          threshold is cut into PARTS: each part is an item of the same work list, one
//                          wavefront sums it into a partial row, and k_combine_parts, next on the stream,
//                          adds a voxel's partial rows to its row in a fixed order.  One-view calls have
//                          k_gather_one: a fixed grid of wavefronts dealt the parts and the size-ordered
//                          list (a workgroup of four wavefronts per large voxel only as the A/B arm,
//                          VP_OPT_ONE_VIEW_SPLIT = 0).
//
// No float atomics (deterministic sums), no MFMA (the path is gather/accumulate, HBM-bound).
//
// One translation unit: this file holds the host side (launch plumbing, C-ABI entry points) and includes
//   vp_plan.h    the split plan of a projector call and the part slots, as pure host arithmetic (plan_split)
//   vp_common.h  error text, timing spans, compile-time dispatch (with_step, with_flags), VP_FLAG_PIPELINE stream state, Params, workspace Layout
//   vp_reduce.h  the fixed-order float64 sums of the loss families (block_tree_sum, k_ordered_sum) and the lane butterflies
//   vp_tables.h  arithmetic contract helpers, occupancy-derived tables, view table
//   vp_march.h   phase 1 (k_first_hit)
//   vp_gather.h  work list and phase 2 (k_worklist; k_gather, k_gather_one: one wavefront per voxel or per part of a split voxel; k_combine_parts)
//   vp_aux.h     RGB projection, nearest-voxel map, streaming-read probe
//   vp_prep.h    feature-map up-sampler (PTD:119-127), occupancy builder (BSO:30-53)
//   vp_aggregate.h  the aggregator's per-view fp16 accumulate over the hit rows (AGG:307-313)
//   vp_render.h  the transpose: every pixel copies the row of its first-hit voxel (k_render_walk, k_render_small)
//   vp_query.h   text query of a feature table: cosine logits, argmax label, softmax margin on the matrix cores (k_query)
//   vp_tilebin.h binning primitives into 16 x 16 tiles: the workspace's shared sections, key emit, sort and tile runs (k_tile_emit, k_tile_ranges)
//   vp_splat.h   tile-based Gaussian splatting of D-channel features with a fused label / confidence epilogue (stage 5.2)
//   vp_lift.h    lifting a 2D feature map onto the Gaussians: the splatter's transpose on the matrix cores (k_splat_lift)
//   vp_splat_render.h  rendering wide feature rows into a view: the splatter's forward on the matrix cores (k_splat_render)
//   vp_eval.h    scoring label maps against ground truth: confusion matrix, boundary band, boundary counts (all integers)
//   vp_feature_loss.h  cosine / L2 loss of a rendered feature image against a 2D feature map, and its binary16 gradient image
//   vp_proto_loss.h    prototype-contrastive loss of a rendered identity image against an instance mask, and its gradient image
//   vp_codebook.h      a code book of global instance labels: the id-by-code score matrix, the loss and its gradients on the matrix cores
//   vp_knn.h           the k nearest other points of every query on the bucketed grid (k_knn_points)
//   vp_reg3d.h         the 3D neighbourhood regulariser: KL divergence to the nearest neighbours' distributions, and its gradient
//   vp_photo_loss.h    photometric loss (L1 + D-SSIM) of a rendered image against a photograph, and its gradient image
//   vp_densify.h       adaptive density control: per-view statistics, the clone / split / prune plan, the row gather, the split
//   vp_sh.h            view-dependent colour: spherical harmonics of degree 0 .. 3 into colour rows, and the adjoint (voxproj_ext.h)
//   vp_mesh.h          triangle-mesh rasterizer: nearest face, depth and label per pixel, integer-decided (voxproj_mesh.h)
//   vp_grid.h          stage 2, the voxel grid of a Gaussian cloud: ball statistics on the bucketed grid, voxelisation (voxproj_grid.h)
//   vp_cluster.h       label sums over a feature table (sort by label, one wavefront per part, ordered combine), inverse row norms (voxproj_cluster.h)
//   vp_project.h the projector's host side: the per-call context and its stages (check, pick set, tables, plan, march, gather, commit)
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <chrono>
#include <initializer_list>
#include <mutex>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "voxproj.h"
#include "voxproj_ext.h"
#include "voxproj_mesh.h"
#include "voxproj_grid.h"
#include "voxproj_cluster.h"

#include "vp_plan.h"
#include "vp_common.h"
#include "vp_reduce.h"
#include "vp_tables.h"
#include "vp_march.h"
#include "vp_gather.h"
#include "vp_aux.h"
#include "vp_prep.h"
#include "vp_aggregate.h"
#include "vp_render.h"
#include "vp_query.h"
#include "vp_tilebin.h"
#include "vp_splat.h"
#include "vp_lift.h"
#include "vp_splat_render.h"
#include "vp_eval.h"
#include "vp_feature_loss.h"
#include "vp_proto_loss.h"
#include "vp_codebook.h"
#include "vp_knn.h"
#include "vp_reg3d.h"
#include "vp_photo_loss.h"
#include "vp_densify.h"
#include "vp_sh.h"
#include "vp_mesh.h"
#include "vp_grid.h"
#include "vp_cluster.h"
#include "vp_project.h"

// The refusal of a caller-provided workspace that is missing, smaller than ``need`` or not 256-byte aligned.
static int check_workspace(const void *workspace, size_t workspace_bytes, size_t need)
{
    if (!workspace || workspace_bytes < need)
        return fail(VP_EWORKSPACE, "workspace has %zu bytes, need %zu", workspace ? workspace_bytes : 0, need);
    if ((uintptr_t)workspace & 255) return fail(VP_EWORKSPACE, "workspace must be 256-byte aligned");
    return VP_OK;
}

// The refusals of a caller-provided buffer by name ("workspace", "backward workspace", "loss workspace", "lift workspace"),
// for the families that tell a NULL buffer from a small one.
static int check_buffer(const void *buf, const char *name)
{
    if (!buf) return fail(VP_EWORKSPACE, "%s is NULL", name);
    if ((uintptr_t)buf & 255) return fail(VP_EWORKSPACE, "%s must be 256-byte aligned", name);
    return VP_OK;
}

static int check_size(size_t have, size_t need, const char *name)
{
    if (have < need) return fail(VP_EWORKSPACE, "%s has %zu bytes, need %zu", name, have, need);
    return VP_OK;
}

// Opening a laid-out workspace: the buffer's refusals, then the layout (lay_out() fills l and is false when a rocprim
// scratch size query fails; those need the device, so every host check of an entry point comes before), then the size.
template <typename L, typename F>
static int open_workspace(const void *buf, size_t have, const L &l, F &&lay_out)
{
    if (int rc = check_buffer(buf, "workspace")) return rc;
    if (!lay_out()) return fail(VP_EHIP, "rocprim scratch size query failed");
    return check_size(have, l.bytes, "workspace");
}

// The tile-binned workspaces: l gets the typed pointers of every section of buf.
static int open_workspace(const void *buf, size_t have, int64_t n, int W, int H, int64_t capacity, SplatLayout &l)
{
    return open_workspace(buf, have, l, [&] { return splat_layout((char *)buf, n, W, H, capacity, l); });
}

static int open_workspace(const void *buf, size_t have, int64_t n, int W, int H, int64_t capacity, MeshLayout &l)
{
    return open_workspace(buf, have, l, [&] { return mesh_layout((char *)buf, n, W, H, capacity, l); });
}

static int check_count(const char *name, int64_t v)
{
    if (v < 0 || v > INT32_MAX) return fail(VP_EINVAL, "%s = %lld outside [0, 2^31 - 1]", name, (long long)v);
    return VP_OK;
}

constexpr int VP_MAX_WH = 32768;                         // the largest image side, of every family that takes an image

static int check_image(int W, int H)
{
    if (W < 1 || W > VP_MAX_WH || H < 1 || H > VP_MAX_WH)
        return fail(VP_EINVAL, "image %d x %d outside [1, %d]^2", W, H, VP_MAX_WH);
    return VP_OK;
}

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

int vp_abi_version(void) { return VP_ABI_VERSION; }

const char *vp_last_error(void) { return g_err; }

size_t vp_workspace_bytes(int B, int V, int H, int W, int C, int dimz, int dimy, int dimx, int64_t n_rows)
{
    if (B <= 0 || V <= 0 || H <= 0 || W <= 0 || C <= 0 || n_rows <= 0 || dimz <= 0 || dimy <= 0 || dimx <= 0) return 0;
    return make_layout(B, V, H, W, C, n_rows, dimz, dimy, dimx).total;
}

static int workspace_status_impl(void *workspace, void *stream_, bool drain_all);

// A projecting call, fp32 or fp16 feature maps: the stages of vp_project.h in order.
static int project_features(ProjectCall &c)
{
    if (c.f16 && (c.C % 8 != 0 || ((uintptr_t)c.feats & 15) != 0 || ((uintptr_t)c.out & 15) != 0))
        return fail(VP_EINVAL, "fp16 feature maps need C %% 8 == 0 and 16-byte aligned feats/out");
    if (!c.feats || !c.count || !c.out || !project_has_pointers(c)) return fail(VP_EINVAL, "null pointer argument");
    c.rec = ws_state(c.workspace, true);
    HitGuard hit_guard{c.rec, false};
    if (int rc = project_check(c)) return rc;
    if (int rc = project_pick_set(c)) return rc;
    if (int rc = project_tables(c)) return rc;
    project_plan(c);
    if (int rc = c.gather_only ? project_relist(c) : project_march(c, c.hit, true)) return rc;
    if (int rc = project_gather(c)) return rc;
    if (int rc = project_commit(c)) return rc;
    hit_guard.keep = true;
    if (c.flags & VP_FLAG_SYNC) return workspace_status_impl(c.workspace, c.s0, true);
    return VP_OK;
}

int vp_project_features(const float *feats, const int64_t *occ, const float *vmi, const float *intr,
                        const float *opts_host, int32_t *count, float *out, int32_t *views_hit,
                        const float *grid_origin_host, float voxel_size,
                        int B, int V, int H, int W, int C, int dimz, int dimy, int dimx, int64_t n_rows,
                        void *workspace, size_t workspace_bytes, void *stream_, int flags)
{
    ProjectCall c{feats, false, occ, vmi, intr, opts_host, count, out, views_hit, grid_origin_host, voxel_size,
                  B, V, H, W, C, dimz, dimy, dimx, n_rows, workspace, workspace_bytes, (hipStream_t)stream_, flags};
    return project_features(c);
}

int vp_project_features_f16(const void *feats_f16, const int64_t *occ, const float *vmi, const float *intr,
                            const float *opts_host, int32_t *count, float *out, int32_t *views_hit,
                            const float *grid_origin_host, float voxel_size,
                            int B, int V, int H, int W, int C, int dimz, int dimy, int dimx, int64_t n_rows,
                            void *workspace, size_t workspace_bytes, void *stream_, int flags)
{
    ProjectCall c{(const float *)feats_f16, true, occ, vmi, intr, opts_host, count, out, views_hit, grid_origin_host, voxel_size,
                  B, V, H, W, C, dimz, dimy, dimx, n_rows, workspace, workspace_bytes, (hipStream_t)stream_, flags};
    return project_features(c);
}

// March only: tables, k_zero_call and k_first_hit writing the first-hit image straight into ids; no plan, no work list, no
// gather.  Such a call leaves nothing for VP_FLAG_GATHER_ONLY or vp_copy_hit_image to take up: the HitGuard withdraws what the
// previous call left, this call replaced it.
int vp_first_hit_ids(const int64_t *occ, const float *vmi, const float *intr, const float *opts_host,
                     const float *grid_origin_host, float voxel_size, int B, int V, int H, int W,
                     int dimz, int dimy, int dimx, int64_t n_rows, int32_t *ids,
                     void *workspace, size_t workspace_bytes, void *stream_, int flags)
{
    const int allowed = VP_FLAG_SYNC | VP_FLAG_REUSE_ACCEL | VP_FLAG_VERIFY_ACCEL | VP_FLAG_EXACT_MARCH;
    if (flags & ~allowed) return fail(VP_EINVAL, "vp_first_hit_ids accepts VP_FLAG_SYNC, _REUSE_ACCEL, _VERIFY_ACCEL and _EXACT_MARCH only (flags 0x%x)", flags);
    ProjectCall c{nullptr, false, occ, vmi, intr, opts_host, nullptr, nullptr, nullptr, grid_origin_host, voxel_size,
                  B, V, H, W, 1, dimz, dimy, dimx, n_rows, workspace, workspace_bytes, (hipStream_t)stream_, flags};
    if (!ids || !project_has_pointers(c)) return fail(VP_EINVAL, "null pointer argument");
    c.rec = ws_state(workspace, true);
    HitGuard hit_guard{c.rec, false};
    if (int rc = project_check(c)) return rc;
    if (int rc = project_pick_set(c)) return rc;
    if (int rc = project_tables(c)) return rc;
    if (int rc = project_march(c, (int *)ids, false)) return rc;
    VP_HIP(hipGetLastError());
    c.rec->last_q = 0;
    if (flags & VP_FLAG_SYNC) return workspace_status_impl(workspace, stream_, true);
    return VP_OK;
}

// blocks of the render kernels (grid-stride beyond: 4 tiles of 64 pixels per block and pass)
#ifndef RENDER_MAX_BLOCKS
#define RENDER_MAX_BLOCKS (1 << 20)
#endif

int vp_render_features(const int32_t *ids, int64_t n_pixels, const float *rows, int64_t n_rows, int C, void *dst,
                       int dst_is_f16, int32_t *bad_ids, void *stream_)
{
    if (!ids || !rows || !dst) return fail(VP_EINVAL, "null pointer argument");
    if (n_pixels <= 0 || n_rows <= 0 || C <= 0) return fail(VP_EINVAL, "non-positive dimension (n_pixels, n_rows or C)");
    hipStream_t stream = (hipStream_t)stream_;
    const long long tiles = (n_pixels + 63) / 64;
    const dim3 grid((unsigned)std::min<long long>((tiles + 3) / 4, RENDER_MAX_BLOCKS));
    const bool al16 = (((uintptr_t)rows | (uintptr_t)dst) & 15) == 0;
    int *bad = (int *)bad_ids;
#define VP_RENDER(KERNEL) hipLaunchKernelGGL(KERNEL, grid, dim3(256), 0, stream, (const int *)ids, (long long)n_pixels, rows, \
                                             (long long)n_rows, C, dst_t, bad)
    // rows narrower than a wavefront's lanes (C < 64, aligned or not) go to k_render_small, which deals a tile's elements to
    // all 64 lanes; the walk would leave most lanes idle on every pixel
    if (dst_is_f16) {
        _Float16 *dst_t = (_Float16 *)dst;
        if (C < 64) VP_RENDER((k_render_small<_Float16>));
        else if (C % 8 == 0 && al16) VP_RENDER((k_render_walk<8, 1, _Float16>));
        else VP_RENDER((k_render_walk<1, 4, _Float16>));
    } else {
        float *dst_t = (float *)dst;
        if (C < 64) VP_RENDER((k_render_small<float>));
        else if (C % 4 == 0 && al16) VP_RENDER((k_render_walk<4, 2, float>));
        else VP_RENDER((k_render_walk<1, 4, float>));
    }
#undef VP_RENDER
    VP_HIP(hipGetLastError());
    return VP_OK;
}

size_t vp_query_workspace_bytes(int P, int C)
{
    if (P < 1 || P > QUERY_MAX_P || C < 1 || C > QUERY_MAX_C) return 0;
    return align256((size_t)query_ppad(P) * query_cpad(C) * sizeof(float));
}

int vp_query_features(const void *rows, int rows_is_f16, int64_t n_rows, int C, int64_t row_stride, const float *text, int P,
                      float scale, float *logits, int32_t *labels, float *margin, int32_t *n_nonfinite, void *workspace,
                      size_t workspace_bytes, void *stream_)
{
    if (!rows || !labels || !text) return fail(VP_EINVAL, "null pointer argument (rows, labels or text)");
    if (n_rows < 1 || n_rows > INT32_MAX) return fail(VP_EINVAL, "n_rows = %lld outside [1, 2^31 - 1]", (long long)n_rows);
    if (C < 1 || C > QUERY_MAX_C) return fail(VP_EINVAL, "C = %d outside [1, %d]", C, QUERY_MAX_C);
    if (P < 1 || P > QUERY_MAX_P) return fail(VP_EINVAL, "P = %d outside [1, %d]", P, QUERY_MAX_P);
    if (row_stride < C) return fail(VP_EINVAL, "row_stride %lld < C = %d", (long long)row_stride, C);
    if (!(scale > 0.0f) || !std::isfinite(scale)) return fail(VP_EINVAL, "scale must be finite and > 0 (got %g)", (double)scale);
    if (int rc = check_workspace(workspace, workspace_bytes, vp_query_workspace_bytes(P, C))) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t esz = rows_is_f16 ? 2 : 4;
    const bool vec = C % (16 / esz) == 0 && ((uintptr_t)rows & 15) == 0 && ((size_t)row_stride * esz) % 16 == 0;
    const dim3 grid((unsigned)((n_rows + 16 * QUERY_WAVES - 1) / (16 * QUERY_WAVES))), block(64 * QUERY_WAVES);
#define VP_QUERY(T, VEC) hipLaunchKernelGGL((k_query<T, VEC, false>), grid, block, 0, stream, (const T *)rows, (long long)n_rows, C, \
                                            (long long)row_stride, (const T *)workspace, P, scale, logits, (int *)labels, margin, \
                                            (int *)n_nonfinite)
#define VP_QUERY1(T) hipLaunchKernelGGL((k_query<T, true, true>), grid, block, 0, stream, (const T *)rows, (long long)n_rows, C, \
                                        (long long)row_stride, (const T *)workspace, P, scale, logits, (int *)labels, margin, \
                                        (int *)n_nonfinite)
    // rows of one chunk with 16-byte loads (C <= 512 fp16, <= 256 fp32): the variant without chunk loops
    if (rows_is_f16) {
        hipLaunchKernelGGL((k_query_text<_Float16>), dim3(query_ppad(P)), dim3(64), 0, stream, text, P, C, (_Float16 *)workspace);
        if (vec && C <= QUERY_NS * QueryTraits<_Float16>::W) VP_QUERY1(_Float16);
        else if (vec) VP_QUERY(_Float16, true);
        else VP_QUERY(_Float16, false);
    } else {
        hipLaunchKernelGGL((k_query_text<float>), dim3(query_ppad(P)), dim3(64), 0, stream, text, P, C, (float *)workspace);
        if (vec && C <= QUERY_NS * QueryTraits<float>::W) VP_QUERY1(float);
        else if (vec) VP_QUERY(float, true);
        else VP_QUERY(float, false);
    }
#undef VP_QUERY
#undef VP_QUERY1
    VP_HIP(hipGetLastError());
    return VP_OK;
}

// ------------------------------------------------------------------------------------------------
// Gaussian splatting.  The checks every entry point repeats, each VP_OK or the refusal; none of them needs a GPU, and every
// entry point makes all of its own before open_workspace (rocprim's scratch sizes depend on the device).
// ------------------------------------------------------------------------------------------------
static int splat_check_rows(int D, int64_t row_stride, int W, int H, int64_t capacity)
{
    if (D < 1 || D > SPLAT_MAX_D) return fail(VP_EINVAL, "D = %d outside [1, %d]", D, SPLAT_MAX_D);
    if (row_stride < D) return fail(VP_EINVAL, "row_stride %lld < D = %d", (long long)row_stride, D);
    if (int rc = check_image(W, H)) return rc;
    return check_count("capacity", capacity);
}

// the pose and the intrinsics into cam; the planes, eps2d and the image size are the caller's to check and fill
static int splat_check_camera(const float *viewmat, float fx, float fy, float cx, float cy, SplatCam &cam)
{
    if (!viewmat) return fail(VP_EINVAL, "null viewmat");
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(viewmat[k])) return fail(VP_EINVAL, "viewmat[%d] is not finite", k);
    if (!(fx > 0.0f) || !(fy > 0.0f) || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy))
        return fail(VP_EINVAL, "fx, fy must be finite and > 0, cx, cy finite (got %g %g %g %g)", (double)fx, (double)fy,
                    (double)cx, (double)cy);
    for (int k = 0; k < 12; ++k) cam.r[k] = viewmat[k];
    cam.fx = fx; cam.fy = fy; cam.cx = cx; cam.cy = cy;
    return VP_OK;
}

size_t vp_splat_workspace_bytes(int64_t n_gaussians, int W, int H, int64_t capacity)
{
    if (n_gaussians < 0 || n_gaussians > INT32_MAX || W < 1 || W > VP_MAX_WH || H < 1 || H > VP_MAX_WH || capacity < 0 ||
        capacity > INT32_MAX)
        return 0;
    SplatLayout l;
    return splat_layout(nullptr, n_gaussians, W, H, capacity, l) ? l.bytes : 0;
}

int vp_splat_project(const float *means, const float *quats, const float *scales, const float *opacities, int64_t n_gaussians,
                     const float *viewmat, float fx, float fy, float cx, float cy, int W, int H, float near_plane,
                     float far_plane, float eps2d, int64_t *n_isect, int32_t *n_nonfinite, void *workspace,
                     size_t workspace_bytes, void *stream_)
{
    if (int rc = check_count("n_gaussians", n_gaussians)) return rc;
    if (n_gaussians > 0 && (!means || !quats || !scales || !opacities))
        return fail(VP_EINVAL, "null pointer argument (means, quats, scales or opacities)");
    SplatCam cam;
    if (int rc = splat_check_camera(viewmat, fx, fy, cx, cy, cam)) return rc;
    if (int rc = check_image(W, H)) return rc;
    if (!(near_plane > 0.0f) || !(far_plane > near_plane) || !(eps2d >= 0.0f) || !std::isfinite(eps2d))
        return fail(VP_EINVAL, "need 0 < near < far and a finite eps2d >= 0 (got %g %g %g)", (double)near_plane,
                    (double)far_plane, (double)eps2d);
    SplatLayout l;
    if (int rc = open_workspace(workspace, workspace_bytes, n_gaussians, W, H, 0, l)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    cam.near_z = near_plane; cam.far_z = far_plane; cam.eps2d = eps2d;
    cam.W = W; cam.H = H; cam.tiles_x = l.tiles_x;
    if (n_gaussians > 0) {
        hipLaunchKernelGGL(k_splat_project, dim3((unsigned)((n_gaussians + 255) / 256)), dim3(256), 0, stream, means, quats,
                           scales, opacities, (long long)n_gaussians, cam, l.rec, l.box, l.count, (int *)n_nonfinite);
        VP_HIP(hipGetLastError());
    }
    return tile_scan(l, n_gaussians, (long long *)n_isect, stream);
}

// The forward after the caller's own checks: the shared checks, the tile sort and the blend.  ls: the loss variant's maps and
// outputs (then loss_stats is summed from its tile pairs), NULL for the plain blend.
static int splat_forward_impl(const float *features, int D, int64_t row_stride, int64_t n_gaussians, int W, int H,
                              int64_t capacity, int32_t *labels, float *confidence, float *alpha, float *logits,
                              int32_t *status, void *workspace, size_t workspace_bytes, const SplatLoss *ls,
                              double *loss_stats, void *stream_)
{
    if (int rc = check_count("n_gaussians", n_gaussians)) return rc;
    if (int rc = splat_check_rows(D, row_stride, W, H, capacity)) return rc;
    SplatLayout l;
    if (int rc = open_workspace(workspace, workspace_bytes, n_gaussians, W, H, capacity, l)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = splat_sort(l, n_gaussians, capacity, status, stream)) return rc;
    const dim3 grid = l.tile_grid(), block(SPLAT_THREADS);
    with_step<8, 16, 32, 64>(D, [&](auto dt) {
        with_flags([&](auto loss) {
            hipLaunchKernelGGL((k_splat_blend<dt.value, loss.value>), grid, block, 0, stream, l.rec, l.vals1, l.ranges, l.total,
                               (long long)capacity, features, D, (long long)row_stride, W, H, (int *)labels, confidence,
                               alpha, logits, ls ? *ls : SplatLoss{});
        }, ls != nullptr);
    });
    VP_HIP(hipGetLastError());
    if (ls) {
        hipLaunchKernelGGL((k_ordered_sum<2, SPLAT_THREADS>), dim3(1), block, 0, stream, (const double *)ls->tile_sums,
                           l.n_tiles(), l.total, (long long)capacity, loss_stats);
        VP_HIP(hipGetLastError());
    }
    return VP_OK;
}

int vp_splat_rasterize(const float *features, int D, int64_t row_stride, int64_t n_gaussians, int W, int H, int64_t capacity,
                       int32_t *labels, float *confidence, float *alpha, float *logits, int32_t *status, void *workspace,
                       size_t workspace_bytes, void *stream_)
{
    if (!labels || (n_gaussians > 0 && !features)) return fail(VP_EINVAL, "null pointer argument (labels or features)");
    return splat_forward_impl(features, D, row_stride, n_gaussians, W, H, capacity, labels, confidence, alpha, logits, status,
                              workspace, workspace_bytes, nullptr, nullptr, stream_);
}

size_t vp_splat_backward_workspace_bytes(int64_t capacity, int D)
{
    if (capacity < 0 || capacity > INT32_MAX || D < 1 || D > SPLAT_MAX_D) return 0;
    return splat_bwd_bytes(capacity, D);
}

// What the three backward entry points pass to their one implementation: the arguments of
// vp_splat_rasterize_backward_geometry in their order (the wrappers initialise it positionally), then what tells the calls apart.
struct SplatBackward {
    const float *means, *quats, *scales, *features;
    int D;
    int64_t row_stride, n_gaussians;
    const float *viewmat;
    float fx, fy, cx, cy;
    int W, H;
    float eps2d;
    int64_t capacity;
    const float *logits;         // the upstream grad_logits; with loss, the forward's logits image (NULL: replay)
    const float *grad_alpha;
    float *grad_means, *grad_quats, *grad_scales, *grad_features, *grad_opacities, *grad_screen;
    int32_t *status;
    void *workspace;
    size_t workspace_bytes;
    void *bwd_workspace;
    size_t bwd_bytes;
    void *stream;
    bool geom;                   // rows with the five screen sums (the geometry sweep and reduce)
    bool chain;                  // grad_means / grad_quats / grad_scales wanted: needs the Gaussians and the camera
    bool loss;                   // the upstream gradient is the cross-entropy's, from ls
    SplatLoss ls;
};

static int splat_backward_impl(const SplatBackward &a)
{
    const int D = a.D;
    const int64_t n_gaussians = a.n_gaussians, capacity = a.capacity;
    if (int rc = check_count("n_gaussians", n_gaussians)) return rc;
    if (n_gaussians > 0 && !a.features) return fail(VP_EINVAL, "null pointer argument (features)");
    if (a.chain && n_gaussians > 0 && (!a.means || !a.quats || !a.scales))
        return fail(VP_EINVAL, "null pointer argument (means, quats or scales, needed by grad_means / grad_quats / grad_scales)");
    if (int rc = splat_check_rows(D, a.row_stride, a.W, a.H, capacity)) return rc;
    SplatCam cam = {};
    if (a.chain) {
        if (int rc = splat_check_camera(a.viewmat, a.fx, a.fy, a.cx, a.cy, cam)) return rc;
        if (!(a.eps2d >= 0.0f) || !std::isfinite(a.eps2d))
            return fail(VP_EINVAL, "need a finite eps2d >= 0 (got %g)", (double)a.eps2d);
        cam.eps2d = a.eps2d;
        cam.W = a.W; cam.H = a.H;
    }
    // the buffers' refusals come before either size's: the workspace, the backward workspace and its size, then the layout
    if (int rc = check_buffer(a.workspace, "workspace")) return rc;
    if (int rc = check_buffer(a.bwd_workspace, "backward workspace")) return rc;
    const size_t bwd_need = a.geom ? splat_geom_bytes(capacity, D) : splat_bwd_bytes(capacity, D);
    if (int rc = check_size(a.bwd_bytes, bwd_need, "backward workspace")) return rc;
    SplatLayout l;
    if (int rc = open_workspace(a.workspace, a.workspace_bytes, n_gaussians, a.W, a.H, capacity, l)) return rc;
    if (n_gaussians == 0) return VP_OK;                  // no rows to write; nothing can exceed a capacity of 0 either
    hipStream_t stream = (hipStream_t)a.stream;
    const long long *total = l.total, *offs = l.offs;
    const int *count = l.count;
    float *part = (float *)a.bwd_workspace;
    const dim3 grid = l.tile_grid(), block(SPLAT_THREADS);
    with_step<8, 16, 32, 64>(D, [&](auto dt) {
        with_flags([&](auto geom, auto loss) {
            hipLaunchKernelGGL((k_splat_blend_backward<dt.value, geom.value, loss.value>), grid, block, 0, stream, l.rec, l.box,
                               count, offs, l.vals1, l.ranges, total, (long long)capacity, a.features, D,
                               (long long)a.row_stride, a.W, a.H, a.logits, a.grad_alpha, part, a.ls);
        }, a.geom, a.loss);
    });
    VP_HIP(hipGetLastError());
    // grid-stride over the Gaussians, at most one resident round (2048 workgroups of 4 wavefronts: 32 per CU on 256 CUs)
    const int gs = splat_reduce_group(a.geom ? D + SPLAT_SCREEN : D);
    const unsigned g_red = (unsigned)std::min<long long>((n_gaussians + 256 / gs - 1) / (256 / gs), 2048LL);
    with_step<16, 32, 64>(gs, [&](auto group) {
        with_flags([&](auto geom) {
            hipLaunchKernelGGL((k_splat_grad_reduce<group.value, geom.value>), dim3(g_red), dim3(256), 0, stream, count, offs,
                               (long long)n_gaussians, total, (long long)capacity, part, D, a.grad_features, a.grad_opacities,
                               a.grad_screen, (int *)a.status);
        }, a.geom);
    });
    VP_HIP(hipGetLastError());
    if (a.chain) {
        hipLaunchKernelGGL(k_splat_geom_chain, dim3((unsigned)((n_gaussians + 255) / 256)), dim3(256), 0, stream, a.means,
                           a.quats, a.scales, (long long)n_gaussians, cam, count, offs, total, (long long)capacity,
                           (const float *)part, D, a.grad_means, a.grad_quats, a.grad_scales);
        VP_HIP(hipGetLastError());
    }
    return VP_OK;
}

int vp_splat_rasterize_backward(const float *features, int D, int64_t row_stride, int64_t n_gaussians, int W, int H,
                                int64_t capacity, const float *grad_logits, const float *grad_alpha, float *grad_features,
                                float *grad_opacities, int32_t *status, void *workspace, size_t workspace_bytes,
                                void *bwd_workspace, size_t bwd_bytes, void *stream_)
{
    return splat_backward_impl({nullptr, nullptr, nullptr, features, D, row_stride, n_gaussians, nullptr, 0.0f, 0.0f, 0.0f, 0.0f,
                                W, H, 0.0f, capacity, grad_logits, grad_alpha, nullptr, nullptr, nullptr, grad_features,
                                grad_opacities, nullptr, status, workspace, workspace_bytes, bwd_workspace, bwd_bytes, stream_,
                                false, false, false, SplatLoss{}});
}

size_t vp_splat_geometry_backward_workspace_bytes(int64_t capacity, int D)
{
    if (capacity < 0 || capacity > INT32_MAX || D < 1 || D > SPLAT_MAX_D) return 0;
    return splat_geom_bytes(capacity, D);
}

int vp_splat_rasterize_backward_geometry(const float *means, const float *quats, const float *scales, const float *features,
                                         int D, int64_t row_stride, int64_t n_gaussians, const float *viewmat, float fx,
                                         float fy, float cx, float cy, int W, int H, float eps2d, int64_t capacity,
                                         const float *grad_logits, const float *grad_alpha, float *grad_means,
                                         float *grad_quats, float *grad_scales, float *grad_features, float *grad_opacities,
                                         float *grad_screen, int32_t *status, void *workspace, size_t workspace_bytes,
                                         void *bwd_workspace, size_t bwd_bytes, void *stream_)
{
    const bool chain = grad_means || grad_quats || grad_scales;
    return splat_backward_impl({means, quats, scales, features, D, row_stride, n_gaussians, viewmat, fx, fy, cx, cy, W, H, eps2d,
                                capacity, grad_logits, grad_alpha, grad_means, grad_quats, grad_scales, grad_features,
                                grad_opacities, grad_screen, status, workspace, workspace_bytes, bwd_workspace, bwd_bytes,
                                stream_, true, chain, false, SplatLoss{}});
}

size_t vp_splat_loss_workspace_bytes(int W, int H)
{
    if (W < 1 || W > VP_MAX_WH || H < 1 || H > VP_MAX_WH) return 0;
    const size_t n_tiles = (size_t)((W + SPLAT_TILE - 1) / SPLAT_TILE) * (size_t)((H + SPLAT_TILE - 1) / SPLAT_TILE);
    return align256(n_tiles * sizeof(double2));
}

int vp_splat_rasterize_loss(const float *features, int D, int64_t row_stride, int64_t n_gaussians, int W, int H,
                            int64_t capacity, const int32_t *target, const float *pixel_weight, double *loss_stats,
                            float *pixel_loss, int32_t *labels, float *confidence, float *alpha, float *logits,
                            int32_t *status, void *workspace, size_t workspace_bytes, void *loss_workspace, size_t loss_bytes,
                            void *stream_)
{
    if (n_gaussians > 0 && !features) return fail(VP_EINVAL, "null pointer argument (features)");
    if (!target || !loss_stats) return fail(VP_EINVAL, "null pointer argument (target or loss_stats)");
    if (int rc = check_image(W, H)) return rc;           // the loss workspace's size needs a valid image
    if (int rc = check_buffer(loss_workspace, "loss workspace")) return rc;
    if (int rc = check_size(loss_bytes, vp_splat_loss_workspace_bytes(W, H), "loss workspace")) return rc;
    SplatLoss ls = {};
    ls.target = (const int *)target;
    ls.weight = pixel_weight;
    ls.pixel_loss = pixel_loss;
    ls.tile_sums = (double2 *)loss_workspace;
    return splat_forward_impl(features, D, row_stride, n_gaussians, W, H, capacity, labels, confidence, alpha, logits, status,
                              workspace, workspace_bytes, &ls, loss_stats, stream_);
}

int vp_splat_loss_backward(const float *means, const float *quats, const float *scales, const float *features, int D,
                           int64_t row_stride, int64_t n_gaussians, const float *viewmat, float fx, float fy, float cx,
                           float cy, int W, int H, float eps2d, int64_t capacity, const int32_t *target,
                           const float *pixel_weight, const float *logits, const double *loss_stats, int reduction,
                           const float *grad_loss, const float *grad_alpha, float *grad_means, float *grad_quats,
                           float *grad_scales, float *grad_features, float *grad_opacities, float *grad_screen,
                           int32_t *status, void *workspace, size_t workspace_bytes, void *bwd_workspace, size_t bwd_bytes,
                           void *stream_)
{
    if (!target || !loss_stats) return fail(VP_EINVAL, "null pointer argument (target or loss_stats)");
    if (reduction != VP_LOSS_SUM && reduction != VP_LOSS_MEAN)
        return fail(VP_EINVAL, "reduction = %d is neither VP_LOSS_SUM nor VP_LOSS_MEAN", reduction);
    const bool chain = grad_means || grad_quats || grad_scales;
    SplatLoss ls = {};
    ls.target = (const int *)target;
    ls.weight = pixel_weight;
    ls.stats = loss_stats;
    ls.grad_loss = grad_loss;
    ls.mean = reduction == VP_LOSS_MEAN;
    return splat_backward_impl({means, quats, scales, features, D, row_stride, n_gaussians, viewmat, fx, fy, cx, cy, W, H, eps2d,
                                capacity, logits, grad_alpha, grad_means, grad_quats, grad_scales, grad_features,
                                grad_opacities, grad_screen, status, workspace, workspace_bytes, bwd_workspace, bwd_bytes,
                                stream_, chain || grad_screen, chain, true, ls});
}

size_t vp_splat_lift_workspace_bytes(int64_t capacity, int C)
{
    if (capacity < 0 || capacity > INT32_MAX || C < 1 || C > LIFT_MAX_C) return 0;
    return lift_bytes(capacity, C);
}

int vp_splat_lift(const void *feats_f16, int C, int64_t pix_stride, const float *pixel_weight, int64_t n_gaussians, int W, int H,
                  int64_t capacity, int sorted, float *sum, int64_t sum_stride, float *wsum, int32_t *status, void *workspace,
                  size_t workspace_bytes, void *lift_workspace, size_t lift_bytes_, void *stream_)
{
    if (int rc = check_count("n_gaussians", n_gaussians)) return rc;
    if (!feats_f16 || !sum) return fail(VP_EINVAL, "null pointer argument (feats_f16 or sum)");
    if (C < 1 || C > LIFT_MAX_C) return fail(VP_EINVAL, "C = %d outside [1, %d]", C, LIFT_MAX_C);
    if (pix_stride < C) return fail(VP_EINVAL, "pix_stride %lld < C = %d", (long long)pix_stride, C);
    if (sum_stride < C) return fail(VP_EINVAL, "sum_stride %lld < C = %d", (long long)sum_stride, C);
    if (sorted != 0 && sorted != 1) return fail(VP_EINVAL, "sorted = %d is neither 0 nor 1", sorted);
    if (int rc = check_image(W, H)) return rc;
    if (int rc = check_count("capacity", capacity)) return rc;
    if (int rc = check_buffer(workspace, "workspace")) return rc;
    if (int rc = check_buffer(lift_workspace, "lift workspace")) return rc;
    if (int rc = check_size(lift_bytes_, lift_bytes(capacity, C), "lift workspace")) return rc;
    SplatLayout l;
    if (int rc = open_workspace(workspace, workspace_bytes, n_gaussians, W, H, capacity, l)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (!sorted)
        if (int rc = splat_sort(l, n_gaussians, capacity, status, stream)) return rc;
    if (n_gaussians == 0) return VP_OK;                  // no rows to add to; nothing can exceed a capacity of 0 either
    const long long *total = l.total, *offs = l.offs;
    const int *count = l.count;
    const _Float16 *feats = (const _Float16 *)feats_f16;
    float *part = (float *)lift_workspace, *wpart = (float *)((char *)lift_workspace + lift_part_bytes(capacity, C));
    const bool vec = C % 8 == 0 && pix_stride % 8 == 0 && ((uintptr_t)feats_f16 & 15) == 0;
    const dim3 grid = l.tile_grid(), block(SPLAT_THREADS);
    with_flags([&](auto wide, auto v) {
        constexpr int CC = wide.value ? 64 : 16;
        static_assert(lift_chunk(wide.value ? 17 : 16) == CC, "the pass width is lift_chunk's");
        // grid-stride over the Gaussians, at most one resident round (as the backward's reduce)
        const unsigned g_red = (unsigned)std::min<long long>((n_gaussians + 256 / CC - 1) / (256 / CC), 2048LL);
        for (int c0 = 0; c0 < C; c0 += CC) {
            float *wp = c0 == 0 && wsum ? wpart : nullptr;
            hipLaunchKernelGGL((k_splat_lift<CC, v.value>), grid, block, 0, stream, l.rec, l.box, count, offs, l.vals1, l.ranges,
                               total, (long long)capacity, feats, C, (long long)pix_stride, c0, pixel_weight, W, H, part, wp);
            hipLaunchKernelGGL((k_splat_lift_reduce<CC>), dim3(g_red), dim3(256), 0, stream, count, offs,
                               (long long)n_gaussians, total, (long long)capacity, (const float *)part, (const float *)wp,
                               std::min(CC, C - c0), c0, sum, (long long)sum_stride, wsum, (int *)status);
        }
    }, C > 16, vec);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

int vp_splat_render(const void *rows, int rows_is_f16, int C, int64_t row_stride, int64_t n_gaussians, int W, int H,
                    int64_t capacity, int sorted, void *out, int out_is_f16, int64_t pix_stride, float *alpha, int32_t *status,
                    void *workspace, size_t workspace_bytes, void *stream_)
{
    if (int rc = check_count("n_gaussians", n_gaussians)) return rc;
    if (!rows || !out) return fail(VP_EINVAL, "null pointer argument (rows or out)");
    if (C < 1 || C > RENDER_MAX_C) return fail(VP_EINVAL, "C = %d outside [1, %d]", C, RENDER_MAX_C);
    if (row_stride < C) return fail(VP_EINVAL, "row_stride %lld < C = %d", (long long)row_stride, C);
    if (pix_stride < C) return fail(VP_EINVAL, "pix_stride %lld < C = %d", (long long)pix_stride, C);
    if (sorted != 0 && sorted != 1) return fail(VP_EINVAL, "sorted = %d is neither 0 nor 1", sorted);
    if (rows_is_f16 != 0 && rows_is_f16 != 1) return fail(VP_EINVAL, "rows_is_f16 = %d is neither 0 nor 1", rows_is_f16);
    if (out_is_f16 != 0 && out_is_f16 != 1) return fail(VP_EINVAL, "out_is_f16 = %d is neither 0 nor 1", out_is_f16);
    if (int rc = check_image(W, H)) return rc;
    if (int rc = check_count("capacity", capacity)) return rc;
    SplatLayout l;
    if (int rc = open_workspace(workspace, workspace_bytes, n_gaussians, W, H, capacity, l)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (!sorted)
        if (int rc = splat_sort(l, n_gaussians, capacity, status, stream)) return rc;
    // n_gaussians == 0 still launches: every tile's run is empty, and every pixel gets its zeros
    const int epl = rows_is_f16 ? 8 : 4;                 // elements of one 16-byte load
    const bool vec = C % epl == 0 && row_stride % epl == 0 && ((uintptr_t)rows & 15) == 0;
    const int CC = render_chunk(C);
    const dim3 grid = l.tile_grid(), block(SPLAT_THREADS);
    // 16-channel tiles of a pass: 1 or 4
    with_step<1, 4>(CC / 16, [&](auto nt) {
        with_flags([&](auto f32, auto v, auto o16) {
            for (int c0 = 0; c0 < C; c0 += CC)
                hipLaunchKernelGGL((k_splat_render<nt.value, f32.value, v.value, o16.value>), grid, block, 0, stream, l.rec,
                                   l.box, l.count, l.offs, l.vals1, l.ranges, l.total, (long long)capacity, rows, C,
                                   (long long)row_stride, c0, W, H, out, (long long)pix_stride, c0 == 0 ? alpha : nullptr,
                                   (int *)status);
        }, !rows_is_f16, vec, out_is_f16 != 0);
    });
    VP_HIP(hipGetLastError());
    return VP_OK;
}

static int read_status(void *workspace, hipStream_t stream, int *st /* [2][ST_WORDS] */)
{
    if (WsState *rec = ws_state(workspace, false)) {
        if (rec->pipe.ok) VP_HIP(hipStreamSynchronize(rec->pipe.side));
    }
    VP_HIP(hipMemcpyAsync(st, workspace, 2 * align256(ST_WORDS * sizeof(int)), hipMemcpyDeviceToHost, stream));
    VP_HIP(hipStreamSynchronize(stream));
    return VP_OK;
}

int vp_nearest_voxel(const float *pts_sorted, const int32_t *perm, const int32_t *cell_start, const double *grid_origin3,
                     double cell_size, int nx, int ny, int nz, const float *queries, int64_t M, int64_t *out,
                     void *stream_)
{
    if (!pts_sorted || !perm || !cell_start || !grid_origin3 || !queries || !out) return fail(VP_EINVAL, "null pointer argument");
    if (!(cell_size > 0.0) || nx <= 0 || ny <= 0 || nz <= 0 || M < 0) return fail(VP_EINVAL, "bad grid or query count");
    if (M == 0) return VP_OK;
    hipLaunchKernelGGL(k_nearest_voxel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, pts_sorted,
                       (const int *)perm, (const int *)cell_start, grid_origin3[0], grid_origin3[1], grid_origin3[2],
                       cell_size, nx, ny, nz, queries, (long long)M, (long long *)out);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

int vp_stream_read(const float *src, int64_t n_floats, float *sink, void *stream_)
{
    if (!src || !sink || n_floats < 4) return fail(VP_EINVAL, "bad argument");
    hipLaunchKernelGGL(k_stream_read, dim3(256 * 8), dim3(256), 0, (hipStream_t)stream_, src, (long long)(n_floats / 4), sink);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

// drain_all: report the highest-priority pending condition, name the others in the message and clear ALL of them (the end of
// a VP_FLAG_SYNC call: every pending error belongs to this call or to asynchronous ones before it, and a word left behind
// would fail the next, valid blocking call); otherwise ONE condition per read, only the reported word is cleared.
static int workspace_status_impl(void *workspace, void *stream_, bool drain_all)
{
    static_assert(ST_WORDS * sizeof(int) == 256, "a status block -- and the record's sticky page -- is one 256-byte slot");
    if (!workspace) return fail(VP_EINVAL, "null workspace");
    WsState *rec = ws_state(workspace, false);
    // everything queued on the workspace's streams has run when this returns: the side stream first (its work feeds the caller's)
    if (rec && rec->pipe.ok) VP_HIP(hipStreamSynchronize(rec->pipe.side));
    VP_HIP(hipStreamSynchronize((hipStream_t)stream_));
    if (!rec || !rec->opened || !rec->sticky_host) return VP_OK;   // no call has run on this workspace yet
    // the sticky words collect the errors of EVERY call since the last read (the per-call words of a buffer set are cleared
    // when the set is reused two pipelined calls later).  They live in the record's own page of pinned host memory, written
    // by the kernels through its device mapping: nothing to copy, and nobody else's to overwrite
    volatile int *sw = rec->sticky_host;
    const int stale = sw[ST_STICKY_STALE], stuck = sw[ST_STICKY_STUCK], badid = sw[ST_STICKY_BADID];
    const int word = stale ? ST_STICKY_STALE : stuck ? ST_STICKY_STUCK : badid ? ST_STICKY_BADID : -1;
    if (word >= 0) {
        if (drain_all) sw[ST_STICKY_STALE] = sw[ST_STICKY_STUCK] = sw[ST_STICKY_BADID] = 0;
        else sw[word] = 0;
    }
    const char *also = !drain_all ? "" : (word == ST_STICKY_STALE && (stuck || badid)) ? " (also pending, now cleared: stuck rays and/or out-of-range IDs)"
                                        : (word == ST_STICKY_STUCK && badid) ? " (also: a ray hit an occupancy ID outside [1, n_rows))" : "";
    if (stale) {
        rec->builds = 0;        // whatever tables the memory held are gone: VP_FLAG_REUSE_ACCEL is refused until a rebuild
        rec->copy_valid = false;
        return fail(VP_EINVAL, "VP_FLAG_REUSE_ACCEL, but the workspace memory no longer holds the tables this library built in it "
                               "(freed and handed out again without vp_workspace_release, or overwritten): those calls did no "
                               "work; call once without the flag%s", also);
    }
    if (stuck)
        return fail(VP_EINVAL, "rayIncrement is too small to advance a float32 ray parameter near depthMax: the reference "
                               "loop would never terminate (those rays were skipped, outputs are incomplete)%s", also);
    if (badid)
        return fail(VP_EBADID, "a ray hit an occupancy ID outside [1, n_rows): outputs are too small for the grid's IDs");
    return VP_OK;
}

int vp_workspace_status(void *workspace, void *stream_) { return workspace_status_impl(workspace, stream_, false); }

int vp_workspace_counters(void *workspace, int32_t *host_words, int n, void *stream_)
{
    if (!workspace || !host_words || n <= 0 || n > ST_WORDS) return fail(VP_EINVAL, "bad argument");
    int st[2 * ST_WORDS];
    int rc = read_status(workspace, (hipStream_t)stream_, st);
    if (rc != VP_OK) return rc;
    WsState *rec = ws_state(workspace, false);
    const int q = rec ? rec->last_q : 0;
    memcpy(host_words, st + q * ST_WORDS, size_t(n) * sizeof(int));
    return VP_OK;
}

int vp_profile_enable(int on)
{
    std::lock_guard<std::mutex> g(g_prof.mu);
    g_prof.on = on != 0;
    g_prof.used = 0;
    return VP_OK;
}

int vp_profile_read(double *ms4, int64_t *launches4)
{
    if (!ms4 || !launches4) return fail(VP_EINVAL, "null pointer argument");
    std::lock_guard<std::mutex> g(g_prof.mu);
    for (int k = 0; k < 4; k++) { ms4[k] = 0.0; launches4[k] = 0; }
    for (size_t i = 0; i < g_prof.used; i++) {
        VP_HIP(hipEventSynchronize(g_prof.pool[i * 2 + 1]));
        float ms = 0.f;
        VP_HIP(hipEventElapsedTime(&ms, g_prof.pool[i * 2], g_prof.pool[i * 2 + 1]));
        ms4[g_prof.kind[i]] += ms;
        launches4[g_prof.kind[i]] += 1;
    }
    g_prof.used = 0;
    return VP_OK;
}

int vp_copy_hit_image(const void *workspace, int32_t *dst, int B, int V, int H, int W, int C,
                      int dimz, int dimy, int dimx, int64_t n_rows, void *stream_)
{
    (void)C; (void)dimz; (void)dimy; (void)dimx; (void)n_rows;
    if (!workspace || !dst) return fail(VP_EINVAL, "null pointer argument");
    WsState *rec = ws_state(workspace, false);
    if (!rec || !rec->has_hit) return fail(VP_EINVAL, "no vp_project_features call has used this workspace");
    const size_t off = rec->hit_off;
    if (rec->pipe.ok) {
        VP_HIP(hipStreamSynchronize(rec->pipe.side));
    }
    VP_HIP(hipMemcpyAsync(dst, (const char *)workspace + off, size_t(B) * V * H * W * sizeof(int),
                          hipMemcpyDeviceToDevice, (hipStream_t)stream_));
    return VP_OK;
}

size_t vp_colors_workspace_bytes(int64_t n_rows)
{
    if (n_rows <= 0) return 0;
    // status words | cell of every ID | the voxel list {ID, cell} in curve order | one count per walking wavefront
    return 256 + align256(size_t(n_rows) * sizeof(int)) + align256(size_t(n_rows) * sizeof(int2)) + align256(size_t(COLOR_WALKERS) * sizeof(int));
}

int vp_project_colors(const int32_t *occ, int dimz, int dimy, int dimx, const float *c2w, const float *intr,
                      int V, const float *grid_origin_host, double voxel_size, const uint8_t *images,
                      int img_h, int img_w, float *color_sum, int32_t *hit_count, int32_t *first_view,
                      int32_t *pixel_uv, int64_t n_rows, int view_base, void *workspace, size_t workspace_bytes,
                      void *stream_)
{
    if (!occ || !c2w || !intr || !grid_origin_host || !images || !color_sum || !hit_count || !workspace)
        return fail(VP_EINVAL, "null pointer argument");
    if (dimz <= 0 || dimy <= 0 || dimx <= 0 || V <= 0 || img_h <= 0 || img_w <= 0 || n_rows <= 0)
        return fail(VP_EINVAL, "non-positive dimension");
    const long long cells = (long long)dimz * dimy * dimx;
    if (cells >= (1ll << 31) || n_rows >= (1ll << 31)) return fail(VP_EINVAL, "occupancy grid or row count >= 2^31");
    if (workspace_bytes < vp_colors_workspace_bytes(n_rows))
        return fail(VP_EWORKSPACE, "workspace has %zu bytes, need %zu", workspace_bytes, vp_colors_workspace_bytes(n_rows));
    if ((uintptr_t)workspace & 255) return fail(VP_EWORKSPACE, "workspace must be 256-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    int *status = (int *)workspace;
    int *cell_of_id = (int *)((char *)workspace + 256);
    int2 *list = (int2 *)((char *)cell_of_id + align256(size_t(n_rows) * sizeof(int)));
    int *counts = (int *)((char *)list + align256(size_t(n_rows) * sizeof(int2)));
    VP_HIP(hipMemsetAsync(status, 0, 256, stream));
    VP_HIP(hipMemsetAsync(cell_of_id, 0xFF, size_t(n_rows) * sizeof(int), stream));
    // the Morton curve over the grid's 4x4x4 blocks, shared by wavefronts that take 64 or more positions each
    ColorCurve curve;
    curve.nbx = (dimx + 3) / 4; curve.nby = (dimy + 3) / 4; curve.nbz = (dimz + 3) / 4;
    const auto bits = [](int n) { int b = 0; while ((1 << b) < n) b++; return b; };
    curve.bx = bits(curve.nbx); curve.by = bits(curve.nby); curve.bz = bits(curve.nbz);
    curve.slots = 1ll << (curve.bx + curve.by + curve.bz);       // < 2^32: < 8 x the blocks of a grid of < 2^31 cells
    const long long want = (curve.slots + 63) / 64;
    const int walkers = (int)(want > COLOR_WALKERS ? COLOR_WALKERS : (want + 3) / 4 * 4);
    hipLaunchKernelGGL(k_color_cells<1>, dim3(walkers / 4), dim3(256), 0, stream, (const int *)occ, dimz, dimy, dimx, curve,
                       cell_of_id, (long long)n_rows, status, counts, list);
    hipLaunchKernelGGL(k_color_scan, dim3(1), dim3(1024), 0, stream, counts, walkers, status);
    hipLaunchKernelGGL(k_color_cells<2>, dim3(walkers / 4), dim3(256), 0, stream, (const int *)occ, dimz, dimy, dimx, curve,
                       cell_of_id, (long long)n_rows, status, counts, list);
    int st[2];
    VP_HIP(hipMemcpyAsync(st, status, sizeof(st), hipMemcpyDeviceToHost, stream));
    VP_HIP(hipStreamSynchronize(stream));
    if (st[CST_BADID]) return fail(VP_EBADID, "an occupancy ID is outside [1, n_rows): outputs are too small for the grid's IDs");
    if (st[CST_DUP]) return fail(VP_EINVAL, "an occupancy ID labels more than one cell: the colour path needs unique IDs "
                                            "(build_sparse_occupancy.py:44-46 produces them)");
    const bool tiny = (long long)V * img_h * img_w * 3 < 4;
#define VP_LAUNCH_COLORS(UV, TINY)                                                                                           \
    hipLaunchKernelGGL((k_project_colors<UV, TINY>), dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, stream,           \
                       (const int *)cell_of_id, (const int2 *)list, (const int *)status, dimy, dimx, c2w, intr, V,           \
                       grid_origin_host[0], grid_origin_host[1], grid_origin_host[2], voxel_size,                            \
                       (const unsigned char *)images, img_h, img_w, color_sum, (int *)hit_count, (int *)first_view,          \
                       (int *)pixel_uv, (long long)n_rows, view_base)
    if (pixel_uv) { if (tiny) VP_LAUNCH_COLORS(true, true); else VP_LAUNCH_COLORS(true, false); }
    else          { if (tiny) VP_LAUNCH_COLORS(false, true); else VP_LAUNCH_COLORS(false, false); }
#undef VP_LAUNCH_COLORS
    VP_HIP(hipGetLastError());
    VP_HIP(hipStreamSynchronize(stream));
    return VP_OK;
}

size_t vp_upsample_workspace_bytes(int C, int h, int w, int src_is_f16)
{
    if (C <= 0 || h <= 0 || w <= 0) return 0;
    return align256(size_t(C) * h * w * (src_is_f16 ? 2 : 4));
}

int vp_upsample_features(const void *src_chw, int src_is_f16, int C, int h, int w, void *dst_hwc, int dst_is_f16,
                         int H, int W, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!src_chw || !dst_hwc || !workspace) return fail(VP_EINVAL, "null pointer argument");
    if (C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return fail(VP_EINVAL, "non-positive dimension");
    if (dst_is_f16 && !src_is_f16) return fail(VP_EINVAL, "a float16 destination needs a float16 source (PTD:126 casts back to the file's dtype)");
    if ((long long)H * W >= (1ll << 31) || (long long)h * w >= (1ll << 31)) return fail(VP_EINVAL, "image has >= 2^31 pixels");
    if (workspace_bytes < vp_upsample_workspace_bytes(C, h, w, src_is_f16))
        return fail(VP_EWORKSPACE, "workspace has %zu bytes, need %zu", workspace_bytes, vp_upsample_workspace_bytes(C, h, w, src_is_f16));
    hipStream_t stream = (hipStream_t)stream_;
    const long long P = (long long)h * w;
    const dim3 tgrid((unsigned)((P + 63) / 64), (unsigned)((C + 63) / 64));
    // cv::resize derives the scale from the destination size: inv_scale = dsize / ssize, scale = 1 / inv_scale
    const double scale_x = 1.0 / ((double)W / (double)w), scale_y = 1.0 / ((double)H / (double)h);
    const unsigned ublocks = (unsigned)(((long long)H * W + 4 * UPS_PIX - 1) / (4 * UPS_PIX));
#define VP_UPS1(TS_, TD_, VEC_, NV_) hipLaunchKernelGGL((k_upsample_hwc<TS_, TD_, VEC_, NV_>), dim3(ublocks), dim3(256), 0, stream, \
        (const TS_ *)workspace, (TD_ *)dst_hwc, C, h, w, H, W, scale_x, scale_y)
    // channel groups a lane owns: the register window of the kernel is instantiated for 1, 2 or 4 of them
#define VP_UPS(TS_, TD_, VEC_)                                           \
    do {                                                                 \
        const int groups_ = (C + 64 * (VEC_) - 1) / (64 * (VEC_));      \
        if (groups_ <= 1) VP_UPS1(TS_, TD_, VEC_, 1);                    \
        else if (groups_ <= 2) VP_UPS1(TS_, TD_, VEC_, 2);               \
        else if (groups_ <= 4) VP_UPS1(TS_, TD_, VEC_, 4);               \
        else VP_UPS1(TS_, TD_, VEC_, 0);                                 \
    } while (0)
    const bool al16 = (((uintptr_t)workspace | (uintptr_t)dst_hwc) & 15) == 0;
    if (src_is_f16) {
        if ((((uintptr_t)src_chw | (uintptr_t)workspace) & 15) == 0 && P % 8 == 0 && C % 8 == 0)
            hipLaunchKernelGGL((k_chw_to_hwc_v16<_Float16>), tgrid, dim3(256), 0, stream, (const _Float16 *)src_chw, (_Float16 *)workspace, C, P);
        else
            hipLaunchKernelGGL((k_chw_to_hwc<_Float16>), tgrid, dim3(256), 0, stream, (const _Float16 *)src_chw, (_Float16 *)workspace, C, P);
        const bool v8 = al16 && C % 8 == 0;
        if (dst_is_f16) { if (v8) VP_UPS(_Float16, _Float16, 8); else VP_UPS(_Float16, _Float16, 1); }
        else { if (v8) VP_UPS(_Float16, float, 8); else VP_UPS(_Float16, float, 1); }
    } else {
        if ((((uintptr_t)src_chw | (uintptr_t)workspace) & 15) == 0 && P % 4 == 0 && C % 4 == 0)
            hipLaunchKernelGGL((k_chw_to_hwc_v16<float>), tgrid, dim3(256), 0, stream, (const float *)src_chw, (float *)workspace, C, P);
        else
            hipLaunchKernelGGL((k_chw_to_hwc<float>), tgrid, dim3(256), 0, stream, (const float *)src_chw, (float *)workspace, C, P);
        if (al16 && C % 4 == 0) VP_UPS(float, float, 4); else VP_UPS(float, float, 1);
    }
#undef VP_UPS1
#undef VP_UPS
    VP_HIP(hipGetLastError());
    return VP_OK;
}

int vp_voxel_coords(const float *points_xyz, int64_t N, const float *grid_origin_host, float voxel_size,
                    int32_t *coords, int32_t *scratch8_dev, int32_t *minmax_host, void *stream_)
{
    if (!points_xyz || !grid_origin_host || !coords || !scratch8_dev || !minmax_host) return fail(VP_EINVAL, "null pointer argument");
    if (N <= 0 || N >= (1ll << 31) - 1) return fail(VP_EINVAL, "point count must be in [1, 2^31 - 2]");
    hipStream_t stream = (hipStream_t)stream_;
    const int init[8] = {2147483647, 2147483647, 2147483647, -2147483647 - 1, -2147483647 - 1, -2147483647 - 1, 0, 0};
    VP_HIP(hipMemcpyAsync(scratch8_dev, init, sizeof(init), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_voxel_coords, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, points_xyz, (long long)N,
                       grid_origin_host[0], grid_origin_host[1], grid_origin_host[2], voxel_size, (int *)coords,
                       (int *)scratch8_dev, (int *)scratch8_dev + 6);
    VP_HIP(hipGetLastError());
    int back[8];
    VP_HIP(hipMemcpyAsync(back, scratch8_dev, sizeof(back), hipMemcpyDeviceToHost, stream));
    VP_HIP(hipStreamSynchronize(stream));
    if (back[6]) return fail(VP_EINVAL, "a point's voxel coordinate is not finite or beyond 2^30 cells from the grid origin");
    memcpy(minmax_host, back, 6 * sizeof(int));
    return VP_OK;
}

int vp_scatter_occupancy(const int32_t *coords, int64_t N, const int32_t *shift3_host, int dimz, int dimy, int dimx,
                         int32_t *occ, int32_t *scratch8_dev, void *stream_)
{
    if (!coords || !shift3_host || !occ || !scratch8_dev) return fail(VP_EINVAL, "null pointer argument");
    if (N <= 0 || N >= (1ll << 31) - 1 || dimz <= 0 || dimy <= 0 || dimx <= 0) return fail(VP_EINVAL, "bad size");
    if ((long long)dimz * dimy * dimx >= (1ll << 31)) return fail(VP_EINVAL, "occupancy grid has >= 2^31 cells");
    hipStream_t stream = (hipStream_t)stream_;
    VP_HIP(hipMemsetAsync(occ, 0, size_t(dimz) * dimy * dimx * sizeof(int), stream));
    VP_HIP(hipMemsetAsync(scratch8_dev, 0, 8 * sizeof(int), stream));
    hipLaunchKernelGGL(k_scatter_occupancy, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, (const int *)coords, (long long)N,
                       shift3_host[0], shift3_host[1], shift3_host[2], dimz, dimy, dimx, (int *)occ, (int *)scratch8_dev);
    VP_HIP(hipGetLastError());
    int bad = 0;
    VP_HIP(hipMemcpyAsync(&bad, scratch8_dev, sizeof(int), hipMemcpyDeviceToHost, stream));
    VP_HIP(hipStreamSynchronize(stream));
    if (bad) return fail(VP_EINVAL, "a shifted voxel coordinate falls outside the [dimz,dimy,dimx] grid");
    return VP_OK;
}

int vp_aggregate_view_f16(float *view_sum, int32_t *view_count, void *run16, int32_t *views, int32_t *first_view,
                          int view_index, int32_t *nonfinite_dev, int64_t n_rows, int C, void *stream_)
{
    if (!view_sum || !view_count || !run16 || !views || !first_view || !nonfinite_dev) return fail(VP_EINVAL, "null pointer argument");
    if (n_rows <= 0 || C <= 0) return fail(VP_EINVAL, "non-positive dimension");
    if (((uintptr_t)view_sum & 15) || ((uintptr_t)run16 & 7)) return fail(VP_EINVAL, "view_sum must be 16-byte, run16 8-byte aligned");
    if (n_rows == 1) return VP_OK;
    hipLaunchKernelGGL(k_aggregate_view_f16, dim3((unsigned)((n_rows - 1 + 3) / 4)), dim3(256), 0, (hipStream_t)stream_, view_sum,
                       (int *)view_count, (_Float16 *)run16, (int *)views, (int *)first_view, view_index, (int *)nonfinite_dev,
                       (long long)n_rows, C);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

// ------------------------------------------------------------------------------------------------
// Scoring label maps (vp_eval.h).  Every check is host arithmetic and comes before the first launch.
// ------------------------------------------------------------------------------------------------
size_t vp_label_scores_workspace_bytes(int W, int H)
{
    if (W < 1 || W > VP_MAX_WH || H < 1 || H > VP_MAX_WH) return 0;
    // the prediction's band | the target's band | the row pass's ok map, one byte per pixel each
    return 3 * align256((size_t)W * H);
}

int vp_label_boundary(const int32_t *labels, int W, int H, int radius, uint8_t *band, void *workspace, size_t workspace_bytes,
                      void *stream_)
{
    if (!labels || !band) return fail(VP_EINVAL, "null pointer argument (labels or band)");
    if (int rc = check_image(W, H)) return rc;
    if (radius < 1 || radius > EVAL_MAX_RADIUS) return fail(VP_EINVAL, "radius = %d outside [1, %d]", radius, EVAL_MAX_RADIUS);
    if (int rc = check_workspace(workspace, workspace_bytes, vp_label_scores_workspace_bytes(W, H))) return rc;
    unsigned char *ok = (unsigned char *)workspace + 2 * align256((size_t)W * H);
    eval_launch_band((const int *)labels, W, H, radius, (unsigned char *)band, ok, (hipStream_t)stream_);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

int vp_label_scores(const int32_t *pred, const int32_t *target, int W, int H, int P, int radius, int64_t *confusion,
                    int64_t *skipped, int64_t *bnd_inter, int64_t *bnd_union, void *workspace, size_t workspace_bytes,
                    void *stream_)
{
    if (!pred || !target || !confusion || !skipped) return fail(VP_EINVAL, "null pointer argument (pred, target, confusion or skipped)");
    if (int rc = check_image(W, H)) return rc;
    if (P < 1 || P > EVAL_MAX_P) return fail(VP_EINVAL, "P = %d outside [1, %d]", P, EVAL_MAX_P);
    if (radius < 0 || radius > EVAL_MAX_RADIUS) return fail(VP_EINVAL, "radius = %d outside [0, %d]", radius, EVAL_MAX_RADIUS);
    if (radius > 0 && (!bnd_inter || !bnd_union)) return fail(VP_EINVAL, "radius > 0 needs bnd_inter and bnd_union");
    if (radius > 0)
        if (int rc = check_workspace(workspace, workspace_bytes, vp_label_scores_workspace_bytes(W, H))) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const long long n = (long long)W * H;
    unsigned char *pband = nullptr, *tband = nullptr;
    if (radius > 0) {
        const size_t plane = align256((size_t)n);
        pband = (unsigned char *)workspace;
        tband = pband + plane;
        unsigned char *ok = tband + plane;
        eval_launch_band((const int *)pred, W, H, radius, pband, ok, stream);
        eval_launch_band((const int *)target, W, H, radius, tband, ok, stream);
    }
    // (radius = 0: the boundary pointers are not touched, whatever they are)
    const dim3 grid((unsigned)std::min<long long>((n + 255) / 256, EVAL_SCORE_BLOCKS));
#define VP_EVAL_SCORES(LDS) hipLaunchKernelGGL((k_eval_scores<LDS>), grid, dim3(256), 0, stream, (const int *)pred, (const int *)target, n, \
        P, (const unsigned char *)pband, (const unsigned char *)tband, (unsigned long long *)confusion,                              \
        (unsigned long long *)skipped, (unsigned long long *)bnd_inter, (unsigned long long *)bnd_union)
    if (P <= EVAL_LDS_P) VP_EVAL_SCORES(true); else VP_EVAL_SCORES(false);
#undef VP_EVAL_SCORES
    VP_HIP(hipGetLastError());
    return VP_OK;
}

// ------------------------------------------------------------------------------------------------
// The feature loss (vp_feature_loss.h).  Every check is host arithmetic and comes before the first launch.
// ------------------------------------------------------------------------------------------------
size_t vp_feature_loss_workspace_bytes(int W, int H)
{
    if (W < 1 || W > VP_MAX_WH || H < 1 || H > VP_MAX_WH) return 0;
    return floss_bytes((long long)W * H);
}

static int floss_check_maps(const void *image, int image_is_f16, int64_t pix_stride, const void *target_f16, int64_t tgt_stride,
                            int C, int W, int H, const void *workspace, size_t workspace_bytes)
{
    if (!image || !target_f16) return fail(VP_EINVAL, "null pointer argument (image or target_f16)");
    if (image_is_f16 != 0 && image_is_f16 != 1) return fail(VP_EINVAL, "image_is_f16 = %d is neither 0 nor 1", image_is_f16);
    if (C < 1 || C > FLOSS_MAX_C) return fail(VP_EINVAL, "C = %d outside [1, %d]", C, FLOSS_MAX_C);
    if (int rc = check_image(W, H)) return rc;
    if (pix_stride < C) return fail(VP_EINVAL, "pix_stride %lld < C = %d", (long long)pix_stride, C);
    if (tgt_stride < C) return fail(VP_EINVAL, "tgt_stride %lld < C = %d", (long long)tgt_stride, C);
    return check_workspace(workspace, workspace_bytes, floss_bytes((long long)W * H));
}

// 16-byte loads: whole chunks of 8 channels, every pixel's row 16-byte aligned in both maps
static bool floss_vec(const void *image, int image_is_f16, int64_t pix_stride, const void *target_f16, int64_t tgt_stride, int C)
{
    return C % 8 == 0 && tgt_stride % 8 == 0 && ((uintptr_t)target_f16 & 15) == 0 && pix_stride % (image_is_f16 ? 8 : 4) == 0 &&
           ((uintptr_t)image & 15) == 0;
}

int vp_feature_loss(const void *image, int image_is_f16, int64_t pix_stride, const void *target_f16, int64_t tgt_stride, int C,
                    int W, int H, const float *pixel_weight, const float *alpha, float min_alpha, int kind, double *loss_stats,
                    float *pixel_loss, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!loss_stats) return fail(VP_EINVAL, "null pointer argument (loss_stats)");
    if (kind != VP_FEATURE_LOSS_COSINE && kind != VP_FEATURE_LOSS_L2)
        return fail(VP_EINVAL, "kind = %d is neither VP_FEATURE_LOSS_COSINE nor VP_FEATURE_LOSS_L2", kind);
    if (int rc = floss_check_maps(image, image_is_f16, pix_stride, target_f16, tgt_stride, C, W, H, workspace, workspace_bytes))
        return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const long long n = (long long)W * H, blocks = floss_blocks(n);
    char *ws = (char *)workspace;
    unsigned *max_bits = (unsigned *)ws;
    double2 *sums = (double2 *)(ws + FLOSS_HEADER);
    float4 *coef = (float4 *)(ws + FLOSS_HEADER + floss_sums_bytes(n));
    VP_HIP(hipMemsetAsync(ws, 0, FLOSS_HEADER, stream));
    const bool vec = floss_vec(image, image_is_f16, pix_stride, target_f16, tgt_stride, C);
    with_step<1, 2, 4, 8>(floss_nch(C), [&](auto nch) {
        with_flags([&](auto v, auto f16, auto cosine) {
            hipLaunchKernelGGL((k_feature_loss<nch.value, v.value, f16.value, cosine.value>), dim3((unsigned)blocks),
                               dim3(FLOSS_THREADS), 0, stream, image, (long long)pix_stride, (const _Float16 *)target_f16,
                               (long long)tgt_stride, C, n, pixel_weight, alpha, min_alpha, coef, sums, max_bits, pixel_loss);
        }, vec, image_is_f16 != 0, kind == VP_FEATURE_LOSS_COSINE);
    });
    hipLaunchKernelGGL((k_ordered_sum<2, FLOSS_THREADS>), dim3(1), dim3(FLOSS_THREADS), 0, stream, (const double *)sums, blocks,
                       (const long long *)nullptr, 0LL, loss_stats);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

int vp_feature_loss_gradient(const void *image, int image_is_f16, int64_t pix_stride, const void *target_f16, int64_t tgt_stride,
                             int C, int W, int H, const double *loss_stats, int reduction, const float *grad_loss, void *grad_f16,
                             int64_t grad_stride, int32_t *grad_exponent, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!loss_stats || !grad_f16 || !grad_exponent)
        return fail(VP_EINVAL, "null pointer argument (loss_stats, grad_f16 or grad_exponent)");
    if (reduction != VP_LOSS_SUM && reduction != VP_LOSS_MEAN)
        return fail(VP_EINVAL, "reduction = %d is neither VP_LOSS_SUM nor VP_LOSS_MEAN", reduction);
    if (grad_stride < C) return fail(VP_EINVAL, "grad_stride %lld < C = %d", (long long)grad_stride, C);
    if (int rc = floss_check_maps(image, image_is_f16, pix_stride, target_f16, tgt_stride, C, W, H, workspace, workspace_bytes))
        return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const long long n = (long long)W * H, blocks = floss_blocks(n);
    const char *ws = (const char *)workspace;
    const float4 *coef = (const float4 *)(ws + FLOSS_HEADER + floss_sums_bytes(n));
    const bool vec = floss_vec(image, image_is_f16, pix_stride, target_f16, tgt_stride, C) && grad_stride % 8 == 0 &&
                     ((uintptr_t)grad_f16 & 15) == 0;
    with_step<1, 2, 4, 8>(floss_nch(C), [&](auto nch) {
        with_flags([&](auto v, auto f16) {
            hipLaunchKernelGGL((k_feature_loss_gradient<nch.value, v.value, f16.value>), dim3((unsigned)blocks),
                               dim3(FLOSS_THREADS), 0, stream, image, (long long)pix_stride, (const _Float16 *)target_f16,
                               (long long)tgt_stride, C, n, coef, (const unsigned *)ws, loss_stats,
                               (int)(reduction == VP_LOSS_MEAN), grad_loss, (_Float16 *)grad_f16, (long long)grad_stride,
                               (int *)grad_exponent);
        }, vec, image_is_f16 != 0);
    });
    VP_HIP(hipGetLastError());
    return VP_OK;
}

// ------------------------------------------------------------------------------------------------
// The prototype-contrastive loss (vp_proto_loss.h).  Every check is host arithmetic and comes before the first launch.
// ------------------------------------------------------------------------------------------------
size_t vp_proto_contrast_workspace_bytes(int D, int W, int H)
{
    if (D < 1 || D > PROTO_MAX_D || W < 1 || W > VP_MAX_WH || H < 1 || H > VP_MAX_WH) return 0;
    return proto_carve(nullptr, D, (long long)W * H).bytes;
}

static int proto_check(const float *image, int D, int W, int H, const int32_t *ids, const void *workspace, size_t workspace_bytes)
{
    if (!image || !ids) return fail(VP_EINVAL, "null pointer argument (image or ids)");
    if (D < 1 || D > PROTO_MAX_D) return fail(VP_EINVAL, "D = %d outside [1, %d]", D, PROTO_MAX_D);
    if (int rc = check_image(W, H)) return rc;
    return check_workspace(workspace, workspace_bytes, vp_proto_contrast_workspace_bytes(D, W, H));
}

int vp_proto_contrast(const float *image, int D, int W, int H, const int32_t *ids, const int32_t *count, int ignore_id,
                      int min_count, float phi_scale, float phi_min, float phi_max, double *stats, float *pixel_loss,
                      float *own_prob, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!stats) return fail(VP_EINVAL, "null pointer argument (stats)");
    if (min_count < 0) return fail(VP_EINVAL, "min_count = %d is negative", min_count);
    if (!std::isfinite(phi_scale) || !std::isfinite(phi_min) || !std::isfinite(phi_max) || !(phi_min > 0.0f) || phi_max < phi_min)
        return fail(VP_EINVAL, "temperatures: need finite phi_scale = %g and 0 < phi_min = %g <= phi_max = %g", (double)phi_scale,
                    (double)phi_min, (double)phi_max);
    if (int rc = proto_check(image, D, W, H, ids, workspace, workspace_bytes)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const long long n = (long long)W * H;
    const int G = proto_grid(n);
    const ProtoWs w = proto_carve(workspace, D, n);
    const size_t lds = (size_t)PROTO_IDS * D * sizeof(float);
    hipError_t attr_rc = hipSuccess;
    with_step<16, 32, 64>(D, [&](auto dp) {
        constexpr int DP = decltype(dp)::value;
        // with the static tiles the two accumulating kernels pass 64 KiB of the CU's 160 at large D: said once per variant
        static hipError_t lds_attr = [] {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_proto_sums<DP>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, PROTO_IDS * DP * (int)sizeof(float));
            if (e == hipSuccess)
                e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_proto_loss<DP>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, PROTO_IDS * DP * (int)sizeof(float));
            return e;
        }();
        if (lds_attr != hipSuccess) {
            attr_rc = lds_attr;
            return;
        }
        hipLaunchKernelGGL(k_proto_sums<DP>, dim3(G), dim3(PROTO_THREADS), lds, stream, image, D, n, ids, count, ignore_id,
                           w.s_part, w.cnt_part, w.norm_part);
        hipLaunchKernelGGL(k_proto_means, dim3(PROTO_IDS), dim3(PROTO_COMBINE), 0, stream, D, G, (const float *)w.s_part,
                           (const unsigned long long *)w.cnt_part, (const double *)w.norm_part, w.n_id, w.u_id, stats);
        hipLaunchKernelGGL(k_proto_spread<DP>, dim3(G), dim3(PROTO_THREADS), 0, stream, image, D, n, ids, count, ignore_id,
                           min_count, (const unsigned long long *)w.n_id, (const float *)w.u_id, w.a_part);
        hipLaunchKernelGGL(k_proto_temps, dim3(1), dim3(PROTO_COMBINE), 0, stream, D, G, min_count, phi_scale, phi_min, phi_max,
                           (const float *)w.a_part, (const unsigned long long *)w.n_id, (const float *)w.u_id, w.hdr, w.slot_of_id,
                           w.inv_phi, w.n_slot, w.utab, stats);
        hipLaunchKernelGGL(k_proto_loss<DP>, dim3(G), dim3(PROTO_THREADS), lds, stream, image, D, n, ids, count,
                           (const ProtoHeader *)w.hdr, (const int *)w.slot_of_id, (const float *)w.utab, pixel_loss, own_prob,
                           w.s_part, w.loss_part);
        hipLaunchKernelGGL(k_proto_protos, dim3(PROTO_IDS), dim3(PROTO_COMBINE), 0, stream, D, G, (const ProtoHeader *)w.hdr,
                           (const float *)w.s_part, (const double *)w.loss_part, (const float *)w.inv_phi,
                           (const float *)w.n_slot, w.gn, stats);
    });
    VP_HIP(attr_rc);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

int vp_proto_contrast_gradient(const float *image, int D, int W, int H, const int32_t *ids, const int32_t *count,
                               float weight_contrast, float weight_norm, const float *grad_loss, float *grad_image,
                               void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!grad_image) return fail(VP_EINVAL, "null pointer argument (grad_image)");
    if (!std::isfinite(weight_contrast) || !std::isfinite(weight_norm))
        return fail(VP_EINVAL, "weights %g and %g must be finite", (double)weight_contrast, (double)weight_norm);
    if (int rc = proto_check(image, D, W, H, ids, workspace, workspace_bytes)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const long long n = (long long)W * H;
    const ProtoWs w = proto_carve(workspace, D, n);
    with_step<16, 32, 64>(D, [&](auto dp) {
        constexpr int DP = decltype(dp)::value;
        hipLaunchKernelGGL(k_proto_gradient<DP>, dim3((unsigned)proto_tiles(n)), dim3(PROTO_THREADS), 0, stream, image, D, n, ids,
                           count, (const ProtoHeader *)w.hdr, (const int *)w.slot_of_id, (const float *)w.utab,
                           (const float *)w.gn, weight_contrast, weight_norm, grad_loss, grad_image);
    });
    VP_HIP(hipGetLastError());
    return VP_OK;
}

// ------------------------------------------------------------------------------------------------
// The photometric loss (vp_photo_loss.h).  Every check is host arithmetic and comes before the first launch.
// ------------------------------------------------------------------------------------------------
size_t vp_photo_loss_workspace_bytes(int C, int W, int H)
{
    if (C < 1 || C > PHOTO_MAX_C || W < 1 || W > VP_MAX_WH || H < 1 || H > VP_MAX_WH) return 0;
    return photo_bytes(C, W, H);
}

static int photo_check(const float *image, const float *target, int C, int W, int H, bool need_workspace, const void *workspace,
                       size_t workspace_bytes)
{
    if (!image || !target) return fail(VP_EINVAL, "null pointer argument (image or target)");
    if (C < 1 || C > PHOTO_MAX_C) return fail(VP_EINVAL, "C = %d outside [1, %d]", C, PHOTO_MAX_C);
    if (int rc = check_image(W, H)) return rc;
    if (!workspace && !need_workspace) return VP_OK;
    return check_workspace(workspace, workspace_bytes, photo_bytes(C, W, H));
}

int vp_photo_loss(const float *image, const float *target, int C, int W, int H, double *loss_stats, float *ssim_map,
                  void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!loss_stats) return fail(VP_EINVAL, "null pointer argument (loss_stats)");
    if (int rc = photo_check(image, target, C, W, H, false, workspace, workspace_bytes)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (!workspace) {
        hipLaunchKernelGGL(k_photo_loss<true>, dim3(1), dim3(PHOTO_THREADS), 0, stream, image, target, C, W, H, ssim_map,
                           (float *)nullptr, (double *)nullptr, loss_stats);
    } else {
        float *maps = (float *)workspace;
        double *sums = (double *)((char *)workspace + photo_maps_bytes(C, W, H));
        hipLaunchKernelGGL(k_photo_loss<false>, dim3((unsigned)photo_tiles_x(W), (unsigned)photo_tiles_x(H), (unsigned)C),
                           dim3(PHOTO_THREADS), 0, stream, image, target, C, W, H, ssim_map, maps, sums, loss_stats);
        hipLaunchKernelGGL((k_ordered_sum<3, PHOTO_THREADS>), dim3(1), dim3(PHOTO_THREADS), 0, stream, (const double *)sums,
                           photo_tiles(C, W, H), (const long long *)nullptr, 0LL, loss_stats);
    }
    VP_HIP(hipGetLastError());
    return VP_OK;
}

int vp_photo_loss_gradient(const float *image, const float *target, int C, int W, int H, float lambda_dssim,
                           const float *grad_loss, float *grad_image, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!grad_image) return fail(VP_EINVAL, "null pointer argument (grad_image)");
    if (!std::isfinite(lambda_dssim) || lambda_dssim < 0.0f || lambda_dssim > 1.0f)
        return fail(VP_EINVAL, "lambda_dssim = %g outside [0, 1]", (double)lambda_dssim);
    if (int rc = photo_check(image, target, C, W, H, true, workspace, workspace_bytes)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const double n = (double)C * (double)W * (double)H;
    const float a = (float)((1.0 - (double)lambda_dssim) / n), b = (float)((double)lambda_dssim / n);
    hipLaunchKernelGGL(k_photo_loss_gradient, dim3((unsigned)photo_tiles_x(W), (unsigned)photo_tiles_x(H), (unsigned)C),
                       dim3(PHOTO_THREADS), 0, stream, image, target, W, H, (const float *)workspace, a, b, grad_loss, grad_image);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

// ------------------------------------------------------------------------------------------------
// Adaptive density control (vp_densify.h).  Every check is host arithmetic and comes before the first launch.
// ------------------------------------------------------------------------------------------------
int vp_densify_accumulate(const float *grad_screen, int64_t n_gaussians, int W, int H, float scale, const float *means,
                          const float *quats, const float *scales, const float *viewmat, float fx, float fy, float cx, float cy,
                          float eps2d, float *grad_accum, int32_t *denom, float *max_radius, const void *workspace,
                          size_t workspace_bytes, void *stream_)
{
    if (int rc = check_count("n_gaussians", n_gaussians)) return rc;
    if (int rc = check_image(W, H)) return rc;
    if (n_gaussians > 0 && (!grad_screen || !grad_accum || !denom))
        return fail(VP_EINVAL, "null pointer argument (grad_screen, grad_accum or denom)");
    if (!std::isfinite(scale)) return fail(VP_EINVAL, "scale = %g is not finite", (double)scale);
    SplatCam cam = {};
    if (max_radius) {
        if (n_gaussians > 0 && (!means || !quats || !scales))
            return fail(VP_EINVAL, "null pointer argument (means, quats or scales, needed by max_radius)");
        if (int rc = splat_check_camera(viewmat, fx, fy, cx, cy, cam)) return rc;
        if (!(eps2d >= 0.0f) || !std::isfinite(eps2d)) return fail(VP_EINVAL, "need a finite eps2d >= 0 (got %g)", (double)eps2d);
        cam.eps2d = eps2d;
        cam.W = W; cam.H = H;
    }
    SplatLayout l;
    if (int rc = open_workspace(workspace, workspace_bytes, n_gaussians, W, H, 0, l)) return rc;
    if (n_gaussians == 0) return VP_OK;
    const double hw = 0.5 * (double)W, hh = 0.5 * (double)H;
    hipLaunchKernelGGL(k_densify_accumulate, dim3((unsigned)((n_gaussians + DENSIFY_THREADS - 1) / DENSIFY_THREADS)),
                       dim3(DENSIFY_THREADS), 0, (hipStream_t)stream_, grad_screen, (long long)n_gaussians, hw * hw, hh * hh,
                       (double)scale, means, quats, scales, cam, l.count, grad_accum, (int *)denom, max_radius);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

size_t vp_densify_plan_workspace_bytes(int64_t n_gaussians)
{
    if (n_gaussians < 0 || n_gaussians > DENSIFY_MAX_N) return 0;
    DensifyLayout l;
    return densify_layout(n_gaussians, l) ? l.bytes : 0;
}

int vp_densify_plan(const float *grad_accum, const int32_t *denom, const float *max_radius, const float *scales,
                    const float *opacities, int64_t n_gaussians, float grad_threshold, float size_threshold, float min_opacity,
                    float max_screen_size, float max_world_size, int32_t *src, uint8_t *kind, int64_t *counts, void *workspace,
                    size_t workspace_bytes, void *stream_)
{
    if (n_gaussians < 0 || n_gaussians > DENSIFY_MAX_N)
        return fail(VP_EINVAL, "n_gaussians = %lld outside [0, 2^30]", (long long)n_gaussians);
    if (!counts) return fail(VP_EINVAL, "null pointer argument (counts)");
    if (n_gaussians > 0 && (!grad_accum || !denom || !scales || !opacities || !src || !kind))
        return fail(VP_EINVAL, "null pointer argument (grad_accum, denom, scales, opacities, src or kind)");
    if (!(grad_threshold > 0.0f)) return fail(VP_EINVAL, "grad_threshold must be > 0 (got %g)", (double)grad_threshold);
    if (std::isnan(size_threshold) || std::isnan(min_opacity) || std::isnan(max_screen_size) || std::isnan(max_world_size))
        return fail(VP_EINVAL, "size_threshold, min_opacity, max_screen_size and max_world_size must not be NaN");
    DensifyLayout l;
    if (int rc = open_workspace(workspace, workspace_bytes, l, [&] { return densify_layout(n_gaussians, l); })) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    char *ws = (char *)workspace;
    unsigned char *flags = (unsigned char *)(ws + l.flags);
    DensifyCnt *sums = (DensifyCnt *)(ws + l.sums);
    const unsigned grid = (unsigned)((std::max<long long>(n_gaussians, 1) + DENSIFY_THREADS - 1) / DENSIFY_THREADS);
    if (n_gaussians > 0) {
        const DensifyRule rule = {grad_threshold, size_threshold, min_opacity, max_screen_size, max_world_size};
        hipLaunchKernelGGL(k_densify_decide, dim3(grid), dim3(DENSIFY_THREADS), 0, stream, grad_accum, (const int *)denom,
                           max_radius, scales, opacities, (long long)n_gaussians, rule, flags);
        VP_HIP(hipGetLastError());
        size_t tmp = l.scan_bytes;
        VP_HIP(rocprim::inclusive_scan(ws + l.scan_tmp, tmp, DensifyFlagIter(flags, DensifyWiden()), sums, (size_t)n_gaussians,
                                       DensifyPlus(), stream));
    }
    hipLaunchKernelGGL(k_densify_emit, dim3(grid), dim3(DENSIFY_THREADS), 0, stream, (const unsigned char *)flags,
                       (const DensifyCnt *)sums, (long long)n_gaussians, (int *)src, (unsigned char *)kind, (long long *)counts);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

static int densify_check_rows(const int32_t *src, const uint8_t *kind, const int64_t *counts, int64_t n_src, int64_t n_out)
{
    if (!counts) return fail(VP_EINVAL, "null pointer argument (counts)");
    if (n_src < 0 || n_src > DENSIFY_MAX_N) return fail(VP_EINVAL, "n_src = %lld outside [0, 2^30]", (long long)n_src);
    if (n_out < 0 || n_out > 2 * n_src) return fail(VP_EINVAL, "n_out = %lld outside [0, 2 n_src]", (long long)n_out);
    if (n_out > 0 && (!src || !kind)) return fail(VP_EINVAL, "null pointer argument (src or kind)");
    return VP_OK;
}

int vp_densify_rows(const vp_densify_array *arrays, int n_arrays, const int32_t *src, const uint8_t *kind,
                    const int64_t *counts, int64_t n_src, int64_t n_out, int32_t *status, void *stream_)
{
    if (!arrays) return fail(VP_EINVAL, "null pointer argument (arrays)");
    if (n_arrays < 1 || n_arrays > VP_DENSIFY_MAX_ARRAYS)
        return fail(VP_EINVAL, "n_arrays = %d outside [1, %d]", n_arrays, VP_DENSIFY_MAX_ARRAYS);
    if (int rc = densify_check_rows(src, kind, counts, n_src, n_out)) return rc;
    DensifyRowsArgs A = {};
    A.n = n_arrays;
    int blocks = 0;
    for (int a = 0; a < n_arrays; ++a) {
        const vp_densify_array &d = arrays[a];
        if (d.width < 1 || d.width > VP_DENSIFY_MAX_WIDTH)
            return fail(VP_EINVAL, "array %d: width = %d outside [1, %d]", a, d.width, VP_DENSIFY_MAX_WIDTH);
        if (d.src_stride < d.width || d.dst_stride < d.width)
            return fail(VP_EINVAL, "array %d: a stride (%lld, %lld) is below the width %d", a, (long long)d.src_stride,
                        (long long)d.dst_stride, d.width);
        if (d.fill != VP_DENSIFY_COPY && d.fill != VP_DENSIFY_ZERO)
            return fail(VP_EINVAL, "array %d: fill = %d is neither VP_DENSIFY_COPY nor VP_DENSIFY_ZERO", a, d.fill);
        if ((n_src > 0 && !d.src) || (n_out > 0 && !d.dst)) return fail(VP_EINVAL, "array %d: null pointer (src or dst)", a);
        if (((uintptr_t)d.src | (uintptr_t)d.dst) & 3) return fail(VP_EINVAL, "array %d: src and dst must be 4-byte aligned", a);
        const bool vec = d.width % 4 == 0 && d.src_stride % 4 == 0 && d.dst_stride % 4 == 0 &&
                         (((uintptr_t)d.src | (uintptr_t)d.dst) & 15) == 0;
        A.a[a] = d;
        A.vec[a] = vec;
        A.lg[a] = (unsigned char)densify_pick_lanes(vec ? d.width / 4 : d.width);
        const long long rpb = (long long)(DENSIFY_THREADS >> A.lg[a]) * DENSIFY_ROWS_IN_FLIGHT;   // rows per workgroup and round
        A.blk_start[a] = blocks;
        blocks += (int)std::min<long long>(std::max<long long>((n_out + rpb - 1) / rpb, 1), DENSIFY_MAX_BLOCKS);
    }
    A.blk_start[n_arrays] = blocks;
    hipLaunchKernelGGL(k_densify_rows, dim3((unsigned)blocks), dim3(DENSIFY_THREADS), 0, (hipStream_t)stream_, A,
                       (const int *)src, (const unsigned char *)kind, (const long long *)counts, (long long)n_src,
                       (long long)n_out, (int *)status);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

int vp_densify_split(const float *means, const float *quats, const float *log_scales, int64_t n_src, const int32_t *src,
                     const uint8_t *kind, const int64_t *counts, int64_t n_out, uint64_t seed, float *out_means,
                     float *out_log_scales, int32_t *status, void *stream_)
{
    if (int rc = densify_check_rows(src, kind, counts, n_src, n_out)) return rc;
    if (n_src > 0 && (!means || !quats || !log_scales))
        return fail(VP_EINVAL, "null pointer argument (means, quats or log_scales)");
    if (n_out > 0 && (!out_means || !out_log_scales)) return fail(VP_EINVAL, "null pointer argument (out_means or out_log_scales)");
    const unsigned grid = (unsigned)((std::max<long long>(n_out, 1) + DENSIFY_THREADS - 1) / DENSIFY_THREADS);
    hipLaunchKernelGGL(k_densify_split, dim3(grid), dim3(DENSIFY_THREADS), 0, (hipStream_t)stream_, means, quats, log_scales,
                       (long long)n_src, (const int *)src, (const unsigned char *)kind, (const long long *)counts,
                       (long long)n_out, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), out_means, out_log_scales,
                       (int *)status);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

// ------------------------------------------------------------------------------------------------
// View-dependent colour (vp_sh.h, declared in voxproj_ext.h).  Every check is host arithmetic and comes before the launch.
// ------------------------------------------------------------------------------------------------
static int sh_check(const char *fn, const float *means, const float *campos, int64_t n, int degree, int max_degree)
{
    if (n < 0 || n > SH_MAX_N) return fail(VP_EINVAL, "%s: n = %lld outside [0, 2^31 - 1]", fn, (long long)n);
    if (degree < 0 || degree > max_degree || max_degree > SH_MAX_DEGREE)
        return fail(VP_EINVAL, "%s: need 0 <= degree <= max_degree <= %d (got %d, %d)", fn, SH_MAX_DEGREE, degree, max_degree);
    if (!campos) return fail(VP_EINVAL, "%s: null campos", fn);
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(campos[k])) return fail(VP_EINVAL, "%s: campos[%d] is not finite", fn, k);
    if (n > 0 && !means) return fail(VP_EINVAL, "%s: null pointer argument (means)", fn);
    return VP_OK;
}

static bool sh_misaligned(std::initializer_list<const void *> ptrs)
{
    uintptr_t bits = 0;
    for (const void *p : ptrs) bits |= (uintptr_t)p;
    return (bits & 3) != 0;
}

int vp_sh_colors(const float *f_dc, const float *f_rest, const float *means, const float *campos, int64_t n, int degree,
                 int max_degree, float *colors, uint8_t *clamped, void *stream_)
{
    if (int rc = sh_check("vp_sh_colors", means, campos, n, degree, max_degree)) return rc;
    if (n > 0 && (!f_dc || !colors || (degree > 0 && !f_rest)))
        return fail(VP_EINVAL, "vp_sh_colors: null pointer argument (f_dc, colors, or f_rest with degree > 0)");
    if (sh_misaligned({f_dc, f_rest, means, colors})) return fail(VP_EINVAL, "vp_sh_colors: the float arrays must be 4-byte aligned");
    if (n == 0) return VP_OK;
    const dim3 grid((unsigned)((n + SH_THREADS - 1) / SH_THREADS)), block(SH_THREADS);
    const int row = 3 * (sh_coeffs(max_degree) - 1);
    hipStream_t stream = (hipStream_t)stream_;
#define VP_SH_FORWARD(D)                                                                                                 \
    hipLaunchKernelGGL(k_sh_colors<D>, grid, block, 0, stream, f_dc, f_rest, means, campos[0], campos[1], campos[2],     \
                       (long long)n, row, colors, (unsigned char *)clamped)
    switch (degree) {
    case 0: VP_SH_FORWARD(0); break;
    case 1: VP_SH_FORWARD(1); break;
    case 2: VP_SH_FORWARD(2); break;
    default: VP_SH_FORWARD(3); break;
    }
#undef VP_SH_FORWARD
    VP_HIP(hipGetLastError());
    return VP_OK;
}

int vp_sh_colors_backward(const float *f_dc, const float *f_rest, const float *means, const float *campos, int64_t n,
                          int degree, int max_degree, const float *grad_colors, const uint8_t *clamped, float *grad_dc,
                          float *grad_rest, float *grad_means, void *stream_)
{
    (void)f_dc;                              // Y_0 is a constant: the adjoint never needs f_dc
    if (int rc = sh_check("vp_sh_colors_backward", means, campos, n, degree, max_degree)) return rc;
    if (n > 0 && (!grad_colors || !clamped)) return fail(VP_EINVAL, "vp_sh_colors_backward: null pointer argument (grad_colors or clamped)");
    if (n > 0 && grad_means && degree > 0 && !f_rest)
        return fail(VP_EINVAL, "vp_sh_colors_backward: grad_means with degree > 0 needs f_rest");
    if (sh_misaligned({f_rest, means, grad_colors, grad_dc, grad_rest, grad_means}))
        return fail(VP_EINVAL, "vp_sh_colors_backward: the float arrays must be 4-byte aligned");
    if (n == 0 || (!grad_dc && !grad_rest && !grad_means)) return VP_OK;
    const dim3 grid((unsigned)((n + SH_THREADS - 1) / SH_THREADS)), block(SH_THREADS);
    const int row = 3 * (sh_coeffs(max_degree) - 1);
    hipStream_t stream = (hipStream_t)stream_;
    const unsigned char *cl = (const unsigned char *)clamped;
#define VP_SH_BACKWARD(D, M)                                                                                             \
    hipLaunchKernelGGL((k_sh_colors_backward<D, M>), grid, block, 0, stream, f_rest, means, campos[0], campos[1],        \
                       campos[2], (long long)n, row, grad_colors, cl, grad_dc, grad_rest, grad_means)
    switch (2 * degree + (grad_means ? 1 : 0)) {
    case 0: VP_SH_BACKWARD(0, false); break;
    case 1: VP_SH_BACKWARD(0, true); break;
    case 2: VP_SH_BACKWARD(1, false); break;
    case 3: VP_SH_BACKWARD(1, true); break;
    case 4: VP_SH_BACKWARD(2, false); break;
    case 5: VP_SH_BACKWARD(2, true); break;
    case 6: VP_SH_BACKWARD(3, false); break;
    default: VP_SH_BACKWARD(3, true); break;
    }
#undef VP_SH_BACKWARD
    VP_HIP(hipGetLastError());
    return VP_OK;
}

// ------------------------------------------------------------------------------------------------
// Triangle-mesh rasterizer (vp_mesh.h, declared in voxproj_mesh.h).  Every check is host arithmetic and comes before
// open_workspace (rocprim's scratch sizes depend on the device) and before any launch.
// ------------------------------------------------------------------------------------------------
static int mesh_check_shape(int64_t n_faces, int W, int H, int64_t capacity)
{
    if (int rc = check_count("n_faces", n_faces)) return rc;
    if (int rc = check_image(W, H)) return rc;
    return check_count("capacity", capacity);
}

size_t vp_mesh_workspace_bytes(int64_t n_faces, int W, int H, int64_t capacity)
{
    if (n_faces < 0 || n_faces > INT32_MAX || W < 1 || W > VP_MAX_WH || H < 1 || H > VP_MAX_WH || capacity < 0 ||
        capacity > INT32_MAX)
        return 0;
    MeshLayout l;
    return mesh_layout(nullptr, n_faces, W, H, capacity, l) ? l.bytes : 0;
}

int vp_mesh_project(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *viewmat,
                    float fx, float fy, float cx, float cy, int W, int H, float near_plane, float far_plane,
                    int64_t *n_isect, int32_t *counters, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (int rc = mesh_check_shape(n_faces, W, H, 0)) return rc;
    if (int rc = check_count("n_verts", n_verts)) return rc;
    if (n_faces > 0 && (!faces || (n_verts > 0 && !verts))) return fail(VP_EINVAL, "null pointer argument (verts or faces)");
    SplatCam sc;
    if (int rc = splat_check_camera(viewmat, fx, fy, cx, cy, sc)) return rc;
    if (!(near_plane > 0.0f) || !(far_plane > near_plane) || !std::isfinite(far_plane))
        return fail(VP_EINVAL, "need 0 < near < far, both finite (got %g %g)", (double)near_plane, (double)far_plane);
    MeshLayout l;
    if (int rc = open_workspace(workspace, workspace_bytes, n_faces, W, H, 0, l)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    MeshCam cam;
    for (int k = 0; k < 12; ++k) cam.r[k] = sc.r[k];
    cam.fx = fx; cam.fy = fy; cam.cx = cx; cam.cy = cy; cam.near_z = near_plane; cam.far_z = far_plane;
    cam.W = W; cam.H = H;
    hipLaunchKernelGGL(k_mesh_project, dim3((unsigned)l.n_blocks), dim3(256), 0, stream, verts, (long long)n_verts,
                       (const int *)faces, (long long)n_faces, cam, l.cam, l.rec, l.box, l.count, l.part);
    VP_HIP(hipGetLastError());
    if (counters) {
        hipLaunchKernelGGL(k_mesh_counters, dim3(1), dim3(256), 0, stream, l.part, l.n_blocks, (int *)counters);
        VP_HIP(hipGetLastError());
    }
    return tile_scan(l, n_faces, (long long *)n_isect, stream);
}

int vp_mesh_rasterize(const uint8_t *vertex_labels, const int32_t *faces, int64_t n_faces, int W, int H, int64_t capacity,
                      int32_t *face_ids, float *depth, uint8_t *labels, int32_t *status, void *workspace,
                      size_t workspace_bytes, void *stream_)
{
    if (int rc = mesh_check_shape(n_faces, W, H, capacity)) return rc;
    if (labels && n_faces > 0 && (!vertex_labels || !faces))
        return fail(VP_EINVAL, "null pointer argument (labels needs vertex_labels and faces)");
    MeshLayout l;
    if (int rc = open_workspace(workspace, workspace_bytes, n_faces, W, H, capacity, l)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = tile_sort(l, nullptr, 0, n_faces, capacity, status, stream)) return rc;
    hipLaunchKernelGGL(k_mesh_tiles, l.tile_grid(), dim3(SPLAT_THREADS), 0, stream, l.rec, l.vals1, l.ranges, l.total,
                       (long long)capacity, l.cam, (const int *)faces, (const unsigned char *)vertex_labels, (int *)face_ids,
                       depth, (unsigned char *)labels);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

// ------------------------------------------------------------------------------------------------
// Stage 2, the voxel grid of a Gaussian cloud (vp_grid.h, declared in voxproj_grid.h).  Every check is host arithmetic and
// comes before grid_layout (rocprim's scratch sizes depend on the device) and before any launch.
// ------------------------------------------------------------------------------------------------
int vp_ball_count(const float *pts_sorted, const int32_t *perm, const int32_t *cell_start, const double *grid_origin3,
                  double cell_size, int nx, int ny, int nz, const float *queries, int64_t M, double radius, const float *radii,
                  const float *point_normals, const float *query_normals, double min_dot, int32_t *count,
                  int32_t *consistent, void *stream_)
{
    if (!pts_sorted || !perm || !cell_start || !grid_origin3 || !queries || !count)
        return fail(VP_EINVAL, "null pointer argument (pts_sorted, perm, cell_start, grid_origin3, queries or count)");
    if (int rc = check_count("M", M)) return rc;
    if (!(cell_size > 0.0) || !std::isfinite(cell_size) || nx <= 0 || ny <= 0 || nz <= 0)
        return fail(VP_EINVAL, "bad grid (cell size %g, dims %d %d %d)", cell_size, nx, ny, nz);
    if ((long long)nx * ny * nz >= (1ll << 31)) return fail(VP_EINVAL, "the grid has >= 2^31 cells");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(grid_origin3[a])) return fail(VP_EINVAL, "grid_origin3[%d] is not finite", a);
    if (!radii && (!(radius >= 0.0) || !std::isfinite(radius)))
        return fail(VP_EINVAL, "radius = %g must be finite and >= 0", radius);
    if ((point_normals != nullptr) != (query_normals != nullptr))
        return fail(VP_EINVAL, "normals for only one side (point_normals and query_normals go together)");
    if (point_normals && !consistent) return fail(VP_EINVAL, "null pointer argument (consistent, with normals)");
    if (point_normals && std::isnan(min_dot)) return fail(VP_EINVAL, "min_dot is NaN");
    if (M == 0) return VP_OK;
    const dim3 grid((unsigned)((M + 255) / 256)), block(256);
    hipStream_t stream = (hipStream_t)stream_;
    auto launch = [&](auto normals) {
        hipLaunchKernelGGL(k_ball_count<decltype(normals)::value>, grid, block, 0, stream, pts_sorted, (const int *)perm,
                           (const int *)cell_start, grid_origin3[0], grid_origin3[1], grid_origin3[2], cell_size, nx, ny, nz,
                           queries, (long long)M, radius, radii, point_normals, query_normals, min_dot, (int *)count,
                           (int *)consistent);
    };
    if (point_normals) launch(std::true_type{});
    else launch(std::false_type{});
    VP_HIP(hipGetLastError());
    return VP_OK;
}

size_t vp_voxel_grid_workspace_bytes(int64_t N)
{
    if (N < 0 || N > INT32_MAX) return 0;
    GridLayout l;
    return grid_layout(N, l) ? l.bytes : 0;
}

int vp_voxel_grid(const float *points, const uint8_t *colors, const uint8_t *keep, int64_t N, double voxel_size,
                  float *centers, uint8_t *voxel_colors, int32_t *counts, int32_t *voxel_index, int32_t *point_voxel,
                  int32_t *n_voxels, float *min_corner, int32_t *status, void *workspace, size_t workspace_bytes,
                  void *stream_)
{
    if (int rc = check_count("N", N)) return rc;
    if (!(voxel_size > 0.0) || !std::isfinite(voxel_size) || !((float)voxel_size > 0.0f) || !std::isfinite((float)voxel_size))
        return fail(VP_EINVAL, "voxel_size = %g must be finite and > 0 (in float32 too)", voxel_size);
    if (!n_voxels || !min_corner) return fail(VP_EINVAL, "null pointer argument (n_voxels or min_corner)");
    if (N > 0 && (!points || !colors || !centers || !voxel_colors || !counts || !voxel_index || !point_voxel))
        return fail(VP_EINVAL, "null pointer argument (points, colors, centers, voxel_colors, counts, voxel_index or point_voxel)");
    GridLayout l;
    if (int rc = open_workspace(workspace, workspace_bytes, l, [&] { return grid_layout(N, l); })) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    char *ws = (char *)workspace;
    GridMeta *meta = (GridMeta *)(ws + l.meta);
    int *over = (int *)(ws + l.over), *total = (int *)(ws + l.total);
    unsigned long long *k0 = (unsigned long long *)(ws + l.keys0), *k1 = (unsigned long long *)(ws + l.keys1);
    int *v0 = (int *)(ws + l.vals0), *v1 = (int *)(ws + l.vals1);
    int *heads = (int *)(ws + l.heads), *rank = (int *)(ws + l.rank), *run_start = (int *)(ws + l.run_start);
    const dim3 per_point((unsigned)((std::max<int64_t>(N, 1) + 255) / 256)), block(256);
    VP_HIP(hipMemsetAsync(over, 0, sizeof(int), stream));
    hipLaunchKernelGGL(k_grid_min_part, dim3((unsigned)l.n_parts), block, 0, stream, points, (const unsigned char *)keep,
                       (long long)N, (float *)(ws + l.part_min), (int *)(ws + l.part_cnt));
    hipLaunchKernelGGL(k_grid_min_final, dim3(1), dim3(GRID_PARTS), 0, stream, (const float *)(ws + l.part_min),
                       (const int *)(ws + l.part_cnt), l.n_parts, meta);
    VP_HIP(hipGetLastError());
    if (N > 0) {
        hipLaunchKernelGGL(k_grid_keys, per_point, block, 0, stream, points, (const unsigned char *)keep, (long long)N,
                           (float)voxel_size, (const GridMeta *)meta, k0, v0, over);
        VP_HIP(hipGetLastError());
        size_t tmp = l.sort_bytes;
        VP_HIP(rocprim::radix_sort_pairs(ws + l.sort_tmp, tmp, k0, k1, v0, v1, (size_t)N, 0u, 64u, stream));
        hipLaunchKernelGGL(k_grid_heads, per_point, block, 0, stream, (const unsigned long long *)k1, (long long)N, heads);
        VP_HIP(hipGetLastError());
        tmp = l.scan_bytes;
        VP_HIP(rocprim::inclusive_scan(ws + l.scan_tmp, tmp, (const int *)heads, rank, (size_t)N, rocprim::plus<int>(), stream));
    }
    hipLaunchKernelGGL(k_grid_total, dim3(1), dim3(1), 0, stream, (const int *)rank, (long long)N, (const GridMeta *)meta,
                       (const int *)over, total, (int *)n_voxels, min_corner, (int *)status);
    VP_HIP(hipGetLastError());
    if (N > 0) {
        hipLaunchKernelGGL(k_grid_points, per_point, block, 0, stream, (const unsigned long long *)k1, (const int *)v1,
                           (const int *)heads, (const int *)rank, (long long)N, (const int *)total, run_start,
                           (int *)point_voxel);
        // one thread per voxel; V <= N is on the device only, so the grid covers N and the surplus threads leave at once
        hipLaunchKernelGGL(k_grid_voxels, per_point, block, 0, stream, (const unsigned long long *)k1, (const int *)v1,
                           (const int *)run_start, (const int *)total, (const GridMeta *)meta, (const unsigned char *)colors,
                           voxel_size, centers, (unsigned char *)voxel_colors, (int *)counts, (int *)voxel_index);
        VP_HIP(hipGetLastError());
    }
    return VP_OK;
}

// ------------------------------------------------------------------------------------------------
// Label sums over a feature table (vp_cluster.h, declared in voxproj_cluster.h).  Every check is host arithmetic and comes
// before cluster_layout (rocprim's scratch sizes depend on the device) and before any launch.
// ------------------------------------------------------------------------------------------------
static int cluster_check_rows(const void *rows, int rows_f16, int64_t n_rows, int C, int64_t stride)
{
    if (int rc = check_count("n_rows", n_rows)) return rc;
    if (n_rows > 0 && !rows) return fail(VP_EINVAL, "null pointer argument (rows)");
    if (rows_f16 != 0 && rows_f16 != 1) return fail(VP_EINVAL, "rows_f16 = %d is neither 0 nor 1", rows_f16);
    if (C < 1 || C > CL_MAX_C) return fail(VP_EINVAL, "C = %d outside [1, %d]", C, CL_MAX_C);
    if (stride < C) return fail(VP_EINVAL, "stride %lld < C = %d", (long long)stride, C);
    return VP_OK;
}

int vp_row_inv_norms(const void *rows, int rows_f16, int64_t n_rows, int C, int64_t stride, float *inv, int32_t *status,
                     void *stream_)
{
    if (int rc = cluster_check_rows(rows, rows_f16, n_rows, C, stride)) return rc;
    if (!status || (n_rows > 0 && !inv)) return fail(VP_EINVAL, "null pointer argument (inv or status)");
    hipStream_t stream = (hipStream_t)stream_;
    VP_HIP(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), stream));
    if (n_rows == 0) return VP_OK;
    const bool vec16 = cluster_vec(rows, rows_f16, C, stride);
    with_flags([&](auto f16, auto vec, auto quarter) {
        constexpr int LPR = decltype(quarter)::value ? 16 : 64;
        const long long per_block = 4 * (64 / LPR);
        hipLaunchKernelGGL((k_row_inv_norms<decltype(f16)::value, decltype(vec)::value, LPR>),
                           dim3((unsigned)((n_rows + per_block - 1) / per_block)), dim3(256), 0, stream, rows, (long long)n_rows, C,
                           (long long)stride, inv, (int *)status);
    }, rows_f16 == 1, vec16, C <= 16 * (vec16 ? (rows_f16 ? 8 : 4) : 1));      // a quarter of a wavefront covers the row
    VP_HIP(hipGetLastError());
    return VP_OK;
}

size_t vp_label_sums_workspace_bytes(int64_t n_rows, int K, int C)
{
    if (n_rows < 0 || n_rows > INT32_MAX || K < 1 || K > CL_MAX_K || C < 1 || C > CL_MAX_C) return 0;
    ClusterLayout l;
    return cluster_layout(n_rows, K, C, 0, l) ? l.bytes : 0;
}

int vp_label_sums(const void *rows, int rows_f16, int64_t n_rows, int C, int64_t stride, const int32_t *labels,
                  const float *row_scale, int K, int64_t part_rows, float *sums, int32_t *counts, int32_t *status,
                  void *workspace, size_t workspace_bytes, void *stream_)
{
    if (int rc = cluster_check_rows(rows, rows_f16, n_rows, C, stride)) return rc;
    if (K < 1 || K > CL_MAX_K) return fail(VP_EINVAL, "K = %d outside [1, %d]", K, CL_MAX_K);
    if (part_rows < 0) return fail(VP_EINVAL, "part_rows = %lld is negative (0 = the default)", (long long)part_rows);
    if (!sums || !counts || !status || (n_rows > 0 && !labels))
        return fail(VP_EINVAL, "null pointer argument (labels, sums, counts or status)");
    ClusterLayout l;
    cluster_layout_own(n_rows, K, C, part_rows, l);
    if (int rc = check_buffer(workspace, "workspace")) return rc;
    if (int rc = check_size(workspace_bytes, l.own_bytes, "workspace")) return rc;      // before the device is asked anything
    if (int rc = open_workspace(workspace, workspace_bytes, l, [&] { return cluster_layout(n_rows, K, C, part_rows, l); })) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    char *ws = (char *)workspace;
    unsigned *k0 = (unsigned *)(ws + l.keys0), *k1 = (unsigned *)(ws + l.keys1);
    int *v0 = (int *)(ws + l.vals0), *v1 = (int *)(ws + l.vals1);
    int *run_start = (int *)(ws + l.run_start), *n_parts = (int *)(ws + l.n_parts), *part_off = (int *)(ws + l.part_off);
    float *partials = (float *)(ws + l.partials);
    VP_HIP(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), stream));
    if (n_rows > 0) {
        hipLaunchKernelGGL(k_label_keys, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, stream, (const int *)labels,
                           (long long)n_rows, K, k0, v0, (int *)status);
        VP_HIP(hipGetLastError());
        size_t tmp = l.sort_bytes;
        VP_HIP(rocprim::radix_sort_pairs(ws + l.sort_tmp, tmp, k0, k1, v0, v1, (size_t)n_rows, 0u, (unsigned)l.bits, stream));
    }
    hipLaunchKernelGGL(k_label_runs, dim3((unsigned)(K / 256 + 1)), dim3(256), 0, stream, (const unsigned *)k1, (int)n_rows, K,
                       l.R, run_start, n_parts);
    VP_HIP(hipGetLastError());
    size_t tmp = l.scan_bytes;
    VP_HIP(rocprim::exclusive_scan(ws + l.scan_tmp, tmp, (const int *)n_parts, part_off, 0, (size_t)(K + 1), rocprim::plus<int>(),
                                   stream));
    if (l.max_parts > 0) {
        const bool vec = cluster_vec(rows, rows_f16, C, stride);
        const int per_slot = 64 * (vec ? (rows_f16 ? 8 : 4) : 1), slots = (C + per_slot - 1) / per_slot;
        const dim3 grid((unsigned)((l.max_parts + CL_WAVES - 1) / CL_WAVES)), block(64 * CL_WAVES);
        with_flags([&](auto f16, auto v) {
            with_step<1, 2, 4>(slots, [&](auto ns) {
                hipLaunchKernelGGL((k_label_part_sums<decltype(f16)::value, decltype(v)::value, decltype(ns)::value>), grid, block, 0,
                                   stream, rows, (long long)stride, C, (const int *)v1, row_scale, (const int *)run_start,
                                   (const int *)part_off, K, l.R, l.max_parts, partials);
            });
        }, rows_f16 == 1, vec);
        VP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_label_combine, dim3((unsigned)K, (unsigned)((C + 63) / 64)), dim3(64), 0, stream, (const float *)partials,
                       (const int *)run_start, (const int *)part_off, C, sums, (int *)counts);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

// ------------------------------------------------------------------------------------------------
// The code book of global instance labels (vp_codebook.h).  Every check is host arithmetic and comes before the first launch.
// ------------------------------------------------------------------------------------------------
size_t vp_codebook_workspace_bytes(int D, int K, int W, int H)
{
    if (D < 1 || D > CB_MAX_D || K < 1 || K > CB_MAX_K || W < 1 || W > VP_MAX_WH || H < 1 || H > VP_MAX_WH) return 0;
    // sized for min(tiles, 256) workgroups, which the plan never exceeds: the size does not shrink when the image grows
    return cb_carve(nullptr, D, K, (int)std::min<long long>(cb_plan(W, H).tiles, CB_GRID)).bytes;
}

static int cb_check(const float *image, int D, int W, int H, const int32_t *ids, const float *codebook, int K,
                    const void *workspace, size_t workspace_bytes)
{
    if (!image || !ids || !codebook) return fail(VP_EINVAL, "null pointer argument (image, ids or codebook)");
    if (D < 1 || D > CB_MAX_D) return fail(VP_EINVAL, "D = %d outside [1, %d]", D, CB_MAX_D);
    if (K < 1 || K > CB_MAX_K) return fail(VP_EINVAL, "K = %d outside [1, %d]", K, CB_MAX_K);
    if (int rc = check_image(W, H)) return rc;
    return check_workspace(workspace, workspace_bytes, vp_codebook_workspace_bytes(D, K, W, H));
}

int vp_codebook_assoc(const float *image, int D, int W, int H, const int32_t *ids, int ignore_id, const float *codebook, int K,
                      double *score, int32_t *id_pixels, int32_t *pred, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!score || !id_pixels) return fail(VP_EINVAL, "null pointer argument (score or id_pixels)");
    if (int rc = cb_check(image, D, W, H, ids, codebook, K, workspace, workspace_bytes)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const CbPlan plan = cb_plan(W, H);
    const CbWs w = cb_carve(workspace, D, K, plan.G);
    hipError_t attr_rc = hipSuccess;
    with_step<16, 32, 64>(D, [&](auto dp) {
        constexpr int DP = decltype(dp)::value;
        // code book and probability tile pass 64 KiB of the CU's 160: said once per variant
        static hipError_t lds_attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_codebook_assoc<DP>),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)cb_assoc_lds(DP, CB_MAX_K));
        if (lds_attr != hipSuccess) {
            attr_rc = lds_attr;
            return;
        }
        hipLaunchKernelGGL(k_codebook_assoc<DP>, dim3(plan.G), dim3(CB_THREADS), cb_assoc_lds(DP, K), stream, image, D, plan.n, ids,
                           ignore_id, codebook, K, plan.tiles, plan.per, w.tab, w.touched, w.cnt, pred);
        hipLaunchKernelGGL(k_codebook_score, dim3(CB_IDS), dim3(CB_THREADS), 0, stream, K, plan.G, (const float *)w.tab,
                           (const int *)w.touched, (const int *)w.cnt, score, id_pixels);
    });
    VP_HIP(attr_rc);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

int vp_codebook_loss(const float *image, int D, int W, int H, const int32_t *ids, int ignore_id, const float *conf,
                     float conf_min, const float *codebook, int K, const int32_t *assign, double *stats, float *grad_cls,
                     float *grad_cluster, float *pixel_loss, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!assign || !stats || !grad_cls || !grad_cluster)
        return fail(VP_EINVAL, "null pointer argument (assign, stats, grad_cls or grad_cluster)");
    if (!std::isfinite(conf_min)) return fail(VP_EINVAL, "conf_min = %g must be finite", (double)conf_min);
    if (int rc = cb_check(image, D, W, H, ids, codebook, K, workspace, workspace_bytes)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const CbPlan plan = cb_plan(W, H);
    const CbWs w = cb_carve(workspace, D, K, plan.G);
    hipError_t attr_rc = hipSuccess;
    with_step<16, 32, 64>(D, [&](auto dp) {
        constexpr int DP = decltype(dp)::value;
        static hipError_t lds_attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_codebook_loss<DP>),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)cb_loss_lds(DP, CB_MAX_K));
        if (lds_attr != hipSuccess) {
            attr_rc = lds_attr;
            return;
        }
        hipLaunchKernelGGL(k_codebook_loss<DP>, dim3(plan.G), dim3(CB_THREADS), cb_loss_lds(DP, K), stream, image, D, plan.n, ids,
                           ignore_id, conf, conf_min, codebook, K, assign, plan.tiles, plan.per, w.gcls, w.gclu, w.dpart,
                           pixel_loss);
        hipLaunchKernelGGL(k_codebook_finish, dim3((K * D + CB_THREADS - 1) / CB_THREADS + 1), dim3(CB_THREADS), 0, stream, K * D,
                           plan.G, (const float *)w.gcls, (const float *)w.gclu, (const double *)w.dpart, grad_cls, grad_cluster,
                           stats);
    });
    VP_HIP(attr_rc);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

// ------------------------------------------------------------------------------------------------
// k nearest other points (vp_knn.h) and the neighbourhood regulariser (vp_reg3d.h).  Every check is host arithmetic and
// comes before the first launch.
// ------------------------------------------------------------------------------------------------
int vp_knn_points(const float *pts_sorted, const int32_t *perm, const int32_t *cell_start, const double *grid_origin3,
                  double cell_size, int nx, int ny, int nz, const float *queries, const int32_t *self_index, int64_t M, int k,
                  int32_t *nbr_idx, double *nbr_d2, void *stream_)
{
    if (!pts_sorted || !perm || !cell_start || !grid_origin3 || !queries || !nbr_idx)
        return fail(VP_EINVAL, "null pointer argument (pts_sorted, perm, cell_start, grid_origin3, queries or nbr_idx)");
    if (!(cell_size > 0.0) || nx <= 0 || ny <= 0 || nz <= 0 || M < 0) return fail(VP_EINVAL, "bad grid or query count");
    if ((long long)nx * ny * nz >= (1ll << 31)) return fail(VP_EINVAL, "the grid has >= 2^31 cells");
    if (k < 1 || k > KNN_MAX_K) return fail(VP_EINVAL, "k = %d outside [1, %d]", k, KNN_MAX_K);
    if (M * (int64_t)k >= (1ll << 40)) return fail(VP_EINVAL, "M k = %lld is too large", (long long)(M * k));
    if (M == 0) return VP_OK;
    const dim3 grid((unsigned)((M + 255) / 256)), block(256);
    hipStream_t stream = (hipStream_t)stream_;
    auto launch = [&](auto kc) {
        hipLaunchKernelGGL(k_knn_points<decltype(kc)::value>, grid, block, 0, stream, pts_sorted, (const int *)perm,
                           (const int *)cell_start, grid_origin3[0], grid_origin3[1], grid_origin3[2], cell_size, nx, ny, nz,
                           queries, (const int *)self_index, (long long)M, k, (int *)nbr_idx, nbr_d2);
    };
    if (k == 1) launch(std::integral_constant<int, 1>{});
    else if (k <= 4) launch(std::integral_constant<int, 4>{});
    else if (k <= 8) launch(std::integral_constant<int, 8>{});
    else launch(std::integral_constant<int, 15>{});
    VP_HIP(hipGetLastError());
    return VP_OK;
}

size_t vp_neighbor_kl_workspace_bytes(int64_t S)
{
    if (S < 0 || S >= (1ll << 31)) return 0;
    return align256((size_t)std::max<int64_t>(S, 1) * sizeof(float)) + align256(KL_PARTS * sizeof(double));
}

// the checks both calls share; *G: the lanes per row
static int kl_check(const float *logits, int64_t N, int P, int64_t row_stride, const int32_t *samples, int64_t S,
                    const int32_t *nbr, int k, const float *row_lse, int lanes, int *G)
{
    if (!logits || !row_lse) return fail(VP_EINVAL, "null pointer argument (logits or row_lse)");
    if (N < 1 || N >= (1ll << 31)) return fail(VP_EINVAL, "N = %lld outside [1, 2^31)", (long long)N);
    if (P < 1 || P > KL_MAX_P) return fail(VP_EINVAL, "P = %d outside [1, %d]", P, KL_MAX_P);
    if (row_stride < P) return fail(VP_EINVAL, "row stride %lld below P = %d", (long long)row_stride, P);
    if (k < 2 || k > KL_MAX_K) return fail(VP_EINVAL, "k = %d outside [2, %d] (k counts the point itself)", k, KL_MAX_K);
    if (S < 0 || S * (int64_t)(k - 1) >= (1ll << 31)) return fail(VP_EINVAL, "S = %lld: S (k - 1) outside [0, 2^31)", (long long)S);
    if (!samples && S != N) return fail(VP_EINVAL, "without a sample list S = %lld must be N = %lld", (long long)S, (long long)N);
    if (S > 0 && !nbr) return fail(VP_EINVAL, "null pointer argument (the neighbour table)");
    *G = lanes ? lanes : kl_pick_lanes(P);
    if (*G < 4 || *G > 64 || (*G & (*G - 1)) || (P + *G - 1) / *G > 4)
        return fail(VP_EINVAL, "lanes = %d: a power of two in [4, 64] with at most four channels of P = %d per lane (0: chosen here)",
                    lanes, P);
    return VP_OK;
}

int vp_neighbor_kl(const float *logits, int64_t N, int P, int64_t row_stride, const int32_t *samples, int64_t S,
                   const int32_t *nbr, int k, float *row_lse, float *sample_loss, double *stats, int lanes, void *workspace,
                   size_t workspace_bytes, void *stream_)
{
    int G = 0;
    if (!stats) return fail(VP_EINVAL, "null pointer argument (stats)");
    if (int rc = kl_check(logits, N, P, row_stride, samples, S, nbr, k, row_lse, lanes, &G)) return rc;
    if (int rc = check_workspace(workspace, workspace_bytes, vp_neighbor_kl_workspace_bytes(S))) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    float *sl = sample_loss ? sample_loss : (float *)workspace;
    double *part = (double *)((char *)workspace + align256((size_t)std::max<int64_t>(S, 1) * sizeof(float)));
    const int per = KL_THREADS / G;
    with_step<1, 2, 4>(kl_cpl(P, G), [&](auto cpl) {
        constexpr int CPL = decltype(cpl)::value;
        hipLaunchKernelGGL(k_kl_lse<CPL>, dim3((unsigned)((N + per - 1) / per)), dim3(KL_THREADS), 0, stream, logits,
                           (long long)row_stride, (long long)N, P, G, row_lse);
        if (S > 0)
            hipLaunchKernelGGL(k_kl_forward<CPL>, dim3((unsigned)((S + per - 1) / per)), dim3(KL_THREADS), 0, stream, logits,
                               (long long)row_stride, (long long)N, P, G, (const int *)samples, (long long)S, (const int *)nbr,
                               k - 1, (const float *)row_lse, sl);
    });
    hipLaunchKernelGGL(k_kl_sum1, dim3(KL_PARTS), dim3(KL_THREADS), 0, stream, (const float *)sl, (long long)S, part);
    hipLaunchKernelGGL(k_kl_sum2, dim3(1), dim3(64), 0, stream, (const double *)part, (long long)S, stats);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

int vp_neighbor_kl_gradient(const float *logits, int64_t N, int P, int64_t row_stride, const int32_t *samples, int64_t S,
                            const int32_t *nbr, int k, const float *row_lse, const int32_t *rev_start, const int32_t *rev_entry,
                            const int32_t *smp_start, const int32_t *smp_entry, double scale, const float *grad_loss,
                            float *grad_logits, int64_t grad_stride, int lanes, void *stream_)
{
    int G = 0;
    if (!grad_logits || !rev_start) return fail(VP_EINVAL, "null pointer argument (grad_logits or rev_start)");
    if (int rc = kl_check(logits, N, P, row_stride, samples, S, nbr, k, row_lse, lanes, &G)) return rc;
    if (S > 0 && !rev_entry) return fail(VP_EINVAL, "null pointer argument (rev_entry)");
    if (samples && (!smp_start || (S > 0 && !smp_entry))) return fail(VP_EINVAL, "a sample list needs smp_start and smp_entry");
    if (grad_stride < P) return fail(VP_EINVAL, "gradient row stride %lld below P = %d", (long long)grad_stride, P);
    if (!std::isfinite(scale)) return fail(VP_EINVAL, "scale = %g must be finite", scale);
    const double coef = S > 0 ? scale / ((double)S * (double)k * (double)P) : 0.0;
    const int per = KL_THREADS / G;
    with_step<1, 2, 4>(kl_cpl(P, G), [&](auto cpl) {
        constexpr int CPL = decltype(cpl)::value;
        hipLaunchKernelGGL(k_kl_gradient<CPL>, dim3((unsigned)((N + per - 1) / per)), dim3(KL_THREADS), 0, (hipStream_t)stream_,
                           logits, (long long)row_stride, (long long)N, P, G, (const int *)samples, (long long)S,
                           (const int *)nbr, k - 1, row_lse, (const int *)rev_start, (const int *)rev_entry,
                           (const int *)smp_start, (const int *)smp_entry, coef, grad_loss, grad_logits, (long long)grad_stride);
    });
    VP_HIP(hipGetLastError());
    return VP_OK;
}

long long vp_workspace_table_builds(const void *workspace)
{
    WsState *rec = ws_state(workspace, false);
    return rec ? rec->builds : 0;
}

int vp_workspace_create(void *workspace, size_t workspace_bytes)
{
    if (!workspace) return fail(VP_EINVAL, "null workspace");
    if ((uintptr_t)workspace & 255) return fail(VP_EWORKSPACE, "workspace must be 256-byte aligned");
    if (workspace_bytes < 2 * align256(ST_WORDS * sizeof(int))) return fail(VP_EWORKSPACE, "workspace has %zu bytes, need at least %zu", workspace_bytes, 2 * align256(ST_WORDS * sizeof(int)));
    ws_forget(workspace);            // whatever this address was before
    (void)ws_state(workspace, true); // a new record, a new generation
    return VP_OK;
}

int vp_workspace_set_option(void *workspace, int option, long long value)
{
    if (!workspace) return fail(VP_EINVAL, "null workspace");
    WsState *rec = ws_state(workspace, true);
    switch (option) {
    case VP_OPT_HEAVY_THRESHOLD: rec->opt_heavy_t = value > 0 ? value : -1; return VP_OK;
    case VP_OPT_MARCH_LDS_KB:
        // the reservation is dynamic LDS of k_first_hit, whose limit without a function attribute is 64 KiB: a larger value
        // would fail every launch on this workspace with a generic HIP error, surfacing (pipelined) only calls later
        if (value > 64) return fail(VP_EINVAL, "VP_OPT_MARCH_LDS_KB = %lld: the march's dynamic-LDS reservation is limited to 64 KiB (0 .. 64; < 0 = default)", value);
        rec->opt_march_lds_kb = value >= 0 ? value : -1; return VP_OK;
    case VP_OPT_ROW_BEGIN:       rec->opt_row_begin = value >= 0 ? value : -1; return VP_OK;
    case VP_OPT_ROW_END:         rec->opt_row_end = value >= 0 ? value : -1; return VP_OK;
    case VP_OPT_ONE_VIEW_GATHER: rec->opt_one_view = value >= 0 ? value : -1; return VP_OK;
    case VP_OPT_PART_PIXELS:     rec->opt_part_px = value > 0 ? value : -1; return VP_OK;
    case VP_OPT_ONE_VIEW_SPLIT:  rec->opt_one_view_split = value >= 0 ? value : -1; return VP_OK;
    default: return fail(VP_EINVAL, "unknown workspace option %d", option);
    }
}

int vp_workspace_release(void *workspace)
{
    ws_forget(workspace);
    return VP_OK;
}

}  // extern "C"

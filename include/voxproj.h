/*
 * voxproj.h -- C-ABI of the MI355X-native 2D -> sparse-voxel feature projector.
 *
 * Plain pointers and sizes only (no torch types).  Every entry point names the reference
 * interface it replaces; paths are relative to
 * /root/reference/cuda_project_image_to_sparse_voxel/ :
 *
 *   K.cu  = project_image_cuda_kernel.cu      W.cpp = project_image_cuda.cpp
 *   DPF   = debug_project_features.py         DPC   = debug_project_colors.py
 *   BSO   = build_sparse_occupancy.py         AGG   = aggregate_voxel_features_onthefly.py
 *
 * All device pointers must belong to the HIP device that is current on the calling thread.
 * Functions return VP_OK (0) or a negative VP_E* code; vp_last_error() gives the message for
 * the calling thread.  Nothing here falls back to a CPU path.
 */
#ifndef VOXPROJ_H
#define VOXPROJ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VP_ABI_VERSION 4   /* 4: the workspace carries part slots for split voxels (vp_workspace_bytes grew), vp_profile_read slot [3]
                              is k_combine_parts, counters [7] / [24] / [25], VP_OPT_PART_PIXELS, VP_OPT_ONE_VIEW_SPLIT; one-view calls
                              split large voxels too.  A caller built against 3 must re-query vp_workspace_bytes */

enum {
    VP_OK = 0,
    VP_EINVAL = -1,      /* bad argument (shape, null pointer, size)                             */
    VP_EWORKSPACE = -2,  /* workspace too small / misaligned                                     */
    VP_EHIP = -3,        /* a HIP runtime call failed                                            */
    VP_EBADID = -4,      /* an occupancy ID hit by a ray is outside [1, n_rows)  (K.cu:71,77:     */
                         /* the reference would write out of bounds)                 */
    VP_EUNSUPPORTED = -5 /* pred_mode = true (K.cu:444-450 is unreachable in the reference too)  */
};

/* flags for vp_project_features */
enum {
    VP_FLAG_SYNC = 1,        /* block until the device work is done and report device-side errors
                                (the reference always does: K.cu:454-457).  EVERY error pending on the
                                workspace is drained by this report: the highest-ranking one is returned, the
                                others are named in vp_last_error, none is left to fail the next call       */
    VP_FLAG_REUSE_ACCEL = 2, /* the occupancy-derived tables in the workspace are still valid for
                                this occupancy grid (same pointer, contents and n_rows): skip
                                rebuilding them.  VP_EINVAL if the library has not built tables on
                                this workspace for the same (B, dims, n_rows)                       */
    VP_FLAG_EXACT_MARCH = 4, /* A/B arm: evaluate every ray sample like K.cu:47-82 does instead of
                                leaping over provably empty space (same results, slower)           */
    VP_FLAG_PIPELINE = 8,    /* asynchronous job mode (excludes VP_FLAG_SYNC): phase 1 (ray-march) runs on a
                                library-owned side stream -- held to a few wavefronts per CU -- so that the
                                march of this call overlaps the gather of the previous call on the same
                                workspace (two buffer sets alternate).  The
                                gather and every write to count/out/views_hit stay on `stream`, in order.
                                The caller promises that occ, vmi and intr are not being written by work
                                still pending on `stream`, keeps them alive and unchanged until the stream
                                has been synchronised (vp_workspace_status does), and uses one stream per
                                workspace.                                                            */
    VP_FLAG_SERIAL_SUMS = 32,  /* sum EVERY voxel with one wavefront in (b, v, y, x) order, however many pixels it got in
                                the call: no voxel is split into parts (one view: shared by a workgroup), so all sums are
                                bit-identical to the serial order of oracle/projector_oracle.c (split voxels are within 1e-4,
                                not bit-equal).
                                For callers that round the sums afterwards and promise the reference's bits -- the
                                aggregator's parity mode (DPF:252 rounds to float16).  Slower only when a voxel is large. */
    VP_FLAG_GATHER_ONLY = 64,  /* phase 2 only: no ray-march; the first-hit images, the per-call histogram and the view table of
                                  the PREVIOUS call on this workspace are used again (same arguments, checked) for the row range
                                  now set with VP_OPT_ROW_BEGIN / VP_OPT_ROW_END.  Two calls -- rows [0, h), then rows [h, n_rows)
                                  with this flag -- leave exactly what one call leaves, and the rows below h are final while
                                  the second gather still runs: a multi-GPU job starts their all-reduce under it.  Runs on the
                                  caller's stream; VP_EINVAL when no SUCCESSFUL call precedes it on the workspace, when that
                                  call had no row range (it gathered every row already), or when its feature maps, poses,
                                  outputs or shapes differ from this call's */
    VP_FLAG_VERIFY_ACCEL = 16  /* blocking calls only (ignored with VP_FLAG_PIPELINE or VP_FLAG_REUSE_ACCEL): the
                                workspace has not been written by anyone else since the previous call on it;
                                compare the occupancy grid with the 32-bit copy kept from the call that built
                                the tables (one pass over the grid + a 4-byte read-back) and rebuild them only
                                if a cell, the shape or n_rows changed.  For callers that pass a NEW tensor with
                                the SAME contents on every call, as debug_project_features.py:143 does.       */
};

int vp_abi_version(void);
const char *vp_last_error(void);

/*
 * Bytes of device scratch memory vp_project_features needs for a call of this shape
 * (first-hit ID image, per-call hit histogram, ID -> cell table, occupancy block masks and block
 * distance field, view table, part slots of C floats for the split voxels' partial rows).
 */
size_t vp_workspace_bytes(int B, int V, int H, int W, int C,
                          int dimz, int dimy, int dimx, int64_t n_rows);

/*
 * Replaces project_features_cuda_forward_impl (K.cu:374-459), i.e. what the extension function
 * project_features_cuda.project_features_cuda(...) (W.cpp:23-79) does after validation, for
 * pred_mode = false.
 *
 *   feats        f32 [B,V,H,W,C] channels-last, device            (K.cu:375)
 *   occ          i64 [B,dimz,dimy,dimx], 0 = empty, else voxel ID  (K.cu:376)
 *   vmi          f32 [B*V*16] row-major camera->world matrices     (K.cu:377, :178-179)
 *   intr         f32 [B,4] = fx, fy, mx, my per batch              (K.cu:378, cudaUtil.h:86-93)
 *   opts_host    f32 [5] HOST = width, height, depthMin, depthMax, rayIncrement (K.cu:400-407)
 *   count        i32 [n_rows]   in/out, count[id] += #pixels        (K.cu:77)
 *   out          f32 [n_rows,C] in/out, out[id,:] += feature rows   (K.cu:85-91)
 *   views_hit    i32 [n_rows]   in/out or NULL, += number of views of this call in which the voxel
 *                received at least one pixel -- the aggregator's "hit_count" (AGG:313 counts VIEWS,
 *                one per debug_project_features run), so that multi-view calls can feed it
 *   grid_origin_host f32 [3] HOST                                  (K.cu:412-413)
 *   voxel_size                                                     (K.cu:414)
 *   workspace    device scratch of >= vp_workspace_bytes(...) bytes, 256-byte aligned
 *   stream       hipStream_t (NULL = default stream)
 *
 * Results: first-hit voxel assignment and counts bit-exact with the arithmetic contract in
 * oracle/projector_oracle.c; feature sums accumulated in fp32 in (b, v, y, x) order per voxel.
 * width/height in opts must equal W/H (the reference indexes features with the opts values,
 * K.cu:74-76; a mismatch reads garbage there and is rejected here).
 */
int vp_project_features(const float *feats, const int64_t *occ, const float *vmi,
                        const float *intr, const float *opts_host,
                        int32_t *count, float *out, int32_t *views_hit,
                        const float *grid_origin_host, float voxel_size,
                        int B, int V, int H, int W, int C,
                        int dimz, int dimy, int dimx, int64_t n_rows,
                        void *workspace, size_t workspace_bytes,
                        void *stream, int flags);

/*
 * Stage-5 front end: index of the nearest voxel for each of M Gaussian centres -- replaces
 * map_gaussians_to_voxels (voxel_to_gaussian/voxeltoGaussian_logits.py:87-105; identical code at
 * voxel_to_gaussian/voxeltoGaussian.py:84-93: sklearn KDTree(leaf_size=16).query(k=1) in float64).
 *   pts_sorted  f32 [N,3] voxel positions sorted by grid cell (device)
 *   perm        i32 [N]   original index of each sorted position
 *   cell_start  i32 [nx*ny*nz + 1] first sorted position of each cell ((z*ny + y)*nx + x order)
 *   grid_origin3 f64 [3] HOST, cell_size, nx, ny, nz: the bucketing grid
 *   queries     f32 [M,3] device;  out i64 [M] device: nearest original index (lowest index on exact ties)
 * Asynchronous on `stream`.
 */
int vp_nearest_voxel(const float *pts_sorted, const int32_t *perm, const int32_t *cell_start,
                     const double *grid_origin3, double cell_size, int nx, int ny, int nz,
                     const float *queries, int64_t M, int64_t *out, void *stream);

/*
 * Measurement aid: streams n_floats (a multiple of 4, 16-byte aligned) from `src` with non-temporal 16-byte
 * loads and discards them -- bench.py times it to quote the gather against the box's own streaming-read
 * ceiling as well as the nominal HBM peak.  No reference counterpart.
 */
int vp_stream_read(const float *src, int64_t n_floats, float *sink, void *stream);

/*
 * Same as vp_project_features with the feature maps stored as IEEE binary16 [B,V,H,W,C] (C % 8 == 0).
 * LSeg features are fp16 at rest (script/extract_lseg_features.py:97) and
 * prepare_tensor_data.py:126 casts the resized maps back to fp16 before widening them, so every value the
 * reference kernel reads is fp16-representable; this entry point reads half the bytes, widens exactly and
 * accumulates in fp32 in the same order -- outputs are bit-identical to the fp32 path on the same data.
 * (No reference counterpart: its wrapper insists on float32, W.cpp:46.)
 */
int vp_project_features_f16(const void *feats_f16, const int64_t *occ, const float *vmi,
                            const float *intr, const float *opts_host,
                            int32_t *count, float *out, int32_t *views_hit,
                            const float *grid_origin_host, float voxel_size,
                            int B, int V, int H, int W, int C,
                            int dimz, int dimy, int dimx, int64_t n_rows,
                            void *workspace, size_t workspace_bytes,
                            void *stream, int flags);

/*
 * Drains the workspace's streams (the library's side stream, then `stream`), then reads the sticky device-side error words of
 * the workspace -- a page of pinned host memory owned by the library's record of the workspace, which the kernels write
 * through its device mapping: no device-to-host copy, and nothing a stranger could have overwritten.  They collect the
 * errors (tables gone from recycled memory: VP_EINVAL; a ray parameter that cannot advance: VP_EINVAL; out-of-range ID:
 * VP_EBADID) of EVERY call made on the workspace since they were last reported, pipelined or not -- no later call erases
 * them.  One condition is reported per call, in that order, and only the reported one is cleared: call again (until
 * VP_OK) to see the others.
 * The reference only prints device errors (K.cu:454-457, cutilCheckMsg); here they surface as a return code.
 * Returns VP_OK when no call has reported anything.
 */
int vp_workspace_status(void *workspace, void *stream);

/*
 * Diagnostic counters of the last call on this workspace, copied to host_words[0..n) after a
 * stream synchronise: [0] = rays that hit an out-of-range ID, [1] = voxels whose search box
 * missed pixels and were rescanned over whole images (performance hint only; results are exact
 * either way), [2] = voxels that collected more pixels than the heavy threshold in this call (summed in
 * parts), [7] = the heavy threshold in force, [8] = pixels of a one-view call whose ray hit a voxel (when the device sizes
 * the parts from it), [9] / [10] = pixels above which a voxel was cut into parts / pixels per part in force, [24] = the parts
 * planned in this call, [25] = the voxels they belong to.  No reference counterpart.
 */
int vp_workspace_counters(void *workspace, int32_t *host_words, int n, void *stream);

/*
 * Per-kernel device timing with HIP events recorded on the stream the kernels are launched on
 * (measurement harness; no reference counterpart -- the reference has no timers).
 * vp_profile_enable(1) starts recording for subsequent vp_project_features calls of this process;
 * vp_profile_read synchronises the recorded events and returns, per kernel group, the summed
 * milliseconds and the number of launches: [0] = table preparation (memsets, occupancy tables, view
 * table), [1] = k_first_hit + work list + view table (phase 1), [2] = k_gather / k_gather_one (phase 2, the parts of the split
 * voxels included), [3] = k_combine_parts (the split voxels' partial rows added to their rows);
 * then clears the record.
 */
int vp_profile_enable(int on);
int vp_profile_read(double *ms4, int64_t *launches4);

/*
 * RGB path: replaces the per-voxel Python loop of DPC:54-81 plus the per-view accumulation of
 * aggregate_voxel_colors_onthefly.py:134-140 for a batch of V views (voxel-driven, nearest pixel, no
 * occlusion test, float64 arithmetic exactly as numpy promotes it there).  One lane per occupied voxel; the
 * lanes take the voxels along the Morton curve of the grid's cells (a list the call builds on the device), which
 * changes no output bit and halves the image lines a launch fetches.
 *
 *   occ        i32 [dimz,dimy,dimx] device, > 0 = voxel ID (BSO:44-46; DPC:50 tests occ > 0).  Every ID must label
 *              exactly ONE cell (build_sparse_occupancy.py guarantees it); a duplicate returns VP_EINVAL
 *   c2w        f32 [V,16] device, row-major camera->world (DPC:61-62 reads R and t from it)
 *   intr       f32 [V,4] device, fx fy cx cy of each view (DPC:64)
 *   images     u8  [V,img_h,img_w,3] device (DPC:52,70)
 *   color_sum  f32 [n_rows,3] in/out: += img[v,u]/255 for every view that sees the voxel, in view order (AGGC:139)
 *   hit_count  i32 [n_rows]   in/out: += number of such views (AGGC:140)
 *   first_view i32 [n_rows]   in/out or NULL: min(view_base + v) over those views -- reproduces the
 *                             dict insertion order of AGGC:136-137 on the host
 *   pixel_uv   i32 [V,n_rows,2] out or NULL: the pixel (u, v) sampled for voxel `id` in view v (DPC:76
 *                             `pixel_indices`), (-1,-1) where the voxel is not seen
 *   workspace  device scratch of >= vp_colors_workspace_bytes(n_rows) bytes (12 per row + 33 KiB), 256-byte aligned
 * Synchronous (returns after the stream has drained).
 */
size_t vp_colors_workspace_bytes(int64_t n_rows);
int vp_project_colors(const int32_t *occ, int dimz, int dimy, int dimx,
                      const float *c2w, const float *intr, int V,
                      const float *grid_origin_host, double voxel_size,
                      const uint8_t *images, int img_h, int img_w,
                      float *color_sum, int32_t *hit_count, int32_t *first_view, int32_t *pixel_uv,
                      int64_t n_rows, int view_base, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Feature-map up-sampler: replaces the 512 x cv2.resize(channel, (W,H), INTER_LINEAR) calls, the cast back to the file's
 * dtype and the permute to channels-last of prepare_tensor_data.py:119-127,152,183-185.
 *   src_chw   f16 or f32 [C,h,w] device (the LSeg .npy layout, script/extract_lseg_features.py:97)
 *   dst_hwc   f32 [H,W,C] (what project_features_cuda reads) or f16 [H,W,C] (for vp_project_features_f16; f16 source only)
 *   workspace >= vp_upsample_workspace_bytes(C,h,w,src_is_f16) bytes: the [h,w,C] transpose of the source
 * Arithmetic = OpenCV's published INTER_LINEAR rule for CV_32F images (half-pixel centres, float32 coefficients,
 * horizontal then vertical pass, no FMA), cast to the source dtype, widened: spelled out in csrc/vp_prep.h and restated in
 * oracle/resize_oracle.py.  Also produces a plain copy when (H,W) == (h,w).  Asynchronous on `stream`.
 */
size_t vp_upsample_workspace_bytes(int C, int h, int w, int src_is_f16);
int vp_upsample_features(const void *src_chw, int src_is_f16, int C, int h, int w,
                         void *dst_hwc, int dst_is_f16, int H, int W,
                         void *workspace, size_t workspace_bytes, void *stream);

/*
 * Occupancy builder: replaces build_sparse_occupancy.py:30-53 in two steps around the one host decision (grid size):
 *   vp_voxel_coords      coords[i] = np.round((pts[i] - origin) / voxel_size) in float32, half to even (BSO:32), written as
 *                        i32 [N,3] (x,y,z); minmax_host[0..2] = per-axis minimum, [3..5] = maximum (BSO:35,40).  Blocking.
 *   vp_scatter_occupancy occ[z,y,x] = i + 1 for coords[i] - shift (BSO:36-39 shifts by the minimum when any is negative),
 *                        the LAST vertex wins on duplicates (BSO:45-46); occ i32 [dimz,dimy,dimx] is zeroed first.  Blocking.
 *   scratch8_dev         8 ints of device scratch
 */
int vp_voxel_coords(const float *points_xyz, int64_t N, const float *grid_origin_host, float voxel_size,
                    int32_t *coords, int32_t *scratch8_dev, int32_t *minmax_host, void *stream);
int vp_scatter_occupancy(const int32_t *coords, int64_t N, const int32_t *shift3_host,
                         int dimz, int dimy, int dimx, int32_t *occ, int32_t *scratch8_dev, void *stream);

/*
 * The aggregator's per-view accumulate in the reference's arithmetic (aggregate_voxel_features_onthefly.py:307-313 on
 * the float16 rows of debug_project_features.py:252), over the rows hit in this view only:
 *   view_sum   f32 [n_rows,C] in: the view's pixel sums (vp_project_features into a zeroed buffer); out: zero again
 *   view_count i32 [n_rows]   in: the view's pixel counts; out: zero again
 *   run16      f16 [n_rows,C] running per-voxel sum: first hit = clone of the fp16-rounded row, later hits fp16 +=
 *   views      i32 [n_rows]   += 1 for every voxel hit in this view (AGG:313 counts VIEWS)
 *   first_view i32 [n_rows]   = view_index where the voxel is hit for the first time (dict insertion order)
 *   nonfinite_dev i32 [1]     |= 1 if a float16 row of this view holds NaN or Inf (AGG:303-304 prints an error)
 * Asynchronous on `stream`.
 */
int vp_aggregate_view_f16(float *view_sum, int32_t *view_count, void *run16, int32_t *views, int32_t *first_view,
                          int view_index, int32_t *nonfinite_dev, int64_t n_rows, int C, void *stream);

/*
 * Workspace lifetime.  The library keeps ONE record per workspace (side stream and events of VP_FLAG_PIPELINE, the shape
 * the occupancy tables in it were built for, its options).  The record is looked up by the workspace's address but is
 * not trusted on the address alone: its generation number is also written into the workspace memory (a header in the
 * first 256 bytes) and compared, on the device, by every call -- so memory that was freed and handed out again, or
 * overwritten, is recognised: calls that trust the tables (VP_FLAG_REUSE_ACCEL) then do no work and the next
 * vp_workspace_status returns VP_EINVAL; calls that rebuild them re-initialise the header.
 *
 *   vp_workspace_create   "this memory is a new workspace": drops any record the address had (streams, tables, options)
 *                         and starts a new generation.  Optional for memory the library has never seen (the first call
 *                         creates the record), REQUIRED manners for memory that is being reused as a workspace.
 *   vp_workspace_release  drains and destroys the record; call before freeing or recycling the memory.
 * No reference counterpart (the reference allocates nothing between calls).
 */
int vp_workspace_create(void *workspace, size_t workspace_bytes);
int vp_workspace_release(void *workspace);

/*
 * Options of a workspace, read by the calls made on it (they replace the environment variables of ABI v2; the
 * library reads no environment variable).  value < 0 (or 0 for the threshold) restores the default.
 *   VP_OPT_HEAVY_THRESHOLD  voxels that collect more than this many pixels in ONE call are not summed by a single wavefront: they
 *                           are cut into parts of VP_OPT_PART_PIXELS pixels, each part summed by a wavefront of the same gather
 *                           launch, the partial rows added to the voxel's row in a fixed order by a follow-up kernel.  Default
 *                           min(256 + 64*B*V, 2048) -- the longest job a wavefront can get bounds the tail of the launch --;
 *                           calls of one view: see VP_OPT_ONE_VIEW_SPLIT;
 *                           VP_FLAG_SERIAL_SUMS overrides it with "never".  Never below the part size
 *   VP_OPT_PART_PIXELS      pixels per part of a split voxel (default: the threshold; 256 for calls of one view); raised to
 *                           2*B*V*H*W / slots when the call is so large that its parts could outnumber the workspace's part
 *                           slots (65536, fewer for rows wider than 2 KiB; 8192 for calls of one view)
 *   VP_OPT_ONE_VIEW_SPLIT   calls of ONE view: voxels that collect more than this many pixels are cut into parts like those of
 *                           multi-view calls (one wavefront of the one-view gather per part, k_combine_parts behind it), the
 *                           others are summed by one wavefront in the oracle's order.  Default (< 0): decided on the device from
 *                           the number of pixels of the view whose ray hit a voxel -- parts of max(32, 2 * hits / 8192) pixels
 *                           (VP_OPT_PART_PIXELS fixes the size), threshold twice the part, at least 256 pixels for views of up
 *                           to 262144 pixels; VP_OPT_HEAVY_THRESHOLD, when set, is taken as this threshold.  0 = never split:
 *                           round 5's behaviour (the four wavefronts of a workgroup share a voxel above VP_OPT_HEAVY_THRESHOLD,
 *                           default 320), the A/B arm.  Never below the part size
 *   VP_OPT_MARCH_LDS_KB     dynamic-LDS reservation of the march kernel in KiB = its occupancy cap (default beside a
 *                           running gather in VP_FLAG_PIPELINE mode: 41 KiB = 3 workgroups per CU, 30 KiB = 5 when a
 *                           feature row is at most 1 KiB -- fp16 maps of 512 channels --; 0 otherwise).  Valid: 0 .. 64
 *                           (a kernel's dynamic-LDS limit); larger values are refused with VP_EINVAL
 *   VP_OPT_ROW_BEGIN / _END phase 2 of the following calls gathers only the voxel IDs in [begin, end) (default: all rows;
 *                           value < 0 restores it).  Phase 1 is not restricted: the histogram it leaves covers every row, so
 *                           that a VP_FLAG_GATHER_ONLY call can gather the other rows from it.  A voxel's parts depend on
 *                           its pixel count and boxes alone, so each ranged gather sums every voxel of its range to the
 *                           same bits as the unsplit call
 *   VP_OPT_ONE_VIEW_GATHER  0 = calls of ONE view (B*V == 1) go through the general gather kernel instead of the one-view
 *                           kernel (A/B arm; same results bit for bit); n > 0 = the one-view kernel with n workgroups per CU
 *                           (default 16; 1000 + g: exactly g workgroups, a test hook); < 0 restores the default
 */
enum { VP_OPT_HEAVY_THRESHOLD = 1, VP_OPT_MARCH_LDS_KB = 2, VP_OPT_ROW_BEGIN = 3, VP_OPT_ROW_END = 4, VP_OPT_ONE_VIEW_GATHER = 5,
       VP_OPT_PART_PIXELS = 6, VP_OPT_ONE_VIEW_SPLIT = 7 };
int vp_workspace_set_option(void *workspace, int option, long long value);

/* How many times the occupancy-derived tables of this workspace have been (re)built so far (0 if never);
 * diagnostic for VP_FLAG_REUSE_ACCEL / VP_FLAG_VERIFY_ACCEL. */
long long vp_workspace_table_builds(const void *workspace);

/*
 * Copies the first-hit ID image i32 [B,V,H,W] of the LAST vp_project_features call on this
 * workspace into dst (device pointer), asynchronously on `stream`.  The parity tests use it to compare the pixel -> voxel
 * assignment of K.cu:47-82 directly (the reference has no such output); it is also how a caller keeps a forward call's
 * assignment for its adjoint: copy it on the same stream right behind the call, before another call on the workspace,
 * and hand it to vp_render_features later (project_features_autograd.py does).  VP_EINVAL when the last call on the
 * workspace failed or was a vp_first_hit_ids call.
 */
int vp_copy_hit_image(const void *workspace, int32_t *dst, int B, int V, int H, int W,
                      int C, int dimz, int dimy, int dimx, int64_t n_rows, void *stream);

/*
 * The projector's transpose.  vp_project_features computes out[id, :] += sum of feats[p, :] over the pixels p whose ray hits
 * voxel id first; its adjoint copies, for every pixel, the row of that voxel:  dst[p, :] = rows[hit[p], :].  The same copy
 * shows a per-voxel table (an aggregation result) from any camera.  No reference counterpart (its autograd Function,
 * tests/backward_test.py:74-79 of the CUDA extension, is the closest).  Added after VP_ABI_VERSION 4 without changing it
 * or any existing entry point: callers detect the two functions by symbol (dlsym), not by the version number.
 *
 * vp_first_hit_ids: the march alone -- the first-hit voxel ID image i32 [B,V,H,W] (0 = the ray hits nothing) that
 *   vp_project_features would leave for the same occ / vmi / intr / opts / grid arguments, bit for bit, written into `ids`
 *   (device).  No feature maps, no work list, no gather.  Arguments as for vp_project_features; the workspace needs
 *   vp_workspace_bytes(B, V, H, W, 1, dimz, dimy, dimx, n_rows) bytes and follows the same rules (tables built on it are
 *   shared with vp_project_features calls of the same grid, VP_FLAG_REUSE_ACCEL / VP_FLAG_VERIFY_ACCEL as there).  flags:
 *   VP_FLAG_SYNC | VP_FLAG_REUSE_ACCEL | VP_FLAG_VERIFY_ACCEL | VP_FLAG_EXACT_MARCH only, any other bit is VP_EINVAL.  Host
 *   checks as vp_project_features (opts width/height = W/H, B*V <= 65535, rayIncrement > 0, workspace size and alignment,
 *   ...); device errors (a ray hitting an ID outside [1, n_rows): the pixel reads 0; stuck rays; stale tables) go to the
 *   workspace's sticky words like those of every other call.  It counts as a call on the workspace: a following
 *   VP_FLAG_GATHER_ONLY call or vp_copy_hit_image returns VP_EINVAL (there is no forward call to take up).
 *
 * vp_render_features: dst[p, :] = rows[ids[p], :] for p < n_pixels (ids flattened, e.g. B*V*H*W of vp_first_hit_ids or
 *   vp_copy_hit_image), rows f32 [n_rows, C] device, dst [n_pixels, C] device, f32 or (dst_is_f16) IEEE binary16 rounded to
 *   nearest-even (torch's .half()).  ID 0 (a miss) gives zeros, NOT rows[0] -- row 0 receives no pixel in the forward, so
 *   this is the exact adjoint.  IDs < 0 or >= n_rows give zeros and are never read; each such pixel adds 1 to *bad_ids
 *   (device i32, may be NULL).  fp32 rows are copied bit for bit.  Any C >= 1 (16-byte loads/stores when C % 4 == 0, or
 *   C % 8 == 0 for an f16 dst, with 16-byte aligned rows and dst); 64-bit offsets.  Asynchronous on `stream`; refused on the
 *   host: null ids / rows / dst, n_pixels <= 0, n_rows <= 0, C <= 0.
 */
int vp_first_hit_ids(const int64_t *occ, const float *vmi, const float *intr, const float *opts_host,
                     const float *grid_origin_host, float voxel_size,
                     int B, int V, int H, int W, int dimz, int dimy, int dimx, int64_t n_rows,
                     int32_t *ids, void *workspace, size_t workspace_bytes, void *stream, int flags);
int vp_render_features(const int32_t *ids, int64_t n_pixels, const float *rows, int64_t n_rows, int C,
                       void *dst, int dst_is_f16, int32_t *bad_ids, void *stream);

/*
 * Text query of a per-voxel feature table (the reference's stage 5.1, the `query` sub-commands of
 * voxel_to_gaussian/voxeltovoxel_logits.py and voxeltoGaussian_logits.py; the margin is logit_confidence_map.py's per-pixel
 * confidence).  Added after VP_ABI_VERSION 4 without changing it or any existing entry point: callers detect the two
 * functions by symbol (dlsym), not by the version number.
 *
 *   x^ = x / max(|x|, 1e-12)   t^_j = t_j / max(|t_j|, 1e-12)   (torch.nn.functional.normalize)
 *   logit_j = scale * (x^ . t^_j),  label = argmax_j logit_j (lowest j on exact ties),
 *   margin  = softmax(logit)[label] - second-largest softmax entry (1 when P = 1).
 *
 * vp_query_workspace_bytes: bytes of the caller's scratch for a query of P prompts of C channels (the normalised text,
 *   zero-padded to 16-prompt / 32-channel tiles); 0 when P is outside [1, 1024] or C outside [1, 2048].  Grows with P and C.
 *
 * vp_query_features: rows [n_rows, C] device, IEEE binary16 (rows_is_f16) or f32, row r at rows + r * row_stride elements
 *   (row_stride >= C); text f32 [P, C] device, row-major, any alignment; scale > 0 multiplies every logit (1: cosine; LSeg's
 *   head uses its logit_scale).  Writes labels i32 [n_rows], and when not NULL logits f32 [n_rows, P] row-major and margin
 *   f32 [n_rows].  fp16 rows run on v_mfma_f32_16x16x32_f16 with the normalised text rounded to binary16; f32 rows on
 *   v_mfma_f32_16x16x4_f32 with f32 text, never rounded to binary16.  Every logit is within
 *   scale * (2^-11 + 2 * C * 2^-24) of the float64 value.  A zero row gives logits 0, label 0, margin 0 (1 when P = 1).  A
 *   row with a non-finite element gives label -1, NaN logits and margin, and adds 1 to *n_nonfinite (device i32, may be
 *   NULL; not reset by the call).  Results are bit-identical from run to run and a row's outputs do not depend on the other
 *   rows of the call (for the same dtype, C and alignment).  16-byte row loads when C % 8 == 0 (fp16) or C % 4 == 0 (f32)
 *   with 16-byte aligned rows and row stride, element loads otherwise; 64-bit offsets.  workspace: device,
 *   vp_query_workspace_bytes(P, C) bytes, 256-byte aligned, not shared with a call still running on another stream.  No
 *   allocation, no host synchronisation: asynchronous on `stream`.  Refused on the host (VP_EINVAL): null rows / labels /
 *   text, n_rows outside [1, 2^31 - 1], C outside [1, 2048], P outside [1, 1024], row_stride < C, scale <= 0 or not
 *   finite; VP_EWORKSPACE: a workspace that is NULL, too small or not 256-byte aligned.
 */
size_t vp_query_workspace_bytes(int P, int C);
int vp_query_features(const void *rows, int rows_is_f16, int64_t n_rows, int C, int64_t row_stride, const float *text,
                      int P, float scale, float *logits, int32_t *labels, float *margin, int32_t *n_nonfinite,
                      void *workspace, size_t workspace_bytes, void *stream);

/*
 * Gaussian splatting of per-Gaussian features (the reference's stage 5.2, voxel_to_gaussian/render_semantics_logits.py,
 * which calls gsplat's rasterization() in classic mode without a background).  Differentiable in the features and the
 * opacities through vp_splat_rasterize_backward, and in the means, quaternions and scales as well through
 * vp_splat_rasterize_backward_geometry (both below); not in the camera.  Added after VP_ABI_VERSION 4
 * without changing it or any existing entry point: callers detect the three functions by symbol (dlsym).
 *
 * Per Gaussian: mean mu (world), quaternion q = (w, x, y, z) (normalised here; |q| = 0 culls), scale s (activated), opacity
 * o (activated), feature row f of D channels.  Camera: world-to-camera [R | t] (COLMAP: x right, y down, z forward), fx, fy,
 * cx, cy, W x H.  z = ((r20 mx + r21 my) + r22 mz) + t2 in fp32 (no FMA); culled when z < near or z > far.
 * Sigma2 = J R Sigma R^T J^T + eps2d I with Sigma = M M^T, M = R(q) diag(s) and gsplat's Jacobian clamp
 * (tx = z clamp(px/z, -(cx/fx + 0.15 W/fx), (W - cx)/fx + 0.15 W/fx), likewise y); culled when det(Sigma2) <= 0.
 * mean2d = (fx px/z + cx, fy py/z + cy).  Pixel (j, i) samples (j + 0.5, i + 0.5); Gaussians in ascending (fp32 z, index):
 * sigma = (A dx^2 + C dy^2)/2 + B dx dy with (A, B, C) = Sigma2^-1 and d = mean2d - sample, skipped when sigma < 0;
 * a = min(0.999, o exp(-sigma)), skipped when a < 1/255; Tn = T (1 - a); when Tn <= 1e-4 the pixel stops (that Gaussian
 * is not added); else out += f a T, T = Tn.  alpha = 1 - T; no background.  Every (Gaussian, pixel) pair with a >= 1/255 is
 * visited: a Gaussian's tiles cover the box |dx| <= sqrt(2 ln(255 o) Sigma2_00), |dy| <= sqrt(2 ln(255 o) Sigma2_11) widened
 * by one pixel.  Epilogue: label = argmax over the D channels (lowest index on ties; 0 where nothing reaches), confidence =
 * softmax top-1 minus top-2 (1 when D = 1).  The projection runs in float64 past the fp32 depth; the blend in fp32 with no
 * atomics: results are bit-identical from run to run.
 *
 * vp_splat_workspace_bytes: bytes of the caller's scratch for n_gaussians Gaussians, a W x H image and room for `capacity`
 *   (tile, Gaussian) intersections; 0 when n_gaussians or capacity is outside [0, 2^31 - 1] or W, H outside [1, 32768],
 *   and 0 without a usable GPU (rocPRIM sizes its scratch for the current device's architecture).
 *   vp_splat_project needs the size at capacity 0, which is a prefix of every larger capacity's layout: a workspace can be
 *   regrown between the two calls by copying those bytes.
 *
 * vp_splat_project: means f32 [n,3], quats f32 [n,4], scales f32 [n,3], opacities f32 [n], device, contiguous; viewmat f32
 *   [4,4] row-major, HOST memory (rows 0-2 read during the call).  Writes the screen-space records and the number of
 *   intersections into the workspace and, when not NULL, into *n_isect (device i64).  A non-finite mean, quaternion, scale
 *   or opacity culls that Gaussian and adds 1 to *n_nonfinite (device i32, may be NULL; not reset by the call).
 *
 * vp_splat_rasterize: after vp_splat_project on the same workspace, stream, n_gaussians, W and H.  features f32, row g at
 *   features + g * row_stride (row_stride >= D, unit channel stride), D in [1, 64].  Sorts `capacity` keys
 *   (rocprim::radix_sort_pairs; pass the project call's count for no wasted work), then blends one 16x16 tile per
 *   workgroup.  Writes labels i32 [H,W] and, each only when not NULL, confidence f32 [H,W], alpha f32 [H,W] and logits f32
 *   planar [D,H,W].  When the device count exceeds `capacity` nothing is written to any output and *status (device i32, may
 *   be NULL; not reset by the call) is set to 1.
 *
 * Both: 64-bit offsets; no allocation, no host synchronisation: asynchronous on `stream`; workspace 256-byte aligned, not
 * shared with a call still running on another stream.  Refused on the host (VP_EINVAL): n_gaussians outside [0, 2^31 - 1],
 * null pointers (the Gaussian arrays / features when n_gaussians > 0, viewmat, labels), W or H outside [1, 32768], a
 * non-finite viewmat, fx, fy <= 0, near <= 0 or far <= near, eps2d < 0, D outside [1, 64], row_stride < D, capacity outside
 * [0, 2^31 - 1]; VP_EWORKSPACE: a workspace that is NULL, smaller than vp_splat_workspace_bytes or not 256-byte aligned.
 */
size_t vp_splat_workspace_bytes(int64_t n_gaussians, int W, int H, int64_t capacity);
int vp_splat_project(const float *means, const float *quats, const float *scales, const float *opacities,
                     int64_t n_gaussians, const float *viewmat, float fx, float fy, float cx, float cy, int W, int H,
                     float near_plane, float far_plane, float eps2d, int64_t *n_isect, int32_t *n_nonfinite,
                     void *workspace, size_t workspace_bytes, void *stream);
int vp_splat_rasterize(const float *features, int D, int64_t row_stride, int64_t n_gaussians, int W, int H,
                       int64_t capacity, int32_t *labels, float *confidence, float *alpha, float *logits,
                       int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The splatting backward: gradients of a loss L through the two differentiable outputs, logits [D,H,W] and alpha [H,W],
 * with respect to the features f [N,D] and the activated opacities o [N].  Added after VP_ABI_VERSION 4 without changing
 * it; detect the two functions by symbol.  Labels and confidence are not differentiable; the geometry's gradients (means,
 * quats, scales) come from vp_splat_rasterize_backward_geometry below.
 *
 * The contract: the backward differentiates the branch the forward took, with the same (z, index) order and the same
 * decisions at every pixel (skip when sigma < 0 or a < 1/255; stop at the first Gaussian that would take T to <= 1e-4, which
 * gets no gradient at that pixel, and neither does any Gaussian after it).  With a = min(0.999, o e^-sigma), w_g = a_g T_g
 * (T_g the transmittance before g), S_g = sum over the Gaussians k added after g of w_k f_k and T_final the pixel's final T,
 * per pixel:
 *   dC_c/df_gc  = w_g                                   (the logits are linear in f)
 *   dC_c/da_g   = T_g f_gc - S_gc / (1 - a_g)
 *   dalpha/da_g = T_final / (1 - a_g)
 *   da/do       = e^-sigma when o e^-sigma < 0.999, else 0.
 * grad_features[g,c] = sum_p G[c,p] w_g(p);  grad_opacities[g] = sum_p (sum_c G[c,p] dC_c/da_g + G_alpha[p] dalpha/da_g) da/do.
 * A culled Gaussian (non-finite, near / far, zero quaternion, off-image, o < 1/255) gets rows of exactly 0, and so does one
 * that no pixel added.  fp32, no float atomics: per-(tile, Gaussian) partials are summed in a fixed order, so gradients are
 * bit-identical from run to run.  The behind-sum S_g . G is the pixel's C . G minus a running prefix; its error is a few
 * ulp of sum_k w_k |f_k . G|.
 *
 * vp_splat_backward_workspace_bytes: bytes of the backward's own scratch, capacity x (D + 1) floats (at least one row),
 *   256-byte rounded; 0 when capacity is outside [0, 2^31 - 1] or D outside [1, 64].  Needs no GPU.
 *
 * vp_splat_rasterize_backward: after vp_splat_rasterize on this workspace with the same n_gaussians, W, H, capacity,
 *   features and stream; the workspace is only read.  grad_logits f32 planar [D,H,W] and grad_alpha f32 [H,W], contiguous,
 *   each may be NULL (read as 0).  Writes grad_features f32 [N,D] (contiguous) and grad_opacities f32 [N], each only when not
 *   NULL.  When the device count exceeds `capacity` nothing is written and *status (device i32, may be NULL; not reset) is
 *   set to 1.  Asynchronous on `stream`, no allocation.  Refused on the host as vp_splat_rasterize refuses (VP_EINVAL), and
 *   with VP_EWORKSPACE for either workspace: NULL, not 256-byte aligned, or smaller than its size function.
 */
size_t vp_splat_backward_workspace_bytes(int64_t capacity, int D);
int vp_splat_rasterize_backward(const float *features, int D, int64_t row_stride, int64_t n_gaussians, int W, int H,
                                int64_t capacity, const float *grad_logits, const float *grad_alpha,
                                float *grad_features, float *grad_opacities, int32_t *status, void *workspace,
                                size_t workspace_bytes, void *bwd_workspace, size_t bwd_bytes, void *stream);

/*
 * The geometry backward: one fused call for the gradients of L with respect to the means [N,3], the quaternions [N,4], the
 * activated scales [N,3], the features and the activated opacities.  Added after VP_ABI_VERSION 4 without changing it;
 * detect the two functions by symbol.  No gradient with respect to the camera (viewmat, fx, fy, cx, cy) is computed.
 *
 * The contract: as above, the branch the forward took is differentiated, with the same (fp32 z, index) order and the same
 * skip / stop decisions at every pixel.  For a pixel that added Gaussian g, with d = mean2d_g - sample,
 * sigma = (A dx^2 + C dy^2)/2 + B dx dy, raw = o e^-sigma and dL/da as above, let q = dL/da raw where raw < 0.999 and q = 0
 * at the clamp.  The screen-space gradients, summed over the pixels that added g, are
 *   g_mx = -sum q (A dx + B dy)    g_my = -sum q (B dx + C dy)
 *   g_A  = -sum q dx^2 / 2         g_B  = -sum q dx dy           g_C = -sum q dy^2 / 2
 * (grad_screen [N,5] in this order: dL/d mean2d and dL/d conic, B counted once as in sigma).  The world-space gradients
 * are these five sums pushed through the adjoint of the forward's own float64 projection, in this order: conic = Sigma2^-1;
 * Sigma2 = J R_w Sigma R_w^T J^T + eps2d I; Sigma = M M^T with M = R(q/|q|) diag(s); mean2d = f p/z + c; p = R_w m + t.
 *   Jacobian clamp: where J clamps p/z the clamped branch is differentiated (tx = z lim: no gradient through p_x / z there,
 *     the one through z stays); mean2d uses the unclamped p/z.
 *   Depth: z here is the float64 p[2].  The fp32 depth only sorts and culls and carries no gradient; neither do the
 *     support box, the 1/255 skip or the 1e-4 stop.
 *   Activations: grad_quats is with respect to the quaternion as passed (not normalised), so it is orthogonal to q;
 *     grad_scales is with respect to the activated scales.  Callers chain their own exp / sigmoid.
 *   Zero rows: a culled Gaussian, and one that no pixel added, gets rows of exactly 0 in every output.
 *   Determinism: fp32 in the tile sweep, no float atomics; per-(tile, Gaussian) partials in the pair's emission slot, summed
 *     per Gaussian in ascending slot order: bit-identical from run to run.
 *   Chain precision: the per-Gaussian chain runs in float64 on the device from the fp32 sums, recomputing the forward's
 *     intermediates from means / quats / scales / camera, and is rounded to fp32 once.
 *
 * vp_splat_geometry_backward_workspace_bytes: bytes of this call's scratch, capacity x (D + 1 + 5) floats (at least one
 *   row), 256-byte rounded; 0 when capacity is outside [0, 2^31 - 1] or D outside [1, 64].  Needs no GPU.
 *
 * vp_splat_rasterize_backward_geometry: after vp_splat_rasterize on this workspace with the same n_gaussians, W, H,
 *   capacity, features and stream, and with the means, quats, scales, viewmat (HOST memory), fx, fy, cx, cy and eps2d of the
 *   vp_splat_project call before it; the workspace is only read.  grad_logits f32 planar [D,H,W] and grad_alpha f32 [H,W],
 *   each may be NULL (read as 0).  Writes, each only when its pointer is not NULL: grad_means f32 [N,3], grad_quats f32
 *   [N,4], grad_scales f32 [N,3], grad_features f32 [N,D], grad_opacities f32 [N], grad_screen f32 [N,5], all contiguous.
 *   grad_features and grad_opacities are bit-identical to vp_splat_rasterize_backward's on the same inputs.  means, quats,
 *   scales and the camera are read only when grad_means, grad_quats or grad_scales is asked for (they may be NULL
 *   otherwise).  When the device count exceeds `capacity` nothing is written and *status (device i32, may be NULL; not
 *   reset) is set to 1.  Asynchronous on `stream`, no allocation.  Refused on the host as vp_splat_rasterize_backward
 *   refuses, with its scratch measured by vp_splat_geometry_backward_workspace_bytes, and, when a world-space gradient is
 *   asked for, as vp_splat_project refuses its Gaussian arrays and camera (VP_EINVAL).
 */
size_t vp_splat_geometry_backward_workspace_bytes(int64_t capacity, int D);
int vp_splat_rasterize_backward_geometry(const float *means, const float *quats, const float *scales, const float *features,
                                         int D, int64_t row_stride, int64_t n_gaussians, const float *viewmat, float fx,
                                         float fy, float cx, float cy, int W, int H, float eps2d, int64_t capacity,
                                         const float *grad_logits, const float *grad_alpha, float *grad_means,
                                         float *grad_quats, float *grad_scales, float *grad_features, float *grad_opacities,
                                         float *grad_screen, int32_t *status, void *workspace, size_t workspace_bytes,
                                         void *bwd_workspace, size_t bwd_bytes, void *stream);

/*
 * Fused softmax cross-entropy on the splatted logits: the loss of one view against a per-pixel target map, computed in the
 * blend's own epilogue, and its backward without a gradient image.  Added after VP_ABI_VERSION 4 without changing it or
 * any existing entry point; detect the three functions by symbol.  tests/splat_loss_reference.py states it in float64.
 *
 * The contract, with C_p the D blended logits of pixel p exactly as vp_splat_rasterize computes them (same branch, same fp32
 * operations, same bits):
 *   Targets and weights: target i32 [H,W], pixel_weight f32 [H,W] or NULL (read as 1).  Pixel p is valid when
 *     0 <= target[p] < D; every other value (-1, 255, ...) means ignored: weight 0, loss 0, no gradient.
 *   Per-pixel loss, fp32, channels ascending:  m = max_c C_c,  l_p = (m + logf(sum_c expf(C_c - m))) - C_t  (the precise
 *     expf / logf, the maximum and the sum of the confidence epilogue).  A pixel nothing reaches has C = 0 and l = log D; it
 *     is valid unless its target says otherwise.
 *   loss_stats (device f64 [2]) = {sum_p w_p l_p, sum_p w_p} over the valid pixels: the fp32 values w_p l_p and w_p summed
 *     in float64 in a fixed order (a halving tree over a tile's 256 pixels, then the tiles in ascending tile index).  A
 *     valid pixel of weight exactly 0 contributes exactly 0, whatever its l.  No atomics: bit-identical from run to run.
 *   pixel_loss (f32 [H,W], optional) = w_p l_p, 0 where ignored.  labels, confidence, alpha, logits: vp_splat_rasterize's,
 *     bit for bit; each may be NULL in this call, labels included.
 *   Gradient: s = grad_loss (device f32 [1], NULL = 1) for VP_LOSS_SUM, and s = (float)(grad_loss / sum w) (the quotient
 *     in float64) for VP_LOSS_MEAN, where sum w = loss_stats[1]; sum w = 0 gives s = 0: gradients of exactly 0, and the mean
 *     loss is defined as 0.  The upstream gradient of the logits is, in fp32,
 *       G[c,p] = (s w_p) (expf(C_c - m) / sum - [c = t_p])   on valid pixels, 0 elsewhere.
 *     grad_alpha is optional as in the backward above.  From G on, the contract is vp_splat_rasterize_backward's and
 *     vp_splat_rasterize_backward_geometry's: same formulas, same zero rows, same fixed-order partials, same determinism.
 *   Two arms supply C_p: with logits = NULL the tile sweep blends the pixel again before its two sweeps (replay: no image
 *     is kept between forward and backward); otherwise C_p is read from `logits`, the planar image the forward call wrote
 *     (saved).  Both arms give bit-identical gradients.
 *
 * vp_splat_loss_workspace_bytes: bytes of the forward's per-tile pairs, 256-byte rounded; 0 when W or H is outside
 *   [1, 32768].  Needs no GPU.
 *
 * vp_splat_rasterize_loss: vp_splat_rasterize (after vp_splat_project on the same workspace; sorts `capacity` keys once)
 *   with the loss epilogue.  Asynchronous on `stream`, no allocation, no host synchronisation.  When the device count
 *   exceeds `capacity` nothing is written (loss_stats included) and *status is set to 1.  Refused on the host as
 *   vp_splat_rasterize refuses (labels may be NULL here), plus VP_EINVAL for a NULL target or loss_stats and VP_EWORKSPACE
 *   for a loss workspace that is NULL, not 256-byte aligned or smaller than vp_splat_loss_workspace_bytes.
 *
 * vp_splat_loss_backward: after vp_splat_rasterize_loss (or vp_splat_rasterize) on this workspace with the same
 *   n_gaussians, W, H, capacity, features and stream; target and pixel_weight as in the forward.  reduction is VP_LOSS_SUM
 *   or VP_LOSS_MEAN; loss_stats (the forward's) is read only for VP_LOSS_MEAN, on the device.  Without grad_means,
 *   grad_quats, grad_scales and grad_screen it runs the sweep of vp_splat_rasterize_backward, with `bwd_workspace`
 *   measured by vp_splat_backward_workspace_bytes; otherwise that of vp_splat_rasterize_backward_geometry, measured by
 *   vp_splat_geometry_backward_workspace_bytes.  grad_features and grad_opacities are bit-identical between the two.
 *   means, quats, scales and the camera (viewmat in HOST memory) are read only when grad_means, grad_quats or grad_scales
 *   is asked for.  Every output is written only when its pointer is not NULL.  When the device count exceeds `capacity`
 *   nothing is written and *status is set to 1.  Asynchronous on `stream`, no allocation, no host synchronisation.
 *   Refused on the host as vp_splat_rasterize_backward_geometry refuses, plus VP_EINVAL for a NULL target, a NULL
 *   loss_stats or an unknown reduction.
 */
#define VP_LOSS_SUM 0
#define VP_LOSS_MEAN 1
size_t vp_splat_loss_workspace_bytes(int W, int H);
int vp_splat_rasterize_loss(const float *features, int D, int64_t row_stride, int64_t n_gaussians, int W, int H,
                            int64_t capacity, const int32_t *target, const float *pixel_weight, double *loss_stats,
                            float *pixel_loss, int32_t *labels, float *confidence, float *alpha, float *logits,
                            int32_t *status, void *workspace, size_t workspace_bytes, void *loss_workspace,
                            size_t loss_bytes, void *stream);
int vp_splat_loss_backward(const float *means, const float *quats, const float *scales, const float *features, int D,
                           int64_t row_stride, int64_t n_gaussians, const float *viewmat, float fx, float fy, float cx,
                           float cy, int W, int H, float eps2d, int64_t capacity, const int32_t *target,
                           const float *pixel_weight, const float *logits /* NULL = replay */, const double *loss_stats,
                           int reduction, const float *grad_loss, const float *grad_alpha, float *grad_means,
                           float *grad_quats, float *grad_scales, float *grad_features, float *grad_opacities,
                           float *grad_screen, int32_t *status, void *workspace, size_t workspace_bytes,
                           void *bwd_workspace, size_t bwd_bytes, void *stream);

/*
 * Lifting a 2D feature map onto the Gaussians: the transpose of the splatter for one view, accumulated into per-Gaussian
 * sums.  Added after VP_ABI_VERSION 4 without changing it or any existing entry point; detect the two functions by symbol.
 * tests/splat_lift_reference.py states the contract in float64.
 *
 * The contract: with w_g(p) = a T the weight vp_splat_rasterize blends Gaussian g into pixel p with, decision for decision
 * (Gaussians in ascending (fp32 z, index) order; skipped when sigma < 0 or a < 1/255; the pixel stops before the Gaussian that
 * would take T to <= 1e-4, which is not added), and m_p the pixel's weight,
 *   sum[g * sum_stride + c] += sum_p m_p w_g(p) feat[p, c]      wsum[g] += sum_p m_p w_g(p).
 * The outputs accumulate and are never cleared: a caller adds view after view and divides at the end.  A sum of exactly 0 is
 * not added, so the rows of a culled Gaussian, and of one that no pixel added, keep their bits.  w_g(p) is fp32 and is
 * not rounded to binary16: the product runs on the matrix cores with the weight split into two binary16 terms that carry 22
 * bits of it (when the weights m_p of one 16x16 tile differ by more than 2^7 the smallest w_g(p) at the smallest m_p keep
 * fewer).  No float atomics: per-(tile, Gaussian) partials go to the pair's emission slot and are summed per Gaussian in
 * ascending slot order, so results are bit-identical from run to run.
 *
 * The map: feats_f16 is binary16, channels-last [H,W,C]: pixel p = y W + x starts at feats_f16 + p * pix_stride elements,
 *   pix_stride >= C, unit channel stride (what vp_upsample_features writes with dst_is_f16).  C in [1, 4096].  16-byte loads
 *   are used when C and pix_stride are multiples of 8 and the base is 16-byte aligned; any other layout is read element by
 *   element.  pixel_weight f32 [H,W] or NULL (read as 1), finite; a value that is not > 0 is read as 0.
 *   A pixel with m_p = 0 contributes nothing whatever its map holds (NaN included).  At every other pixel the map must be
 *   finite: a non-finite element there leaves channel c of `sum` unspecified for every Gaussian with a tile over that pixel
 *   (in a matrix product 0 * Inf is NaN, so Gaussians that never blended into the pixel are affected too).
 *
 * The workspace: the call runs after vp_splat_project on `workspace` with the same n_gaussians, W, H and stream.
 *   vp_splat_project leaves the records, the tile boxes, the counts, their scan and the device total; the sort
 *   (vp_splat_rasterize, vp_splat_rasterize_loss, or this call with sorted = 0) emits `capacity` keys, sorts them and writes
 *   the sorted values and every tile's run, which stay valid until the next vp_splat_project on the workspace.
 *   sorted = 0: the call sorts first, exactly as vp_splat_rasterize does; valid directly after vp_splat_project.
 *   sorted = 1: a vp_splat_rasterize or vp_splat_rasterize_loss call with the same capacity already sorted this workspace
 *     (the backward's precondition); the workspace is only read.  Any other value: VP_EINVAL.
 *
 * vp_splat_lift_workspace_bytes: bytes of the lift's own scratch; with Cc = 16 when C <= 16, else 64 (the channels of one
 *   pass) and n = max(capacity, 1):  round256(n * Cc * 4) + round256(n * 4)  -- one partial row of Cc floats and one weight
 *   partial per intersection.  0 when capacity is outside [0, 2^31 - 1] or C outside [1, 4096].  Needs no GPU.  Channels are
 *   processed in ceil(C / Cc) passes over this scratch; a larger lift_bytes is accepted and not used.
 *
 * vp_splat_lift: when the device count exceeds `capacity` nothing is written and *status (device i32, may be NULL; not
 *   reset) is set to 1.  wsum may be NULL.  Asynchronous on `stream`, no allocation, no host synchronisation, 64-bit offsets.
 *   VP_EINVAL: NULL feats_f16 or sum, C outside [1, 4096], pix_stride < C, sum_stride < C, a bad `sorted`, n_gaussians or
 *   capacity outside [0, 2^31 - 1], W or H outside [1, 32768].  VP_EWORKSPACE for either workspace: NULL, not 256-byte
 *   aligned, or smaller than its size function.  A refused call writes nothing.
 */
size_t vp_splat_lift_workspace_bytes(int64_t capacity, int C);
int vp_splat_lift(const void *feats_f16, int C, int64_t pix_stride, const float *pixel_weight, int64_t n_gaussians, int W,
                  int H, int64_t capacity, int sorted, float *sum, int64_t sum_stride, float *wsum, int32_t *status,
                  void *workspace, size_t workspace_bytes, void *lift_workspace, size_t lift_bytes, void *stream);

/*
 * Rendering wide per-Gaussian feature rows into a view: the splatter's forward for rows of up to 4096 channels, the
 * operation vp_splat_lift is the transpose of.  Added after VP_ABI_VERSION 4 without changing it or any existing entry
 * point; detect the function by symbol.  tests/splat_reference.py (splat64, any number of channels) states the contract in
 * float64.
 *
 * The contract: with w_g(p) = a T exactly the weight vp_splat_rasterize blends Gaussian g into pixel p with, decision for
 * decision (Gaussians in ascending (fp32 z, index) order; skipped when sigma < 0 or a < 1/255; the pixel stops before the
 * Gaussian that would take T to <= 1e-4, which is not added),
 *   out[p * pix_stride + c] = sum_g w_g(p) row[g, c]   for c < C,      alpha[p] = 1 - T.
 * Elements C .. pix_stride - 1 of a pixel are never touched.  A pixel nothing reaches gets C zeros (and alpha 0): every
 * pixel of the image is written by every accepted call.  alpha is f32 [H,W], may be NULL, and is bit-identical to the alpha
 * vp_splat_rasterize writes from the same workspace: it is the same fp32 chain.
 * w_g(p) is fp32 and is not rounded to binary16: the product runs on the matrix cores (v_mfma_f32_16x16x32_f16, the
 * Gaussians of a tile's run as the k dimension, fp32 accumulators held for the whole run and written once) with the
 * weight split into two binary16 terms that carry 22 bits of it, as vp_splat_lift stages it.  No float atomics, a fixed
 * order of every sum: results are bit-identical from run to run.  No scratch beyond the splat workspace.
 *
 * The rows: binary16 (rows_is_f16 = 1) or f32 (0), row g at rows + g * row_stride elements, row_stride >= C, unit channel
 *   stride; C in [1, 4096].  binary16 rows enter the product as they stand.  f32 rows are split into two binary16 terms as
 *   well, after an exact power-of-two scaling chosen per channel and per batch of 32 Gaussians of a run, so that any finite
 *   f32 value is representable and a small channel beside a large one keeps its own precision.  16-byte loads are used when
 *   C and row_stride are multiples of 8 (binary16) or 4 (f32) and the base is 16-byte aligned; any other layout is read
 *   element by element, with the same bits as the result.
 *   Rows of Gaussians that are in no tile's run (culled, or with an opacity below 1/255) are never read.  Every other row
 *   must be finite: a non-finite element in a row that is staged leaves channel c of `out` unspecified for every pixel of
 *   the tiles the Gaussian covers (in a matrix product 0 * Inf is NaN, so pixels that never blended the Gaussian are
 *   affected too).  Whether a row behind every pixel's stop is staged is not specified.
 *
 * The image: out is channels-last [H,W,C], pixel p = y W + x at out + p * pix_stride elements, pix_stride >= C, f32
 *   (out_is_f16 = 0) or binary16 (1): the fp32 result rounded once, to nearest even (torch's .half() of the f32 image, bit
 *   for bit); a magnitude above 65504 becomes Inf.  A [H W, C] binary16 image with its pixel stride is what
 *   vp_query_features takes as rows.
 *
 * Accuracy: for finite rows, on pixels where no decision lies within the oracle's fragile band (a relative 1e-5 of a
 *   threshold), every f32 output element is within  1e-4 * max_g |row[g, c]| + 1e-6 * max |row|  of the float64 value: the
 *   forward's bound (tests/test_gpu_splat.py), taken per channel.  Measured: 0.01 of that bound.
 *
 * The workspace: as for vp_splat_lift.  The call runs after vp_splat_project on `workspace` with the same n_gaussians, W, H
 *   and stream.  sorted = 0: the call sorts first, exactly as vp_splat_rasterize does; valid directly after
 *   vp_splat_project.  sorted = 1: vp_splat_rasterize, vp_splat_rasterize_loss, vp_splat_lift with sorted = 0 or this call
 *   with sorted = 0 already sorted this workspace with the same capacity; the workspace is only read.
 *
 * When the device count exceeds `capacity` nothing is written and *status (device i32, may be NULL; not reset) is set to
 *   1.  Asynchronous on `stream`, no allocation, no host synchronisation, 64-bit offsets.  n_gaussians = 0 is valid (zeros).
 *   VP_EINVAL: NULL rows or out, C outside [1, 4096], row_stride < C, pix_stride < C, sorted, rows_is_f16 or out_is_f16
 *   neither 0 nor 1, n_gaussians or capacity outside [0, 2^31 - 1], W or H outside [1, 32768].  VP_EWORKSPACE: a workspace
 *   that is NULL, not 256-byte aligned, or smaller than vp_splat_workspace_bytes.  A refused call writes nothing.
 */
int vp_splat_render(const void *rows, int rows_is_f16, int C, int64_t row_stride, int64_t n_gaussians, int W, int H,
                    int64_t capacity, int sorted, void *out, int out_is_f16, int64_t pix_stride, float *alpha,
                    int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Scoring label maps against ground truth: the confusion matrix of a predicted and a target label map, the boundary band
 * of a label map and the per-class boundary intersections and unions, from which the host forms mIoU, fwIoU, pixel accuracy
 * and boundary IoU.  Added after VP_ABI_VERSION 4 without changing it or any existing entry point; detect the three
 * functions by symbol.  Everything computed is an integer: results are exact and bit-identical from run to run (integer
 * atomics, whose sum does not depend on order).  tests/label_scores_reference.py states the contract in numpy.
 *
 * The contract, for maps of n = W x H pixels (i32, row-major [H,W]) and P classes:
 *   Valid: a label v is valid when 0 <= v < P; every other value (-1, 255, ...) is not.
 *   Confusion (device i64 [P,P], rows are ground truth): a pixel with a valid target t and a valid prediction p adds 1 to
 *     confusion[t * P + p].  A pixel whose target is not valid adds 1 to skipped[0]; one with a valid target and a
 *     prediction that is not valid adds 1 to skipped[1] (device i64 [2]).
 *   Boundary band (u8 [H,W]) of one map for a radius r: band[y,x] = 1 iff some (x', y') with |x' - x| <= r and |y' - y| <= r
 *     lies outside the image or holds a label different from labels[y,x]; 0 otherwise.  Labels that are not valid take part
 *     as labels of their own.  For every class c, band & (labels == c) is what r iterations of a 3 x 3 erosion of the
 *     zero-padded mask labels == c remove from it: a mask the image border truncates is boundary there.
 *   Boundary counts (device i64 [P] each), over the pixels with a valid target, with pband / tband the bands of the
 *     prediction and the target:
 *       bnd_inter[c] += [pred == c and pband and target == c and tband]
 *       bnd_union[c] += [(pred == c and pband) or (target == c and tband)]
 *     A pixel with pred = a != b = target and both in their bands counts in bnd_union[a] and in bnd_union[b]; a valid target
 *     under a prediction that is not valid contributes its target side only.
 *   Accumulation: confusion, skipped, bnd_inter and bnd_union are added to (+=), never cleared: a caller adds view after
 *     view and zeroes the buffers when it wants a per-view result.
 *
 * vp_label_scores_workspace_bytes: bytes of the scratch of either call, three 256-byte rounded planes of W x H bytes (the
 *   two bands and the row pass's map); 0 when W or H is outside [1, 32768].  Needs no GPU.
 *
 * vp_label_boundary: writes `band` for `labels` and `radius` in [1, 4096]; correct for a radius that exceeds W, H or both.
 *   Asynchronous on `stream`, no allocation, no host synchronisation.  VP_EINVAL on the host for a NULL labels or band, W or
 *   H outside [1, 32768] and a radius outside [1, 4096]; VP_EWORKSPACE for a workspace that is NULL, not 256-byte aligned or
 *   smaller than vp_label_scores_workspace_bytes.  A refused call writes nothing.
 *
 * vp_label_scores: adds one view to confusion and skipped and, with radius > 0, to bnd_inter and bnd_union (the bands of
 *   both maps are taken into the workspace first).  radius = 0 means confusion only: bnd_inter, bnd_union and the workspace
 *   are not touched and may be NULL.  Asynchronous on `stream`, no allocation, no host synchronisation.  VP_EINVAL on the
 *   host for a NULL pred, target, confusion or skipped; W or H outside [1, 32768]; P outside [1, 256]; radius outside
 *   [0, 4096]; radius > 0 with a NULL bnd_inter or bnd_union.  VP_EWORKSPACE, when radius > 0, as vp_label_boundary.  A
 *   refused call writes nothing.
 */
size_t vp_label_scores_workspace_bytes(int W, int H);
int vp_label_boundary(const int32_t *labels, int W, int H, int radius, uint8_t *band, void *workspace, size_t workspace_bytes,
                      void *stream);
int vp_label_scores(const int32_t *pred, const int32_t *target, int W, int H, int P, int radius, int64_t *confusion,
                    int64_t *skipped, int64_t *bnd_inter, int64_t *bnd_union, void *workspace, size_t workspace_bytes,
                    void *stream);

/*
 * The loss between a rendered feature image and a 2D feature map, and its gradient image in the binary16 form vp_splat_lift
 * reads: the two calls between vp_splat_render and vp_splat_lift that train per-Gaussian rows against feature maps.  Added
 * after VP_ABI_VERSION 4 without changing it or any existing entry point; detect the three functions by symbol.
 * tests/feature_loss_reference.py states the contract in float64.
 *
 * The maps, n = W x H pixels, pixel p = y W + x, unit channel stride, C in [1, 4096], W and H in [1, 32768], 64-bit offsets:
 *   image       channels-last [H,W,C], binary16 (image_is_f16 = 1) or f32 (0), pixel p at image + p * pix_stride elements,
 *               pix_stride >= C: what vp_splat_render writes.  Row o of a pixel below.
 *   target_f16  binary16 channels-last, pixel p at target_f16 + p * tgt_stride elements, tgt_stride >= C: what
 *               vp_upsample_features writes with dst_is_f16 and vp_splat_lift reads.  Row t of a pixel below.
 *   pixel_weight f32 [H,W] or NULL (read as 1): m_p; a value that is not > 0 (0, -0, negative, NaN) is read as 0.
 *   alpha       f32 [H,W] or NULL, with min_alpha: see validity.
 *   Elements C .. stride - 1 of a pixel are never read and never written.  16-byte loads and stores are used when C and
 *   the binary16 strides are multiples of 8, an f32 image's stride is a multiple of 4 and the bases are 16-byte aligned; any
 *   other layout is read and written element by element and gives the same bits.
 *
 * Validity: pixel p is valid when m_p > 0, and alpha is NULL or alpha[p] >= min_alpha, and, for the cosine kind, the fp32
 *   sums a = sum_c o_c^2 and b = sum_c t_c^2 are both > 0.  An invalid pixel has loss 0, weight 0 and a gradient row of exact
 *   zeros whatever its image or map holds, NaN included (vp_splat_lift's rule for m_p = 0); when the weight or alpha
 *   decides, its rows are not read at all.  At a valid pixel both rows must be finite.
 *
 * Per-pixel loss, fp32, with d = sum_c o_c t_c:
 *   VP_FEATURE_LOSS_COSINE   l_p = 1 - d / (sqrtf(a) sqrtf(b))
 *   VP_FEATURE_LOSS_L2       l_p = (sum_c (o_c - t_c)^2) / C
 *   Each sum is taken per lane over the lane's channels (lane L of 64 holds channels 512 j + 8 L .. + 7, j ascending) and
 *   then over the lanes in a butterfly: a fixed order, the same in every run and for both load paths.
 *   loss_stats (device f64 [2]) = {sum_p m_p l_p, sum_p m_p} over the valid pixels: the fp32 values m_p l_p and m_p summed in
 *     float64 in a fixed order (a halving tree over a workgroup's 256 consecutive pixels, then the workgroups in ascending
 *     index).  No float atomics: bit-identical from run to run (vp_splat_rasterize_loss's rule).
 *   pixel_loss (f32 [H,W], optional) = m_p l_p, 0 where invalid.
 *
 * Gradient of the image: s = grad_loss (device f32 [1], NULL = 1) for VP_LOSS_SUM, and s = (float)(grad_loss / sum m) (the
 *   quotient in float64, sum m = loss_stats[1] read on the device) for VP_LOSS_MEAN; sum m = 0 gives s = 0, an all-zero
 *   gradient, and the mean loss is defined as 0: exactly vp_splat_loss_backward's scalar.  For both kinds the row is a
 *   combination of the two rows,  G[p,c] = (s m_p) (A_p t_c + B_p o_c)  in fp32 as written, with
 *     cosine:  A = -1 / (|o| |t|),  B = cos / |o|^2  (|o| |t| = sqrtf(a) sqrtf(b), |o|^2 = a)        L2:  B = 2 / C,  A = -B.
 *   vp_feature_loss leaves {m_p (0 when invalid), A_p, B_p, m_p max_c |A_p t_c + B_p o_c|} per pixel in the workspace and the
 *   largest of the last over the map in its header (an integer atomic max over the bit patterns of these non-negative
 *   floats: the result does not depend on the order of arrival).
 *   vp_feature_loss_gradient derives the exponent on the device, by splat_autograd.quantize_gradient_map's rule:
 *   k = 14 - ceil(log2(|s| max)), at most 126; k = 0 and an image of zeros when |s| max is 0 (or not finite).  It writes
 *   grad_f16[p * grad_stride + c] = f16(G[p,c] 2^k) (grad_stride >= C; the product with 2^k is exact, the one rounding is the
 *   one to binary16, to nearest even) and *grad_exponent = k (device i32).  The image is vp_splat_lift's feats_f16 as it
 *   stands; the caller divides the lifted sums by 2^k.  The largest element lands in (2^13, 2^14] up to the last bit of
 *   (s m) v against s (m v).
 *   Scale hazard: with one exponent per map every element is rounded to 11 bits relative to the map's largest.  A near-empty
 *   pixel with a tiny |o| has a cosine gradient proportional to 1 / |o| and would take the exponent, flushing the rows of
 *   every other pixel towards zero.  alpha and min_alpha exist to exclude such pixels (pass vp_splat_render's alpha).
 *
 * vp_feature_loss_workspace_bytes: 256 + round256(16 ceil(W H / 256)) + round256(16 W H); 0 when W or H is outside
 *   [1, 32768].  Needs no GPU.
 * vp_feature_loss: writes loss_stats, pixel_loss when given, and the workspace.  Asynchronous on `stream`, no allocation,
 *   no host synchronisation.
 * vp_feature_loss_gradient: after vp_feature_loss on this workspace with the same image, target, C, W, H and stream (the
 *   kind, the weights and alpha reach it through the workspace, which it only reads).  loss_stats (the forward's) is read
 *   only for VP_LOSS_MEAN.  Writes C elements of every pixel of grad_f16, and grad_exponent.
 * Refused on the host, no GPU needed, nothing written: VP_EINVAL for a NULL image, target_f16 or loss_stats (and grad_f16 or
 *   grad_exponent), an unknown kind, reduction or image_is_f16, C, W or H out of range, a stride < C; VP_EWORKSPACE for a
 *   workspace that is NULL, not 256-byte aligned or smaller than vp_feature_loss_workspace_bytes.
 */
#define VP_FEATURE_LOSS_COSINE 0
#define VP_FEATURE_LOSS_L2     1
size_t vp_feature_loss_workspace_bytes(int W, int H);
int vp_feature_loss(const void *image, int image_is_f16, int64_t pix_stride, const void *target_f16, int64_t tgt_stride, int C,
                    int W, int H, const float *pixel_weight, const float *alpha, float min_alpha, int kind, double *loss_stats,
                    float *pixel_loss, void *workspace, size_t workspace_bytes, void *stream);
int vp_feature_loss_gradient(const void *image, int image_is_f16, int64_t pix_stride, const void *target_f16,
                             int64_t tgt_stride, int C, int W, int H, const double *loss_stats, int reduction,
                             const float *grad_loss, void *grad_f16, int64_t grad_stride, int32_t *grad_exponent,
                             void *workspace, size_t workspace_bytes, void *stream);

/*
 * The prototype-contrastive loss between a rendered identity image and one view's instance mask, and its gradient image:
 * the two calls between vp_splat_rasterize and vp_splat_rasterize_backward(_geometry) that train per-Gaussian identity rows
 * against masks whose ids mean nothing across views.  Added after VP_ABI_VERSION 4 without changing it or any existing
 * entry point; detect the three functions by symbol.  tests/proto_loss_reference.py states the contract in float64.
 *
 *   image, grad_image  f32 planar [D,H,W], contiguous: vp_splat_rasterize's logits and the backward's grad_logits as they
 *               stand.  D in [1, 64], W and H in [1, 32768], 64-bit offsets.  Row f_p of pixel p = y W + x below.
 *   ids         i32 [H,W]: the mask.        count  i32 [H,W] or NULL (read as 1): m_p, how many times pixel p was drawn.
 *
 * Samples: pixel p is a sample when m_p > 0, 0 <= ids[p] < VP_PROTO_MAX_IDS and ids[p] != ignore_id (-1: none).  Id k is
 *   active when n_k = sum_{p in k} m_p > min_count (integers); a sample of an inactive id is not valid; K = active ids.
 * Per pixel, fp32:  r_p = sqrtf(sum_c f_pc^2),  s_p = f_p / (r_p + 1e-6)  (the divisor is a constant for the gradient).
 * Per active id:    u_k = (sum_{p in k} m_p s_p) / n_k,
 *                   phi_k = clip(phi_scale sum_{p in k} m_p |s_p - u_k| / (n_k logf(n_k + 10)), phi_min, phi_max), a constant
 *                   for the gradient.
 * Loss:  z_pk = s_p . (u_k / phi_k) over the active k, c = the pixel's own id,  l_p = logf(sum_k expf(z_pk) + 1e-6) - z_pc,
 *   own_prob[p] = expf(z_pc) / (sum_k expf(z_pk) + 1e-6),  pixel_loss[p] = m_p l_p  (both optional, both exactly 0 at a pixel
 *   that is not a valid sample).
 *   stats (device f64 [4]) = {sum_p m_p l_p, K, sum_p (r_p - 1)^2 over ALL W H pixels, sum m_p over the valid samples}.
 * Order: no float atomics.  Every sum over pixels runs over tiles of 256 consecutive pixels; workgroup b of
 *   G = min(tiles, 768) takes tiles b, b + G, ..., adds a tile's samples in ascending pixel order, and the workgroups' sums
 *   are added in one fixed shape: 16 chunks of 48 consecutive workgroups, each in ascending b, then the 16 chunk sums in
 *   ascending order (a workgroup at or beyond G adds nothing).  The two statistics are fp32 terms added in float64: a halving tree over the
 *   workgroup's 256 threads, then a halving tree over 1024 slots, one per workgroup.  Every output is bit-identical from run to run.
 * Gradient of  L = weight_contrast (sum_p m_p l_p) / K + weight_norm (sum_p (r_p - 1)^2) / (W H), times grad_loss (device f32
 *   [1], NULL = 1), through the prototypes:  with P_pk the softmax above (its 1e-6 included), q_pk = P_pk - [k = c_p] at a
 *   valid sample and 0 elsewhere, g_k = (sum_p m_p q_pk s_p) / phi_k,
 *     dL/ds_p = (weight_contrast / K) m_p (sum_k q_pk u_k / phi_k + g_c / n_c),
 *     grad_image[c,p] = grad_loss (dL/ds_pc / (r_p + 1e-6) + (weight_norm / (W H)) 2 (r_p - 1) f_pc / r_p),
 *   the norm term 0 where r_p = 0, the contrastive part exactly 0 when K = 0.  Every element of grad_image is written.
 *
 * vp_proto_contrast_workspace_bytes: host arithmetic, 0 when D, W or H is out of range.  At most 18 KiB + 3 KiB D + 768 (3 KiB + 1 KiB D).
 * vp_proto_contrast: three reads of the image (the second and third of valid samples' rows only).  Leaves u / phi, g / n, K
 *   and the active list in the workspace.  Asynchronous on `stream`, no allocation, no host synchronisation.
 * vp_proto_contrast_gradient: after vp_proto_contrast on this workspace with the same image, D, W, H, ids, count and
 *   stream; it only reads the workspace (ignore_id and min_count reach it through the active list).  One read, one write.
 * Refused on the host, no GPU needed, nothing written: VP_EINVAL for a NULL image, ids, stats or grad_image, D, W or H out
 *   of range, min_count < 0, a non-finite phi_*, phi_min <= 0, phi_max < phi_min, a non-finite weight; VP_EWORKSPACE for a
 *   workspace that is NULL, not 256-byte aligned or smaller than vp_proto_contrast_workspace_bytes.
 */
#define VP_PROTO_MAX_IDS 256
size_t vp_proto_contrast_workspace_bytes(int D, int W, int H);
int vp_proto_contrast(const float *image, int D, int W, int H, const int32_t *ids, const int32_t *count, int ignore_id,
                      int min_count, float phi_scale, float phi_min, float phi_max, double *stats, float *pixel_loss,
                      float *own_prob, void *workspace, size_t workspace_bytes, void *stream);
int vp_proto_contrast_gradient(const float *image, int D, int W, int H, const int32_t *ids, const int32_t *count,
                               float weight_contrast, float weight_norm, const float *grad_loss, float *grad_image,
                               void *workspace, size_t workspace_bytes, void *stream);

/*
 * A code book of global instance labels against a rendered identity image and one view's instance mask: the id-by-code
 * score matrix that a linear assignment turns into "virtual labels", and the cross-entropy / clustering loss against those
 * labels with its gradient with respect to the code book (the image is a constant).  Added after VP_ABI_VERSION 4 without
 * changing it or any existing entry point; detect the three functions by symbol.  tests/codebook_reference.py states the
 * contract in float64.
 *
 *   image     f32 planar [D,H,W], contiguous: vp_splat_rasterize's logits.  D in [1, 64], W and H in [1, 32768], 64-bit
 *             offsets.  Row f_p of pixel p = y W + x below; the raw row enters the logits.
 *   ids       i32 [H,W]: the mask.       codebook  f32 [K,D], K in [1, VP_CODEBOOK_MAX_CODES].
 *   conf      f32 [H,W] or NULL: a confidence map (vp_proto_contrast's own_prob).
 *
 * Pixel p is valid when 0 <= ids[p] < 256 and ids[p] != ignore_id (-1: none); confident when valid and (conf is NULL or
 *   conf[p] > conf_min).  All arithmetic fp32:  z_pk = sum_c B_kc f_pc,  P_pk = expf(z_pk - max_k z_pk) / sum_k of the same,
 *   pred[p] = argmax_k z_pk (lowest k on exact ties; -1 at a pixel that is not valid),  r_p = sqrtf(sum_c f_pc^2),
 *   s_p = f_p / (r_p + 1e-6).
 *
 * vp_codebook_assoc:  score f64 [256,K]: score[l,k] = sum over valid p with ids[p] = l of P_pk;  id_pixels i32 [256]: the
 *   valid pixels per id;  pred i32 [H,W] or NULL.  Every element of every output is written.
 * vp_codebook_loss:  assign i32 [256] on the device maps id -> code, a value outside [0, K) meaning "takes no part";
 *   v_p = assign[ids[p]]; a pixel takes part when it is confident and v_p is a code.
 *   stats f64 [4] = {sum over participating p of (max_k z_pk + logf(sum_k expf(z_pk - max)) - z_pv): the cross-entropy
 *                    without an epsilon,
 *                    sum over participating p of |s_p - B_v|_2,
 *                    the participating pixels,
 *                    the valid pixels whose v_p is a code and pred[p] != v_p, confident or not}.
 *   grad_cls f32 [K,D] = sum over participating p of (P_pk - [k = v_p]) f_p.
 *   grad_cluster f32 [K,D]: row k = sum over participating p with v_p = k of (B_k - s_p) / |s_p - B_k|_2, a term being 0
 *     where the distance is 0.  Both are unscaled sums of the gradients of stats[0] and stats[1]; the caller scales them.
 *   pixel_loss f32 [H,W] or NULL: the cross-entropy term, exactly 0 where a pixel takes no part.
 *   One deliberate difference from the method this follows: there the pixels of an id that received no code (more ids than
 *   codes) train towards code 0, an artefact of initialising the label image with zeros.  Here they take no part.
 * Order: no float atomics.  Tiles are 64 consecutive pixels; with T = ceil(tiles / 256), workgroup b of G = ceil(tiles / T)
 *   takes tiles b T .. (b + 1) T - 1 in ascending order.  score: per workgroup and code, the probabilities of the valid
 *   pixels in ascending order, a run of one id summed in fp32 from 0 and added to the workgroup's fp32 sum of that id when
 *   the id changes; then the workgroups' sums in float64 in ascending b.  The gradients: per workgroup, fp32 accumulation
 *   over its tiles in ascending order, each tile in 16 steps of four pixels (step (q, i), q = 0 .. 3, i = 0 .. 3, takes
 *   pixels 16 q + i + {0, 4, 8, 12} of the tile in one matrix instruction); then the workgroups' sums in float64 in
 *   ascending b, rounded to fp32 once.  stats: fp32 terms added in float64, per lane in tile order, a halving tree over the
 *   workgroup's 256 threads, the workgroups in ascending b.  Every output is bit-identical from run to run.
 *
 * vp_codebook_workspace_bytes: host arithmetic, 0 when D, K, W or H is out of range.  One workspace serves both calls.  At
 *   most G (1 KiB K + 2 KiB + 8 K D bytes + 256 bytes) with G = min(tiles, 256): 64.5 MiB + 32 MiB at K = 256, D = 64 on an
 *   image of 16384 pixels or more, 72.5 MiB at D = 16, and proportional to the number of tiles below that.
 * Both calls are asynchronous on `stream`, allocate nothing and do not synchronise with the host; the workspace may be
 *   recycled memory (nothing in it is read before it is written).
 * Refused on the host, no GPU needed, nothing written: VP_EINVAL for a NULL image, ids, codebook, score, id_pixels, stats,
 *   assign, grad_cls or grad_cluster, for D, K, W or H out of range and for a non-finite conf_min; VP_EWORKSPACE for a
 *   workspace that is NULL, not 256-byte aligned or smaller than vp_codebook_workspace_bytes.
 */
#define VP_CODEBOOK_MAX_CODES 256
size_t vp_codebook_workspace_bytes(int D, int K, int W, int H);
int vp_codebook_assoc(const float *image, int D, int W, int H, const int32_t *ids, int ignore_id, const float *codebook, int K,
                      double *score, int32_t *id_pixels, int32_t *pred, void *workspace, size_t workspace_bytes, void *stream);
int vp_codebook_loss(const float *image, int D, int W, int H, const int32_t *ids, int ignore_id, const float *conf,
                     float conf_min, const float *codebook, int K, const int32_t *assign, double *stats, float *grad_cls,
                     float *grad_cluster, float *pixel_loss, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * k nearest OTHER points (csrc/vp_knn.h) and the 3D neighbourhood regulariser built on them (csrc/vp_reg3d.h), the counterpart
 * of the reference's loss_cls_3d (utils/loss_utils.py:74-115).  Added after ABI version 4: detected by symbol.
 *
 * vp_knn_points: the point set bucketed on a uniform grid exactly as vp_nearest_voxel takes it (pts_sorted, perm,
 *   cell_start, grid_origin3, cell_size, nx ny nz; nx ny nz < 2^31).  queries f32 [M,3];  self_index i32 [M] or NULL: the
 *   original index of a point that is left out of that query's result (anything outside [0, N) leaves nothing out);
 *   1 <= k <= VP_KNN_MAX_K.  nbr_idx i32 [M,k], nbr_d2 f64 [M,k] or NULL: the k nearest points by the key (d2, original
 *   index), ascending; d2 is the float64 sum of squares of the float64-converted fp32 differences (vp_nearest_voxel's).
 *   Ties, coincident points included, go to the lowest index: the result is a function of the inputs alone and
 *   bit-identical from run to run.  Where fewer than k other points exist the tail is -1 / +inf.  The search is exact: shells
 *   of cells are visited until the k-th best d2 is no larger than (r cell_size)^2; queries outside the grid, grids one cell
 *   thick and far outliers terminate like vp_nearest_voxel.  Needs no workspace.  Asynchronous on `stream`.
 *   Refused on the host (VP_EINVAL): a NULL pts_sorted, perm, cell_start, grid_origin3, queries or nbr_idx, a bad grid,
 *   M < 0, k out of range.
 *
 * vp_neighbor_kl / vp_neighbor_kl_gradient.  logits z f32 [N,P] with `row_stride` floats between rows (>= P), 1 <= P <=
 *   VP_NEIGHBOR_KL_MAX_P; samples i32 [S] or NULL (NULL: every row in order, S = N); indices in [0, N), repeats allowed;
 *   nbr i32 [S,k-1]: the neighbours of every sample position, -1 (or anything outside [0, N)) = no neighbour, skipped.
 *   k counts the point itself, as the reference's k does (its cdist returns the point first, at distance 0, with a KL term of
 *   exactly 0): 2 <= k <= VP_NEIGHBOR_KL_MAX_K, the table holds the k - 1 others and the mean divides by k.
 *   With p_i = softmax(z_i) and eps = 1e-10:
 *       sum  = sum_s sum_j sum_c p_sc (log(p_sc + eps) - log(p_jc + eps)),      loss = scale / (S k P) sum   (0 when S = 0)
 *   forward:  row_lse f32 [N] = the log-sum-exp of every row (the gradient call reads it);  sample_loss f32 [S] or NULL: the
 *     sum's term of every sample position, unscaled;  stats f64 [2] = {sum, S}: the fp32 terms added in float64 in a fixed
 *     order.  The caller applies scale / (S k P).
 *   gradient:  grad_logits f32 [N,P] (`grad_stride` floats between rows), every row written, zeros for a row that nobody
 *     names:  with g the gradient with respect to the probabilities, a sample row receives log(p_s + eps) - log(p_j + eps) +
 *     p_s / (p_s + eps) per neighbour and a neighbour row - p_s / (p_j + eps) per sample position that lists it; then
 *     dz = scale / (S k P) grad_loss p (g - <g, p>), grad_loss f32 [1] on the device or NULL (1).  No float atomics: row i
 *     gathers first what it receives as a sample -- through smp_start i32 [N+1] / smp_entry i32 [S], the CSR form of "the
 *     sample positions that name row i" (both NULL when samples is NULL) -- then what it receives as a neighbour, through
 *     rev_start i32 [N+1] / rev_entry i32 [S (k-1)], the CSR form of "the entries s (k-1) + j of nbr that name row i"; within
 *     a row both lists are walked in the order given, so equal tables give equal bits.
 *   lanes: lanes per row, a power of two in [4, 64] with ceil(P / lanes) <= 4; 0 = the library's choice (the smallest power
 *     of two with 4 lanes >= P, eight for P in 9..16).  A test / measurement switch: every value computes the same sums in another association.
 *   vp_neighbor_kl_workspace_bytes(S): host arithmetic, 0 when S is out of range; the workspace may be recycled memory.
 *   Both calls are asynchronous on `stream`, allocate nothing and do not synchronise with the host.
 *   Refused on the host (VP_EINVAL / VP_EWORKSPACE), nothing written: a NULL logits, row_lse, stats, grad_logits, rev_start,
 *     a NULL table with S > 0, N, P, k, S, a stride or lanes out of range, S != N without samples, samples without
 *     smp_start / smp_entry, a non-finite scale, a workspace that is NULL, misaligned or too small.
 */
#define VP_KNN_MAX_K 15
#define VP_NEIGHBOR_KL_MAX_P 256
#define VP_NEIGHBOR_KL_MAX_K 16
int vp_knn_points(const float *pts_sorted, const int32_t *perm, const int32_t *cell_start, const double *grid_origin3,
                  double cell_size, int nx, int ny, int nz, const float *queries, const int32_t *self_index, int64_t M, int k,
                  int32_t *nbr_idx, double *nbr_d2, void *stream);
size_t vp_neighbor_kl_workspace_bytes(int64_t S);
int vp_neighbor_kl(const float *logits, int64_t N, int P, int64_t row_stride, const int32_t *samples, int64_t S,
                   const int32_t *nbr, int k, float *row_lse, float *sample_loss, double *stats, int lanes, void *workspace,
                   size_t workspace_bytes, void *stream);
int vp_neighbor_kl_gradient(const float *logits, int64_t N, int P, int64_t row_stride, const int32_t *samples, int64_t S,
                            const int32_t *nbr, int k, const float *row_lse, const int32_t *rev_start, const int32_t *rev_entry,
                            const int32_t *smp_start, const int32_t *smp_entry, double scale, const float *grad_loss,
                            float *grad_logits, int64_t grad_stride, int lanes, void *stream);

/*
 * The photometric loss between a rendered image and a photograph, L1 + D-SSIM, and its gradient image: the two calls between
 * vp_splat_rasterize and vp_splat_rasterize_backward(_geometry) that fit colours, opacities and geometry to photographs, the
 * counterpart of the reference's l1_loss and ssim (utils/loss_utils.py:15-71).  Added after VP_ABI_VERSION 4 without changing
 * it or any existing entry point; detect the three functions by symbol.  tests/photo_loss_reference.py states the contract
 * in float64.
 *
 *   image, target, ssim_map, grad_image  f32 planar [C,H,W], contiguous: vp_splat_rasterize's logits and the backward's
 *               grad_logits as they stand.  C in [1, 64], W and H in [1, 32768], 64-bit offsets, n = C W H.  Inputs must be finite.
 *
 * The window, per channel: w(i, j) = g[i] g[j], i, j = 0 .. 10, centred on (5, 5), with g[i] = fp32(exp(-(i - 5)^2 / 4.5))
 *   divided by the fp32 sum of the eleven, rounded to fp32 (the reference's gaussian(11, 1.5)):
 *     g[0] = g[10] = 0x1.0d956cp-10   g[1] = g[9] = 0x1.f1fe02p-8   g[2] = g[8] = 0x1.26eb18p-5   g[3] = g[7] = 0x1.bff0fep-4
 *     g[4] = g[6]  = 0x1.b43c3ep-3    g[5] = 0x1.10656p-2
 *   (The reference multiplies the two rows in fp32, so its 121 weights are these products rounded once more: a relative
 *   difference of at most 2^-24 per weight, far inside the error bounds of an fp32 evaluation.)
 *   Zero padding: a tap outside the image contributes nothing and the weights are not renormalised.
 * At centre q, with x = image, y = target, C1 = 0.01^2, C2 = 0.03^2 and every sum over the window:
 *     mu1 = sum w x,  mu2 = sum w y,  e11 = sum w x^2,  e22 = sum w y^2,  e12 = sum w x y,
 *     s1 = e11 - mu1^2,  s2 = e22 - mu2^2,  s12 = e12 - mu1 mu2,
 *     A1 = 2 mu1 mu2 + C1,  A2 = 2 s12 + C2,  B1 = mu1^2 + mu2^2 + C1,  B2 = s1 + s2 + C2,     m = A1 A2 / (B1 B2).
 *   All of it fp32: the eleven taps along a row in ascending order, then the eleven row sums down a column in ascending order.
 *
 * vp_photo_loss:  loss_stats (device f64 [3]) = {sum |x - y|, sum (x - y)^2, sum m} over all n elements;  ssim_map f32
 *   [C,H,W] or NULL receives m.  The caller's arithmetic on three numbers:
 *     loss = (1 - lambda) stats[0] / n + lambda (1 - stats[2] / n),     PSNR = -10 log10(stats[1] / n).
 *   Order: no float atomics.  The image is cut into tiles of 32 x 32 pixels per channel, tile index (c, tile row, tile column)
 *   ascending; the fp32 terms of a tile are added in float64 by a halving tree over its 1024 pixels (pixel (tx, ty) of the
 *   tile in slot 32 ty + tx, a pixel outside the image adding 0), then the tiles in ascending index (k_ordered_sum,
 *   csrc/vp_reduce.h).  Bit-identical from run to run, with or without ssim_map and workspace.
 *   workspace may be NULL: evaluation only.  The same stats bits, but the tiles are then walked by ONE workgroup, because there
 *   is nowhere to keep a sum per tile: slow on a large image, and nothing is left for a gradient call.  Otherwise the
 *   workspace holds vp_photo_loss_workspace_bytes and the forward leaves three f32 maps [3,C,H,W] at its start, followed
 *   by the tiles' sums:
 *     Q = dm/ds1 = -A1 A2 / (B1 B2^2),     R = dm/ds12 = 2 A1 / (B1 B2),
 *     P = 2 mu2 A2 / (B1 B2) - 2 mu1 A1 A2 / (B1^2 B2) - 2 mu1 Q - mu2 R      (dm/dmu1 with e11, e12 held).
 * vp_photo_loss_gradient: after vp_photo_loss on this workspace with the same image, target, C, W, H and stream; it only
 *   reads the workspace.  The window is symmetric, so with * the same zero-padded convolution
 *     d(sum m)/dx(p) = (w * P)(p) + 2 x(p) (w * Q)(p) + y(p) (w * R)(p),
 *     grad_image[c,p] = s (a sgn(x - y) - b d(sum m)/dx(p)),   a = fp32((1 - lambda) / n),  b = fp32(lambda / n) from float64,
 *   sgn(0) = 0, s = *grad_loss (device f32 [1], read on the device; NULL = 1).  Every element of grad_image is written.  No
 *   gradient flows to target.
 * vp_photo_loss_workspace_bytes: host arithmetic, 0 when C, W or H is out of range:
 *     align256(12 n) + align256(24 C ceil(W / 32) ceil(H / 32)).  The workspace may be recycled memory.
 * Both calls are asynchronous on `stream`, allocate nothing and do not synchronise with the host.  Traffic with a workspace:
 *   2 n reads + 3 n writes forward (+ n with ssim_map), 5 n reads + n writes backward, of 4 bytes.
 * Refused on the host, no GPU needed, nothing written: VP_EINVAL for a NULL image, target, loss_stats or grad_image, C, W or
 *   H out of range, a lambda_dssim that is not finite or outside [0, 1]; VP_EWORKSPACE for a non-NULL workspace that is not
 *   256-byte aligned or smaller than vp_photo_loss_workspace_bytes, and for a NULL workspace in the gradient call.
 */
size_t vp_photo_loss_workspace_bytes(int C, int W, int H);
int vp_photo_loss(const float *image, const float *target, int C, int W, int H, double *loss_stats, float *ssim_map,
                  void *workspace, size_t workspace_bytes, void *stream);
int vp_photo_loss_gradient(const float *image, const float *target, int C, int W, int H, float lambda_dssim,
                           const float *grad_loss, float *grad_image, void *workspace, size_t workspace_bytes,
                           void *stream);

/*
 * Adaptive density control: the step of the reference's training loop that changes the size of the point cloud
 * (train_unified_lift.py:463-473, scene/gaussian_model.py:399-608).  Per training view vp_densify_accumulate adds the
 * screen-space gradient of the visible Gaussians to a running statistic; every few hundred steps vp_densify_plan turns the
 * statistic into one decision per Gaussian and one source row per output row, vp_densify_rows moves every per-Gaussian array
 * (parameters and optimiser moments) in one launch and vp_densify_split writes the means and log-scales of the new cloud.
 * Added after VP_ABI_VERSION 4 without changing it or any existing entry point; detect the five functions by symbol.
 * tests/densify_reference.py states the contract in NumPy.  No float atomics: every result is bit-identical from run to run.
 * All calls are asynchronous on `stream`, allocate nothing and do not synchronise with the host.
 *
 * vp_densify_accumulate: after vp_splat_project (and the geometry backward that wrote grad_screen) of one view, on the same
 *   splat workspace, which is only read.  A Gaussian is VISIBLE when the projection gave it at least one tile: the rule by
 *   which the backward writes non-zero rows.  grad_screen f32 [N,5] (columns 0, 1 = dL/d mean2d in pixels).  Per visible g:
 *     grad_accum[g] += (float)(sqrt((double)gx gx (W/2)^2 + (double)gy gy (H/2)^2) * (double)scale)      (one fp32 addition)
 *     denom[g] += 1                                                                                       (i32)
 *     max_radius[g] = max(max_radius[g], (float)(3 sqrt(mid + sqrt(max(0.1, ((s00 - s11) / 2)^2 + s01^2)))))  when not NULL,
 *   mid = (s00 + s11) / 2, with s00, s01, s11 the float64 screen covariance of vp_splat_project's own chain for the means,
 *   quats, scales, viewmat, intrinsics and eps2d given (those of the project call; read only when max_radius is not NULL).
 *   W/2 and H/2 turn the pixel gradient into the NDC gradient the reference's threshold 0.0002 is stated in; scale undoes a
 *   caller's 1/k when a step averages k views.  The radius is the reference rasterizer's without its ceil: compared with >
 *   against an integer threshold it decides the same.  Invisible Gaussians are untouched.
 *   VP_EINVAL: NULL grad_screen / grad_accum / denom (N > 0), N outside [0, 2^31 - 1], W or H outside [1, 32768], a scale that
 *   is not finite, with max_radius a NULL geometry array or a bad camera / eps2d; VP_EWORKSPACE: a NULL, misaligned or too
 *   small workspace (vp_splat_workspace_bytes(N, W, H, 0)).
 *
 * vp_densify_plan: grad_accum f32 [N], denom i32 [N], max_radius f32 [N] or NULL, activated scales f32 [N,3] and opacities
 *   f32 [N] on the device; host floats grad_threshold (> 0), size_threshold (percent_dense x extent, rounded to fp32 by the
 *   caller), min_opacity, max_screen_size (0: the size rules are off), max_world_size (0.1 x extent).  N in [0, 2^30].
 *   The rule per Gaussian g, every comparison in fp32:
 *     gm    = denom ? grad_accum / (float)denom : 0        (a NaN counts as 0)
 *     smax  = fmaxf of the three scales
 *     sel   = gm >= grad_threshold;  clone = sel && smax <= size_threshold;  split = sel && smax > size_threshold
 *     low   = opacity < min_opacity;  on = max_screen_size > 0
 *     bigw(s) = on && s > max_world_size;  bigv = on && max_radius != NULL && max_radius[g] > max_screen_size
 *     the original survives    iff !split && !low && !bigv && !bigw(smax)
 *     one clone is emitted     iff clone && !low && !bigw(smax)
 *     two children are emitted iff split && !low && !bigw(smax * 0.625f)              (0.625f = 1 / (0.8 x 2), exact)
 *   Output order: the surviving originals in ascending index; the clones in ascending source index; child 0 of every
 *   emitting source in ascending index; child 1 likewise.  This is the reference's order (clone-append, split-append, remove
 *   the split sources, prune) with its prune folded in.  The one deliberate difference: the reference zeroes max_radii2D in
 *   densification_postfix before its prune reads it, so its screen-size rule never fires; here the rule is live for the rows
 *   that existed while the statistics were taken (new rows have no radius yet, as in the reference).
 *   src i32 [2N] and kind u8 [2N] (0 kept, 1 clone, 2 / 3 split child 0 / 1): rows [0, total) are written, the rest is left
 *   alone; total <= 2N always.  counts i64 [4] = {total, kept, clones, splitting sources}, on the device.
 *   The offsets come from one rocprim inclusive scan; vp_densify_plan_workspace_bytes(N) measures its scratch (0 when N is out
 *   of range).  VP_EINVAL / VP_EWORKSPACE as above; grad_threshold must be > 0 and the five floats not NaN.
 *
 * vp_densify_rows: resamples n_arrays (1 .. VP_DENSIFY_MAX_ARRAYS) arrays of 32-bit words (f32 or i32) in one launch.  For
 *   every array a and output row r < n_out:  dst_a[r] = src_a[src[r]] bit for bit when kind[r] == 0 or fill is
 *   VP_DENSIFY_COPY;  zeros when fill is VP_DENSIFY_ZERO and kind[r] != 0 (the Adam moments of new rows).  Widths 1 .. 4096
 *   words, strides >= width in words; only the `width` words of a row are written.  src and dst must not overlap.
 *   n_out is the host's copy of counts[0]: when the device's total differs, nothing is written and *status (device i32,
 *   may be NULL) becomes 1.  A source index outside [0, n_src) writes nothing for that row and raises the status too.
 *
 * vp_densify_split: out_means f32 [n_out,3] and out_log_scales f32 [n_out,3] for all rows; kinds 0 and 1 copy bit for bit.
 *   For child c (kind 2 + c) of source g:  out_log_scale = log_scale[g] + fp32(ln 0.625) (one fp32 addition);  r0..r3 =
 *   Philox4x32-10 with counter (g, c, 0, 0) and key (seed & 0xffffffff, seed >> 32);  u_i = (r_i + 0.5) 2^-32;
 *   xi0 = sqrt(-2 ln u0) cos(2 pi u1), xi1 the same with sin, xi2 = sqrt(-2 ln u2) cos(2 pi u3);  s = exp((double)log_scale[g]);
 *   out_mean = (float)(mean[g] + R(q / |q|) (s * xi)), all float64, rounded once.  The same seed and inputs give the same bits.
 *   n_out / status as vp_densify_rows.
 */
#define VP_DENSIFY_MAX_ARRAYS 16
#define VP_DENSIFY_MAX_WIDTH 4096
#define VP_DENSIFY_COPY 0
#define VP_DENSIFY_ZERO 1
typedef struct {
    const void *src;         /* [n_src, src_stride] 32-bit words */
    void *dst;               /* [n_out, dst_stride] */
    int32_t width;           /* words of a row that are moved */
    int32_t fill;            /* VP_DENSIFY_COPY or VP_DENSIFY_ZERO */
    int64_t src_stride, dst_stride;   /* in words, >= width */
} vp_densify_array;
int vp_densify_accumulate(const float *grad_screen, int64_t n_gaussians, int W, int H, float scale, const float *means,
                          const float *quats, const float *scales, const float *viewmat, float fx, float fy, float cx,
                          float cy, float eps2d, float *grad_accum, int32_t *denom, float *max_radius, const void *workspace,
                          size_t workspace_bytes, void *stream);
size_t vp_densify_plan_workspace_bytes(int64_t n_gaussians);
int vp_densify_plan(const float *grad_accum, const int32_t *denom, const float *max_radius, const float *scales,
                    const float *opacities, int64_t n_gaussians, float grad_threshold, float size_threshold, float min_opacity,
                    float max_screen_size, float max_world_size, int32_t *src, uint8_t *kind, int64_t *counts, void *workspace,
                    size_t workspace_bytes, void *stream);
int vp_densify_rows(const vp_densify_array *arrays, int n_arrays, const int32_t *src, const uint8_t *kind,
                    const int64_t *counts, int64_t n_src, int64_t n_out, int32_t *status, void *stream);
int vp_densify_split(const float *means, const float *quats, const float *log_scales, int64_t n_src, const int32_t *src,
                     const uint8_t *kind, const int64_t *counts, int64_t n_out, uint64_t seed, float *out_means,
                     float *out_log_scales, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VOXPROJ_H */

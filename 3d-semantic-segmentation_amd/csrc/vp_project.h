// vp_project.h -- host side of the projector (vp_project_features, _f16, vp_first_hit_ids): one per-call context and the stages
// a call goes through.  A projecting call: project_check, project_pick_set, project_tables, project_plan, project_march (or,
// with VP_FLAG_GATHER_ONLY, project_relist), project_gather, project_commit.  A march-only call stops behind project_march.
// The drivers are in voxproj.hip; every stage returns VP_OK or the refusal, and any early return withdraws has_hit (HitGuard).
#pragma once

namespace {

// rows in flight per wavefront in the fp16 gather
#ifndef VP_F16_U
#define VP_F16_U 4
#endif

// The row variant <R, VEC, U> of k_gather, k_gather_one and k_combine_parts for a call, handed to f as three
// std::integral_constants; vec_ok: 0 = scalar fp32 path, 1 = 16-byte vector fp32 path, 2 = fp16 feature maps.  A kernel with
// a fourth template argument gets it from its call site.
template <class F>
inline void project_with_rows(int vec_ok, int C, F &&f)
{
    using std::integral_constant;
    if (vec_ok == 2) f(integral_constant<int, 1>{}, integral_constant<int, 8>{}, integral_constant<int, VP_F16_U>{});
    else if (vec_ok && C > 256) f(integral_constant<int, 2>{}, integral_constant<int, 4>{}, integral_constant<int, 4>{});
    else if (vec_ok) f(integral_constant<int, 1>{}, integral_constant<int, 4>{}, integral_constant<int, 4>{});
    else f(integral_constant<int, 4>{}, integral_constant<int, 1>{}, integral_constant<int, 4>{});
}

struct ProjectCall {
    // the caller's arguments (march-only calls: feats, count, out, views_hit NULL and C = 1)
    const float *feats; bool f16; const int64_t *occ; const float *vmi, *intr, *opts_host;
    int32_t *count; float *out; int32_t *views_hit;
    const float *grid_origin_host; float voxel_size;
    int B, V, H, W, C, dimz, dimy, dimx; int64_t n_rows;
    void *workspace; size_t workspace_bytes; hipStream_t s0; int flags;
    // project_check
    WsState *rec = nullptr;            // the workspace's record (set by the driver, in front of the HitGuard)
    Params p = {};
    Layout l = {};
    LastCall now = {};                 // this call, as the next VP_FLAG_GATHER_ONLY call will compare it
    bool pipe = false, gather_only = false;
    // project_pick_set: the buffer set, the stream of phase 1, and the workspace's buffers (those of set q where there are two)
    int q = 0;
    hipStream_t s1 = nullptr;
    int *status = nullptr, *status0 = nullptr, *cell_of_id = nullptr, *occ_copy = nullptr, *cnt_call = nullptr, *heavy_list = nullptr;
    int *work = nullptr, *hit = nullptr, *hit_waves = nullptr;
    unsigned long long *mask64 = nullptr;
    NearRec *near2 = nullptr;
    unsigned char *dist = nullptr, *dist_tmp = nullptr;
    ViewEntry *viewtab = nullptr;
    int4 *parts = nullptr, *split = nullptr, *pmeta = nullptr;
    float *prow = nullptr;
    // project_tables
    unsigned expect_tables = 0;
    // project_plan (march-only calls keep these: nothing is split, no hits are counted)
    SplitPlan sp = {{2147483647, 2147483647, 0, 1, 0, 0, 0, 0}, 2147483647, false, false, false};
    bool ranged = false;
    long long row_lo = 1, row_hi = 0;
};

struct HitGuard { WsState *st; bool keep; ~HitGuard() { if (!keep) st->has_hit = false; } };

// the pointers every call needs
inline bool project_has_pointers(const ProjectCall &c)
{
    return c.occ && c.vmi && c.intr && c.opts_host && c.grid_origin_host && c.workspace;
}

// the workspace's occupancy tables were built for this call's grid and row count
inline bool project_tables_match(const ProjectCall &c)
{
    const WsState &rec = *c.rec;
    return rec.B == c.B && rec.dimz == c.dimz && rec.dimy == c.dimy && rec.dimx == c.dimx && rec.n_rows == c.n_rows;
}

// Every refusal that needs no launch, Params and Layout.  What VP_FLAG_GATHER_ONLY and vp_copy_hit_image rely on (first-hit
// images of the last call, its arguments) is valid only once a call has queued all of its launches: withdrawn when a call fails
// -- refused arguments, refused flag, HIP error -- so that a later gather-only call cannot match the call before the failed one
// (the driver's HitGuard).  VP_FLAG_REUSE_ACCEL is refused by project_tables, behind the drain of project_pick_set.
int project_check(ProjectCall &c)
{
    const int B = c.B, V = c.V, H = c.H, W = c.W, C = c.C, dimz = c.dimz, dimy = c.dimy, dimx = c.dimx, flags = c.flags;
    const int64_t n_rows = c.n_rows;
    WsState &rec = *c.rec;
    if (B <= 0 || V <= 0 || H <= 0 || W <= 0 || C <= 0 || dimz <= 0 || dimy <= 0 || dimx <= 0 || n_rows <= 0)
        return fail(VP_EINVAL, "non-positive dimension");
    if ((long long)B * V > 65535) return fail(VP_EINVAL, "B*V = %lld exceeds 65535", (long long)B * V);
    if ((long long)dimz * dimy * dimx >= (1ll << 31)) return fail(VP_EINVAL, "occupancy grid has >= 2^31 cells per batch");
    if ((long long)H * W >= (1ll << 31) || n_rows >= (1ll << 31)) return fail(VP_EINVAL, "image or row count >= 2^31");
    if ((flags & VP_FLAG_SYNC) && (flags & VP_FLAG_PIPELINE)) return fail(VP_EINVAL, "VP_FLAG_SYNC and VP_FLAG_PIPELINE exclude each other");
    Params &p = c.p;
    p.width = (int)(c.opts_host[0] + 0.5f);    // K.cu:403
    p.height = (int)(c.opts_host[1] + 0.5f);   // K.cu:404
    if (p.width != W || p.height != H)
        return fail(VP_EINVAL, "opts width/height (%d,%d) must equal the feature map's (%d,%d)", p.width, p.height, W, H);
    p.dmin = c.opts_host[2]; p.dmax = c.opts_host[3]; p.inc = c.opts_host[4];
    if (!(p.inc > 0.0f)) return fail(VP_EINVAL, "rayIncrement must be > 0 (the reference would never terminate)");
    p.ox = c.grid_origin_host[0]; p.oy = c.grid_origin_host[1]; p.oz = c.grid_origin_host[2];
    p.vs = c.voxel_size;
    p.dimz = dimz; p.dimy = dimy; p.dimx = dimx;
    p.B = B; p.V = V; p.C = C; p.n_rows = n_rows;

    c.l = make_layout(B, V, H, W, C, n_rows, dimz, dimy, dimx, c.workspace_bytes);
    if (c.workspace_bytes < c.l.total) return fail(VP_EWORKSPACE, "workspace has %zu bytes, need %zu", c.workspace_bytes, c.l.total);
    if ((uintptr_t)c.workspace & 255) return fail(VP_EWORKSPACE, "workspace must be 256-byte aligned");
    // (every check above is host arithmetic; from here on the device is touched)
    if (!sticky_open(rec)) return fail(VP_EHIP, "could not allocate the workspace record's page of pinned host memory (sticky error words)");

    c.pipe = (flags & VP_FLAG_PIPELINE) != 0;
    if (c.pipe && !pipe_open(rec.pipe)) return fail(VP_EHIP, "could not create the side stream / events for VP_FLAG_PIPELINE");
    // VP_FLAG_GATHER_ONLY: phase 2 once more, on another row range, from what the previous call's phase 1 left in ITS
    // buffer set; everything runs on the caller's stream, behind that call's gather
    c.gather_only = (flags & VP_FLAG_GATHER_ONLY) != 0;
    c.now.feats = c.feats; c.now.out = c.out; c.now.count = c.count; c.now.vmi = c.vmi;
    c.now.B = B; c.now.V = V; c.now.H = H; c.now.W = W; c.now.C = C; c.now.f16 = c.f16;
    if (c.gather_only) {
        if (!rec.has_hit || !rec.last.matches(c.now) || !project_tables_match(c))
            return fail(VP_EINVAL, "VP_FLAG_GATHER_ONLY repeats phase 2 of the previous call on this workspace: there is none (or it "
                                   "failed), or its feature maps / poses / outputs / shapes differ from this call's");
        if (rec.opt_row_begin < 0 && rec.opt_row_end < 0)
            return fail(VP_EINVAL, "VP_FLAG_GATHER_ONLY without a row range (VP_OPT_ROW_BEGIN / VP_OPT_ROW_END) would gather every row twice");
        if (!rec.last.ranged)
            return fail(VP_EINVAL, "VP_FLAG_GATHER_ONLY after a call that had no row range: that call gathered every row already");
    }
    return VP_OK;
}

// buffer set and streams: plain calls use set 0 on the caller's stream only; pipelined calls alternate sets and run phase 1 on
// the side stream; a gather-only call stays on its predecessor's set
int project_pick_set(ProjectCall &c)
{
    PipeState &ps = c.rec->pipe;
    c.q = 0;
    c.s1 = c.s0;
    if (c.gather_only) {
        c.q = c.rec->last_q;
    } else if (c.pipe) {
        c.q = (int)(ps.calls & 1);
        c.s1 = ps.side;
    } else if (ps.ok && (ps.used[0] || ps.used[1])) {
        // a plain call after pipelined ones on this workspace: drain the side streams first
        VP_HIP(hipStreamSynchronize(ps.side));
        ps.used[0] = ps.used[1] = false;
    }
    char *ws = (char *)c.workspace;
    const Layout &l = c.l;
    const int q = c.q;
    c.status = (int *)(ws + l.status[q]);
    c.status0 = (int *)(ws + l.status[0]);      // header + sticky words live in the block of set 0
    c.cell_of_id = (int *)(ws + l.cell_of_id);
    c.mask64 = (unsigned long long *)(ws + l.mask64);
    c.near2 = (NearRec *)(ws + l.near2);
    c.dist = (unsigned char *)(ws + l.dist);
    c.dist_tmp = (unsigned char *)(ws + l.dist_tmp);
    c.occ_copy = (int *)(ws + l.occ_copy);
    c.cnt_call = (int *)(ws + l.cnt_call[q]);
    c.heavy_list = (int *)(ws + l.heavy[q]);
    c.work = (int *)(ws + l.work[q]);
    c.viewtab = (ViewEntry *)(ws + l.viewtab[q]);
    c.hit = (int *)(ws + l.hit[q]);
    c.parts = (int4 *)(ws + l.parts[q]); c.split = (int4 *)(ws + l.split[q]); c.pmeta = (int4 *)(ws + l.pmeta[q]);
    c.prow = (float *)(ws + l.prow[q]);
    c.hit_waves = (int *)(ws + l.hitcnt[q]);
    return VP_OK;
}

// Occupancy-derived tables: rebuilt unless the caller vouches for them (VP_FLAG_REUSE_ACCEL) or asks for a
// check (VP_FLAG_VERIFY_ACCEL, blocking calls only): then the grid is compared with the copy the tables were
// built from, and they are rebuilt only if a cell changed.
int project_tables(ProjectCall &c)
{
    const int B = c.B, dimz = c.dimz, dimy = c.dimy, dimx = c.dimx, flags = c.flags;
    const int64_t n_rows = c.n_rows;
    const Layout &l = c.l;
    const bool pipe = c.pipe, gather_only = c.gather_only;
    hipStream_t s0 = c.s0;
    WsState &rec = *c.rec;
    PipeState &ps = rec.pipe;
    const long long cells = (long long)dimz * dimy * dimx;
    const bool rec_matches = project_tables_match(c);
    const bool verify = (flags & VP_FLAG_VERIFY_ACCEL) && !pipe && !gather_only && !(flags & VP_FLAG_REUSE_ACCEL);
    const int cmp_blocks = (int)((cells * B + 255) / 256 > 8192 ? 8192 : (cells * B + 255) / 256);
    bool rebuild = !gather_only && !(flags & VP_FLAG_REUSE_ACCEL);
    // VP_FLAG_REUSE_ACCEL is a promise about the tables in THIS workspace: refuse it when the library never built
    // them here (fresh or recycled memory) or built them for another grid shape / row count -- the march would leap on
    // garbage and silently miss hits
    if (!rebuild && !gather_only && (rec.builds == 0 || !rec_matches))
        return fail(VP_EINVAL, "VP_FLAG_REUSE_ACCEL, but this workspace holds no occupancy tables for a grid of this shape "
                               "(B, dims, n_rows): call once without the flag");
    if (rebuild || !rec.opened) {
        // The workspace header (magic, this record's generation) and the sticky error words: initialised by the first call
        // of a record and whenever the memory does not carry this record's generation (any more) -- decided on the
        // device, no read-back.  A call that trusts the tables never initialises: it must find the header intact.
        if (pipe && ps.ok) {
            VP_HIP(hipStreamSynchronize(ps.side));
        }
        hipLaunchKernelGGL(k_ws_open, dim3(1), dim3(64), 0, s0, c.status0, (int *)((char *)c.workspace + l.status[1]), WS_MAGIC, rec.gen, rebuild ? 1 : 0);
        rec.opened = true;
    }
    if (verify && rec_matches && rec.copy_valid) {
        // the verdict comes back through the record's page of pinned host memory (no memset, no device-to-host copy)
        volatile int *differs = rec.sticky_host + ST_OCCDIFF;
        *differs = 0;
        hipLaunchKernelGGL(k_occ_compare_copy, dim3(cmp_blocks), dim3(256), 0, s0, (const long long *)c.occ, c.occ_copy, cells * B, rec.sticky_dev + ST_OCCDIFF);
        VP_HIP(hipStreamSynchronize(s0));
        rebuild = *differs != 0;      // the copy is already up to date either way
    } else if (rebuild) {
        if (verify) {
            // first checked call on this workspace / new shape: take the copy now
            hipLaunchKernelGGL(k_occ_compare_copy, dim3(cmp_blocks), dim3(256), 0, s0, (const long long *)c.occ, c.occ_copy, cells * B, c.status + ST_OCCDIFF);
            rec.copy_valid = true;
        } else {
            rec.copy_valid = false;  // tables rebuilt without refreshing the copy
        }
    }
    if (rebuild) {
        // the tables are shared by both buffer sets: nothing of an earlier call may still be running
        if (pipe) {
            VP_HIP(hipStreamSynchronize(ps.side));
            VP_HIP(hipStreamSynchronize(s0));
        }
        ProfSpan sp; sp.begin(0, s0);
        VP_HIP(hipMemsetAsync(c.cell_of_id, 0xFF, size_t(B) * n_rows * sizeof(int), s0));
        VP_HIP(hipMemsetAsync(c.mask64, 0, size_t(B) * l.nblk * sizeof(unsigned long long), s0));
        const int blocks = (int)((cells * B + 255) / 256 > 16384 ? 16384 : (cells * B + 255) / 256);
        hipLaunchKernelGGL(k_build_cells, dim3(blocks), dim3(256), 0, s0, (const long long *)c.occ, c.cell_of_id,
                           c.mask64, dimz, dimy, dimx, l.nby, l.nbx, l.nblk, B, (long long)n_rows);
        const int db = (int)(((long long)l.nbz * l.nby * l.nbx * B + 255) / 256);
        hipLaunchKernelGGL(k_block_dist, dim3(db), dim3(256), 0, s0, c.mask64, (const unsigned char *)nullptr, c.dist, l.nbz, l.nby, l.nbx, l.nblk, B, 0);
        hipLaunchKernelGGL(k_block_dist, dim3(db), dim3(256), 0, s0, c.mask64, (const unsigned char *)c.dist, c.dist_tmp, l.nbz, l.nby, l.nbx, l.nblk, B, 1);
        hipLaunchKernelGGL(k_block_dist, dim3(db), dim3(256), 0, s0, c.mask64, (const unsigned char *)c.dist_tmp, c.dist, l.nbz, l.nby, l.nbx, l.nblk, B, 2);
        const long long near_waves = (long long)l.nbz * l.nby * l.nbx * B;
        hipLaunchKernelGGL(k_build_near, dim3((unsigned)((near_waves + 3) / 4)), dim3(256), 0, s0, c.mask64, (const unsigned char *)c.dist,
                           c.near2, dimz, dimy, dimx, l.nbz, l.nby, l.nbx, l.nblk, B);
        rec.B = B; rec.dimz = dimz; rec.dimy = dimy; rec.dimx = dimx; rec.n_rows = n_rows;
        rec.builds++;
        // seal: the header now names the tables this memory holds
        hipLaunchKernelGGL(k_ws_seal, dim3(1), dim3(1), 0, s0, c.status0, tables_key(B, dimz, dimy, dimx, n_rows, rec.builds));
        sp.end();
        if (pipe) VP_HIP(hipStreamSynchronize(s0));   // rare: the side stream must see the finished tables
    }
    c.expect_tables = tables_key(rec.B, rec.dimz, rec.dimy, rec.dimx, rec.n_rows, rec.builds);
    return VP_OK;
}

// The row range of phase 2 and the split plan (plan_split, vp_plan.h); host arithmetic only.
void project_plan(ProjectCall &c)
{
    const WsState &rec = *c.rec;
    // Row range of phase 2 (VP_OPT_ROW_BEGIN / _END).  The heavy list is the march's, i.e. the whole call's: the workgroup
    // role of a ranged gather skips the listed IDs outside its range, so the gathers of a split call share the list without
    // summing a voxel twice -- and every voxel is summed by the same role (and so to the same bits) as in the unsplit call.
    c.ranged = rec.opt_row_begin >= 0 || rec.opt_row_end >= 0;
    c.row_lo = std::max<long long>(1, rec.opt_row_begin);
    c.row_hi = rec.opt_row_end < 0 ? (long long)c.n_rows : std::min<long long>(rec.opt_row_end, (long long)c.n_rows);
    c.sp = plan_split(PlanIn{c.B, c.V, c.H, c.W, c.C, (c.flags & VP_FLAG_SERIAL_SUMS) != 0, rec.opt_heavy_t, rec.opt_part_px,
                             rec.opt_one_view, rec.opt_one_view_split});
    if (c.gather_only) {      // the thresholds of the call whose march is reused
        c.sp.plan = rec.last.plan;
        c.sp.heavy_t = c.sp.plan.heavy_t;
        c.sp.plans_parts = plan_has_parts(c.sp.plan);
    }
#ifdef VP_DIAG
    if (c.flags & VP_FLAG_DIAG_EVALS) c.sp.heavy_t = -1;      // diagnostic build only: the hit image then holds evaluation counts
    if (c.flags & VP_FLAG_DIAG_WAVES) c.sp.heavy_t = -2;      // ... per-wavefront clock stamps
#endif
}

// the gather's work list: touched voxels by size class, largest first (needs the finished histogram); its trailing
// workgroups compute the view table, which is phase 2's too
void project_list_work(const ProjectCall &c, hipStream_t stream)
{
    const int wl_blocks = (int)((c.n_rows + 256 * WL_PER_THREAD - 1) / (256 * WL_PER_THREAD));
    hipLaunchKernelGGL(k_worklist, dim3((unsigned)(wl_blocks + (c.B * c.V + 255) / 256)), dim3(256), 0, stream, (const int *)c.cnt_call,
                       c.sp.plan, (long long)c.n_rows, c.work, c.status, wl_blocks, c.vmi, c.viewtab, c.B * c.V, c.row_lo, c.row_hi,
                       c.parts, c.split, (int)c.l.slot_cap, c.rec->sticky_dev, (const int *)c.cell_of_id, (const int *)c.hit_waves,
                       (int)c.l.n_hitcnt);
}

// VP_FLAG_GATHER_ONLY in place of phase 1: the work list of the new row range, from the histogram the previous call's march left
int project_relist(ProjectCall &c)
{
    VP_HIP(hipMemsetAsync(c.status + ST_WORK0, 0, ST_PLAN_WORDS * sizeof(int), c.s0));
    project_list_work(c, c.s0);
    return VP_OK;
}

// Phase 1, on s1: the first-hit image into hit_dst (the buffer set's, or the caller's own for a march-only call) and the
// per-call histogram; list_work: the gather's work list behind it.
int project_march(ProjectCall &c, int *hit_dst, bool list_work)
{
    const Layout &l = c.l;
    const PlanArgs &plan = c.sp.plan;
    WsState &rec = *c.rec;
    PipeState &ps = rec.pipe;
    hipStream_t s1 = c.s1;
    const int q = c.q;
    // set q was last used two calls ago: its gather must be over before phase 1 overwrites hit/cnt
    if (c.pipe && ps.used[q]) VP_HIP(hipStreamWaitEvent(s1, ps.call_done[q], 0));
    {
        ProfSpan sp; sp.begin(0, s1);
        // one launch clears the per-call status words and the per-call histogram, and checks the workspace header
        hipLaunchKernelGGL(k_zero_call, dim3((unsigned)((c.n_rows + 1023) / 1024)), dim3(256), 0, s1, c.status, c.cnt_call, (long long)c.n_rows,
                           c.status0, rec.sticky_dev, WS_MAGIC, rec.gen, c.expect_tables, c.hit_waves,
                           plan.dyn_px_min > 0 ? l.n_hitcnt : 0ll);
        sp.end();
    }
    FirstHitArgs fa;
    fa.occ = (const long long *)c.occ; fa.vmi = c.vmi; fa.intr = c.intr; fa.near2 = c.near2; fa.dist = c.dist;
    fa.nby = l.nby; fa.nbx = l.nbx; fa.nblk = l.nblk; fa.hit = hit_dst; fa.cnt_call = c.cnt_call;
    fa.heavy_list = c.heavy_list;
    // (the march enlists heavy voxels for one-view calls without parts only)
    fa.heavy_t = ((c.sp.one_view && !c.sp.one_split) || c.sp.heavy_t < 0) ? c.sp.heavy_t : 2147483647;
    fa.hit_waves = (plan.dyn_px_min > 0 && l.n_hitcnt > 0) ? c.hit_waves : nullptr;
    fa.status = c.status; fa.sticky = rec.sticky_dev;
    const dim3 grid((c.W + 15) / 16, (c.H + 15) / 16, c.B * c.V);
    ProfSpan sp; sp.begin(1, s1);
    if (c.flags & VP_FLAG_EXACT_MARCH) {
        hipLaunchKernelGGL(k_first_hit<0>, grid, dim3(256), 0, s1, fa, c.p);
    } else {
        // Occupancy shaping for the pipelined mode: a 41-KiB dynamic-LDS reservation (the kernel does not touch
        // it) admits at most 3 march workgroups = 12 wavefronts per CU.  Spread that thin the march still
        // finishes under the gather of the previous call (40 ms vs 50 ms per R2 pass) and costs the gather
        // ~1 % instead of ~8 % (measured: mean 55.3 -> 53.5 ms per pass); alone it runs unrestricted.
        // Only while the previous call's gather is still queued or running: behind an idle GPU (first call of
        // a job, or after the caller synchronised) the march has nothing to spare and runs unrestricted.
        bool beside_gather = false;
        if (c.pipe && ps.used[q ^ 1]) {
            beside_gather = hipEventQuery(ps.call_done[q ^ 1]) == hipErrorNotReady;
            (void)hipGetLastError();   // hipErrorNotReady is an answer, not a failure
        }
        // Rows of up to 1 KiB (fp16 maps of 512 channels, fp32 maps of 256): the gather moves half the bytes per view, so a
        // march held to 3 workgroups per CU takes longer than the gather it hides under and becomes the critical path
        // (30.1 vs 29.2 ms per fp16 pass); 5 workgroups per CU (30 KiB) bring the pass from 33.1-33.7 to 29.5-31.6 ms,
        // 6 and 4 are worse (profiles/r03_march_occupancy_cap_sweep.log).
        const size_t row_bytes = size_t(c.C) * (c.f16 ? 2 : 4);
        size_t lds_req = beside_gather ? (row_bytes <= 1024 ? 30 : 41) * 1024 : 0;
        if (rec.opt_march_lds_kb >= 0) lds_req = size_t(std::min<long long>(rec.opt_march_lds_kb, 64)) * 1024;   // VP_OPT_MARCH_LDS_KB
        hipLaunchKernelGGL(k_first_hit<1>, grid, dim3(256), lds_req, s1, fa, c.p);
    }
    // the work list behind the march, not in front of it (in pipelined mode a kernel with that many registers waits for a
    // wavefront of the previous call's gather to retire)
    if (list_work) project_list_work(c, s1);
    sp.end();
    if (c.pipe) VP_HIP(hipEventRecord(ps.fh_done[q], s1));
    return VP_OK;
}

// the split voxels' partial rows -> their rows in `out`, in slot order
void project_combine(const ProjectCall &c, const GatherArgs &g, int vec_ok)
{
    ProfSpan sp; sp.begin(3, c.s0);
    const dim3 cgrid((unsigned)std::max<long long>(1, std::min<long long>(COMBINE_BLOCKS, c.l.slot_cap / 2)));
    project_with_rows(vec_ok, c.C, [&](auto R, auto VEC, auto U) {
        hipLaunchKernelGGL((k_combine_parts<decltype(R)::value, decltype(VEC)::value, decltype(U)::value>), cgrid, dim3(256), 0, c.s0, g, c.p);
    });
    sp.end();
}

// the one-view gather (vp_gather.h, k_gather_one) and, where the view has split voxels, k_combine_parts
void project_gather_one(ProjectCall &c, GatherArgs &g, int vec_ok)
{
    WsState &rec = *c.rec;
    const int64_t n_rows = c.n_rows;
    const bool plans_parts = c.sp.plans_parts;
    // a fixed number of workgroups per CU.  The kernel's registers admit 4 at a time; 16 are launched, so that the
    // dispatcher evens out what the static deal leaves uneven (one R2 view: 2 / 4 / 8 / 16 / 32 / 64 per CU -> 229 / 219 /
    // 210-226 / 217 / 220 / 222 us, R1: 99 / 95 / 87 / 83 / 83.5 / 82.6 us, profiles/r04_one_view_gather.log) -- a
    // quarter of the workgroups k_gather launches for the same call, none of them without work.
    // VP_OPT_ONE_VIEW_GATHER = n > 0 overrides it.
    ProfSpan sp; sp.begin(2, c.s0);
    const int per_cu = rec.opt_one_view > 0 ? (int)std::min<long long>(rec.opt_one_view, 256) : 16;
    // (values from 1000 on: a grid of exactly n - 1000 workgroups -- tests walk the batches of 64 entries per wavefront)
    const long long want = rec.opt_one_view >= 1000 ? rec.opt_one_view - 1000 : (long long)device_cus() * per_cu;
    const long long cap = (n_rows - 1 + 3) / 4;           // never more wavefronts than voxel IDs
    const unsigned nblk = (unsigned)std::max<long long>(1, std::min(want, cap));
    // every workgroup of the grid takes heavy voxels first (round 5; rounds 1-4: the first 128): on a close-up frame EVERY
    // voxel of the view is heavy -- 300-400 of them -- and 128 workgroups summed them three apiece while the rest of the grid
    // had nothing to deal (0.70 ms per call instead of 0.3, profiles/r05_dropin_trajectory.log)
    g.heavy_blocks = (c.sp.heavy_t != 2147483647 && !plans_parts) ? (int)nblk : 0;
    // A BLOCKING call (the drop-in module's) launches k_combine_parts only if the view has split voxels: most frames of a
    // walk through a room have none, and the empty launch is 6-7 us of a 0.14-0.3 ms call.  The gather's first wavefront
    // writes the count (final since k_worklist) into the record's pinned page, tagged with this call's sequence number; the
    // host, which would otherwise sleep in the stream synchronise, reads it a few microseconds into the gather -- long before
    // the gather ends.  Nothing depends on the note arriving: without it (2 ms) the launch goes out as for any other call.
    volatile int *note = nullptr;
    if ((c.flags & VP_FLAG_SYNC) && plans_parts && n_rows > 1) {
        rec.split_seq = (rec.split_seq + 1) & 0x7fffu;
        note = rec.sticky_host + ST_HOST_NSPLIT;
        *note = 0;
        g.host_word = rec.sticky_dev + ST_HOST_NSPLIT; g.host_seq = (int)rec.split_seq;
    }
    // SMALL: the view has few pixels (up to GATHER_G32_SMALL_IMAGE): a voxel gets a handful of rows and the launch is bounded
    // by the round trips per voxel, not by bandwidth -- 8 rows of 16-byte fp32 lanes in flight per wavefront instead of 4 (3
    // wavefronts per SIMD instead of 4): one R1 view 86.4 -> 75.5 us; one R2 view 225 -> 228 us, so large views keep 4
    // (profiles/r04_one_view_gather.log)
    const auto launch = [&](auto SMALL) {
        project_with_rows(vec_ok, c.C, [&](auto R, auto VEC, auto U) {
            constexpr int rows = (decltype(SMALL)::value && decltype(R)::value == 2) ? 8 : decltype(U)::value;
            hipLaunchKernelGGL((k_gather_one<decltype(R)::value, decltype(VEC)::value, rows>), dim3(nblk), dim3(256), 0, c.s0, g, c.p);
        });
    };
    if (n_rows > 1) {
        if ((long long)c.H * c.W <= GATHER_G32_SMALL_IMAGE) launch(std::true_type{});
        else launch(std::false_type{});
    }
    sp.end();
    bool combine = n_rows > 1 && plans_parts;
    if (combine && note) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spin = 0;; spin++) {
            const unsigned v = (unsigned)*note;
            if ((v >> 31) && ((v >> 16) & 0x7fffu) == rec.split_seq) { combine = (v & 0xffffu) != 0; break; }
            if ((spin & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
            __builtin_ia32_pause();
        }
    }
    if (combine) project_combine(c, g, vec_ok);
}

// k_gather: one wavefront per item of the work list, and k_combine_parts behind it (with VP_FLAG_SERIAL_SUMS nothing is
// split: the launch is left out)
void project_gather_views(ProjectCall &c, const GatherArgs &g, int vec_ok)
{
    const int part_px = c.sp.plan.part_px;
    const long long px2 = 2ll * c.B * c.V * (long long)c.H * c.W;
    // at most one item per voxel row that is not split, plus the parts (the parts of a call: at most 2 * pixels / part_px, and
    // never more than the slots)
    const long long items = (c.n_rows - 1) + (part_px > 0 ? std::min<long long>(c.l.slot_cap, px2 / part_px + 1) : 0);
    // the fourth template argument: the views whose first ID tile is fetched together (vp_gather.h); the grouped fetch on
    // small fp32 images needs views to group
    const auto launch = [&](auto G32) {
        const dim3 ggrid((unsigned)((items + 3) / 4));
        project_with_rows(vec_ok, c.C, [&](auto R, auto VEC, auto U) {
            constexpr int G = decltype(VEC)::value == 8 ? GATHER_G16 : decltype(VEC)::value == 4 ? decltype(G32)::value : 1;
            hipLaunchKernelGGL((k_gather<decltype(R)::value, decltype(VEC)::value, decltype(U)::value, G>), ggrid, dim3(256), 0, c.s0, g, c.p);
        });
    };
    {
        ProfSpan sp; sp.begin(2, c.s0);
        if ((long long)c.B * c.V >= 8 && (long long)c.H * c.W <= GATHER_G32_SMALL_IMAGE) launch(std::integral_constant<int, 4>{});
        else launch(std::integral_constant<int, 1>{});
        sp.end();
    }
    if (part_px > 0) project_combine(c, g, vec_ok);
}

// Phase 2, on the caller's stream (pipelined calls: behind the march's event)
int project_gather(ProjectCall &c)
{
    GatherArgs g;
    g.feats = c.feats; g.hit = c.hit; g.viewtab = c.viewtab; g.intr = c.intr; g.cell_of_id = c.cell_of_id;
    g.cnt_call = c.cnt_call; g.heavy_list = c.heavy_list; g.n_heavy = c.status + ST_NHEAVY;
    g.row_lo = (int)c.row_lo; g.row_hi = (int)c.row_hi;
    g.work = c.work; g.work_n = c.status + ST_WORK0;
    g.parts = c.parts; g.split = c.split; g.pmeta = c.pmeta; g.prow = c.prow;
    g.host_word = nullptr; g.host_seq = 0;
    g.parts_on = (c.sp.one_view && c.sp.plans_parts) ? 1 : 0; g.slot_cap = (int)c.l.slot_cap; g.count = c.count; g.views_hit = c.views_hit;
    g.out = c.out; g.status = c.status;
    g.heavy_blocks = 0;
    const int vec_ok = c.f16 ? 2 : ((c.C % 4 == 0) && (((uintptr_t)c.feats & 15) == 0) && (((uintptr_t)c.out & 15) == 0)) ? 1 : 0;
    if (c.pipe && !c.gather_only) VP_HIP(hipStreamWaitEvent(c.s0, c.rec->pipe.fh_done[c.q], 0));
    if (c.sp.one_view) project_gather_one(c, g, vec_ok);
    else if (c.n_rows > 1) project_gather_views(c, g, vec_ok);
    return VP_OK;
}

// the call is queued: its event, and what the record keeps of it
int project_commit(ProjectCall &c)
{
    WsState &rec = *c.rec;
    PipeState &ps = rec.pipe;
    if (c.pipe) {
        // (a gather-only call re-records the event of the set it shares with its predecessor and does not advance the sets)
        VP_HIP(hipEventRecord(ps.call_done[c.q], c.s0));
        ps.used[c.q] = true;
        if (!c.gather_only) ps.calls++;
    }
    rec.last_q = c.q;
    VP_HIP(hipGetLastError());
    rec.last = c.now;
    rec.last.ranged = c.ranged; rec.last.plan = c.sp.plan;
    rec.has_hit = true; rec.hit_off = c.l.hit[c.q];
    return VP_OK;
}

}  // namespace

// vp_gather.h -- the work list and phase 2: the feature rows of the pixels that first-hit a voxel are gathered and summed.
//   k_worklist       bins the voxels a call touched by size and plans the PARTS of the voxels above the split threshold;
//   k_gather         calls with more than one view: wavefront w takes item w of the work list -- a part (gather_part_wave:
//                    a partial row into the part's slot) or a whole voxel (gather_voxel_wave: the oracle's order and bits);
//   k_gather_one     one-view calls: a fixed grid of wavefronts dealt the parts (gather_part_one) and the size-ordered
//                    list; with VP_OPT_ONE_VIEW_SPLIT = 0 (the A/B arm) workgroups of four wavefronts take the march's
//                    heavy voxels first (gather_voxel_block);
//   k_combine_parts  follows either gather on the stream: adds the partial rows of each split voxel to its row in a fixed
//                    order, and redoes over whole images (gather_voxel_block) a voxel whose parts came up short.
// The pieces every role is made of are written once, in this order: a lane's share of a row (Row, scan_box, acc_*), the
// pixel box of a voxel (voxel_box, only_view_box), the walk over a voxel's views (for_view_groups, for_views), the
// whole-image redo of a wavefront (redo_whole_images), the meeting of four wavefronts in LDS (lds_meet).
// Included by voxproj.hip only.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// A lane's share of a row
// ------------------------------------------------------------------------------------------------
template <int K, int VEC>
struct Acc {
    float a[K * VEC];
};

typedef _Float16 v8h_ __attribute__((ext_vector_type(8)));
typedef float v4f_ __attribute__((ext_vector_type(4)));

// One pass covers the channels cb .. cb + CB of a row.  A lane holds K CHUNKS of it, chunk k = the VEC channels from
// (k * 64 + lane) * VEC on, in acc.a[k * VEC ...]: one 16-byte load per chunk from the feature map (VEC == 8 selects the
// fp16 feature-map mode: 8 halves; values are widened exactly and summed in fp32 in the same order, so the outputs equal
// the fp32 path's on the same data).  Towards fp32 memory (the output row, a part's row, LDS) a chunk is VEC / PW PIECES of
// PW floats, PW = 4 (a float4) or 1: piece i of the lane's NP is acc.a[i * PW ...].  A chunk is inside the row or outside
// it as a whole.  Every loop over a lane's registers of a row takes its channels from here.
template <int PW> struct piece_type { typedef float4 type; };
template <> struct piece_type<1> { typedef float type; };
template <int K, int VEC>
struct Row {
    static constexpr int CB = 64 * K * VEC;
    static constexpr int PW = VEC == 1 ? 1 : 4;
    static constexpr int NP = K * VEC / PW;
    typedef typename piece_type<PW>::type piece_t;
    // first channel, within the pass, of chunk k / of piece i
    static __device__ __forceinline__ int chunk_ch(int k, int lane) { return (k * 64 + lane) * VEC; }
    static __device__ __forceinline__ int piece_ch(int i, int lane) { return chunk_ch(i * PW / VEC, lane) + i * PW % VEC; }
    static __device__ __forceinline__ bool piece_in(int i, int lane, int cb, int C) { return cb + chunk_ch(i * PW / VEC, lane) < C; }
};

// a piece between acc.a and fp32 memory: P = float4 or float
template <class P> __device__ __forceinline__ P piece_of(const float *a);
template <> __device__ __forceinline__ float4 piece_of<float4>(const float *a) { return make_float4(a[0], a[1], a[2], a[3]); }
template <> __device__ __forceinline__ float piece_of<float>(const float *a) { return a[0]; }
__device__ __forceinline__ void piece_to(float *a, float4 v) { a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w; }
__device__ __forceinline__ void piece_to(float *a, float v) { a[0] = v; }

// Feature pointers are carried as `const float *`; this advances one by `elems` ELEMENTS of the mode's input type.
template <int VEC>
__device__ __forceinline__ const float *feat_ptr(const float *base, long long elems)
{
    return reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + elems * (VEC == 8 ? 2 : 4));
}

// The chunk at element `elem` of a feature map, as it stays in flight: 8 halves in 4 registers (widened when added --
// what keeps k_gather<1, 8, 4, 4> at its register count), 4 floats or 1 float.  Feature rows are read exactly once:
// non-temporal loads keep them out of L2/MALL (+12 % gather bandwidth measured against plain loads).
template <int VEC>
__device__ __forceinline__ auto ld_feat(const float *fv, long long elem)
{
    if constexpr (VEC == 8) return __builtin_nontemporal_load(reinterpret_cast<const v8h_ *>(feat_ptr<8>(fv, elem)));
    else if constexpr (VEC == 4) return __builtin_nontemporal_load(reinterpret_cast<const v4f_ *>(fv + elem));
    else return fv[elem];
}
template <class T> __device__ __forceinline__ float feat_elem(const T &r, int e) { return (float)r[e]; }
__device__ __forceinline__ float feat_elem(float r, int) { return r; }

// inclusive pixel box.  Passed BY VALUE everywhere: as `const Box &` into scan_box it cost k_gather_one 19-56 VGPRs and a
// wavefront per SIMD in <2,4,4> and <2,4,8> (profiles/r16_gather_refactor.txt, section 1)
struct Box {
    int x0, y0, x1, y1;
};

// 64 lanes cover a tile of tw x th pixels of a box, tw = smallest power of two >= box width (capped at 64), th = 64 / tw:
// lane `lane` covers the pixel (lx, ly) of the tile.
struct TileShape {
    int tw, th, lx, ly;
};
__device__ __forceinline__ TileShape tile_shape(const Box bx, int lane)
{
    const int bw = bx.x1 - bx.x0 + 1;
    const int lg = bw >= 64 ? 6 : (bw <= 1 ? 0 : 32 - __builtin_clz(bw - 1));
    return {1 << lg, 64 >> lg, lane & ((1 << lg) - 1), lane >> lg};
}

// ID of the pixel this lane covers in the FIRST 64-pixel tile of the box (0 outside the box): the load scan_box would
// issue for that tile, split off so that a caller can have the first tiles of several views in flight at once
__device__ __forceinline__ int first_tile_id(const int *__restrict__ hv, int W, const Box bx, int lane)
{
    const TileShape t = tile_shape(bx, lane);
    const int px = bx.x0 + t.lx, py = bx.y0 + t.ly;
    return ((px <= bx.x1) && (py <= bx.y1)) ? hv[py * W + px] : 0;
}

// Scan the pixel box bx of one view's ID image for pixels whose first hit is `id`, in raster order, and add their
// feature rows (channels cb .. cb + CB) to acc: tiles (tile_shape) and the lanes inside a tile are visited in raster
// order, the hit pixels of a tile U at a time -- U rows in flight, added pixel after pixel, chunk after chunk, element
// after element.  have_first: the caller fetched the first tile's IDs (first_tile_id) into h_first.
template <int K, int VEC, int U>
__device__ __forceinline__ void scan_box(const float *__restrict__ fv, const int *__restrict__ hv, int W, int C, int id,
                                         const Box bx, int cb, int lane, Acc<K, VEC> &acc, int &found,
                                         bool have_first = false, int h_first = 0)
{
    const TileShape t = tile_shape(bx, lane);
    for (int ty = bx.y0; ty <= bx.y1; ty += t.th) {
        const int py = ty + t.ly;
        for (int tx = bx.x0; tx <= bx.x1; tx += t.tw) {
            const int px = tx + t.lx;
            const bool inb = (px <= bx.x1) && (py <= bx.y1);
            const int pix = py * W + px;
            int h;
            if (have_first && ty == bx.y0 && tx == bx.x0) h = h_first;
            else h = inb ? hv[pix] : 0;
            unsigned long long m = __ballot(h == id);
            found += __popcll(m);
            while (m) {
                int n = 0;
                long long off[U];
#pragma unroll
                for (int j = 0; j < U; j++) {
                    off[j] = 0;
                    if (m) {
                        const int l = __builtin_ctzll(m);
                        m &= m - 1;
                        off[j] = (long long)__builtin_amdgcn_readlane(pix, l) * C + cb;
                        n = j + 1;
                    }
                }
                decltype(ld_feat<VEC>(fv, 0)) r[U][K];
#pragma unroll
                for (int j = 0; j < U; j++)
                    if (j < n) {
#pragma unroll
                        for (int k = 0; k < K; k++) {
                            const int ch = Row<K, VEC>::chunk_ch(k, lane);
                            if (cb + ch < C) r[j][k] = ld_feat<VEC>(fv, off[j] + ch);
                            else r[j][k] = {};
                        }
                    }
#pragma unroll
                for (int j = 0; j < U; j++)
                    if (j < n) {
#pragma unroll
                        for (int k = 0; k < K; k++)
#pragma unroll
                            for (int e = 0; e < VEC; e++) acc.a[k * VEC + e] += feat_elem(r[j][k], e);
                    }
            }
        }
    }
}

// Conservative pixel box of a voxel cube (centre c, half edge h) in view ve; returns false if empty.
// Every ray sample has camera depth >= depthMin (t >= depthMin/camDir.z, K.cu:31-32), so the cube is
// clipped against the plane z = zn = 0.98*depthMin before it is projected: vertices in front of the
// plane are projected as they are, edges crossing it contribute their intersection point.
__device__ __forceinline__ bool voxel_box(const ViewEntry &ve, float fx, float fy, float mx, float my,
                                          float cxw, float cyw, float czw, float h, float zn, int W, int H,
                                          int &x0, int &y0, int &x1, int &y1)
{
    x0 = 0; y0 = 0; x1 = W - 1; y1 = H - 1;
    if (ve.ok == 0.0f) return true;
    const float dx = cxw - ve.pos[0], dy = cyw - ve.pos[1], dz = czw - ve.pos[2];
    const float camx = ve.inv[0] * dx + ve.inv[1] * dy + ve.inv[2] * dz;
    const float camy = ve.inv[3] * dx + ve.inv[4] * dy + ve.inv[5] * dz;
    const float camz = ve.inv[6] * dx + ve.inv[7] * dy + ve.inv[8] * dz;
    const float ez = h * (fabsf(ve.inv[6]) + fabsf(ve.inv[7]) + fabsf(ve.inv[8]));
    if (!(camz + ez > zn)) return false;                   // cube entirely nearer than any sample
    float umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
    float qx[8], qy[8], qz[8];
#pragma unroll
    for (int s = 0; s < 8; s++) {
        const float a = (s & 1) ? h : -h, b = (s & 2) ? h : -h, c = (s & 4) ? h : -h;
        qx[s] = camx + ve.inv[0] * a + ve.inv[1] * b + ve.inv[2] * c;
        qy[s] = camy + ve.inv[3] * a + ve.inv[4] * b + ve.inv[5] * c;
        qz[s] = camz + ve.inv[6] * a + ve.inv[7] * b + ve.inv[8] * c;
        if (qz[s] >= zn) {
            const float u = fx * (qx[s] / qz[s]) + mx, v = fy * (qy[s] / qz[s]) + my;
            umin = fminf(umin, u); umax = fmaxf(umax, u);
            vmin = fminf(vmin, v); vmax = fmaxf(vmax, v);
        }
    }
    if (!(camz - ez >= zn)) {
        // some vertices are behind the plane: add the 12 edges' crossings with z = zn
#pragma unroll
        for (int s = 0; s < 8; s++) {
#pragma unroll
            for (int ax = 0; ax < 3; ax++) {
                const int o = s ^ (1 << ax);
                if (o < s) continue;
                const bool fs = qz[s] >= zn, fo = qz[o] >= zn;
                if (fs == fo) continue;
                const float tt = (zn - qz[s]) / (qz[o] - qz[s]);
                const float ix = qx[s] + tt * (qx[o] - qx[s]), iy = qy[s] + tt * (qy[o] - qy[s]);
                const float u = fx * (ix / zn) + mx, v = fy * (iy / zn) + my;
                umin = fminf(umin, u); umax = fmaxf(umax, u);
                vmin = fminf(vmin, v); vmax = fmaxf(vmax, v);
            }
        }
        // crossing points are computed with cancellation: widen by 2 % of the box and 2 px
        const float pu = 0.02f * (umax - umin) + 2.0f, pv = 0.02f * (vmax - vmin) + 2.0f;
        umin -= pu; umax += pu; vmin -= pv; vmax += pv;
    }
    if (!(umin == umin) || !(umax == umax) || !(vmin == vmin) || !(vmax == vmax)) return true;
    if (!(umin <= umax) || !(vmin <= vmax)) return true;   // nothing in front although the depth test passed
    const float fW = (float)W, fH = (float)H;
    if (umax < -2.0f || vmax < -2.0f || umin > fW + 1.0f || vmin > fH + 1.0f) return false;
    x0 = max(0, (int)floorf(fmaxf(umin, 0.0f)) - 1);
    y0 = max(0, (int)floorf(fmaxf(vmin, 0.0f)) - 1);
    x1 = min(W - 1, (int)ceilf(fminf(umax, fW)) + 1);
    y1 = min(H - 1, (int)ceilf(fminf(vmax, fH)) + 1);
    return x0 <= x1 && y0 <= y1;
}

struct GatherArgs {
    const float *feats;
    const int *hit;
    const ViewEntry *viewtab;
    const float *intr;
    const int *cell_of_id;
    const int *cnt_call;
    const int *heavy_list;   // one-view calls: IDs whose pixel count exceeds heavy_t (appended by phase 1)
    const int *n_heavy;
    int parts_on;            // k_gather_one: the call's work list has part items (one-view calls that split large voxels)
    int *host_word;          // nullable (blocking one-view calls): pinned host word that receives "split voxels of this call" when the
    int host_seq;            // gather starts, tagged with the call's sequence number -- the host then launches k_combine_parts only if any
    int slot_cap;            // part slots of the buffer set: the consumers never walk past it, whatever the counters say
    int row_lo, row_hi;      // phase 2 of this launch covers the voxel IDs in [row_lo, row_hi) (VP_OPT_ROW_BEGIN / _END)
    int heavy_blocks;        // k_gather_one, VP_OPT_ONE_VIEW_SPLIT = 0 only: workgroups that take the march's heavy voxels before they join the deal
    const int *work;         // work list of this call: WORK_CLASSES arrays of n_rows voxel IDs, by size class (k_worklist)
    const int *work_n;       // voxels per class; [WORK_CLASSES] = parts planned, [WORK_CLASSES + 1] = split voxels (ST_NPARTS, ST_NSPLIT)
    const int4 *parts;       // part items of the split voxels: {id, part, P, first slot of the voxel}; the item's index is its slot
    const int4 *split;       // split voxels: {id, first slot, P, pixels in the call}
    int4 *pmeta;             // per slot: {pixels found, views that contributed, first such view, last such view}
    float *prow;             // per slot: the part's C-wide partial row
    int *count;
    int *views_hit;          // nullable: += number of views of this call in which the voxel got >= 1 pixel
    float *out;
    int *status;
};

constexpr int GW_MERGED = 4;     // wavefronts of a workgroup that share one voxel: k_combine_parts, its whole-image redo, and the A/B arm of k_gather_one
constexpr int COMBINE_BLOCKS = 512; // grid of k_combine_parts (a workgroup per split voxel at a time)
// (the split plan's numbers -- PlanArgs, ONE_VIEW_*, GATHER_G32_SMALL_IMAGE, the part slots -- are host arithmetic: vp_plan.h)
// Views whose first ID tile is fetched together by the one-wavefront gather on fp16 rows (template argument G of k_gather): 4
// (-1 % pipelined, round 2); fp32 rows: GATHER_G32_SMALL_IMAGE, vp_plan.h
constexpr int GATHER_G16 = 4;

// Output rows are read once and written once per call by the wavefront that owns the voxel: no reuse inside a launch.
// The finished row is stored WRITE-THROUGH (buffer_store_dwordx4 with the sc0 sc1 cache-policy bits): stores that leave
// dirty lines in L2 cost this read-bound kernel far more than their bytes, and on some (feature pool, output rows)
// placement pairs several times more (profiles/r03_probe_row_stores_microbenchmark.log: +3.9 % per launch for one plain 2-KiB store per 272 rows
// read, +12.7 % on a bad pair; +2.3 % / +4.6 % written through; the same through uncached memory or a non-temporal store).
// In the gather itself: -0.3 ... -1.5 % per launch (profiles/r03_ab_output_row_store_policy.log).  The row's load stays a
// plain load (a non-temporal load of the row was measured slower).  Visibility is that of a plain store: the line goes
// to memory at system scope and the next kernel reads it from there.
typedef int v4i_ __attribute__((ext_vector_type(4)));
constexpr int OUT_ST_POLICY = 0x11;     // aux bits of the raw buffer store on gfx940+: sc0 (bit 0) | sc1 (bit 4)

// store 16 bytes at row + byte_off, row wave-uniform (one buffer descriptor per row chunk: base = the row, no bound)
__device__ __forceinline__ void st_out4(__amdgpu_buffer_rsrc_t row, int byte_off, float4 v)
{
    const v4f_ t = {v.x, v.y, v.z, v.w};
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i_, t), row, byte_off, 0, OUT_ST_POLICY);
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t out_row_rsrc(float *orow)
{
    // raw buffer, stride 0, num_records = 2^31 bytes (the callers bound their accesses themselves), gfx9 dword 3 for 32-bit data
    return __builtin_amdgcn_make_buffer_rsrc(orow, 0, 0x7fffffff, 0x00020000);
}

// the piece at channel ch of the row: written through (float4 pieces only; the row's descriptor is made once per row, the
// compiler merges the copies) or plainly
template <bool WT>
__device__ __forceinline__ void st_piece(float *orow, int ch, float4 v)
{
    if constexpr (WT) st_out4(out_row_rsrc(orow), ch * 4, v);
    else *reinterpret_cast<float4 *>(orow + ch) = v;
}
template <bool WT>
__device__ __forceinline__ void st_piece(float *orow, int ch, float v)
{
    orow[ch] = v;
}

template <int K, int VEC>
__device__ __forceinline__ void acc_zero(Acc<K, VEC> &acc)
{
#pragma unroll
    for (int i = 0; i < K * VEC; i++) acc.a[i] = 0.f;
}

// orow: the row's channel cb (as everywhere below); channels beyond the row read as zero
template <int K, int VEC>
__device__ __forceinline__ void acc_load(Acc<K, VEC> &acc, const float *orow, int cb, int C, int lane)
{
    typedef Row<K, VEC> R;
    typedef typename R::piece_t P;
#pragma unroll
    for (int i = 0; i < R::NP; i++) {
        const P *src = reinterpret_cast<const P *>(orow + R::piece_ch(i, lane));
        piece_to(acc.a + i * R::PW, R::piece_in(i, lane, cb, C) ? *src : P{});
    }
}

// WT: write-through stores (the multi-view launches); false: plain stores -- the one-view-per-call variant of k_gather stays
// at 96 VGPRs = 5 wavefronts per SIMD that way (the buffer form costs 5 registers), which is worth more to a 0.25-ms launch.
template <int K, int VEC, bool WT>
__device__ __forceinline__ void acc_store(const Acc<K, VEC> &acc, float *orow, int cb, int C, int lane)
{
    typedef Row<K, VEC> R;
    typedef typename R::piece_t P;
#pragma unroll
    for (int i = 0; i < R::NP; i++)
        if (R::piece_in(i, lane, cb, C)) st_piece<WT>(orow, R::piece_ch(i, lane), piece_of<P>(acc.a + i * R::PW));
}

// the lane's registers to their channels of an LDS row of CB floats
template <int K, int VEC>
__device__ __forceinline__ void acc_stage(const Acc<K, VEC> &acc, float *dst, int lane)
{
    typedef Row<K, VEC> R;
    typedef typename R::piece_t P;
#pragma unroll
    for (int i = 0; i < R::NP; i++) *reinterpret_cast<P *>(dst + R::piece_ch(i, lane)) = piece_of<P>(acc.a + i * R::PW);
}

// scan_box on view bv (= b * V + v) of the call
template <int K, int VEC, int U>
__device__ __forceinline__ void scan_view(const GatherArgs &g, const Params &p, long long bv, int id, const Box bx, int cb,
                                          int lane, Acc<K, VEC> &acc, int &found, bool have_first = false, int h_first = 0)
{
    const long long HW = (long long)p.height * p.width;
    scan_box<K, VEC, U>(feat_ptr<VEC>(g.feats, bv * HW * p.C), g.hit + bv * HW, p.width, p.C, id, bx, cb, lane, acc, found,
                        have_first, h_first);
}

// ------------------------------------------------------------------------------------------------
// The pixel box of a voxel, the walk over a voxel's views
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float box_half_edge(const Params &p)
{
    return 0.5f * fabsf(p.vs) * 1.02f +
           1e-6f * (fabsf(p.ox) + fabsf(p.oy) + fabsf(p.oz) + fabsf(p.vs) * (p.dimx + p.dimy + p.dimz));
}

// camera depth below which no ray sample exists (t starts at depthMin/camDir.z); a non-positive or
// non-finite depthMin degrades to a tiny positive plane (boxes grow, results stay exact)
__device__ __forceinline__ float near_plane(const Params &p)
{
    const float zn = 0.98f * p.dmin;
    return (zn > 1e-6f && zn < 1e30f) ? zn : 1e-6f;
}

// world-space centre of grid cell `cell`
__device__ __forceinline__ void cell_centre(const Params &p, int cell, float &cxw, float &cyw, float &czw)
{
    const int czi = cell / (p.dimy * p.dimx);
    const int rem = cell - czi * (p.dimy * p.dimx);
    const int cyi = rem / p.dimx, cxi = rem - cyi * p.dimx;
    cxw = p.ox + (float)cxi * p.vs; cyw = p.oy + (float)cyi * p.vs; czw = p.oz + (float)czi * p.vs;
}

// One-view calls: the pixel box, in the call's only view, of the voxel in `cell`; x1 < x0 if there is no cell (< 0) or no box
__device__ __forceinline__ Box only_view_box(const GatherArgs &g, const Params &p, int cell)
{
    Box bx = {0, 0, -1, -1};
    if (cell >= 0) {
        float cxw, cyw, czw;
        cell_centre(p, cell, cxw, cyw, czw);
        int a0, a1, a2, a3;
        if (voxel_box(g.viewtab[0], g.intr[0], g.intr[1], g.intr[2], g.intr[3], cxw, cyw, czw, box_half_edge(p), near_plane(p),
                      p.width, p.height, a0, a1, a2, a3))
            bx = {a0, a1, a2, a3};
    }
    return bx;
}

// The boxes of one voxel in the views vbase .. vbase + 63 of batch b, the box of view vbase + lane on lane `lane`: `mine` =
// this lane's view exists and its box is not empty, mask = the ballot of `mine`.
struct ViewGroup {
    int b, vbase;
    Box bx;
    bool mine;
    unsigned long long mask;
};

// view vbase + l's box, to every lane
__device__ __forceinline__ Box box_of(const ViewGroup &vg, int l)
{
    return {__builtin_amdgcn_readlane(vg.bx.x0, l), __builtin_amdgcn_readlane(vg.bx.y0, l),
            __builtin_amdgcn_readlane(vg.bx.x1, l), __builtin_amdgcn_readlane(vg.bx.y1, l)};
}

// THE view walk: for each batch whose grid holds voxel `id` (its cell -> world centre, the batch's intrinsics), for each
// group of 64 views, one view per lane through voxel_box: f(group), while go().  whole_image: every view of every batch,
// the box the whole image -- correctness never depends on the boxes.
template <class Go, class F>
__device__ __forceinline__ void for_view_groups(const GatherArgs &g, const Params &p, int id, int lane, bool whole_image, Go &&go,
                                                F &&f)
{
    const int W = p.width, H = p.height;
    const float hh = box_half_edge(p);
    const float zn = near_plane(p);
    for (int b = 0; b < p.B && go(); b++) {
        float cxw = 0.f, cyw = 0.f, czw = 0.f;
        if (!whole_image) {
            const int cell = g.cell_of_id[(long long)b * p.n_rows + id];
            if (cell < 0) continue;      // the grid of batch b does not hold the ID
            cell_centre(p, cell, cxw, cyw, czw);
        }
        const float fx = g.intr[b * 4 + 0], fy = g.intr[b * 4 + 1], mx = g.intr[b * 4 + 2], my = g.intr[b * 4 + 3];
        for (int vbase = 0; vbase < p.V && go(); vbase += 64) {
            const int v = vbase + lane;
            ViewGroup vg = {b, vbase, {0, 0, W - 1, H - 1}, v < p.V, 0ull};
            if (vg.mine && !whole_image) {
                Box &bx = vg.bx;
                vg.mine = voxel_box(g.viewtab[b * p.V + v], fx, fy, mx, my, cxw, cyw, czw, hh, zn, W, H, bx.x0, bx.y0, bx.x1, bx.y1);
            }
            vg.mask = __ballot(vg.mine);   // identical in every wavefront of a workgroup
            f(vg);
        }
    }
}

// ... one view at a time: f(bv = b * V + v, the view's box), in view order, while go()
template <class Go, class F>
__device__ __forceinline__ void for_views(const GatherArgs &g, const Params &p, int id, int lane, bool whole_image, Go &&go, F &&f)
{
    for_view_groups(g, p, id, lane, whole_image, go, [&](const ViewGroup &vg) {
        for (unsigned long long vm = vg.mask; vm && go(); vm &= vm - 1) {
            const int l = __builtin_ctzll(vm);
            f((long long)vg.b * p.V + vg.vbase + l, box_of(vg, l));
        }
    });
}

// The whole-image redo of the one-wavefront roles: the search box(es) missed pixels of voxel `id` (an ID labelling several
// cells, a degenerate pose ...), so its n_bv views are summed again over whole images, on top of the row the caller has put
// back into acc.  Correctness never depends on the boxes.
template <int K, int VEC, int U>
__device__ __forceinline__ void redo_whole_images(const GatherArgs &g, const Params &p, int id, long long n_bv, int cb, int lane,
                                                  Acc<K, VEC> &acc, int &found, int &nviews)
{
    if (lane == 0 && cb == 0) atomicAdd(&g.status[ST_BOXMISS], 1);
    found = 0;
    nviews = 0;
    for (long long bv = 0; bv < n_bv; bv++) {
        const int before = found;
        scan_view<K, VEC, U>(g, p, bv, id, Box{0, 0, p.width - 1, p.height - 1}, cb, lane, acc, found);
        nviews += found > before;
    }
}

// ------------------------------------------------------------------------------------------------
// Normal role: one wavefront sums all pixels of one voxel, in (b, v, y, x) order, starting from the
// row already in `out` -- bit-identical to the oracle's serial accumulation.
// ------------------------------------------------------------------------------------------------
template <int K, int VEC, int U, int G, bool WT>
__device__ __forceinline__ void gather_voxel_wave(const GatherArgs &g, const Params &p, int id, int expected, int lane)
{
    const int W = p.width, C = p.C;
    const long long HW = (long long)p.height * W;
    for (int cb = 0; cb < C; cb += Row<K, VEC>::CB) {
        Acc<K, VEC> acc;
        float *orow = g.out + (long long)id * C + cb;
        acc_load<K, VEC>(acc, orow, cb, C, lane);
        const Acc<K, VEC> acc0 = acc;
        int found = 0, nviews = 0;
        const auto go = [&] { return found < expected; };
        for_view_groups(g, p, id, lane, false, go, [&](const ViewGroup &vg) {
            unsigned long long vm = vg.mask;
            const long long bv0 = (long long)vg.b * p.V + vg.vbase;
            // Views are taken G at a time: the ID-image loads of the first tile of all G views go out together (one
            // memory latency instead of G dependent ones -- most boxes are a single 64-pixel tile, and many views of
            // a voxel yield no pixel at all), then the views are summed one after the other, in order.
            while (vm && go()) {
                // the group: the lowest G set bits of vm
                unsigned long long mg = 0ull;
#pragma unroll
                for (int q = 0; q < G; q++)
                    if (vm) { mg |= vm & (~vm + 1ull); vm &= vm - 1; }
                int gh[G];
                if constexpr (G > 1) {
                    unsigned long long t = mg;
#pragma unroll
                    for (int q = 0; q < G; q++) {
                        gh[q] = 0;
                        if (t) {
                            const int l = __builtin_ctzll(t);
                            t &= t - 1;
                            gh[q] = first_tile_id(g.hit + (bv0 + l) * HW, W, box_of(vg, l), lane);
                        }
                    }
                }
                int q = 0;
#pragma unroll 1
                for (unsigned long long t = mg; t && go(); q++) {
                    const int l = __builtin_ctzll(t);
                    t &= t - 1;
                    int hq = 0;
                    if constexpr (G > 1) {
                        hq = gh[0];
#pragma unroll
                        for (int k = 1; k < G; k++) hq = (q == k) ? gh[k] : hq;
                    }
                    const int before = found;
                    scan_view<K, VEC, U>(g, p, bv0 + l, id, box_of(vg, l), cb, lane, acc, found, G > 1, hq);
                    nviews += found > before;
                }
            }
        });
        if (found != expected) {
            acc = acc0;
            redo_whole_images<K, VEC, U>(g, p, id, (long long)p.B * p.V, cb, lane, acc, found, nviews);
        }
        acc_store<K, VEC, WT>(acc, orow, cb, C, lane);
        if (cb == 0 && lane == 0) {
            g.count[id] += found;   // K.cu:77 (one add of the per-call total)
            if (g.views_hit) g.views_hit[id] += nviews;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Split voxels (round 5).  A voxel that collected more than heavy_t pixels in the call -- a surface patch a hand-held camera
// stares at from 0.3 m for sixty consecutive frames collects 10^5 and more -- is not one wavefront's job: at the ~5 GB/s one
// wavefront pulls, 200 MB of rows last longer than the whole launch.  Rounds 1-4 gave such a voxel to ONE workgroup of the
// launch's first 128 (four wavefronts splitting each view's box rows, combined through LDS view by view): enough for the
// benign room (76 voxels of <= 8.8 k pixels per pass), 0.25-0.27 of peak on a trajectory whose close-ups put 70-100 % of a
// call's pixels into such voxels (profiles/r05_before_*.log).  Now:
//   * k_worklist PLANS: a voxel with c > heavy_t pixels becomes P = ceil(c / part_px) parts; each part is an item
//     {id, part, P} in its own slot, and the parts lead the work list (they are the longest items);
//   * a PART is a contiguous piece of the voxel's pixel sequence in (b, v, y, x) order, cut by search-box AREA: with
//     A = the summed area of the voxel's pixel boxes over all views of the call, part k owns the box rows whose first
//     pixel's running area index lies in [A k / P, A (k+1) / P) -- every row of every view belongs to exactly one part,
//     whatever the boxes are.  One wavefront sums its rows in order from zero into a partial row (gather_part_wave);
//   * k_combine_parts (one workgroup per split voxel, after the gather on the same stream) adds the partial rows to the
//     row in `out` in slot order -- a fixed tree, so results are reproducible run to run and independent of which
//     wavefront ran when; they differ from the serial order in the last bits only (inside the 1e-4 bar, tested per
//     element); pixel counts add exactly; a view shared by two neighbouring parts is counted once.  If the parts found
//     fewer pixels than the march counted (the boxes are only hints), the voxel is redone over whole images.
// No float atomics, no inter-workgroup hand-off inside a launch (the partial rows cross a kernel boundary).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long wave_sum_nonneg(int v)
{
    long long s = 0;
    unsigned long long m = __ballot(v != 0);
    while (m) {
        const int l = __builtin_ctzll(m);
        m &= m - 1;
        s += __builtin_amdgcn_readlane(v, l);
    }
    return s;
}

template <int K, int VEC, int U>
__device__ __forceinline__ void gather_part_wave(const GatherArgs &g, const Params &p, int slot, int lane)
{
    const int4 it = g.parts[slot];
    const int id = it.x, part = it.y, P = it.z;
    const int C = p.C;
    // pass 1: the voxel's total box area over the call's views
    long long A = 0;
    for_view_groups(g, p, id, lane, false, [] { return true; }, [&](const ViewGroup &vg) {
        A += wave_sum_nonneg(vg.mine ? (vg.bx.x1 - vg.bx.x0 + 1) * (vg.bx.y1 - vg.bx.y0 + 1) : 0);
    });
    const long long lo = A * part / P, hi = A * (part + 1) / P;      // A < 2^47, P <= 2^15
    int found0 = 0, nviews = 0, first_v = -1, last_v = -1;
    for (int cb = 0; cb < C; cb += Row<K, VEC>::CB) {
        Acc<K, VEC> acc;
        acc_zero(acc);
        int found = 0;
        long long a0 = 0;      // area of the boxes in front of the current view
        for_views(g, p, id, lane, false, [&] { return a0 < hi; }, [&](long long bv, const Box bx) {
            const int bw = bx.x1 - bx.x0 + 1, bh = bx.y1 - bx.y0 + 1;
            const long long av = (long long)bw * bh;
            // rows r of this box with lo <= a0 + r*bw < hi.  A box that ends before lo owns none of them -- most views of a
            // part in the middle of a long voxel: no division for those; the others divide 32-bit numbers (lo - a0, hi - a0
            // < av < 2^31; two 64-bit divisions per view and part were a third of a part's instructions)
            const long long a1 = a0 + av;
            const long long b0 = a0;
            a0 = a1;
            if (a1 <= lo) return;
            const int r_lo = lo > b0 ? (int)(((unsigned)(lo - b0) + (unsigned)bw - 1u) / (unsigned)bw) : 0;
            const int r_hi = hi < a1 ? (int)(((unsigned)(hi - b0) + (unsigned)bw - 1u) / (unsigned)bw) : bh;
            if (r_lo >= r_hi) return;
            const int before = found;
            scan_view<K, VEC, U>(g, p, bv, id, Box{bx.x0, bx.y0 + r_lo, bx.x1, bx.y0 + r_hi - 1}, cb, lane, acc, found);
            if (cb == 0 && found > before) {
                nviews++;
                if (first_v < 0) first_v = (int)bv;
                last_v = (int)bv;
            }
        });
        acc_store<K, VEC, false>(acc, g.prow + (long long)slot * C + cb, cb, C, lane);
        if (cb == 0) found0 = found;
    }
    if (lane == 0) g.pmeta[slot] = make_int4(found0, nviews, first_v, last_v);
}

// A part of a ONE-VIEW call (B*V == 1): part k of P owns the rows [ceil(h k / P), ceil(h (k+1) / P)) of the voxel's pixel box of h
// rows -- consecutive, disjoint, all of them, whatever P (more parts than rows: some own none) --, with the box computed once, by
// every lane alike, from the cell k_worklist left in the item (one dependent load fewer in front of the first row; 32-bit
// arithmetic: h k < 2^31 for any image the library accepts with P <= 8192 slots).  No cell or no box: the part finds nothing and
// k_combine_parts redoes the voxel over the whole image.
template <int K, int VEC, int U>
__device__ __forceinline__ void gather_part_one(const GatherArgs &g, const Params &p, int slot, int lane)
{
    const int4 it = g.parts[slot];
    const int id = it.x, part = it.y, P = it.z, cell = it.w;
    const int C = p.C;
    const Box bx = only_view_box(g, p, cell);
    const int bh = bx.y1 - bx.y0 + 1;
    int r_lo = 0, r_hi = 0;
    if (bh > 0 && bx.x1 >= bx.x0) {
        const unsigned up = (unsigned)P;
        r_lo = (int)(((unsigned long long)(unsigned)bh * (unsigned)part + up - 1u) / up);
        r_hi = (int)(((unsigned long long)(unsigned)bh * ((unsigned)part + 1u) + up - 1u) / up);
    }
    int found0 = 0;
    for (int cb = 0; cb < C; cb += Row<K, VEC>::CB) {
        Acc<K, VEC> acc;
        acc_zero(acc);
        int found = 0;
        if (r_lo < r_hi) scan_view<K, VEC, U>(g, p, 0, id, Box{bx.x0, bx.y0 + r_lo, bx.x1, bx.y0 + r_hi - 1}, cb, lane, acc, found);
        acc_store<K, VEC, false>(acc, g.prow + (long long)slot * C + cb, cb, C, lane);
        if (cb == 0) found0 = found;
    }
    if (lane == 0) g.pmeta[slot] = make_int4(found0, found0 > 0 ? 1 : 0, found0 > 0 ? 0 : -1, found0 > 0 ? 0 : -1);
}

// ------------------------------------------------------------------------------------------------
// Four wavefronts, one voxel: the meeting in LDS
// ------------------------------------------------------------------------------------------------
// The channels of a pass as the GW * 64 threads of a workgroup hold them: thread tid has channel tid + r * GW * 64 in v[r].
template <int CB, int GW>
struct Run {
    static constexpr int R = (CB + GW * 64 - 1) / (GW * 64);
    float v[R];
    // f(r, channel within the pass), for the thread's channels inside the pass
    template <class F>
    static __device__ __forceinline__ void channels(F &&f)
    {
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int c = (int)threadIdx.x + r * GW * 64;
            if (c < CB) f(r, c);
        }
    }
    __device__ __forceinline__ void load(const float *orow, int cb, int C)
    {
#pragma unroll
        for (int r = 0; r < R; r++) v[r] = 0.f;
        channels([&](int r, int c) { if (cb + c < C) v[r] = orow[c]; });
    }
    __device__ __forceinline__ void store(float *orow, int cb, int C) const
    {
        channels([&](int r, int c) { if (cb + c < C) orow[c] = v[r]; });
    }
};

// The GW wavefronts of a workgroup meet: each stages its lanes' sums in its LDS row, and after the barrier every thread adds
// the GW rows to its channels of `run` in wavefront order -- a fixed summation tree.  The caller's next barrier frees `part`.
template <int K, int VEC, int GW>
__device__ __forceinline__ void lds_meet(const Acc<K, VEC> &acc, float (*part)[64 * K * VEC], Run<64 * K * VEC, GW> &run)
{
    acc_stage(acc, part[threadIdx.x >> 6], threadIdx.x & 63);
    __syncthreads();
    run.channels([&](int r, int c) {
#pragma unroll
        for (int ww = 0; ww < GW; ww++) run.v[r] += part[ww][c];
    });
}

// Workgroup role: the GW wavefronts of a workgroup share one voxel.  Used by k_combine_parts to redo a split voxel whose parts came
// up short (whole images) and by k_gather_one's A/B arm (VP_OPT_ONE_VIEW_SPLIT = 0: every voxel above heavy_t pixels in the call).  Per view the box rows are cut into GW contiguous ranges,
// each wavefront sums its range in raster order, and the partial rows are combined through LDS in
// wavefront order -- a fixed summation tree, so results are reproducible run to run (they differ from
// the serial order in the last bits only, well inside the 1e-4 bar).  false: the boxes missed pixels and the caller redoes the
// voxel with whole_image; nothing has been stored then, because every channel pass finds the same pixels, so the shortfall
// shows in the first pass, before any store.
template <int K, int VEC, int U, int GW>
__device__ bool gather_voxel_block(const GatherArgs &g, const Params &p, int id, int expected,
                                   float (*part)[64 * K * VEC], int *part_found, bool whole_image)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int C = p.C;
    int found_total = 0, nviews = 0;
    for (int cb = 0; cb < C; cb += Row<K, VEC>::CB) {
        Run<Row<K, VEC>::CB, GW> run;
        float *orow = g.out + (long long)id * C + cb;
        run.load(orow, cb, C);
        found_total = 0;
        nviews = 0;
        for_views(g, p, id, lane, whole_image, [&] { return found_total < expected; }, [&](long long bv, const Box bx) {
            const int per = (bx.y1 - bx.y0 + GW) / GW;
            const int ry0 = bx.y0 + w * per, ry1 = min(bx.y1, ry0 + per - 1);
            Acc<K, VEC> acc;
            acc_zero(acc);
            int f = 0;
            if (ry0 <= ry1) scan_view<K, VEC, U>(g, p, bv, id, Box{bx.x0, ry0, bx.x1, ry1}, cb, lane, acc, f);
            if (lane == 0) part_found[w] = f;
            lds_meet<K, VEC, GW>(acc, part, run);
            int fview = 0;
#pragma unroll
            for (int ww = 0; ww < GW; ww++) fview += part_found[ww];
            found_total += fview;
            nviews += fview > 0;
            __syncthreads();
        });
        if (found_total != expected) return false;
        run.store(orow, cb, C);
    }
    if (threadIdx.x == 0) {
        g.count[id] += found_total;
        if (g.views_hit) g.views_hit[id] += nviews;
    }
    return true;
}

// Work list of a call: the voxels that received pixels (and are not heavy), binned by size class -- class k holds the
// voxels with floor(log2(pixels)) == k + 3 (clamped to 0 .. WORK_CLASSES-1).  k_gather walks the classes from the largest
// down, so the long voxels start first and the short ones fill the tail (longest-processing-time-first).  The grid is
// still sized for every row (the host does not know how many voxels a call touches): the wavefronts beyond the end of the
// list read the eight class counters and exit -- no box, no ID image, no output row is touched for an untouched voxel.
// Inside a class the IDs keep roughly their ascending order (neighbouring voxels read neighbouring pixels).  One lane per
// ID, appends aggregated per workgroup.  (Each class has room for every row -- 8 x n_rows ints per buffer set, 64 B of
// workspace per voxel row -- because the class sizes are only known once every workgroup has counted.)
constexpr int WL_PER_THREAD = 16;   // IDs per lane of k_worklist: a 256-thread workgroup bins 4096 voxel IDs

// [row_lo, row_hi): the IDs this call's phase 2 gathers (VP_OPT_ROW_BEGIN / _END; [1, n_rows) when no range is set).
// part_px > 0: the launch also PLANS the split voxels (see "Split voxels" above): a voxel with more than part_t pixels
// gets P = ceil(c / part_px) consecutive part slots and an entry in the split list; slots and entries are handed out per
// workgroup (LDS counters, two global atomics per workgroup).  part_px and part_t >= part_px are such that the parts of a
// call cannot outnumber slot_cap (plan_split, vp_plan.h; PlanArgs for the numbers derived here); the guard below only keeps a broken
// promise from writing out of bounds, and the consumers clamp what they walk to slot_cap.
// One-view calls without parts (VP_OPT_ONE_VIEW_SPLIT = 0): the voxels above heavy_t are in the march's heavy list (a workgroup
// of k_gather_one sums each) and stay out of this list, ST_NHEAVY is the march's count.  part_px == 0: nothing is split.
__global__ __launch_bounds__(256) void k_worklist(const int *__restrict__ cnt_call, PlanArgs plan, long long n_rows,
                                                  int *__restrict__ work, int *status, int wl_blocks,
                                                  const float *__restrict__ vmi, ViewEntry *viewtab, int n_views,
                                                  long long row_lo, long long row_hi, int4 *__restrict__ parts,
                                                  int4 *__restrict__ split, int slot_cap, int *sticky,
                                                  const int *__restrict__ cell_of_id, const int *__restrict__ hit_waves, int n_hit_waves)
{
    if ((int)blockIdx.x >= wl_blocks) {
        // trailing workgroups: the call's view table (phase 2's world->camera maps), one thread per view -- riding on
        // this launch saves one kernel launch per call
        const int v = ((int)blockIdx.x - wl_blocks) * 256 + (int)threadIdx.x;
        if (v < n_views) view_entry(vmi, viewtab, v);
        return;
    }
    int heavy_t = plan.heavy_t, part_t = plan.part_t, part_px = plan.part_px;
    __shared__ int n_cls[WORK_CLASSES + 2], base_cls[WORK_CLASSES + 2], n_split2, hits_lds;
    // this workgroup's 4096 pixel counts: requested first, so that they travel together with the loads of the hit total below
    // (the launch is a chain of dependent round trips -- counts, the classes' global bases, the list entries -- of 1.5 us each)
    const long long id0 = (long long)blockIdx.x * (256 * WL_PER_THREAD);
    int cv[WL_PER_THREAD];
#pragma unroll
    for (int j = 0; j < WL_PER_THREAD; j++) {
        // consecutive lanes take consecutive IDs, so the ranks inside a class follow the ID order closely
        const long long id = id0 + (long long)j * 256 + threadIdx.x;
        cv[j] = (id >= row_lo && id < row_hi) ? cnt_call[id] : 0;
    }
    if (plan.dyn_px_min > 0) {
        // the march has finished: every workgroup adds up its per-wavefront hit counts (a few thousand ints from L2) -- no
        // atomic on one hot word in the march, no second launch.  2 * hits / part_px <= slot_cap bounds the parts (see above)
        if (threadIdx.x == 0) hits_lds = 0;
        __syncthreads();
        // (16 ints per thread and round, all four loads in flight: one dependent load per round was 5 us of this launch)
        int mine = 0;
        const int4 *hw4 = reinterpret_cast<const int4 *>(hit_waves);      // 256-byte aligned, a multiple of four ints
        const int n4 = n_hit_waves >> 2;
        for (int j = threadIdx.x; j < n4; j += 1024) {
            int4 a[4];
#pragma unroll
            for (int u = 0; u < 4; u++) a[u] = j + u * 256 < n4 ? hw4[j + u * 256] : make_int4(0, 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 4; u++) mine += a[u].x + a[u].y + a[u].z + a[u].w;
        }
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
        if ((threadIdx.x & 63) == 0) atomicAdd(&hits_lds, mine);
        __syncthreads();
        const long long hits = hits_lds;
        if (blockIdx.x == 0 && threadIdx.x == 0) status[ST_NHIT] = (int)hits;
        part_px = (int)max((long long)max(part_px, plan.dyn_px_min), (2 * hits + slot_cap - 1) / slot_cap);
    }
    if (plan.dyn_t_ratio > 0) heavy_t = part_t = (int)min(max((long long)part_px * plan.dyn_t_ratio, (long long)plan.dyn_t_floor), 2147483646ll);
    if (part_px > 0 && part_t < part_px) { part_t = part_px; heavy_t = max(heavy_t, part_t); }
    int *work_n = status + ST_WORK0;
    if (blockIdx.x == 0 && threadIdx.x == 0) { status[ST_HEAVY_T] = heavy_t; status[ST_PART_T] = part_t; status[ST_PART_PX] = part_px; }
    // Appends are aggregated per WORKGROUP through LDS: a handful of global atomics per 4096 IDs.  (Returning integer
    // atomics on a few hot addresses are exactly what slows a concurrently running gather -- DESIGN.md section 2.)
    // Counters WORK_CLASSES and WORK_CLASSES + 1: part slots and split voxels.
    if (threadIdx.x < WORK_CLASSES + 2) n_cls[threadIdx.x] = 0;
    if (threadIdx.x == 0) n_split2 = 0;
    __syncthreads();
    int cls[WL_PER_THREAD], rank[WL_PER_THREAD];
#pragma unroll
    for (int j = 0; j < WL_PER_THREAD; j++) {
        const int c = cv[j];
        cls[j] = -1;
        rank[j] = 0;
        if (c > 0 && c <= heavy_t) {
            cls[j] = min(WORK_CLASSES - 1, max(0, 28 - __builtin_clz(c)));     // floor(log2 c) - 3
            rank[j] = atomicAdd(&n_cls[cls[j]], 1);
        } else if (c > part_t && part_px > 0) {
            cls[j] = WORK_CLASSES;
            rank[j] = atomicAdd(&n_cls[WORK_CLASSES], (c + part_px - 1) / part_px);
            atomicAdd(&n_cls[WORK_CLASSES + 1], 1);
        }
    }
    __syncthreads();
    if (threadIdx.x < WORK_CLASSES + 2) {
        const int n = n_cls[threadIdx.x];
        base_cls[threadIdx.x] = n > 0 ? atomicAdd(&work_n[threadIdx.x], n) : 0;
        if (threadIdx.x == WORK_CLASSES + 1 && n > 0 && plan.count_heavy) atomicAdd(&status[ST_NHEAVY], n);      // the counter tests and the bench read
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < WL_PER_THREAD; j++) {
        const int id = (int)(id0 + (long long)j * 256 + threadIdx.x);
        if (cls[j] >= 0 && cls[j] < WORK_CLASSES) {
            work[(long long)cls[j] * n_rows + base_cls[cls[j]] + rank[j]] = id;
        } else if (cls[j] == WORK_CLASSES) {
            const int c = cv[j];
            const int P = (c + part_px - 1) / part_px;
            const int base = base_cls[WORK_CLASSES] + rank[j];
            const int sidx = base_cls[WORK_CLASSES + 1] + atomicAdd(&n_split2, 1);
            if (base + P > slot_cap || sidx >= slot_cap) {      // cannot happen (see above); loud rather than out of bounds
                atomicOr(&status[ST_BADID], 1);
                *(volatile int *)&sticky[ST_STICKY_BADID] = 1;
                continue;
            }
            split[sidx] = make_int4(id, base, P, c);
            const int w4 = plan.cell_in_item ? cell_of_id[id] : base;
            for (int q = 0; q < P; q++) parts[base + q] = make_int4(id, q, P, w4);
        }
    }
}

// Entry w of the size-ordered list: the classes are walked from the largest down (n[k] = voxels of class k); 0 beyond its end
__device__ __forceinline__ int work_item(const GatherArgs &g, const Params &p, long long w, const int *n)
{
    int id = 0;
#pragma unroll
    for (int k = WORK_CLASSES - 1; k >= 0; k--) {
        if (id == 0 && w < n[k]) id = g.work[(long long)k * p.n_rows + w];
        w -= n[k];
    }
    return id;
}

// The gather of every call with more than one view.  Wavefront w of the grid takes item w of the call's work list: first
// the parts of the split voxels (the longest items), then the voxels of the size classes from the largest class down --
// long items start first, short ones fill the tail.  104-112 VGPRs allocated = 4 wavefronts per SIMD -- in pipelined mode a
// gain, because a fifth gather wave would take the room the next call's march needs (forcing <= 96 registers with
// __launch_bounds__(256, 5), one allocation: pipelined +2.5 % fp16 / +2 % R1 / -0.4 % fp32; serial phases -1.0 .. -1.4 %).
// The grid is sized for every row plus every part slot (the host does not know how many a call uses): the wavefronts
// beyond the end of the list read the ten counters and exit.
template <int K, int VEC, int U, int G>
__global__ __launch_bounds__(256) void k_gather(GatherArgs g, Params p)
{
    // The gather is HBM-bound: what matters is that its few instructions (address arithmetic, load issue) go out
    // the moment data returns.  Raised wave priority lets it win instruction arbitration against the issue-bound
    // march waves of the next call that share the SIMD in pipelined mode.
    __builtin_amdgcn_s_setprio(3);
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n_parts = min(g.work_n[WORK_CLASSES], g.slot_cap);
    if (w < n_parts) {
        gather_part_wave<K, VEC, U>(g, p, (int)w, lane);
        return;
    }
    const int id = work_item(g, p, w - n_parts, g.work_n);
    if (id == 0) return;
    gather_voxel_wave<K, VEC, U, G, true>(g, p, id, g.cnt_call[id], lane);
}

// pixels found, distinct views, first and last contributing view of a run of parts.  Parts cover ascending, contiguous
// stretches of the view sequence, so only the boundary views of two neighbours can repeat: such a view is counted once.
struct PartMeta {
    int found = 0, nviews = 0, first = -1, last = -1;
    __device__ __forceinline__ void fold(int f, int nv, int first_v, int last_v)
    {
        found += f;
        if (nv > 0) {
            nviews += nv - (first_v == last ? 1 : 0);
            if (first < 0) first = first_v;
            last = last_v;
        }
    }
};

// After k_gather on the same stream: one workgroup per split voxel at a time adds the voxel's partial rows to its row in
// `out`, in slot order.  The four wavefronts take four consecutive runs of the P slots (U rows in flight each), their
// sums meet in LDS and are added to the old row in wavefront order: a fixed tree for a given P.  Pixel counts add exactly,
// views by PartMeta's rule, over a wavefront's slots and then over the wavefronts.  Parts that found fewer pixels than the
// march counted: the search boxes missed some (an ID labelling several cells, a degenerate pose) -- the voxel is redone
// over whole images.
template <int K, int VEC, int U>
__global__ __launch_bounds__(256) void k_combine_parts(GatherArgs g, Params p)
{
    __shared__ __attribute__((aligned(16))) float part[GW_MERGED][64 * K * VEC];
    __shared__ int part_found[GW_MERGED];
    __shared__ int meta[GW_MERGED][4];
    const int n_split = min(g.work_n[WORK_CLASSES + 1], g.slot_cap);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, tid = threadIdx.x;
    const int C = p.C;
    for (int j = blockIdx.x; j < n_split; j += gridDim.x) {
        const int4 sp = g.split[j];
        const int id = sp.x, base = sp.y, P = sp.z, expected = sp.w;
        if (base < 0 || P <= 0 || (long long)base + P > g.slot_cap) continue;      // never written by k_worklist (its guard fired: ST_BADID is up)
        const int q0 = (int)((long long)P * w / GW_MERGED), q1 = (int)((long long)P * (w + 1) / GW_MERGED);
        PartMeta mine, all;
        for (int q = q0; q < q1; q++) {      // this wavefront's run of slots
            const int4 m = g.pmeta[base + q];
            mine.fold(m.x, m.y, m.z, m.w);
        }
        if (lane == 0) { meta[w][0] = mine.found; meta[w][1] = mine.nviews; meta[w][2] = mine.first; meta[w][3] = mine.last; }
        __syncthreads();
#pragma unroll
        for (int ww = 0; ww < GW_MERGED; ww++) all.fold(meta[ww][0], meta[ww][1], meta[ww][2], meta[ww][3]);
        __syncthreads();
        if (all.found != expected) {
            if (tid == 0) atomicAdd(&g.status[ST_BOXMISS], 1);
            gather_voxel_block<K, VEC, U, GW_MERGED>(g, p, id, expected, part, part_found, true);      // count / views_hit included
            __syncthreads();
            continue;
        }
        for (int cb = 0; cb < C; cb += Row<K, VEC>::CB) {
            Acc<K, VEC> acc;
            acc_zero(acc);
            for (int q = q0; q < q1; q += U) {
                Acc<K, VEC> r[U];
#pragma unroll
                for (int u = 0; u < U; u++)
                    if (q + u < q1) acc_load<K, VEC>(r[u], g.prow + (long long)(base + q + u) * C + cb, cb, C, lane);
#pragma unroll
                for (int u = 0; u < U; u++)
                    if (q + u < q1) {
#pragma unroll
                        for (int i = 0; i < K * VEC; i++) acc.a[i] += r[u].a[i];
                    }
            }
            Run<Row<K, VEC>::CB, GW_MERGED> run;
            float *orow = g.out + (long long)id * C + cb;
            run.load(orow, cb, C);
            lds_meet<K, VEC, GW_MERGED>(acc, part, run);
            run.store(orow, cb, C);
            __syncthreads();
        }
        if (tid == 0) {
            g.count[id] += all.found;
            if (g.views_hit) g.views_hit[id] += all.nviews;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// One-view calls (B*V == 1): what the unchanged reference pipeline issues, once per image (debug_project_features.py:201-208),
// and what the aggregator's parity mode issues.  A one-view gather is SHORT -- R2: ~27 k touched voxels of ~20 pixels each,
// 1.09 GB, a quarter of a millisecond -- so what k_gather spends per voxel outside the row loads is most of it: a workgroup
// launched per 4 voxel IDs of the scene (50 000 for R2, 45 % of which find nothing to do), and in every wavefront a chain
// of dependent steps before the first row load goes out (work-list entry -> cell of the voxel -> view entry -> box on one
// lane -> ID tile -> ballot).  Here:
//   * the grid is a fixed number of wavefronts (a few per SIMD); wavefront w takes the entries w, w + NW, w + 2 NW, ... of
//     the size-ordered work list -- a static deal of a list that is sorted longest-first, no queue word to contend for;
//   * lane j of the wavefront takes the j-th of ITS entries: the IDs, cells and pixel counts of all the wavefront's voxels
//     arrive in one round of loads instead of one chain per voxel, and their pixel boxes are computed side by side, one
//     voxel per lane (in k_gather the box computation is laid out lane = view: for one view, ~350 VALU instructions on ONE
//     lane at the head of every voxel's chain);
//   * while voxel j's rows stream, the ID tile and the output row of voxel j + 1 are already in flight.
// Every voxel up to the split threshold is still summed by one wavefront in (y, x) order from the row already in `out`: the
// oracle's bits.  Voxels above it are cut into parts (round 6, gather_part_one): the parts lead the deal, k_combine_parts follows on
// the stream.  With VP_OPT_ONE_VIEW_SPLIT = 0 (round 5's path, the A/B arm) the voxels above 320 pixels go to workgroups of the same
// launch instead, four wavefronts per voxel, which join the deal afterwards.
// ------------------------------------------------------------------------------------------------
template <int K, int VEC, int U>
__global__ __launch_bounds__(256) void k_gather_one(GatherArgs g, Params p)
{
    __builtin_amdgcn_s_setprio(3);
    // rows in flight per wavefront of the heavy role: 8 (the deal's wavefronts: U) -- a close-up frame is ALL heavy voxels, a few
    // hundred workgroups of four wavefronts each: with 4 rows of 2 KiB per wavefront too few bytes are in flight to fill HBM
    constexpr int UH = (VEC == 4 && U < 8) ? 8 : U;
    __shared__ __attribute__((aligned(16))) float part[GW_MERGED][64 * K * VEC];
    __shared__ int part_found[GW_MERGED];
    if ((int)blockIdx.x < g.heavy_blocks) {
        const int n_heavy = *g.n_heavy;
        for (int h = blockIdx.x; h < n_heavy; h += g.heavy_blocks) {
            const int id = g.heavy_list[h];
            if (id < g.row_lo || id >= g.row_hi) continue;
            const int expected = g.cnt_call[id];
            if (!gather_voxel_block<K, VEC, UH, GW_MERGED>(g, p, id, expected, part, part_found, false)) {
                if (threadIdx.x == 0) atomicAdd(&g.status[ST_BOXMISS], 1);
                gather_voxel_block<K, VEC, UH, GW_MERGED>(g, p, id, expected, part, part_found, true);
            }
        }
    }
    const int lane = threadIdx.x & 63;
    const long long NW = (long long)gridDim.x * 4;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    // Parts of the view's split voxels (round 6) lead the deal -- they are its longest items: the items of the launch are the
    // n_parts parts, then the size-ordered list; wavefront w takes the items w, w + NW, w + 2 NW, ...  One wavefront per part, into
    // the part's slot; k_combine_parts follows on the stream.
    long long first = w;      // this wavefront's first entry of the list
    if (g.host_word && blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_store(g.host_word, (int)(0x80000000u | ((unsigned)g.host_seq << 16) | (unsigned)min(g.work_n[WORK_CLASSES + 1], 0xffff)),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (g.parts_on) {
        const long long n_parts = min(g.work_n[WORK_CLASSES], g.slot_cap);
        long long s = w;
        for (; s < n_parts; s += NW) gather_part_one<K, VEC, U>(g, p, (int)s, lane);
        first = s - n_parts;
    }
    int n[WORK_CLASSES];
    long long total = 0;
#pragma unroll
    for (int k = 0; k < WORK_CLASSES; k++) { n[k] = g.work_n[k]; total += n[k]; }
    const int W = p.width, H = p.height, C = p.C;
    for (long long base = first; base < total; base += 64 * NW) {
        // lane j: the j-th entry of this wavefront in this batch -- ID, box (x1 < x0: none, scan the whole image), pixel count
        const long long r = base + (long long)lane * NW;
        const int id_l = r < total ? work_item(g, p, r, n) : 0;
        Box bx_l = {0, 0, -1, -1};
        int cnt_l = 0;
        if (id_l != 0) {
            cnt_l = g.cnt_call[id_l];
            bx_l = only_view_box(g, p, g.cell_of_id[id_l]);
        }
        const int nv = __popcll(__ballot(id_l != 0));      // the entries of a wavefront fill its lanes from 0 upwards
        // the first voxel's ID tile and output row
        int id = 0, expected = 0, tile = 0;
        Box bx = {0, 0, -1, -1};
        Acc<K, VEC> acc;
        auto fetch = [&](int j) {
            id = __builtin_amdgcn_readlane(id_l, j);
            expected = __builtin_amdgcn_readlane(cnt_l, j);
            bx = {__builtin_amdgcn_readlane(bx_l.x0, j), __builtin_amdgcn_readlane(bx_l.y0, j),
                  __builtin_amdgcn_readlane(bx_l.x1, j), __builtin_amdgcn_readlane(bx_l.y1, j)};
            if (bx.x1 < bx.x0 || bx.y1 < bx.y0) bx = {0, 0, W - 1, H - 1};      // no box: the whole image
            tile = first_tile_id(g.hit, W, bx, lane);
            acc_load<K, VEC>(acc, g.out + (long long)id * C, 0, C, lane);
        };
        if (nv > 0) fetch(0);
        for (int j = 0; j < nv; j++) {
            const int cid = id, cexp = expected, ctile = tile;
            const Box cbx = bx;
            Acc<K, VEC> cacc = acc;
            if (j + 1 < nv) fetch(j + 1);       // in flight while this voxel's rows stream
            for (int cb = 0; cb < C; cb += Row<K, VEC>::CB) {
                float *orow = g.out + (long long)cid * C + cb;
                if (cb > 0) acc_load<K, VEC>(cacc, orow, cb, C, lane);
                int found = 0;
                scan_view<K, VEC, U>(g, p, 0, cid, cbx, cb, lane, cacc, found, cb == 0, ctile);
                int nviews = found > 0;
                if (found != cexp) {      // redo from the row as it still is in memory
                    acc_load<K, VEC>(cacc, orow, cb, C, lane);
                    redo_whole_images<K, VEC, U>(g, p, cid, 1, cb, lane, cacc, found, nviews);
                }
                acc_store<K, VEC, false>(cacc, orow, cb, C, lane);
                if (cb == 0 && lane == 0) {
                    g.count[cid] += found;
                    if (g.views_hit) g.views_hit[cid] += nviews;
                }
            }
        }
    }
}

}  // namespace

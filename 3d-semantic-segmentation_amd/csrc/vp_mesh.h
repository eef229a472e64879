// vp_mesh.h -- triangle-mesh rasterizer: per pixel the nearest face of an annotated mesh, its depth and its label (the
// ground-truth maps evaluate_label_maps.py scores against).  Included by voxproj.hip only, after vp_tilebin.h (the tile
// binning) and vp_splat.h (SPLAT_TILE, SPLAT_THREADS).
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// The contract (include/voxproj_mesh.h; tests/mesh_reference.py is its NumPy statement, which the kernels replay bit for
// bit).  All float arithmetic is float64 on the fp32 inputs in the written order (no contraction: the Makefile's
// -ffp-contract=off; float64 division is correctly rounded); everything that decides coverage is int64.
//
// k_mesh_project  one thread per face (mesh_setup).  Camera space c[k] = ((R[k][0] x + R[k][1] y) + R[k][2] z) + t[k]; a
//   vertex is inside when c.z >= near; a face with an inside vertex is clipped (Sutherland-Hodgman; the point on an edge from
//   its inside end s to its outside end e: tt = (near - s.z) / (e.z - s.z), q = s + tt (e - s), q.z = near) into 3 or 4
//   points, snapped to 1/256 pixel, X = floor((fx (x / z) + cx) 256 + 0.5), and fanned into the sub-triangles (p0 p1 p2),
//   (p0 p2 p3), each oriented to a positive int64 area (zero area: no sub-triangle).  The record holds both sub-triangles'
//   points, a bit per sub-triangle whose pixel box meets the image, and the plane of the UNCLIPPED face, n = (c1 - c0) x
//   (c2 - c0), d = n . c0, with the face's depth range.  The face's tiles are those of the union of its sub-triangles' pixel
//   boxes.  A face with a vertex index outside [0, n_verts), a non-finite vertex or a snapped coordinate that is non-finite
//   or beyond +-2^29 has no tiles; its kind is counted per workgroup by ballot (no atomics) and k_mesh_counters adds the
//   workgroups' counts to counters[3].
// tile_sort       the tile binning of vp_tilebin.h with 32-bit keys, the tile alone: each tile's run is in ascending face
//   index.
// k_mesh_tiles    one 256-thread workgroup per 16x16 tile, one pixel per thread, the pixel's depth and face in registers; the
//   tile's run is staged through LDS in batches of MESH_BATCH records (104 bytes each; every thread reads the same record:
//   broadcasts).  Per (pixel, sub-triangle): three edge values E = dx (P.y - a.y) - dy (P.x - a.x) with P = (256 j + 128,
//   256 i + 128), each two 32 x 32 -> 64 bit products (every factor is below 2^31: the guard band); covered when E > 0, or
//   E == 0 on an edge with dy < 0 or dy == 0 and dx > 0.  A covered sample divides once: z = d / ((n.x rx + n.y ry) + n.z),
//   NaN dropped, clamped to the face's range, kept inside [near, far], rounded to fp32; the strict < keeps the lowest face
//   index on equal depths.  Epilogue: face id (-1), depth (0), majority label of the face's three vertex labels (255).
// Every kernel after the scan reads the device total first, as vp_tilebin.h states it.
// ------------------------------------------------------------------------------------------------
constexpr int MESH_BATCH = 256;                  // records per LDS staging: 26 KiB
constexpr double MESH_GUARD = 536870912.0;       // 2^29 sub-pixel units

struct MeshCam {
    double r[12];                // world -> camera [R | t], row-major 3 x 4
    double fx, fy, cx, cy, near_z, far_z;
    int W, H;
};

struct MeshRec {                 // 104 bytes per face
    int p[12];                   // sub-triangle 0: p[0..5] = x0 y0 x1 y1 x2 y2, sub-triangle 1: p[6..11]; positive area
    int mask, pad;               // bit k: sub-triangle k exists and its pixel box meets the image
    double nx, ny, nz, d, zmin, zmax;
};
constexpr int MESH_REC_WORDS = sizeof(MeshRec) / sizeof(int);
static_assert(sizeof(MeshRec) == 104 && MESH_REC_WORDS * sizeof(int) == sizeof(MeshRec), "MeshRec layout");

// One sub-triangle of snapped points a, b, c into slot k of the record: oriented, its pixel box joined to pb (x0 y0 x1 y1).
__device__ inline void mesh_sub(int k, int ax, int ay, int bx, int by, int cx, int cy, int W, int H, MeshRec &r, int4 &pb)
{
    const long long area = (long long)(bx - ax) * (cy - ay) - (long long)(by - ay) * (cx - ax);
    if (area == 0) return;
    if (area < 0) {
        int t = bx; bx = cx; cx = t;
        t = by; by = cy; cy = t;
    }
    // pixel j's sample is 256 j + 128: the pixels whose samples lie in [min, max]
    const int j0 = max((min(ax, min(bx, cx)) + 127) >> 8, 0), j1 = min((max(ax, max(bx, cx)) - 128) >> 8, W - 1);
    const int i0 = max((min(ay, min(by, cy)) + 127) >> 8, 0), i1 = min((max(ay, max(by, cy)) - 128) >> 8, H - 1);
    if (j0 > j1 || i0 > i1) return;
    int *p = r.p + 6 * k;
    p[0] = ax; p[1] = ay; p[2] = bx; p[3] = by; p[4] = cx; p[5] = cy;
    r.mask |= 1 << k;
    pb.x = min(pb.x, j0); pb.y = min(pb.y, i0); pb.z = max(pb.z, j1); pb.w = max(pb.w, i1);
}

// Set up face i: its record, its tile box (0, 0, -1, -1 without tiles) and its kind: 0 kept or skipped, 1 a vertex index
// outside [0, n_verts), 2 a non-finite vertex, 3 beyond the guard band.
__device__ inline int mesh_setup(const float *__restrict__ verts, long long n_verts, const int *__restrict__ faces, long long i,
                                 const MeshCam &cam, MeshRec &r, int4 &tb)
{
    r = MeshRec{};
    tb = make_int4(0, 0, -1, -1);
    const int idx[3] = {faces[3 * i], faces[3 * i + 1], faces[3 * i + 2]};
    for (int v = 0; v < 3; ++v)
        if (idx[v] < 0 || idx[v] >= n_verts) return 1;
    double c[3][3];
    bool in[3], finite = true;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const float x = verts[3LL * idx[v]], y = verts[3LL * idx[v] + 1], z = verts[3LL * idx[v] + 2];
        finite &= isfinite(x) && isfinite(y) && isfinite(z);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[v][k] = ((cam.r[4 * k] * x + cam.r[4 * k + 1] * y) + cam.r[4 * k + 2] * z) + cam.r[4 * k + 3];
        in[v] = c[v][2] >= cam.near_z;
    }
    if (!finite) return 2;
    if (!in[0] && !in[1] && !in[2]) return 0;
    // clip and snap: qx, qy take the 3 or 4 points in order
    int qx[4] = {0, 0, 0, 0}, qy[4] = {0, 0, 0, 0}, np = 0;
    bool guard = false;
    auto push = [&](double x, double y, double z) {
        const double sx = floor((cam.fx * (x / z) + cam.cx) * 256.0 + 0.5), sy = floor((cam.fy * (y / z) + cam.cy) * 256.0 + 0.5);
        if (!(fabs(sx) <= MESH_GUARD) || !(fabs(sy) <= MESH_GUARD)) {       // also a NaN
            guard = true;
            return;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k == np) {
                qx[k] = (int)sx;
                qy[k] = (int)sy;
            }
        ++np;
    };
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int a = e, b = (e + 1) % 3;
        if (in[a]) push(c[a][0], c[a][1], c[a][2]);
        if (in[a] != in[b]) {
            const bool fwd = in[a];                           // s = the inside end, o = the outside end
            const double sx = fwd ? c[a][0] : c[b][0], sy = fwd ? c[a][1] : c[b][1], sz = fwd ? c[a][2] : c[b][2];
            const double ox = fwd ? c[b][0] : c[a][0], oy = fwd ? c[b][1] : c[a][1], oz = fwd ? c[b][2] : c[a][2];
            const double tt = (cam.near_z - sz) / (oz - sz);
            push(sx + tt * (ox - sx), sy + tt * (oy - sy), cam.near_z);
        }
    }
    if (guard) return 3;
    int4 pb = make_int4(cam.W, cam.H, -1, -1);
    mesh_sub(0, qx[0], qy[0], qx[1], qy[1], qx[2], qy[2], cam.W, cam.H, r, pb);
    if (np == 4) mesh_sub(1, qx[0], qy[0], qx[2], qy[2], qx[3], qy[3], cam.W, cam.H, r, pb);
    if (!r.mask) return 0;
    const double ax = c[1][0] - c[0][0], ay = c[1][1] - c[0][1], az = c[1][2] - c[0][2];
    const double bx = c[2][0] - c[0][0], by = c[2][1] - c[0][1], bz = c[2][2] - c[0][2];
    r.nx = ay * bz - az * by;
    r.ny = az * bx - ax * bz;
    r.nz = ax * by - ay * bx;
    r.d = (r.nx * c[0][0] + r.ny * c[0][1]) + r.nz * c[0][2];
    r.zmin = fmin(fmin(c[0][2], c[1][2]), c[2][2]);
    r.zmax = fmax(fmax(c[0][2], c[1][2]), c[2][2]);
    tb = make_int4(pb.x / SPLAT_TILE, pb.y / SPLAT_TILE, pb.z / SPLAT_TILE, pb.w / SPLAT_TILE);
    return 0;
}

// Thread 0 of workgroup 0 also leaves the camera in the workspace, where k_mesh_tiles reads it.
__global__ __launch_bounds__(256) void k_mesh_project(const float *__restrict__ verts, long long n_verts,
                                                      const int *__restrict__ faces, long long n, MeshCam cam,
                                                      MeshCam *__restrict__ cam_out, MeshRec *__restrict__ rec,
                                                      int4 *__restrict__ box, int *__restrict__ count, int *__restrict__ part)
{
    __shared__ int s_cnt[4][3];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * blockDim.x + tid;
    if (i == 0) *cam_out = cam;
    int kind = 0;
    if (i < n) {
        MeshRec r;
        int4 tb;
        kind = mesh_setup(verts, n_verts, faces, i, cam, r, tb);
        rec[i] = r;
        box[i] = tb;
        count[i] = (tb.z - tb.x + 1) * (tb.w - tb.y + 1);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned long long m = __ballot(kind == k + 1);
        if ((tid & 63) == 0) s_cnt[tid >> 6][k] = __popcll(m);
    }
    __syncthreads();
    if (tid < 3) part[3LL * blockIdx.x + tid] = s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid];
}

// counters[k] += the sum of the workgroups' counts (integers: any order gives the same sum).  One workgroup.
__global__ __launch_bounds__(256) void k_mesh_counters(const int *__restrict__ part, long long n_blocks, int *counters)
{
    __shared__ int s_sum[256][3];
    const int tid = threadIdx.x;
    int a[3] = {0, 0, 0};
    for (long long b = tid; b < n_blocks; b += 256)
        for (int k = 0; k < 3; ++k) a[k] += part[3 * b + k];
    for (int k = 0; k < 3; ++k) s_sum[tid][k] = a[k];
    __syncthreads();
    for (int h = 128; h >= 1; h /= 2) {
        if (tid < h)
            for (int k = 0; k < 3; ++k) s_sum[tid][k] += s_sum[tid + h][k];
        __syncthreads();
    }
    if (tid < 3) counters[tid] += s_sum[0][tid];
}

// Is the sample (PX, PY) covered by the positively oriented sub-triangle p = x0 y0 x1 y1 x2 y2?  Every difference is below
// 2^31 (coordinates within +-2^29, samples within [0, 2^23]), every product below 2^61.
__device__ inline bool mesh_covers(const int *p, int PX, int PY)
{
    bool in = true;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int ax = p[2 * e], ay = p[2 * e + 1], bx = p[2 * ((e + 1) % 3)], by = p[2 * ((e + 1) % 3) + 1];
        const int dx = bx - ax, dy = by - ay;
        const long long E = (long long)dx * (PY - ay) - (long long)dy * (PX - ax);
        const bool owner = dy < 0 || (dy == 0 && dx > 0);
        in &= E > (owner ? -1LL : 0LL);
    }
    return in;
}

// the majority of three labels, the smallest when all differ (numpy's bincount(t).argmax())
__device__ inline unsigned char mesh_majority(unsigned char a, unsigned char b, unsigned char c)
{
    if (a == b || a == c) return a;
    if (b == c) return b;
    return min(a, min(b, c));
}

__global__ __launch_bounds__(SPLAT_THREADS) void k_mesh_tiles(
    const MeshRec *__restrict__ rec, const int *__restrict__ vals, const longlong2 *__restrict__ ranges, const long long *total_p,
    long long capacity, const MeshCam *__restrict__ cam_p, const int *__restrict__ faces,
    const unsigned char *__restrict__ vertex_labels, int *__restrict__ face_ids, float *__restrict__ depth,
    unsigned char *__restrict__ labels)
{
    __shared__ __attribute__((aligned(16))) int s_rec[MESH_BATCH * MESH_REC_WORDS];
    __shared__ int s_id[MESH_BATCH];
    if (*total_p > capacity) return;
    const int tid = threadIdx.x;
    const int W = cam_p->W, H = cam_p->H;
    const double near_z = cam_p->near_z, far_z = cam_p->far_z;
    const int px = blockIdx.x * SPLAT_TILE + (tid & (SPLAT_TILE - 1)), py = blockIdx.y * SPLAT_TILE + tid / SPLAT_TILE;
    const bool inside = px < W && py < H;
    const int PX = 256 * px + 128, PY = 256 * py + 128;
    const double rx = ((px + 0.5) - cam_p->cx) / cam_p->fx, ry = ((py + 0.5) - cam_p->cy) / cam_p->fy;
    const longlong2 rg = ranges[(long long)blockIdx.y * gridDim.x + blockIdx.x];
    float best = INFINITY;
    int id = -1;
    for (long long b0 = rg.x; b0 < rg.y; b0 += MESH_BATCH) {
        const int nb = (int)(rg.y - b0 < MESH_BATCH ? rg.y - b0 : MESH_BATCH);
        __syncthreads();                                   // the previous batch has been read
        for (int k = tid; k < nb; k += SPLAT_THREADS) s_id[k] = vals[b0 + k];
        for (int e = tid; e < nb * MESH_REC_WORDS; e += SPLAT_THREADS) {
            const int k = e / MESH_REC_WORDS, w = e % MESH_REC_WORDS;
            s_rec[e] = ((const int *)(rec + vals[b0 + k]))[w];
        }
        __syncthreads();
        if (!inside) continue;
        for (int k = 0; k < nb; ++k) {
            const MeshRec *r = (const MeshRec *)(s_rec + k * MESH_REC_WORDS);
            const int mask = r->mask;
            if (!((mask & 1) && mesh_covers(r->p, PX, PY)) && !((mask & 2) && mesh_covers(r->p + 6, PX, PY))) continue;
            const double zr = r->d / ((r->nx * rx + r->ny * ry) + r->nz);
            if (zr != zr) continue;
            const double z = fmin(fmax(zr, r->zmin), r->zmax);
            if (!(z >= near_z && z <= far_z)) continue;
            const float zf = (float)z;
            if (zf < best) {
                best = zf;
                id = s_id[k];
            }
        }
    }
    if (!inside) return;
    const long long pix = (long long)py * W + px;
    if (face_ids) face_ids[pix] = id;
    if (depth) depth[pix] = id >= 0 ? best : 0.0f;
    if (labels) {
        unsigned char lab = 255;
        if (id >= 0) {
            const int *f = faces + 3LL * id;
            lab = mesh_majority(vertex_labels[f[0]], vertex_labels[f[1]], vertex_labels[f[2]]);
        }
        labels[pix] = lab;
    }
}

// workspace of one (n_faces, W, H, capacity): the tile bins with the camera and the records after `total`, and the
// workgroups' drop counts (n_blocks of them, k_mesh_project's grid) after `offs`
struct MeshLayout : TileBins<unsigned> {
    MeshCam *cam;
    MeshRec *rec;
    int *part;
    long long n_blocks;
};

inline bool mesh_layout(char *base, long long n, int W, int H, long long capacity, MeshLayout &l)
{
    l.n_blocks = (std::max<long long>(n, 1) + 255) / 256;
    return tile_layout(base, n, W, H, capacity, l, [&](Sections &s, int at) {
        if (at == 0) {
            s.place(l.cam, sizeof(MeshCam));
            s.place(l.rec, (size_t)n * sizeof(MeshRec));
        } else {
            s.place(l.part, (size_t)l.n_blocks * 3 * sizeof(int));
        }
    });
}

}  // namespace

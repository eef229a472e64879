// vp_grid.h -- stage 2, the sparse voxel grid of a Gaussian cloud: ball statistics on the bucketed grid (vp_ball_count) and the
// voxelisation (vp_voxel_grid).  include/voxproj_grid.h states the contract, tests/voxel_grid_reference.py states it in NumPy.
// Included by voxproj.hip only.
//
// k_ball_count: one lane per query.  The lane takes the box of cells that covers [q - r, q + r], padded by a cell on every
// side (any superset of the ball is correct: every candidate takes the exact float64 test), clamps it to the grid and reads
// each row of the box as ONE range of the sorted points (consecutive cells hold consecutive points, k_knn_points' rule).
// Launched in cell order the lanes of a wavefront share their box, so a row's loads are the same addresses across the
// wavefront.  No array is indexed at run time: nothing goes to scratch.
//
// vp_voxel_grid's kernels: per-block partial minima and their combination (float min is exact, so the order does not
// matter), 64-bit keys x << 42 | y << 21 | z (lexicographic (x, y, z) order, ~0 for a point not kept: it sorts last), the
// heads of the runs of equal keys after the sort, their inclusive scan (the voxel's row + 1), then one thread per voxel
// (integer colour sums over its run) and one thread per sorted point (point_voxel).  No atomics anywhere.
#pragma once

namespace {

constexpr int GRID_KEY_BITS = 21;
constexpr unsigned long long GRID_NO_KEY = ~0ull;
constexpr int GRID_PARTS = 256;                 // workgroups of the min reduction

template <bool NORMALS>
__global__ __launch_bounds__(256) void k_ball_count(const float *__restrict__ pts, const int *__restrict__ perm,
                                                    const int *__restrict__ cell_start, double gx, double gy, double gz, double h,
                                                    int nx, int ny, int nz, const float *__restrict__ q, long long M, double radius,
                                                    const float *__restrict__ radii, const float *__restrict__ pn,
                                                    const float *__restrict__ qn, double min_dot, int *__restrict__ count,
                                                    int *__restrict__ consistent)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const double qx = (double)q[i * 3 + 0], qy = (double)q[i * 3 + 1], qz = (double)q[i * 3 + 2];
    const double r = radii ? (double)radii[i] : radius;
    const double r2 = r * r, ra = fabs(r);
    double mx = 0.0, my = 0.0, mz = 0.0;
    if (NORMALS) {
        mx = (double)qn[i * 3 + 0];
        my = (double)qn[i * 3 + 1];
        mz = (double)qn[i * 3 + 2];
    }
    // the box: a NaN bound falls to an end of [-lim, lim] through fmax / fmin and the range below is empty or clamped
    const double lim = 1.0e9;
    const auto cell = [&](double v, double g) { return (long long)fmin(fmax(floor((v - g) / h), -lim), lim); };
    const long long x0 = max(cell(qx - ra, gx) - 1, 0ll), x1 = min(cell(qx + ra, gx) + 1, (long long)nx - 1);
    const long long y0 = max(cell(qy - ra, gy) - 1, 0ll), y1 = min(cell(qy + ra, gy) + 1, (long long)ny - 1);
    const long long z0 = max(cell(qz - ra, gz) - 1, 0ll), z1 = min(cell(qz + ra, gz) + 1, (long long)nz - 1);
    int cnt = 0, con = 0;
    if (x0 <= x1)
        for (long long z = z0; z <= z1; z++)
            for (long long y = y0; y <= y1; y++) {
                const long long row = (z * ny + y) * nx;
                const int b = cell_start[row + x0], e = cell_start[row + x1 + 1];
                for (int t = b; t < e; ++t) {
                    const double dx = qx - (double)pts[(long long)t * 3 + 0];
                    const double dy = qy - (double)pts[(long long)t * 3 + 1];
                    const double dz = qz - (double)pts[(long long)t * 3 + 2];
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    const bool in = d2 <= r2;
                    cnt += in ? 1 : 0;
                    if (NORMALS && in) {
                        const long long j = perm[t];
                        const double dot = (mx * (double)pn[j * 3 + 0] + my * (double)pn[j * 3 + 1]) + mz * (double)pn[j * 3 + 2];
                        con += dot > min_dot ? 1 : 0;
                    }
                }
            }
    count[i] = cnt;
    if (NORMALS && consistent) consistent[i] = con;
}

// ---- voxelisation ----
struct GridMeta {            // one per call, in the workspace
    float mc[3];             // min corner of the kept points (+inf without any)
    int n_kept;
    int bad;                 // a kept point that is not finite, or a cell index above 2^21 - 1
};

// per-block minima, kept counts and non-finite flags: part_min [GRID_PARTS][3], part_cnt [GRID_PARTS][2]
__global__ __launch_bounds__(256) void k_grid_min_part(const float *__restrict__ p, const unsigned char *__restrict__ keep,
                                                       long long N, float *__restrict__ part_min, int *__restrict__ part_cnt)
{
    __shared__ float s_min[3][256];
    __shared__ int s_cnt[2][256];
    float m0 = INFINITY, m1 = INFINITY, m2 = INFINITY;
    int n = 0, bad = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
        if (keep && !keep[i]) continue;
        const float x = p[i * 3 + 0], y = p[i * 3 + 1], z = p[i * 3 + 2];
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) bad = 1;
        m0 = fminf(m0, x);
        m1 = fminf(m1, y);
        m2 = fminf(m2, z);
        ++n;
    }
    s_min[0][threadIdx.x] = m0; s_min[1][threadIdx.x] = m1; s_min[2][threadIdx.x] = m2;
    s_cnt[0][threadIdx.x] = n; s_cnt[1][threadIdx.x] = bad;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            for (int a = 0; a < 3; ++a) s_min[a][threadIdx.x] = fminf(s_min[a][threadIdx.x], s_min[a][threadIdx.x + s]);
            s_cnt[0][threadIdx.x] += s_cnt[0][threadIdx.x + s];
            s_cnt[1][threadIdx.x] |= s_cnt[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        for (int a = 0; a < 3; ++a) part_min[blockIdx.x * 3 + a] = s_min[a][0];
        part_cnt[blockIdx.x * 2 + 0] = s_cnt[0][0];
        part_cnt[blockIdx.x * 2 + 1] = s_cnt[1][0];
    }
}

// one workgroup of GRID_PARTS threads: the parts into the meta record
__global__ __launch_bounds__(GRID_PARTS) void k_grid_min_final(const float *__restrict__ part_min, const int *__restrict__ part_cnt,
                                                               int n_parts, GridMeta *__restrict__ meta)
{
    __shared__ float s_min[3][GRID_PARTS];
    __shared__ int s_cnt[2][GRID_PARTS];
    const int t = threadIdx.x;
    const bool have = t < n_parts;
    for (int a = 0; a < 3; ++a) s_min[a][t] = have ? part_min[t * 3 + a] : INFINITY;
    s_cnt[0][t] = have ? part_cnt[t * 2 + 0] : 0;
    s_cnt[1][t] = have ? part_cnt[t * 2 + 1] : 0;
    __syncthreads();
    for (int s = GRID_PARTS / 2; s > 0; s >>= 1) {
        if (t < s) {
            for (int a = 0; a < 3; ++a) s_min[a][t] = fminf(s_min[a][t], s_min[a][t + s]);
            s_cnt[0][t] += s_cnt[0][t + s];
            s_cnt[1][t] |= s_cnt[1][t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        for (int a = 0; a < 3; ++a) meta->mc[a] = s_min[a][0];
        meta->n_kept = s_cnt[0][0];
        meta->bad = s_cnt[1][0];
    }
}

// over_flag: set (every writer stores the same 1) when a kept point's cell index does not fit the key
__global__ __launch_bounds__(256) void k_grid_keys(const float *__restrict__ p, const unsigned char *__restrict__ keep, long long N,
                                                   float vs, const GridMeta *__restrict__ meta, unsigned long long *__restrict__ keys,
                                                   int *__restrict__ vals, int *__restrict__ over_flag)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    unsigned long long key = GRID_NO_KEY;
    if (!keep || keep[i]) {
        const float top = (float)((1 << GRID_KEY_BITS) - 1);
        const float fx = floorf((p[i * 3 + 0] - meta->mc[0]) / vs), fy = floorf((p[i * 3 + 1] - meta->mc[1]) / vs),
                    fz = floorf((p[i * 3 + 2] - meta->mc[2]) / vs);
        if (fx >= 0.0f && fx <= top && fy >= 0.0f && fy <= top && fz >= 0.0f && fz <= top)
            key = ((unsigned long long)fx << (2 * GRID_KEY_BITS)) | ((unsigned long long)fy << GRID_KEY_BITS) | (unsigned long long)fz;
        else
            *over_flag = 1;                  // also a NaN index (a non-finite point: meta->bad says so already)
    }
    keys[i] = key;
    vals[i] = (int)i;
}

__global__ __launch_bounds__(256) void k_grid_heads(const unsigned long long *__restrict__ keys, long long N, int *__restrict__ heads)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= N) return;
    const unsigned long long k = keys[t];
    heads[t] = (k != GRID_NO_KEY && (t == 0 || keys[t - 1] != k)) ? 1 : 0;
}

// one thread: the verdict of the call.  total[0] = V, or 0 when the call is refused; total[1] = refused
__global__ void k_grid_total(const int *__restrict__ rank, long long N, const GridMeta *__restrict__ meta,
                             const int *__restrict__ over_flag, int *__restrict__ total, int *__restrict__ n_voxels,
                             float *__restrict__ min_corner, int *__restrict__ status)
{
    const int bad = (meta->bad || *over_flag) ? 1 : 0;
    const int V = (bad || N == 0) ? 0 : rank[N - 1];
    total[0] = V;
    total[1] = bad;
    *n_voxels = V;
    if (status) *status = bad;
    if (!bad)
        for (int a = 0; a < 3; ++a) min_corner[a] = meta->mc[a];
}

// one thread per sorted position: the start of every run, and the voxel of every point
__global__ __launch_bounds__(256) void k_grid_points(const unsigned long long *__restrict__ keys, const int *__restrict__ vals,
                                                     const int *__restrict__ heads, const int *__restrict__ rank, long long N,
                                                     const int *__restrict__ total, int *__restrict__ run_start,
                                                     int *__restrict__ point_voxel)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= N || total[1]) return;
    const bool kept = keys[t] != GRID_NO_KEY;
    const int v = rank[t] - 1;                       // >= 0 for a kept point: its run's head is at or before t
    if (heads[t]) run_start[v] = (int)t;
    point_voxel[vals[t]] = kept ? v : -1;
}

// one thread per voxel: its run of the sorted points
__global__ __launch_bounds__(256) void k_grid_voxels(const unsigned long long *__restrict__ keys, const int *__restrict__ vals,
                                                     const int *__restrict__ run_start, const int *__restrict__ total,
                                                     const GridMeta *__restrict__ meta, const unsigned char *__restrict__ colors,
                                                     double voxel_size, float *__restrict__ centers,
                                                     unsigned char *__restrict__ voxel_colors, int *__restrict__ counts,
                                                     int *__restrict__ voxel_index)
{
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    const int V = total[0];
    if (v >= V) return;
    const int b = run_start[v], e = v + 1 < V ? run_start[v + 1] : meta->n_kept;
    unsigned long long s0 = 0, s1 = 0, s2 = 0;
    for (int t = b; t < e; ++t) {
        const long long i = vals[t];
        s0 += colors[i * 3 + 0];
        s1 += colors[i * 3 + 1];
        s2 += colors[i * 3 + 2];
    }
    const unsigned long long key = keys[b], mask = (1ull << GRID_KEY_BITS) - 1;
    const int idx[3] = {(int)(key >> (2 * GRID_KEY_BITS)), (int)((key >> GRID_KEY_BITS) & mask), (int)(key & mask)};
    const double n = (double)(e - b);
    const unsigned long long s[3] = {s0, s1, s2};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        voxel_index[v * 3 + a] = idx[a];
        centers[v * 3 + a] = (float)((double)idx[a] * voxel_size + (double)meta->mc[a]);
        voxel_colors[v * 3 + a] = (unsigned char)(float)((double)s[a] / n);
    }
    counts[v] = e - b;
}

// workspace layout of one N
struct GridLayout {
    size_t meta, over, total, part_min, part_cnt, keys0, keys1, vals0, vals1, heads, rank, run_start, scan_tmp, sort_tmp, bytes;
    size_t scan_bytes, sort_bytes;
    int n_parts;
};

// host only: the rocprim calls with a NULL scratch pointer only report their scratch sizes
inline bool grid_layout(long long n, GridLayout &l)
{
    l.n_parts = (int)std::min<long long>((std::max<long long>(n, 1) + 255) / 256, GRID_PARTS);
    l.scan_bytes = 0;
    l.sort_bytes = 0;
    if (n > 0 && rocprim::inclusive_scan(nullptr, l.scan_bytes, (const int *)nullptr, (int *)nullptr, (size_t)n,
                                         rocprim::plus<int>()) != hipSuccess)
        return false;
    if (n > 0 && rocprim::radix_sort_pairs(nullptr, l.sort_bytes, (const unsigned long long *)nullptr,
                                           (unsigned long long *)nullptr, (const int *)nullptr, (int *)nullptr, (size_t)n, 0u,
                                           64u) != hipSuccess)
        return false;
    size_t off = 0;
    l.meta = off;      off += align256(sizeof(GridMeta));
    l.over = off;      off += align256(sizeof(int));
    l.total = off;     off += align256(2 * sizeof(int));
    l.part_min = off;  off += align256(GRID_PARTS * 3 * sizeof(float));
    l.part_cnt = off;  off += align256(GRID_PARTS * 2 * sizeof(int));
    l.keys0 = off;     off += align256((size_t)n * sizeof(unsigned long long));
    l.keys1 = off;     off += align256((size_t)n * sizeof(unsigned long long));
    l.vals0 = off;     off += align256((size_t)n * sizeof(int));
    l.vals1 = off;     off += align256((size_t)n * sizeof(int));
    l.heads = off;     off += align256((size_t)n * sizeof(int));
    l.rank = off;      off += align256((size_t)n * sizeof(int));
    l.run_start = off; off += align256((size_t)n * sizeof(int));
    l.scan_tmp = off;  off += align256(l.scan_bytes);
    l.sort_tmp = off;  off += align256(l.sort_bytes);
    l.bytes = off;
    return true;
}

}  // namespace

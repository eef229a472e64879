// vp_knn.h -- the k nearest OTHER points of every query among a point set bucketed on a uniform grid (vp_knn_points): the
// k-nearest version of k_nearest_voxel's shell search (vp_aux.h).  include/voxproj.h states the contract,
// tests/reg3d_reference.py states it in float64 by brute force.  Included by voxproj.hip only.
//
// One lane per query.  The lane walks Chebyshev shells of cells round the query's cell and keeps the KC best (d2, index) pairs
// sorted in registers (KC = 1, 4, 8 or 15, the smallest that holds k: every loop over the list is unrolled, so nothing is
// indexed at run time and nothing goes to scratch).  A point in a cell r + 1 shells away is at least r h from the query, so
// the walk ends once the k-th best d2 is no larger than (r h)^2; r0 (the first shell that can touch the grid) and rmax (r0 plus
// the grid's longest axis plus one: the shell that has covered the whole grid) are k_nearest_voxel's, so a query outside the
// grid, a grid one cell thick and a query with fewer than k other points all terminate.  Rows of a shell's two z faces and
// two y faces are runs of consecutive cells, and consecutive cells hold consecutive points: such a run is ONE range of the
// sorted points (two cell_start loads instead of two per cell); the other rows offer the two cells x = cx -+ r only.
// Distances: float64 sums of squares of float64-converted fp32 differences, exactly k_nearest_voxel's.  Order: the pair
// (d2, original index), a total order, so the result does not depend on the order in which cells or points are visited.
#pragma once

namespace {

constexpr int KNN_MAX_K = VP_KNN_MAX_K;
constexpr int KNN_NONE = 0x7fffffff;      // index of an empty slot of the list: after every real index in the order

template <int KC>
__global__ __launch_bounds__(256) void k_knn_points(const float *__restrict__ pts, const int *__restrict__ perm,
                                                    const int *__restrict__ cell_start, double gx, double gy, double gz, double h,
                                                    int nx, int ny, int nz, const float *__restrict__ q,
                                                    const int *__restrict__ self, long long M, int k, int *__restrict__ nbr_idx,
                                                    double *__restrict__ nbr_d2)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const double qx = (double)q[i * 3 + 0], qy = (double)q[i * 3 + 1], qz = (double)q[i * 3 + 2];
    const int me = self ? self[i] : -1;
    const double fx = floor((qx - gx) / h), fy = floor((qy - gy) / h), fz = floor((qz - gz) / h);
    const double lim = 1.0e9;
    const long long cx = (long long)fmin(fmax(fx, -lim), lim), cy = (long long)fmin(fmax(fy, -lim), lim),
                    cz = (long long)fmin(fmax(fz, -lim), lim);
    long long r0 = 0;
    r0 = max(r0, max(-cx, cx - (nx - 1)));
    r0 = max(r0, max(-cy, cy - (ny - 1)));
    r0 = max(r0, max(-cz, cz - (nz - 1)));
    const long long rmax = r0 + (long long)max(nx, max(ny, nz)) + 1;
    double bd[KC];
    int bi[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) {
        bd[j] = INFINITY;
        bi[j] = KNN_NONE;
    }
    // points [b, e) of the sorted set into the list
    const auto scan = [&](int b, int e) {
        for (int t = b; t < e; ++t) {
            const double dx = qx - (double)pts[(long long)t * 3 + 0];
            const double dy = qy - (double)pts[(long long)t * 3 + 1];
            const double dz = qz - (double)pts[(long long)t * 3 + 2];
            const double d2 = dx * dx + dy * dy + dz * dz;
            const int idx = perm[t];
            if (idx == me) continue;
            if (d2 < bd[KC - 1] || (d2 == bd[KC - 1] && idx < bi[KC - 1])) {
                bd[KC - 1] = d2;
                bi[KC - 1] = idx;
#pragma unroll
                for (int j = KC - 1; j > 0; --j)
                    if (bd[j] < bd[j - 1] || (bd[j] == bd[j - 1] && bi[j] < bi[j - 1])) {
                        const double td = bd[j]; bd[j] = bd[j - 1]; bd[j - 1] = td;
                        const int ti = bi[j]; bi[j] = bi[j - 1]; bi[j - 1] = ti;
                    }
            }
        }
    };
    for (long long r = r0; r <= rmax; r++) {
        const long long z0 = max(cz - r, 0ll), z1 = min(cz + r, (long long)nz - 1);
        const long long y0 = max(cy - r, 0ll), y1 = min(cy + r, (long long)ny - 1);
        const long long x0 = max(cx - r, 0ll), x1 = min(cx + r, (long long)nx - 1);
        for (long long z = z0; z <= z1; z++)
            for (long long y = y0; y <= y1; y++) {
                const long long row = (z * ny + y) * nx;
                if ((llabs(z - cz) == r) || (llabs(y - cy) == r)) {
                    if (x0 <= x1) scan(cell_start[row + x0], cell_start[row + x1 + 1]);
                } else {                                              // r > 0 here: the two cells are distinct
                    if (cx - r >= 0 && cx - r < nx) scan(cell_start[row + cx - r], cell_start[row + cx - r + 1]);
                    if (cx + r >= 0 && cx + r < nx) scan(cell_start[row + cx + r], cell_start[row + cx + r + 1]);
                }
            }
        double kd = bd[0];
        int ki = bi[0];
#pragma unroll
        for (int j = 1; j < KC; ++j)
            if (j == k - 1) {
                kd = bd[j];
                ki = bi[j];
            }
        const double bound = (double)r * h;          // everything in shells > r is at least r h away
        if (ki != KNN_NONE && kd <= bound * bound) break;
    }
#pragma unroll
    for (int j = 0; j < KC; ++j)
        if (j < k) {
            const bool none = bi[j] == KNN_NONE;
            nbr_idx[i * k + j] = none ? -1 : bi[j];
            if (nbr_d2) nbr_d2[i * k + j] = none ? (double)INFINITY : bd[j];
        }
}

}  // namespace

// vp_densify.h -- adaptive density control: the per-view statistic (vp_densify_accumulate), the per-Gaussian decision and the
// source row of every output row (vp_densify_plan), the row gather that moves every per-Gaussian array (vp_densify_rows) and
// the geometry of the split children (vp_densify_split).  include/voxproj.h states the contract, tests/densify_reference.py
// states it in NumPy.  Included by voxproj.hip only, after vp_splat.h (SplatCam, splat_chain, SplatLayout, rocprim's scan).
//
//   k_densify_accumulate  one thread per Gaussian; a Gaussian without tiles (count == 0 in the splat workspace) is left alone.
//                         The radius comes from splat_chain, the projection's own float64 chain.
//   k_densify_decide      one thread per Gaussian: the rule below, once, into three bits (densify_rule is its only statement).
//   rocprim::inclusive_scan over the bits widened to {kept, clones, splitting} counters (a transform iterator, no copy).
//   k_densify_emit        one thread per Gaussian: its rows' positions from the scan, in the fixed output order; the thread
//                         of the last Gaussian writes counts.
//   k_densify_rows        the hot path: a group of G lanes per output row, G a power of two in [1, 64] picked per array from
//                         its width (densify_pick_lanes), 16-byte accesses when width, strides and pointers allow.  Lane 0 of
//                         a group reads src / kind and the group takes them by a shuffle.  All arrays go in one launch: the
//                         grid is cut into one stretch of workgroups per array, each stretch strides over the rows.  The kept
//                         rows are in ascending source order, so the gather streams; the clones and children re-read rows
//                         the kept stretch has just pulled through the caches.  A group keeps four rows in flight (indices,
//                         then loads, then stores): measured on the MI355X at 1 000 000 Gaussians and 16 arrays
//                         (profiles/r25_densify.jsonl) one row per round moved 784 MB in 0.317 ms, four in 0.176 ms.
//   k_densify_split       one thread per output row; Philox4x32-10 and Box-Muller in float64 for the children.
// Every kernel that takes n_out reads the device total first and writes nothing when they differ (status = 1); every source
// index is checked against n_src before it is used as an address.
#pragma once

#include <rocprim/iterator/transform_iterator.hpp>

namespace {

constexpr int DENSIFY_THREADS = 256;
constexpr long long DENSIFY_MAX_N = 1LL << 30;           // 2 N output rows fit an int
constexpr int DENSIFY_MAX_BLOCKS = 1 << 16;              // workgroups per array in k_densify_rows (grid-stride beyond)
constexpr int DENSIFY_ROWS_IN_FLIGHT = 4;                // rows a lane group of k_densify_rows moves per round
constexpr float DENSIFY_CHILD_SCALE = 0.625f;            // 1 / (0.8 * 2), exact in binary
constexpr float DENSIFY_CHILD_LOG = -0.47000362924573555f;   // rounds to the fp32 nearest to ln 0.625

struct alignas(16) DensifyCnt {
    int kept, clone, split, pad;
};

struct DensifyPlus {
    __host__ __device__ DensifyCnt operator()(const DensifyCnt &a, const DensifyCnt &b) const
    {
        return DensifyCnt{a.kept + b.kept, a.clone + b.clone, a.split + b.split, 0};
    }
};

struct DensifyWiden {                                    // the decision bits as counters
    __host__ __device__ DensifyCnt operator()(unsigned char f) const { return DensifyCnt{f & 1, (f >> 1) & 1, (f >> 2) & 1, 0}; }
};

using DensifyFlagIter = rocprim::transform_iterator<const unsigned char *, DensifyWiden, DensifyCnt>;

struct DensifyRule {
    float grad_threshold, size_threshold, min_opacity, max_screen_size, max_world_size;
};

// The rule, stated once (include/voxproj.h has it in words): bit 0 the original survives, bit 1 one clone, bit 2 two children.
__device__ __forceinline__ unsigned densify_rule(float accum, int den, const float *max_radius, long long g, float s0, float s1,
                                                 float s2, float opacity, const DensifyRule &r)
{
    float gm = den ? accum / (float)den : 0.0f;
    if (gm != gm) gm = 0.0f;
    const float smax = fmaxf(fmaxf(s0, s1), s2);
    const bool sel = gm >= r.grad_threshold;
    const bool clone = sel && smax <= r.size_threshold, split = sel && smax > r.size_threshold;
    const bool low = opacity < r.min_opacity, on = r.max_screen_size > 0.0f;
    const bool bigw = on && smax > r.max_world_size, bigw_child = on && smax * DENSIFY_CHILD_SCALE > r.max_world_size;
    const bool bigv = on && max_radius && max_radius[g] > r.max_screen_size;
    const unsigned keep = !split && !low && !bigv && !bigw;
    const unsigned one = clone && !low && !bigw;
    const unsigned two = split && !low && !bigw_child;
    return keep | (one << 1) | (two << 2);
}

__global__ __launch_bounds__(DENSIFY_THREADS) void k_densify_accumulate(const float *__restrict__ grad_screen, long long n,
                                                                        double hw2, double hh2, double scale,
                                                                        const float *__restrict__ means,
                                                                        const float *__restrict__ quats,
                                                                        const float *__restrict__ scales, SplatCam cam,
                                                                        const int *__restrict__ count,
                                                                        float *__restrict__ grad_accum, int *__restrict__ denom,
                                                                        float *__restrict__ max_radius)
{
    const long long i = (long long)blockIdx.x * DENSIFY_THREADS + threadIdx.x;
    if (i >= n || count[i] <= 0) return;
    const float gx = grad_screen[SPLAT_SCREEN * i], gy = grad_screen[SPLAT_SCREEN * i + 1];
    const double norm = sqrt((double)gx * gx * hw2 + (double)gy * gy * hh2) * scale;
    grad_accum[i] += (float)norm;
    denom[i] += 1;
    if (max_radius) {
        SplatChain ch;
        splat_chain(means[3 * i], means[3 * i + 1], means[3 * i + 2], quats[4 * i], quats[4 * i + 1], quats[4 * i + 2],
                    quats[4 * i + 3], scales[3 * i], scales[3 * i + 1], scales[3 * i + 2], cam, ch);
        const double mid = 0.5 * (ch.s00 + ch.s11), hd = 0.5 * (ch.s00 - ch.s11);
        const float rad = (float)(3.0 * sqrt(mid + sqrt(fmax(0.1, hd * hd + ch.s01 * ch.s01))));
        max_radius[i] = fmaxf(max_radius[i], rad);
    }
}

__global__ __launch_bounds__(DENSIFY_THREADS) void k_densify_decide(const float *__restrict__ grad_accum,
                                                                    const int *__restrict__ denom,
                                                                    const float *__restrict__ max_radius,
                                                                    const float *__restrict__ scales,
                                                                    const float *__restrict__ opac, long long n, DensifyRule rule,
                                                                    unsigned char *__restrict__ flags)
{
    const long long g = (long long)blockIdx.x * DENSIFY_THREADS + threadIdx.x;
    if (g >= n) return;
    flags[g] = (unsigned char)densify_rule(grad_accum[g], denom[g], max_radius, g, scales[3 * g], scales[3 * g + 1],
                                           scales[3 * g + 2], opac[g], rule);
}

// at least one workgroup: without Gaussians thread 0 writes the four zeros
__global__ __launch_bounds__(DENSIFY_THREADS) void k_densify_emit(const unsigned char *__restrict__ flags,
                                                                  const DensifyCnt *__restrict__ sums, long long n,
                                                                  int *__restrict__ src, unsigned char *__restrict__ kind,
                                                                  long long *__restrict__ counts)
{
    const long long g = (long long)blockIdx.x * DENSIFY_THREADS + threadIdx.x;
    if (n == 0) {
        if (g == 0) counts[0] = counts[1] = counts[2] = counts[3] = 0;
        return;
    }
    if (g >= n) return;
    const DensifyCnt tot = sums[n - 1], inc = sums[g];
    const unsigned f = flags[g];
    const long long K = tot.kept, C = tot.clone, S = tot.split;
    if (f & 1) {
        const long long r = inc.kept - 1;
        src[r] = (int)g;
        kind[r] = 0;
    }
    if (f & 2) {
        const long long r = K + inc.clone - 1;
        src[r] = (int)g;
        kind[r] = 1;
    }
    if (f & 4) {
        const long long r0 = K + C + inc.split - 1, r1 = r0 + S;
        src[r0] = (int)g;
        kind[r0] = 2;
        src[r1] = (int)g;
        kind[r1] = 3;
    }
    if (g == n - 1) {
        counts[0] = K + C + 2 * S;
        counts[1] = K;
        counts[2] = C;
        counts[3] = S;
    }
}

// lanes per row: the smallest power of two that covers the row's accesses in one pass, 64 at the most
static inline int densify_pick_lanes(int units)
{
    int lg = 0;
    while ((1 << lg) < units && lg < 6) ++lg;
    return lg;
}

struct DensifyRowsArgs {
    vp_densify_array a[VP_DENSIFY_MAX_ARRAYS];
    int blk_start[VP_DENSIFY_MAX_ARRAYS + 1];            // the workgroups [blk_start[a], blk_start[a + 1]) serve array a
    unsigned char lg[VP_DENSIFY_MAX_ARRAYS];             // log2 of the lanes per row
    unsigned char vec[VP_DENSIFY_MAX_ARRAYS];            // 16-byte accesses
    int n;
};

__device__ __forceinline__ void densify_zero(unsigned &v) { v = 0u; }
__device__ __forceinline__ void densify_zero(uint4 &v) { v = make_uint4(0u, 0u, 0u, 0u); }

// One array's stretch of workgroups: T is the access (a word, or four where DensifyRowsArgs::vec allows), `units` the
// accesses of a row.  Every lane group has DENSIFY_ROWS_IN_FLIGHT rows in flight: their indices first, then their loads, then
// their stores, so a lane waits for memory once per round and not once per row.
template <typename T>
__device__ __forceinline__ void densify_rows_stretch(const vp_densify_array &d, int lg, long long blk, long long nblk,
                                                     const int *__restrict__ src, const unsigned char *__restrict__ kind,
                                                     long long n_src, long long n_out, int *status)
{
    constexpr int U = DENSIFY_ROWS_IN_FLIGHT, WORDS = sizeof(T) / 4;
    const int G = 1 << lg, rpb = DENSIFY_THREADS >> lg, l = threadIdx.x & (G - 1), units = d.width / WORDS;
    const long long sstride = d.src_stride / WORDS, dstride = d.dst_stride / WORDS;
    const T *sbase = (const T *)d.src;
    T *dbase = (T *)d.dst;
    const bool zero_new = d.fill == VP_DENSIFY_ZERO;
    for (long long row0 = blk * rpb * U; row0 < n_out; row0 += nblk * rpb * U) {
        long long r[U];
        int s[U], k[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            r[u] = row0 + (long long)u * rpb + (threadIdx.x >> lg);
            s[u] = -1;
            k[u] = 0;
            if (r[u] < n_out && l == 0) {
                s[u] = src[r[u]];
                k[u] = kind[r[u]];
            }
        }
        if (G > 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                s[u] = __shfl(s[u], 0, G);
                k[u] = __shfl(k[u], 0, G);
            }
        }
        bool ok[U], copy[U];
        T v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ok[u] = r[u] < n_out && s[u] >= 0 && s[u] < n_src;
            if (r[u] < n_out && !ok[u] && l == 0 && status) *status = 1;
            copy[u] = ok[u] && !(zero_new && k[u] != 0);
            densify_zero(v[u]);
            if (copy[u] && l < units) v[u] = sbase[(long long)s[u] * sstride + l];
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (ok[u] && l < units) dbase[r[u] * dstride + l] = v[u];
        // rows wider than one pass of the group (more than 64 accesses)
        for (int c = l + G; c < units; c += G) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                densify_zero(v[u]);
                if (copy[u]) v[u] = sbase[(long long)s[u] * sstride + c];
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (ok[u]) dbase[r[u] * dstride + c] = v[u];
        }
    }
}

__global__ __launch_bounds__(DENSIFY_THREADS) void k_densify_rows(const DensifyRowsArgs A, const int *__restrict__ src,
                                                                  const unsigned char *__restrict__ kind,
                                                                  const long long *__restrict__ counts, long long n_src,
                                                                  long long n_out, int *status)
{
    if (counts[0] != n_out) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && status) *status = 1;
        return;
    }
    int a = 0;
    while (a + 1 < A.n && (int)blockIdx.x >= A.blk_start[a + 1]) ++a;
    const vp_densify_array d = A.a[a];
    const long long blk = (int)blockIdx.x - A.blk_start[a], nblk = A.blk_start[a + 1] - A.blk_start[a];
    if (A.vec[a]) densify_rows_stretch<uint4>(d, A.lg[a], blk, nblk, src, kind, n_src, n_out, status);
    else densify_rows_stretch<unsigned>(d, A.lg[a], blk, nblk, src, kind, n_src, n_out, status);
}

// Philox4x32-10 (Salmon et al., SC'11): counter c[4], key k[2]; the result replaces c
__device__ __forceinline__ void densify_philox(unsigned (&c)[4], unsigned k0, unsigned k1)
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1,
                       n3 = (unsigned)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

__global__ __launch_bounds__(DENSIFY_THREADS) void k_densify_split(const float *__restrict__ means,
                                                                   const float *__restrict__ quats,
                                                                   const float *__restrict__ log_scales, long long n_src,
                                                                   const int *__restrict__ src,
                                                                   const unsigned char *__restrict__ kind,
                                                                   const long long *__restrict__ counts, long long n_out,
                                                                   unsigned seed_lo, unsigned seed_hi,
                                                                   float *__restrict__ out_means,
                                                                   float *__restrict__ out_log_scales, int *status)
{
    if (counts[0] != n_out) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && status) *status = 1;
        return;
    }
    const long long r = (long long)blockIdx.x * DENSIFY_THREADS + threadIdx.x;
    if (r >= n_out) return;
    const long long g = src[r];
    const int k = kind[r];
    if (g < 0 || g >= n_src) {
        if (status) *status = 1;
        return;
    }
    float m[3] = {means[3 * g], means[3 * g + 1], means[3 * g + 2]};
    float ls[3] = {log_scales[3 * g], log_scales[3 * g + 1], log_scales[3 * g + 2]};
    if (k >= 2) {
        unsigned c[4] = {(unsigned)g, (unsigned)(k - 2), 0u, 0u};
        densify_philox(c, seed_lo, seed_hi);
        double u[4];
        for (int j = 0; j < 4; ++j) u[j] = ((double)c[j] + 0.5) * 0x1p-32;
        const double two_pi = 6.283185307179586;
        const double r0 = sqrt(-2.0 * log(u[0])), r2 = sqrt(-2.0 * log(u[2]));
        const double xi[3] = {r0 * cos(two_pi * u[1]), r0 * sin(two_pi * u[1]), r2 * cos(two_pi * u[3])};
        const float qw = quats[4 * g], qx = quats[4 * g + 1], qy = quats[4 * g + 2], qz = quats[4 * g + 3];
        const double qi = 1.0 / sqrt(splat_quat_norm2(qw, qx, qy, qz)), w = qw * qi, x = qx * qi, y = qy * qi, z = qz * qi;
        const double R[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)},
                                {2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)},
                                {2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)}};
        double v[3];
        for (int j = 0; j < 3; ++j) v[j] = exp((double)ls[j]) * xi[j];
        for (int j = 0; j < 3; ++j) {
            m[j] = (float)((double)m[j] + ((R[j][0] * v[0] + R[j][1] * v[1]) + R[j][2] * v[2]));
            ls[j] = ls[j] + DENSIFY_CHILD_LOG;
        }
    }
    for (int j = 0; j < 3; ++j) {
        out_means[3 * r + j] = m[j];
        out_log_scales[3 * r + j] = ls[j];
    }
}

// scratch of vp_densify_plan: the decision bits, the scanned counters, rocprim's own scratch
struct DensifyLayout {
    size_t flags, sums, scan_tmp, bytes, scan_bytes;
};

inline bool densify_layout(long long n, DensifyLayout &l)
{
    l.scan_bytes = 0;
    if (n > 0 && rocprim::inclusive_scan(nullptr, l.scan_bytes, DensifyFlagIter(nullptr, DensifyWiden()), (DensifyCnt *)nullptr,
                                         (size_t)n, DensifyPlus()) != hipSuccess)
        return false;
    size_t off = 0;
    l.flags = off;    off += align256((size_t)n);
    l.sums = off;     off += align256((size_t)n * sizeof(DensifyCnt));
    l.scan_tmp = off; off += align256(l.scan_bytes);
    l.bytes = off > 0 ? off : 256;
    return true;
}

}  // namespace

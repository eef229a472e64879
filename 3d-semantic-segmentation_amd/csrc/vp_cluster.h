// vp_cluster.h -- label sums over a feature table (vp_label_sums) and the rows' inverse norms (vp_row_inv_norms).
// include/voxproj_cluster.h states the contract, tests/label_sums_reference.py states it in NumPy.  Included by voxproj.hip only.
//
// The projector's voxel-major gather as a primitive: sort the rows by destination, then one wavefront per destination (or per
// part of R rows of a long one) sums its rows in registers in ascending row index; a second pass adds a label's partial rows
// in float64 in part order.  A lane keeps the channels its 16-byte slot of the row holds, so no sum crosses lanes and the
// order of every float32 addition is fixed by the contract, not by the schedule.  No float atomics; the only atomics are
// the integer counts of the status words.
#pragma once

namespace {

constexpr int CL_MAX_K = 65536;
constexpr int CL_MAX_C = 4096;
constexpr int CL_U = 4;                          // rows in flight per wavefront of the sum pass
constexpr int CL_WAVES = 4;                      // wavefronts per workgroup of the sum pass
constexpr long long CL_DEFAULT_PARTS = 32768;    // the default R cuts the table into about this many parts ...
constexpr long long CL_MIN_PART_ROWS = 256;      // ... of at least this many rows

inline long long cl_part_rows(long long n_rows, long long part_rows)
{
    // a part longer than the table is the whole of every label: the cap keeps position arithmetic within 2^31 + n_rows
    if (part_rows > 0) return std::min(part_rows, std::max(n_rows, 1ll));
    return std::max(CL_MIN_PART_ROWS, (n_rows + CL_DEFAULT_PARTS - 1) / CL_DEFAULT_PARTS);
}

// the most parts n_rows rows in K labels can make: sum_k ceil(n_k / R) <= n_rows / R + (labels with a row), and <= n_rows
inline long long cl_max_parts(long long n_rows, int K, long long R)
{
    return std::min(n_rows, n_rows / R + std::min<long long>(K, n_rows));
}

inline int cl_key_bits(int K)                    // the bits of the largest key, K
{
    int b = 1;
    while ((K >> b) != 0) ++b;
    return b;
}

// ---- the rows: W channels per lane and slot, as one 16-byte load (VEC) or one element ----
template <bool F16, bool VEC> struct ClRow {
    using T = std::conditional_t<F16, _Float16, float>;
    static constexpr int W = VEC ? (F16 ? 8 : 4) : 1;
    using Raw = std::conditional_t<VEC, uint4, T>;
    static __device__ __forceinline__ Raw load(const T *p) { return *(const Raw *)p; }
    static __device__ __forceinline__ void unpack(const Raw &raw, float (&x)[W])
    {
        if constexpr (!VEC) {
            x[0] = (float)raw;
        } else if constexpr (F16) {
            typedef _Float16 h8 __attribute__((ext_vector_type(8)));
            const h8 h = __builtin_bit_cast(h8, raw);
#pragma unroll
            for (int i = 0; i < 8; i++) x[i] = (float)h[i];
        } else {
            x[0] = __uint_as_float(raw.x); x[1] = __uint_as_float(raw.y); x[2] = __uint_as_float(raw.z); x[3] = __uint_as_float(raw.w);
        }
    }
};

// ---- vp_row_inv_norms: LPR lanes per row (64, or 16 for rows that a quarter of a wavefront covers) ----
template <bool F16, bool VEC, int LPR>
__global__ __launch_bounds__(256) void k_row_inv_norms(const void *__restrict__ rows_, long long n_rows, int C, long long stride,
                                                       float *__restrict__ inv, int *__restrict__ status)
{
    using R = ClRow<F16, VEC>;
    using T = typename R::T;
    constexpr int W = R::W, RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, sub = lane % LPR;
    const long long r = ((long long)blockIdx.x * (256 / 64) + (threadIdx.x >> 6)) * RPW + lane / LPR;
    const bool have = r < n_rows;
    const T *row = (const T *)rows_ + (have ? r : 0) * stride;
    double ss = 0.0;
    if (have)
        for (int c = sub * W; c < C; c += LPR * W) {
            float x[W];
            R::unpack(R::load(row + c), x);
#pragma unroll
            for (int i = 0; i < W; i++) ss += (double)x[i] * (double)x[i];
        }
#pragma unroll
    for (int m = LPR / 2; m > 0; m >>= 1) ss += __shfl_xor(ss, m, 64);
    if (have && sub == 0) {
        float v = 0.0f;
        if (!isfinite(ss)) atomicAdd(&status[1], 1);                 // a NaN or an infinity among the squares
        else if (ss == 0.0) atomicAdd(&status[0], 1);                // a square of a non-zero element never rounds to zero in float64
        else v = (float)(1.0 / fmax(sqrt(ss), 1e-12));
        inv[r] = v;
    }
}

// ---- vp_label_sums ----
// keys: the label, or K for a row that is left out; status[0] counts label < 0, status[1] label >= K (one integer add per wavefront)
__global__ __launch_bounds__(256) void k_label_keys(const int *__restrict__ labels, long long n, int K, unsigned *__restrict__ keys,
                                                    int *__restrict__ vals, int *__restrict__ status)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lab = i < n ? labels[i] : 0;
    const bool neg = lab < 0, over = lab >= K;
    if (i < n) {
        keys[i] = (neg || over) ? (unsigned)K : (unsigned)lab;
        vals[i] = (int)i;
    }
    const unsigned long long m_neg = __ballot(neg), m_over = __ballot(over);
    if ((threadIdx.x & 63) == 0) {
        if (m_neg) atomicAdd(&status[0], __popcll(m_neg));
        if (m_over) atomicAdd(&status[1], __popcll(m_over));
    }
}

__device__ __forceinline__ int cl_lower_bound(const unsigned *__restrict__ keys, int n, unsigned k)
{
    int lo = 0, hi = n;                          // keys[< lo] < k <= keys[>= hi]
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one thread per k in [0, K]: run_start[k] = the first sorted position with key >= k (run_start[K] = the rows kept),
// n_parts[k] = ceil(n_k / R), n_parts[K] = 0 (the scan then leaves the total in part_off[K])
__global__ __launch_bounds__(256) void k_label_runs(const unsigned *__restrict__ keys, int n, int K, long long R,
                                                    int *__restrict__ run_start, int *__restrict__ n_parts)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k > K) return;
    const int b = cl_lower_bound(keys, n, (unsigned)k);
    run_start[k] = b;
    n_parts[k] = k < K ? (int)(((long long)(cl_lower_bound(keys, n, (unsigned)k + 1u) - b) + R - 1) / R) : 0;
}

// One wavefront per part.  NS slots of 64 * W channels per pass over the part's rows, CL_U rows in flight.
template <bool F16, bool VEC, int NS>
__global__ __launch_bounds__(64 * CL_WAVES) void k_label_part_sums(const void *__restrict__ rows_, long long stride, int C,
                                                                   const int *__restrict__ vals, const float *__restrict__ scale,
                                                                   const int *__restrict__ run_start, const int *__restrict__ part_off,
                                                                   int K, long long R, long long max_parts, float *__restrict__ partials)
{
    using Rw = ClRow<F16, VEC>;
    using T = typename Rw::T;
    constexpr int W = Rw::W;
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * CL_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= max_parts || w >= part_off[K]) return;
    int lo = 0, hi = K;                          // part_off[lo] <= w < part_off[hi]; the last such lo is a label with a part
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (part_off[mid] <= w) lo = mid;
        else hi = mid;
    }
    const long long b = run_start[lo] + (w - part_off[lo]) * R, e = min(b + R, (long long)run_start[lo + 1]);
    const T *rows = (const T *)rows_;
    float *out = partials + w * C;
    for (int cb = 0; cb < C; cb += 64 * W * NS) {
        float acc[NS][W];
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
            for (int i = 0; i < W; i++) acc[s][i] = 0.0f;
        for (long long t = b; t < e; t += CL_U) {
            typename Rw::Raw raw[CL_U][NS];
            float sc[CL_U];
#pragma unroll
            for (int u = 0; u < CL_U; u++)
                if (t + u < e) {
                    const long long r = vals[t + u];
                    sc[u] = scale ? scale[r] : 1.0f;
#pragma unroll
                    for (int s = 0; s < NS; s++) {
                        const int c = cb + (s * 64 + lane) * W;
                        if (c < C) raw[u][s] = Rw::load(rows + r * stride + c);
                    }
                }
#pragma unroll
            for (int u = 0; u < CL_U; u++)
                if (t + u < e) {
#pragma unroll
                    for (int s = 0; s < NS; s++) {
                        const int c = cb + (s * 64 + lane) * W;
                        if (c < C) {
                            float x[W];
                            Rw::unpack(raw[u][s], x);
#pragma unroll
                            for (int i = 0; i < W; i++) acc[s][i] += __fmul_rn(x[i], sc[u]);
                        }
                    }
                }
        }
#pragma unroll
        for (int s = 0; s < NS; s++) {
            const int c = cb + (s * 64 + lane) * W;
            if (c < C) {
#pragma unroll
                for (int i = 0; i < W; i++) out[c + i] = acc[s][i];
            }
        }
    }
}

// One wavefront per label and 64 channels: the label's partial rows in part order, in float64; the label's count.
__global__ __launch_bounds__(64) void k_label_combine(const float *__restrict__ partials, const int *__restrict__ run_start,
                                                      const int *__restrict__ part_off, int C, float *__restrict__ sums,
                                                      int *__restrict__ counts)
{
    const int k = blockIdx.x, c = blockIdx.y * 64 + threadIdx.x;
    if (blockIdx.y == 0 && threadIdx.x == 0) counts[k] = run_start[k + 1] - run_start[k];
    if (c >= C) return;
    const long long p0 = part_off[k], p1 = part_off[k + 1];
    double s = 0.0;
    long long p = p0;
    for (; p + 4 <= p1; p += 4) {
        const float v0 = partials[p * C + c], v1 = partials[(p + 1) * C + c], v2 = partials[(p + 2) * C + c],
                    v3 = partials[(p + 3) * C + c];
        s = (((s + (double)v0) + (double)v1) + (double)v2) + (double)v3;
    }
    for (; p < p1; p++) s += (double)partials[p * C + c];
    sums[(long long)k * C + c] = (float)s;
}

// workspace layout of one (n_rows, K, C, R): the sections of its own first, rocprim's scratch, the partial rows last
struct ClusterLayout {
    size_t keys0, keys1, vals0, vals1, run_start, n_parts, part_off, scan_tmp, sort_tmp, partials, bytes;
    size_t own_bytes, scan_bytes, sort_bytes;
    long long R, max_parts;
    int bits;
};

// host arithmetic only: everything but rocprim's scratch (own_bytes: what a workspace must hold at the least)
inline void cluster_layout_own(long long n, int K, int C, long long part_rows, ClusterLayout &l)
{
    l.R = cl_part_rows(n, part_rows);
    l.max_parts = cl_max_parts(n, K, l.R);
    l.bits = cl_key_bits(K);
    l.scan_bytes = 0;
    l.sort_bytes = 0;
    l.own_bytes = 2 * align256((size_t)n * sizeof(unsigned)) + 2 * align256((size_t)n * sizeof(int)) +
                  3 * align256((size_t)(K + 1) * sizeof(int)) + align256((size_t)l.max_parts * C * sizeof(float));
}

// the rocprim calls with a NULL scratch pointer only report their scratch sizes (they ask the device: false without one)
inline bool cluster_layout(long long n, int K, int C, long long part_rows, ClusterLayout &l)
{
    cluster_layout_own(n, K, C, part_rows, l);
    if (rocprim::exclusive_scan(nullptr, l.scan_bytes, (const int *)nullptr, (int *)nullptr, 0, (size_t)(K + 1),
                                rocprim::plus<int>()) != hipSuccess)
        return false;
    if (n > 0 && rocprim::radix_sort_pairs(nullptr, l.sort_bytes, (const unsigned *)nullptr, (unsigned *)nullptr,
                                           (const int *)nullptr, (int *)nullptr, (size_t)n, 0u, (unsigned)l.bits) != hipSuccess)
        return false;
    size_t off = 0;
    l.keys0 = off;     off += align256((size_t)n * sizeof(unsigned));
    l.keys1 = off;     off += align256((size_t)n * sizeof(unsigned));
    l.vals0 = off;     off += align256((size_t)n * sizeof(int));
    l.vals1 = off;     off += align256((size_t)n * sizeof(int));
    l.run_start = off; off += align256((size_t)(K + 1) * sizeof(int));
    l.n_parts = off;   off += align256((size_t)(K + 1) * sizeof(int));
    l.part_off = off;  off += align256((size_t)(K + 1) * sizeof(int));
    l.scan_tmp = off;  off += align256(l.scan_bytes);
    l.sort_tmp = off;  off += align256(l.sort_bytes);
    l.partials = off;  off += align256((size_t)l.max_parts * C * sizeof(float));
    l.bytes = off;
    return true;
}

// the row variant of a call: 16-byte loads where C, the base and the row stride allow
inline bool cluster_vec(const void *rows, int rows_f16, int C, long long stride)
{
    const int W = rows_f16 ? 8 : 4;
    const size_t el = rows_f16 ? 2 : 4;
    return C % W == 0 && ((uintptr_t)rows & 15) == 0 && ((size_t)stride * el) % 16 == 0;
}

}  // namespace

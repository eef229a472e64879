// vp_feature_loss.h -- the loss between a rendered feature image and a 2D feature map, and its gradient image in the
// binary16 form vp_splat_lift reads (include/voxproj.h states the contract; tests/feature_loss_reference.py in float64).
//
//   k_feature_loss           one wavefront per pixel, 64 pixels per wavefront, 256 per workgroup.  Lane L holds channels
//                            (64 j + L) 8 .. + 7 of both rows for j = 0 .. NCH - 1 in registers (as loaded: binary16 stays
//                            binary16), sums a = sum o^2, b = sum t^2, d = sum o t (or sum (o - t)^2) over its channels in
//                            ascending order, the wavefront adds the 64 lane sums in a butterfly (every lane ends with the same
//                            bits), and a second pass over the registers takes max_c |A t_c + B o_c|.  Lane i keeps pixel i's
//                            results, so the per-pixel outputs are written coalesced; {m l, m} go through the tree and the
//                            ordered sum of vp_reduce.h: slot t of workgroup b is pixel 256 b + t, one pair per workgroup; the
//                            largest m max_c |...| of a wavefront goes to the map's maximum with one integer atomic max
//                            (non-negative floats order like their bit patterns; a maximum does not depend on the order of
//                            arrival).
//   k_feature_loss_gradient  the same lane layout.  Every thread derives s and the exponent k from loss_stats, grad_loss and
//                            the map's maximum; a pixel reads its {m, A, B} and writes f16((s m) (A t_c + B o_c) 2^k).
//
// A chunk of 8 channels is loaded with 16-byte loads (VEC) or element by element; elements at or beyond C read as zeros,
// which add nothing to a sum and never win a maximum, so both paths give the same bits.
#pragma once

constexpr int FLOSS_MAX_C = 4096;
constexpr int FLOSS_THREADS = 256;        // = pixels per workgroup
constexpr int FLOSS_HEADER = 256;         // bytes: word 0 = the bit pattern of the map's maximum

typedef _Float16 floss_h8 __attribute__((ext_vector_type(8)));

static inline long long floss_blocks(long long n) { return (n + FLOSS_THREADS - 1) / FLOSS_THREADS; }
// header | one double2 per workgroup | one float4 {m, A, B, m max|A t + B o|} per pixel
static inline size_t floss_sums_bytes(long long n) { return align256((size_t)floss_blocks(n) * sizeof(double2)); }
static inline size_t floss_bytes(long long n) { return FLOSS_HEADER + floss_sums_bytes(n) + align256((size_t)n * sizeof(float4)); }

// 8 channels of one row as loaded
template <bool F16> struct FlossRow8;
template <> struct FlossRow8<true> {
    floss_h8 v;
    __device__ __forceinline__ float get(int e) const { return (float)v[e]; }
    template <bool VEC> __device__ __forceinline__ void load(const void *row, int c0, int C)
    {
        const _Float16 *p = (const _Float16 *)row;
        v = (floss_h8)(_Float16)0.0f;
        if (c0 >= C) return;
        if constexpr (VEC) v = *(const floss_h8 *)(p + c0);          // C is a multiple of 8 here: the chunk is whole
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c0 + e < C) v[e] = p[c0 + e];
        }
    }
};
template <> struct FlossRow8<false> {
    float v[8];
    __device__ __forceinline__ float get(int e) const { return v[e]; }
    template <bool VEC> __device__ __forceinline__ void load(const void *row, int c0, int C)
    {
        const float *p = (const float *)row;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.0f;
        if (c0 >= C) return;
        if constexpr (VEC) {
            const float4 lo = *(const float4 *)(p + c0), hi = *(const float4 *)(p + c0 + 4);
            v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
            v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c0 + e < C) v[e] = p[c0 + e];
        }
    }
};

template <int NCH, bool VEC, bool F16, bool COS>
__global__ __launch_bounds__(FLOSS_THREADS) void k_feature_loss(
    const void *__restrict__ image, long long pix_stride, const _Float16 *__restrict__ target, long long tgt_stride, int C,
    long long n, const float *__restrict__ weight, const float *__restrict__ alpha, float min_alpha, float4 *__restrict__ coef,
    double2 *__restrict__ block_sums, unsigned *max_bits, float *__restrict__ pixel_loss)
{
    __shared__ double s_red[2 * FLOSS_THREADS];
    const int tid = threadIdx.x, lane = tid & 63;
    const long long p_mine = (long long)blockIdx.x * FLOSS_THREADS + tid;
    // lane i of a wavefront owns pixel i of the wavefront's 64: its weight here, its results below
    float m_mine = 0.0f;
    if (p_mine < n) {
        const float w = weight ? weight[p_mine] : 1.0f;
        m_mine = w > 0.0f ? w : 0.0f;                                 // not > 0 (0, -0, negative, NaN) reads as 0
        if (alpha && !(alpha[p_mine] >= min_alpha)) m_mine = 0.0f;
    }
    float l_mine = 0.0f, A_mine = 0.0f, B_mine = 0.0f, mx_mine = 0.0f;
    const long long p0 = p_mine - lane;
    const size_t esize = F16 ? 2 : 4;
    for (int i = 0; i < 64; ++i) {
        const long long p = p0 + i;
        if (p >= n) break;
        const float m = __shfl(m_mine, i);                            // the same value in every lane: the branches are uniform
        if (m == 0.0f) continue;                                      // an invalid pixel's rows are never read
        const char *orow = (const char *)image + (size_t)p * (size_t)pix_stride * esize;
        const _Float16 *trow = target + (size_t)p * (size_t)tgt_stride;
        FlossRow8<F16> o[NCH];
        FlossRow8<true> t[NCH];
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int c0 = (j * 64 + lane) * 8;
            o[j].template load<VEC>(orow, c0, C);
            t[j].template load<VEC>(trow, c0, C);
        }
        float a = 0.0f, b = 0.0f, d = 0.0f;                           // L2: a = sum (o - t)^2 only
#pragma unroll
        for (int j = 0; j < NCH; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float ov = o[j].get(e), tv = t[j].get(e);
                if constexpr (COS) {
                    a += ov * ov;
                    b += tv * tv;
                    d += ov * tv;
                } else {
                    const float df = ov - tv;
                    a += df * df;
                }
            }
        a = lanes_sum_up<64>(a);
        float l, A, B;
        bool valid = true;
        if constexpr (COS) {
            b = lanes_sum_up<64>(b);
            d = lanes_sum_up<64>(d);
            valid = a > 0.0f && b > 0.0f;                             // false for a NaN sum as well
            const float nn = sqrtf(a) * sqrtf(b);
            const float cs = d / nn;
            l = 1.0f - cs;
            A = -1.0f / nn;
            B = cs / a;
        } else {
            l = a / (float)C;
            B = 2.0f / (float)C;
            A = -B;
        }
        float mx = 0.0f;
        if (valid) {
#pragma unroll
            for (int j = 0; j < NCH; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e) mx = fmaxf(mx, fabsf(A * t[j].get(e) + B * o[j].get(e)));
            mx = lanes_max<64>(mx) * m;
        }
        if (lane == i) {
            if (valid) { l_mine = l; A_mine = A; B_mine = B; mx_mine = mx; }
            else m_mine = 0.0f;
        }
    }
    const float wl = m_mine != 0.0f ? m_mine * l_mine : 0.0f;
    if (p_mine < n) {
        coef[p_mine] = make_float4(m_mine, A_mine, B_mine, mx_mine);
        if (pixel_loss) pixel_loss[p_mine] = wl;
    }
    const float wmax = lanes_max<64>(mx_mine);
    if (lane == 0 && wmax > 0.0f) atomicMax(max_bits, __float_as_uint(wmax));
    double sums[2] = {(double)wl, (double)m_mine};
    block_tree_sum<FLOSS_THREADS>(sums, s_red);
    if (tid == 0) block_sums[blockIdx.x] = make_double2(sums[0], sums[1]);
}

template <int NCH, bool VEC, bool F16>
__global__ __launch_bounds__(FLOSS_THREADS) void k_feature_loss_gradient(
    const void *__restrict__ image, long long pix_stride, const _Float16 *__restrict__ target, long long tgt_stride, int C,
    long long n, const float4 *__restrict__ coef, const unsigned *__restrict__ max_bits, const double *__restrict__ loss_stats,
    int mean, const float *__restrict__ grad_loss, _Float16 *__restrict__ grad, long long grad_stride, int *__restrict__ grad_exponent)
{
    const int tid = threadIdx.x, lane = tid & 63;
    // s and k, the same in every thread: s = grad_loss (SUM) or (float)(grad_loss / sum m) (MEAN; sum m = 0 gives 0);
    // k = 14 - ceil(log2(|s| max)), at most 126; a product that is not a positive finite number gives k = 0 and zeros
    const float g = grad_loss ? *grad_loss : 1.0f;
    float s = g;
    if (mean) {
        const double sm = loss_stats[1];
        s = sm > 0.0 ? (float)((double)g / sm) : 0.0f;
    }
    const float x = fabsf(s) * __uint_as_float(*max_bits);
    const bool live = x > 0.0f && x <= 3.402823466e38f;
    int k = 0;
    if (live) {
        int ex;
        const float mant = frexpf(x, &ex);                            // x = mant 2^ex, mant in [0.5, 1)
        k = min(14 - (mant == 0.5f ? ex - 1 : ex), 126);
    }
    const float scale = ldexpf(1.0f, k);                              // k in [-113, 126]: a normal float, so the product is exact
    if (blockIdx.x == 0 && tid == 0) *grad_exponent = k;

    const long long p0 = (long long)blockIdx.x * FLOSS_THREADS + (tid - lane);
    const size_t esize = F16 ? 2 : 4;
    for (int i = 0; i < 64; ++i) {
        const long long p = p0 + i;
        if (p >= n) break;
        _Float16 *grow = grad + (size_t)p * (size_t)grad_stride;
        const float4 cf = live ? coef[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // one address per wavefront
        if (cf.x == 0.0f) {                                           // an invalid pixel: a row of zeros, its maps never read
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int c0 = (j * 64 + lane) * 8;
                if (c0 >= C) continue;
                if constexpr (VEC) *(floss_h8 *)(grow + c0) = (floss_h8)(_Float16)0.0f;
                else {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (c0 + e < C) grow[c0 + e] = (_Float16)0.0f;
                }
            }
            continue;
        }
        const char *orow = (const char *)image + (size_t)p * (size_t)pix_stride * esize;
        const _Float16 *trow = target + (size_t)p * (size_t)tgt_stride;
        const float sm = s * cf.x, A = cf.y, B = cf.z;
        FlossRow8<F16> o[NCH];
        FlossRow8<true> t[NCH];
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int c0 = (j * 64 + lane) * 8;
            o[j].template load<VEC>(orow, c0, C);
            t[j].template load<VEC>(trow, c0, C);
        }
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int c0 = (j * 64 + lane) * 8;
            if (c0 >= C) continue;
            floss_h8 q;
#pragma unroll
            for (int e = 0; e < 8; ++e) q[e] = (_Float16)((sm * (A * t[j].get(e) + B * o[j].get(e))) * scale);
            if constexpr (VEC) *(floss_h8 *)(grow + c0) = q;
            else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (c0 + e < C) grow[c0 + e] = q[e];
            }
        }
    }
}

// chunks of 512 channels a wavefront holds per row: 1, 2, 4 or 8
static inline int floss_nch(int C) { return C <= 512 ? 1 : C <= 1024 ? 2 : C <= 2048 ? 4 : 8; }

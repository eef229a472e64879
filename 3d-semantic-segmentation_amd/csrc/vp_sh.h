// vp_sh.h -- view-dependent colour: the spherical-harmonics pre-pass that turns f_dc [N,3] and f_rest [N,Kr,3] into the colour
// rows [N,3] the splatter takes (vp_sh_colors), and its adjoint to the coefficients and, through the view direction, to the
// means (vp_sh_colors_backward).  include/voxproj_ext.h states the contract, tests/sh_reference.py states it in NumPy.
// Included by voxproj.hip only.
//
// The contract (fp32, no contraction; Kr = (Dmax + 1)^2 - 1, active degree d <= Dmax <= 3, sh[0] = f_dc, sh[k] = f_rest[k - 1]):
//   p = mean - campos;  r = sqrtf((p.x p.x + p.y p.y) + p.z p.z);  (x, y, z) = r > 0 ? p / r : (0, 0, 0)
//   pre[c]    = (sum_{k < (d + 1)^2} Y_k sh[k][c], added in ascending k) + 0.5
//   colour[c] = max(pre[c], 0);  bit c of clamped = pre[c] < 0
//   Y_0  =  0.28209479177387814
//   Y_1  = -0.4886025119029199 y            Y_2  =  0.4886025119029199 z             Y_3  = -0.4886025119029199 x
//   Y_4  =  1.0925484305920792 xy           Y_5  = -1.0925484305920792 yz            Y_6  =  0.31539156525252005 (2zz - xx - yy)
//   Y_7  = -1.0925484305920792 xz           Y_8  =  0.5462742152960396 (xx - yy)
//   Y_9  = -0.5900435899266435 y (3xx - yy) Y_10 =  2.890611442640554 xyz            Y_11 = -0.4570457994644658 y (4zz - xx - yy)
//   Y_12 =  0.3731763325901154 z (2zz - 3xx - 3yy)                                   Y_13 = -0.4570457994644658 x (4zz - xx - yy)
//   Y_14 =  1.445305721320277 z (xx - yy)   Y_15 = -0.5900435899266435 x (xx - 3yy)
// Backward, with g[c] = clamped bit c ? 0 : grad_colors[c]:
//   grad_sh[k][c] = Y_k g[c]  (k < (d + 1)^2; zeros beyond);   v_k = sum_c sh[k][c] g[c];   q = sum_k v_k grad Y_k (x, y, z)
//   grad_mean = r > 0 ? (q - dir (dir . q)) / r : 0            (the adjoint of the normalisation)
//
// Layout: one workgroup of SH_THREADS lanes serves SH_THREADS consecutive Gaussians.  Their f_rest rows are ONE contiguous
// stretch of memory (180 bytes a row at Dmax = 3), so the workgroup copies the stretch into LDS with consecutive lanes on
// consecutive 16-byte words (sh_stage_in) and each lane then reads its own row from LDS: the row stride is 3 Kr words, odd at
// Dmax 1 and 3, so those reads meet no bank conflict (Dmax 2: 24 words, 8-way, still far below the time the stretch takes
// to arrive).  The [N,3] arrays go the same way (sh_rows3_issue / _commit: one 16-byte word per lane), every load of a lane
// is issued before its first wait, and the outputs leave through LDS in the mirror image (sh_stage_out).  Measured at
// 1 000 000 Gaussians, degree 3 (profiles/r26_sh.jsonl): staging the inputs one after the other with four loads in flight
// ran the forward in 0.088 ms, all loads up front in 0.034 ms, 0.91 of a device copy of the same bytes.  The
// LDS copy mirrors memory from the 16-byte boundary at or below the stretch: element i sits at word s + i, s = the
// pointer's word offset from that boundary, so a base that is only 4-byte aligned (an f_rest[1:] view starts 180 bytes in)
// still moves in aligned 16-byte accesses, and only the first and last word of a stretch fall back to single floats.  With
// d < Dmax only the active head of each row is read (sh_stage_rows, single floats, consecutive lanes on consecutive words of
// a row).  No atomics, no workspace; every output element is written by exactly one lane: bit-identical from run to run.
#pragma once

namespace {

constexpr int SH_THREADS = 128;
constexpr int SH_LOADS_IN_FLIGHT = 12;                  // 16-byte loads of a lane that cover its share of the longest stretch
constexpr int SH_MAX_DEGREE = 3;
constexpr int SH_MAX_ROW = 3 * ((SH_MAX_DEGREE + 1) * (SH_MAX_DEGREE + 1) - 1);   // 45 words of f_rest per Gaussian
constexpr long long SH_MAX_N = 2147483647LL;

constexpr float SH_C0 = 0.28209479177387814f, SH_C1 = 0.4886025119029199f;
constexpr float SH_C2_0 = 1.0925484305920792f, SH_C2_2 = 0.31539156525252005f, SH_C2_4 = 0.5462742152960396f;
constexpr float SH_C3_0 = 0.5900435899266435f, SH_C3_1 = 2.890611442640554f, SH_C3_2 = 0.4570457994644658f,
                SH_C3_3 = 0.3731763325901154f, SH_C3_5 = 1.445305721320277f;

constexpr int sh_coeffs(int degree) { return (degree + 1) * (degree + 1); }

// g[0, count) -> lds[s, s + count), s returned; consecutive lanes on consecutive 16-byte words of memory.  One round: every
// lane issues all its loads (SH_LOADS_IN_FLIGHT cover the longest stretch) before it stores the first into LDS, so a stretch
// costs one wait for memory.
__device__ __forceinline__ int sh_stage_in(float *lds, const float *__restrict__ g, int count)
{
    static_assert(SH_LOADS_IN_FLIGHT * SH_THREADS * 4 >= SH_THREADS * SH_MAX_ROW + 6, "one round covers a workgroup's f_rest stretch");
    const int s = (int)(((uintptr_t)g >> 2) & 3);
    const int nq = (s + count + 3) >> 2;
    float4 v[SH_LOADS_IN_FLIGHT];
#pragma unroll
    for (int u = 0; u < SH_LOADS_IN_FLIGHT; ++u) {
        const int q = (int)threadIdx.x + u * SH_THREADS, i0 = 4 * q - s;
        v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i0 >= 0 && i0 + 4 <= count) v[u] = *reinterpret_cast<const float4 *>(g + i0);
    }
#pragma unroll
    for (int u = 0; u < SH_LOADS_IN_FLIGHT; ++u) {
        const int q = (int)threadIdx.x + u * SH_THREADS, i0 = 4 * q - s;
        if (i0 >= 0 && i0 + 4 <= count) {
            reinterpret_cast<float4 *>(lds)[q] = v[u];
        } else if (q < nq) {                         // the first or last word of the stretch: only the floats inside it
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (i0 + c >= 0 && i0 + c < count) lds[4 * q + c] = g[i0 + c];
        }
    }
    return s;
}

// An [rows,3] array (at most SH_THREADS * 3 words: one 16-byte word per lane) in two steps, so that a kernel can issue the
// loads of all its inputs before it waits for any: sh_rows3_issue starts the lane's load, sh_rows3_commit stores it into LDS.
struct SHRows3 {
    float4 v;
    int s;
    bool whole;
};

__device__ __forceinline__ SHRows3 sh_rows3_issue(const float *__restrict__ g, int count)
{
    static_assert((3 * SH_THREADS + 3 + 3) / 4 <= SH_THREADS, "one 16-byte word per lane covers an [SH_THREADS,3] array");
    SHRows3 r;
    r.s = (int)(((uintptr_t)g >> 2) & 3);
    const int i0 = 4 * (int)threadIdx.x - r.s;
    r.whole = i0 >= 0 && i0 + 4 <= count;
    r.v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (r.whole) r.v = *reinterpret_cast<const float4 *>(g + i0);
    return r;
}

__device__ __forceinline__ int sh_rows3_commit(float *lds, const SHRows3 &r, const float *__restrict__ g, int count)
{
    const int q = threadIdx.x, i0 = 4 * q - r.s;
    if (r.whole) {
        reinterpret_cast<float4 *>(lds)[q] = r.v;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (i0 + c >= 0 && i0 + c < count) lds[4 * q + c] = g[i0 + c];
    }
    return r.s;
}

// the first `act` words of `rows` rows of `row` words each -> the same places of lds (s = 0); act is a constant of the kernel
template <int ACT>
__device__ __forceinline__ void sh_stage_rows(float *lds, const float *__restrict__ g, int rows, int row)
{
    if (ACT == 0) return;
    for (int j = threadIdx.x; j < rows * ACT; j += SH_THREADS) {
        const int r = j / (ACT > 0 ? ACT : 1), c = j - r * ACT;
        lds[r * row + c] = g[(long long)r * row + c];
    }
}

// lds[s, s + count) -> g[0, count), the mirror image of sh_stage_in (s = g's word offset from its 16-byte boundary)
__device__ __forceinline__ void sh_stage_out(float *__restrict__ g, const float *lds, int count)
{
    const int s = (int)(((uintptr_t)g >> 2) & 3);
    const int nq = (s + count + 3) >> 2;
    for (int q = threadIdx.x; q < nq; q += SH_THREADS) {
        const int i0 = 4 * q - s;
        if (i0 >= 0 && i0 + 4 <= count) {
            *reinterpret_cast<float4 *>(g + i0) = reinterpret_cast<const float4 *>(lds)[q];
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (i0 + c >= 0 && i0 + c < count) g[i0 + c] = lds[4 * q + c];
        }
    }
}

__device__ __forceinline__ int sh_shift(const float *g) { return (int)(((uintptr_t)g >> 2) & 3); }

// the view direction of one Gaussian: (x, y, z) and r = |mean - campos|; the direction is 0 when the mean is the camera centre
__device__ __forceinline__ void sh_direction(const float *m, float cx, float cy, float cz, float &x, float &y, float &z, float &r)
{
    const float px = m[0] - cx, py = m[1] - cy, pz = m[2] - cz;
    r = sqrtf((px * px + py * py) + pz * pz);
    const bool ok = r > 0.0f;
    x = ok ? px / r : 0.0f;
    y = ok ? py / r : 0.0f;
    z = ok ? pz / r : 0.0f;
}

// Y_1 .. Y_{(D+1)^2 - 1} into Y[k - 1]
template <int D>
__device__ __forceinline__ void sh_basis(float x, float y, float z, float *Y)
{
    if (D > 0) {
        Y[0] = -SH_C1 * y;
        Y[1] = SH_C1 * z;
        Y[2] = -SH_C1 * x;
    }
    if (D > 1) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        Y[3] = SH_C2_0 * xy;
        Y[4] = -SH_C2_0 * yz;
        Y[5] = SH_C2_2 * ((2.0f * zz - xx) - yy);
        Y[6] = -SH_C2_0 * xz;
        Y[7] = SH_C2_4 * (xx - yy);
        if (D > 2) {
            Y[8] = (-SH_C3_0 * y) * (3.0f * xx - yy);
            Y[9] = (SH_C3_1 * xy) * z;
            Y[10] = (-SH_C3_2 * y) * ((4.0f * zz - xx) - yy);
            Y[11] = (SH_C3_3 * z) * ((2.0f * zz - 3.0f * xx) - 3.0f * yy);
            Y[12] = (-SH_C3_2 * x) * ((4.0f * zz - xx) - yy);
            Y[13] = (SH_C3_5 * z) * (xx - yy);
            Y[14] = (-SH_C3_0 * x) * (xx - 3.0f * yy);
        }
    }
}

// q += v[k - 1] grad Y_k over the active coefficients (Y_0 is a constant)
template <int D>
__device__ __forceinline__ void sh_basis_adjoint(float x, float y, float z, const float *v, float &qx, float &qy, float &qz)
{
    qx = qy = qz = 0.0f;
    if (D > 0) {
        qy = -SH_C1 * v[0];
        qz = SH_C1 * v[1];
        qx = -SH_C1 * v[2];
    }
    if (D > 1) {
        const float a4 = SH_C2_0 * v[3], a5 = -SH_C2_0 * v[4], a6 = SH_C2_2 * v[5], a7 = -SH_C2_0 * v[6], a8 = SH_C2_4 * v[7];
        qx += a4 * y;          qy += a4 * x;
        qy += a5 * z;          qz += a5 * y;
        qx += a6 * (-2.0f * x); qy += a6 * (-2.0f * y); qz += a6 * (4.0f * z);
        qx += a7 * z;          qz += a7 * x;
        qx += a8 * (2.0f * x); qy += a8 * (-2.0f * y);
    }
    if (D > 2) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        const float a9 = -SH_C3_0 * v[8], a10 = SH_C3_1 * v[9], a11 = -SH_C3_2 * v[10], a12 = SH_C3_3 * v[11],
                    a13 = -SH_C3_2 * v[12], a14 = SH_C3_5 * v[13], a15 = -SH_C3_0 * v[14];
        qx += a9 * (6.0f * xy);                    qy += a9 * (3.0f * xx - 3.0f * yy);
        qx += a10 * yz;                            qy += a10 * xz;                            qz += a10 * xy;
        qx += a11 * (-2.0f * xy);                  qy += a11 * ((4.0f * zz - xx) - 3.0f * yy); qz += a11 * (8.0f * yz);
        qx += a12 * (-6.0f * xz);                  qy += a12 * (-6.0f * yz);                  qz += a12 * ((6.0f * zz - 3.0f * xx) - 3.0f * yy);
        qx += a13 * ((4.0f * zz - 3.0f * xx) - yy); qy += a13 * (-2.0f * xy);                  qz += a13 * (8.0f * xz);
        qx += a14 * (2.0f * xz);                   qy += a14 * (-2.0f * yz);                  qz += a14 * (xx - yy);
        qx += a15 * (3.0f * xx - 3.0f * yy);       qy += a15 * (-6.0f * xy);
    }
}

// LDS of both kernels: the f_rest stretch (or the grad_rest stretch on its way out) and four [SH_THREADS,3] arrays, each with
// room for the alignment shift of up to 3 words and a whole last 16-byte word
struct SHShared {
    float4 rest[(SH_THREADS * SH_MAX_ROW + 3) / 4 + 1];
    float4 a[4][(SH_THREADS * 3 + 3) / 4 + 1];
};

// The f_rest stretch of this workgroup into LDS; returns the word offset of row 0.  `row` = 3 Kr words.
template <int D>
__device__ __forceinline__ int sh_stage_rest(float *lds, const float *__restrict__ f_rest, long long g0, int rows, int row)
{
    constexpr int ACT = 3 * (sh_coeffs(D) - 1);
    if (ACT == 0) return 0;
    const float *base = f_rest + g0 * row;
    if (row == ACT) return sh_stage_in(lds, base, rows * row);
    sh_stage_rows<ACT>(lds, base, rows, row);
    return 0;
}

template <int D>
__global__ __launch_bounds__(SH_THREADS) void k_sh_colors(const float *__restrict__ f_dc, const float *__restrict__ f_rest,
                                                          const float *__restrict__ means, float cx, float cy, float cz,
                                                          long long n, int row, float *__restrict__ colors,
                                                          unsigned char *__restrict__ clamped)
{
    constexpr int K = sh_coeffs(D) - 1;
    __shared__ SHShared S;
    float *rest = reinterpret_cast<float *>(S.rest), *sm = reinterpret_cast<float *>(S.a[0]),
          *sd = reinterpret_cast<float *>(S.a[1]), *so = reinterpret_cast<float *>(S.a[2]);
    const long long g0 = (long long)blockIdx.x * SH_THREADS;
    const int rows = (int)(n - g0 < SH_THREADS ? n - g0 : SH_THREADS), t = threadIdx.x;
    const SHRows3 lm = sh_rows3_issue(means + 3 * g0, 3 * rows), ld = sh_rows3_issue(f_dc + 3 * g0, 3 * rows);
    const int s_rest = sh_stage_rest<D>(rest, f_rest, g0, rows, row);
    const int s_m = sh_rows3_commit(sm, lm, means + 3 * g0, 3 * rows), s_d = sh_rows3_commit(sd, ld, f_dc + 3 * g0, 3 * rows);
    const int s_o = sh_shift(colors + 3 * g0);
    __syncthreads();
    if (t < rows) {
        float x, y, z, r, Y[K > 0 ? K : 1];
        sh_direction(sm + s_m + 3 * t, cx, cy, cz, x, y, z, r);
        sh_basis<D>(x, y, z, Y);
        const float *sh = rest + s_rest + t * row;
        unsigned bits = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float acc = SH_C0 * sd[s_d + 3 * t + c];
#pragma unroll
            for (int k = 0; k < K; ++k) acc += Y[k] * sh[3 * k + c];
            const float pre = acc + 0.5f;
            bits |= (pre < 0.0f ? 1u : 0u) << c;
            so[s_o + 3 * t + c] = fmaxf(pre, 0.0f);
        }
        if (clamped) clamped[g0 + t] = (unsigned char)bits;
    }
    __syncthreads();
    sh_stage_out(colors + 3 * g0, so, 3 * rows);
}

// MEANS: grad_means is wanted, and only then a coefficient is read
template <int D, bool MEANS>
__global__ __launch_bounds__(SH_THREADS) void k_sh_colors_backward(const float *__restrict__ f_rest,
                                                                   const float *__restrict__ means, float cx, float cy,
                                                                   float cz, long long n, int row,
                                                                   const float *__restrict__ grad_colors,
                                                                   const unsigned char *__restrict__ clamped,
                                                                   float *__restrict__ grad_dc, float *__restrict__ grad_rest,
                                                                   float *__restrict__ grad_means)
{
    constexpr int K = sh_coeffs(D) - 1;
    __shared__ SHShared S;
    float *rest = reinterpret_cast<float *>(S.rest), *sm = reinterpret_cast<float *>(S.a[0]),
          *sg = reinterpret_cast<float *>(S.a[1]), *so_dc = reinterpret_cast<float *>(S.a[2]),
          *so_m = reinterpret_cast<float *>(S.a[3]);
    const long long g0 = (long long)blockIdx.x * SH_THREADS;
    const int rows = (int)(n - g0 < SH_THREADS ? n - g0 : SH_THREADS), t = threadIdx.x;
    const SHRows3 lm = sh_rows3_issue(means + 3 * g0, 3 * rows), lg = sh_rows3_issue(grad_colors + 3 * g0, 3 * rows);
    int s_rest = 0;
    if (MEANS) s_rest = sh_stage_rest<D>(rest, f_rest, g0, rows, row);
    const int s_m = sh_rows3_commit(sm, lm, means + 3 * g0, 3 * rows), s_g = sh_rows3_commit(sg, lg, grad_colors + 3 * g0, 3 * rows);
    __syncthreads();
    float x = 0.0f, y = 0.0f, z = 0.0f, r = 0.0f, g[3] = {0.0f, 0.0f, 0.0f}, Y[K > 0 ? K : 1];
    if (t < rows) {
        const unsigned bits = clamped[g0 + t];
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = (bits >> c) & 1u ? 0.0f : sg[s_g + 3 * t + c];
        sh_direction(sm + s_m + 3 * t, cx, cy, cz, x, y, z, r);
        sh_basis<D>(x, y, z, Y);
        if (MEANS) {
            const float *sh = rest + s_rest + t * row;
            float v[K > 0 ? K : 1], qx, qy, qz;
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = (sh[3 * k] * g[0] + sh[3 * k + 1] * g[1]) + sh[3 * k + 2] * g[2];
            sh_basis_adjoint<D>(x, y, z, v, qx, qy, qz);
            const float dq = (x * qx + y * qy) + z * qz;
            const bool ok = r > 0.0f;
            const int o = sh_shift(grad_means + 3 * g0) + 3 * t;
            so_m[o] = ok ? (qx - x * dq) / r : 0.0f;
            so_m[o + 1] = ok ? (qy - y * dq) / r : 0.0f;
            so_m[o + 2] = ok ? (qz - z * dq) / r : 0.0f;
        }
        if (grad_dc) {
            const int o = sh_shift(grad_dc + 3 * g0) + 3 * t;
#pragma unroll
            for (int c = 0; c < 3; ++c) so_dc[o + c] = SH_C0 * g[c];
        }
    }
    if (grad_rest && row > 0) {
        __syncthreads();                     // every lane has read its coefficients: the stretch now carries the gradient
        if (t < rows) {
            float *out = rest + sh_shift(grad_rest + g0 * row) + t * row;
#pragma unroll
            for (int k = 0; k < K; ++k) {
#pragma unroll
                for (int c = 0; c < 3; ++c) out[3 * k + c] = Y[k] * g[c];
            }
            for (int j = 3 * K; j < row; ++j) out[j] = 0.0f;
        }
    }
    __syncthreads();
    if (grad_rest && row > 0) sh_stage_out(grad_rest + g0 * row, rest, rows * row);
    if (grad_dc) sh_stage_out(grad_dc + 3 * g0, so_dc, 3 * rows);
    if (MEANS) sh_stage_out(grad_means + 3 * g0, so_m, 3 * rows);
}

}  // namespace

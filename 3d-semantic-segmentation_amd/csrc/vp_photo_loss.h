// vp_photo_loss.h -- the photometric loss (L1 + D-SSIM) between a rendered image and a photograph, and its gradient image
// (include/voxproj.h states the contract; tests/photo_loss_reference.py in float64).
//
// The 11 x 11 window is the product of two 11-tap rows, so both convolutions are two passes through LDS.  A workgroup of 1024
// threads owns one 32 x 32 tile of one channel:
//
//   k_photo_loss           the tile and its 5-pixel halo of x and y (42 x 42 each, zeros outside the image) are loaded once,
//                          row by row; pass 1 takes the 11 taps along a row for the five quantities x, y, x^2, y^2, x y at
//                          42 rows x 32 columns into LDS; pass 2 takes the 11 taps down a column into registers, one pixel
//                          per thread; the epilogue computes m and the three maps P, Q, R the gradient needs, and the
//                          three sums go through the tree (written out here, in planes) and the ordered sum of
//                          vp_reduce.h: slot 32 ty + tx is the tile's pixel (tx, ty), zeros outside the image; one triple
//                          per tile, tile index (c, tile row, tile).
//   k_photo_loss_gradient  the same two passes over P, Q, R; the epilogue combines them with x(p), y(p).
//
// Without a workspace there is nowhere to keep one triple per tile, so k_photo_loss<true> walks the tiles in ascending index
// in ONE workgroup and adds each tile's triple as it goes: the same sums in the same order, the same bits, at the speed of one
// compute unit.  It is the evaluation path; a call that is timed passes a workspace.
//
// The tile.  The ordered sum over the tiles is one thread's work, so the tile is as large as a workgroup gets: 32 x 32 reads
// 1.7 times its area with the halo (16 x 16: 2.6 times) and leaves a quarter as many triples to add.  LDS: ds_read_b32 /
// ds_write_b32 resolve conflicts within a 32-lane half over 32 banks, and a half is one row of 32 consecutive columns in every
// access of both passes (the halo rows are packed, stride 42; the pass-1 rows have stride 32): conflict-free without padding.
// 2 x 7056 + 26880 = 40992 bytes forward, 3 x 7056 + 16128 = 37296 backward: two workgroups of sixteen wavefronts per compute
// unit, the wavefront limit, so LDS does not bound the occupancy.
#pragma once

constexpr int PHOTO_MAX_C = 64;
constexpr int PHOTO_T = 32;                               // the tile
constexpr int PHOTO_R = 5;                                // the window's radius
constexpr int PHOTO_TAPS = 2 * PHOTO_R + 1;
constexpr int PHOTO_HALO = PHOTO_T + 2 * PHOTO_R;         // 42
constexpr int PHOTO_STRIDE = PHOTO_HALO;                  // floats between halo rows in LDS
constexpr int PHOTO_THREADS = PHOTO_T * PHOTO_T;
constexpr int PHOTO_ITEMS = PHOTO_HALO * PHOTO_T;         // pass-1 outputs per quantity: 42 rows x 32 columns
static_assert(PHOTO_THREADS == 1024 && PHOTO_T == 32, "a 32-lane half is one tile row: see the LDS note above");
static_assert(5 * PHOTO_ITEMS * sizeof(float) >= 3 * PHOTO_THREADS * sizeof(double), "the tree reuses the pass-1 rows");

// the window's row: fp32(exp(-(i - 5)^2 / 4.5)) divided by their fp32 sum (include/voxproj.h lists them)
#define PHOTO_ROW                                                                                                              \
    {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,                           \
     0x1.b43c3ep-3f,  0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f}

constexpr float PHOTO_C1 = 0.0001f, PHOTO_C2 = 0.0009f;   // fp32(0.01^2), fp32(0.03^2)

static inline long long photo_tiles_x(int W) { return (W + PHOTO_T - 1) / PHOTO_T; }
static inline long long photo_tiles(int C, int W, int H) { return (long long)C * photo_tiles_x(W) * photo_tiles_x(H); }
// three maps [3,C,H,W] | one float64 triple per tile
static inline size_t photo_maps_bytes(int C, int W, int H) { return align256((size_t)3 * C * W * H * sizeof(float)); }
static inline size_t photo_bytes(int C, int W, int H)
{
    return photo_maps_bytes(C, W, H) + align256((size_t)photo_tiles(C, W, H) * 3 * sizeof(double));
}

// 42 x 42 values round the tile at (x0, y0) of one plane, zeros outside the image; consecutive threads read along a row
__device__ __forceinline__ void photo_load_halo(const float *__restrict__ plane, int W, int H, int x0, int y0, float *s)
{
    for (int i = threadIdx.x; i < PHOTO_HALO * PHOTO_HALO; i += PHOTO_THREADS) {
        const int r = i / PHOTO_HALO, c = i - r * PHOTO_HALO;
        const int gx = x0 - PHOTO_R + c, gy = y0 - PHOTO_R + r;
        float v = 0.0f;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) v = plane[(size_t)gy * (size_t)W + (size_t)gx];
        s[r * PHOTO_STRIDE + c] = v;
    }
}

// pass 2: 11 taps down column tx from row ty of a pass-1 image, ascending
__device__ __forceinline__ float photo_down(const float *h, int tx, int ty)
{
    constexpr float g[PHOTO_TAPS] = PHOTO_ROW;
    float a = 0.0f;
#pragma unroll
    for (int k = 0; k < PHOTO_TAPS; ++k) a += g[k] * h[(ty + k) * PHOTO_T + tx];
    return a;
}

// One tile of one plane.  Every thread returns the tile's {sum |x - y|, sum (x - y)^2, sum m} in t3.
__device__ __forceinline__ void photo_tile(const float *__restrict__ xp, const float *__restrict__ yp, int W, int H, int x0,
                                           int y0, float *__restrict__ mp, float *__restrict__ Pp, float *__restrict__ Qp,
                                           float *__restrict__ Rp, float *s_x, float *s_y, float *s_h, double (&t3)[3])
{
    constexpr float g[PHOTO_TAPS] = PHOTO_ROW;
    const int tid = threadIdx.x, tx = tid & (PHOTO_T - 1), ty = tid / PHOTO_T;
    photo_load_halo(xp, W, H, x0, y0, s_x);
    photo_load_halo(yp, W, H, x0, y0, s_y);
    __syncthreads();
    for (int i = tid; i < PHOTO_ITEMS; i += PHOTO_THREADS) {
        const int r = i / PHOTO_T, c = i & (PHOTO_T - 1);
        float a1 = 0.0f, a2 = 0.0f, a11 = 0.0f, a22 = 0.0f, a12 = 0.0f;
#pragma unroll
        for (int k = 0; k < PHOTO_TAPS; ++k) {
            const float xv = s_x[r * PHOTO_STRIDE + c + k], yv = s_y[r * PHOTO_STRIDE + c + k];
            a1 += g[k] * xv;
            a2 += g[k] * yv;
            a11 += g[k] * (xv * xv);
            a22 += g[k] * (yv * yv);
            a12 += g[k] * (xv * yv);
        }
        s_h[i] = a1;
        s_h[PHOTO_ITEMS + i] = a2;
        s_h[2 * PHOTO_ITEMS + i] = a11;
        s_h[3 * PHOTO_ITEMS + i] = a22;
        s_h[4 * PHOTO_ITEMS + i] = a12;
    }
    __syncthreads();
    const float mu1 = photo_down(s_h, tx, ty), mu2 = photo_down(s_h + PHOTO_ITEMS, tx, ty);
    const float e11 = photo_down(s_h + 2 * PHOTO_ITEMS, tx, ty), e22 = photo_down(s_h + 3 * PHOTO_ITEMS, tx, ty);
    const float e12 = photo_down(s_h + 4 * PHOTO_ITEMS, tx, ty);
    const int gx = x0 + tx, gy = y0 + ty;
    float l1 = 0.0f, l2 = 0.0f, m = 0.0f;
    if (gx < W && gy < H) {
        const float x = s_x[(ty + PHOTO_R) * PHOTO_STRIDE + tx + PHOTO_R], y = s_y[(ty + PHOTO_R) * PHOTO_STRIDE + tx + PHOTO_R];
        const float d = x - y;
        l1 = fabsf(d);
        l2 = d * d;
        const float mu11 = mu1 * mu1, mu22 = mu2 * mu2, mu12 = mu1 * mu2;
        const float s1 = e11 - mu11, s2 = e22 - mu22, s12 = e12 - mu12;
        const float A1 = 2.0f * mu12 + PHOTO_C1, A2 = 2.0f * s12 + PHOTO_C2;
        const float B1 = (mu11 + mu22) + PHOTO_C1, B2 = (s1 + s2) + PHOTO_C2;
        const float D = B1 * B2;
        m = (A1 * A2) / D;
        const size_t at = (size_t)gy * (size_t)W + (size_t)gx;
        if (mp) mp[at] = m;
        if (Pp) {
            const float R = (2.0f * A1) / D;
            const float Q = -(m / B2);
            // dm/dmu1 with s1, s12 written through e11, e12:  mu2 (2 A2 / D - R) - 2 mu1 (m / B1 + Q)
            const float P = mu2 * ((2.0f * A2) / D - R) - (2.0f * mu1) * (m / B1 + Q);
            Pp[at] = P;
            Qp[at] = Q;
            Rp[at] = R;
        }
    }
    // The tree of vp_reduce.h, written out with its three values in planes: the one-workgroup evaluation path runs it once per
    // tile, and block_tree_sum's interleaved slots (24 bytes apart) measured 1.7 % slower there.
    __syncthreads();                                                   // pass 2 is over: its rows become the tree's
    double *red = (double *)s_h;
    red[tid] = (double)l1;
    red[PHOTO_THREADS + tid] = (double)l2;
    red[2 * PHOTO_THREADS + tid] = (double)m;
    __syncthreads();
    for (int h = PHOTO_THREADS / 2; h >= 1; h /= 2) {
        if (tid < h) {
            red[tid] += red[tid + h];
            red[PHOTO_THREADS + tid] += red[PHOTO_THREADS + tid + h];
            red[2 * PHOTO_THREADS + tid] += red[2 * PHOTO_THREADS + tid + h];
        }
        __syncthreads();
    }
    t3[0] = red[0];
    t3[1] = red[PHOTO_THREADS];
    t3[2] = red[2 * PHOTO_THREADS];
}

// SERIAL = false: grid (tiles of a row, tile rows, C), one tile per workgroup, the triple to block_sums[tile].
// SERIAL = true:  one workgroup, every tile in ascending index, the total to loss_stats; no maps are kept.
template <bool SERIAL>
__global__ __launch_bounds__(PHOTO_THREADS) void k_photo_loss(const float *__restrict__ image, const float *__restrict__ target,
                                                              int C, int W, int H, float *__restrict__ ssim_map,
                                                              float *__restrict__ maps, double *__restrict__ block_sums,
                                                              double *__restrict__ loss_stats)
{
    __shared__ float s_x[PHOTO_HALO * PHOTO_STRIDE], s_y[PHOTO_HALO * PHOTO_STRIDE];
    __shared__ __attribute__((aligned(16))) float s_h[5 * PHOTO_ITEMS];
    const size_t hw = (size_t)W * (size_t)H, n = hw * (size_t)C;
    const int TX = (W + PHOTO_T - 1) / PHOTO_T, TY = (H + PHOTO_T - 1) / PHOTO_T;
    double t3[3];
    if constexpr (!SERIAL) {
        const int c = blockIdx.z;
        const size_t off = (size_t)c * hw;
        photo_tile(image + off, target + off, W, H, (int)blockIdx.x * PHOTO_T, (int)blockIdx.y * PHOTO_T,
                   ssim_map ? ssim_map + off : nullptr, maps + off, maps + n + off, maps + 2 * n + off, s_x, s_y, s_h, t3);
        if (threadIdx.x == 0) {
            const size_t b = ((size_t)c * TY + blockIdx.y) * TX + blockIdx.x;
            block_sums[3 * b] = t3[0];
            block_sums[3 * b + 1] = t3[1];
            block_sums[3 * b + 2] = t3[2];
        }
    } else {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int c = 0; c < C; ++c) {
            const size_t off = (size_t)c * hw;
            for (int by = 0; by < TY; ++by)
                for (int bx = 0; bx < TX; ++bx) {
                    photo_tile(image + off, target + off, W, H, bx * PHOTO_T, by * PHOTO_T, ssim_map ? ssim_map + off : nullptr,
                               nullptr, nullptr, nullptr, s_x, s_y, s_h, t3);
                    a0 += t3[0];
                    a1 += t3[1];
                    a2 += t3[2];
                    __syncthreads();                                   // the tree's slots are read: the next tile may write
                }
        }
        if (threadIdx.x == 0) {
            loss_stats[0] = a0;
            loss_stats[1] = a1;
            loss_stats[2] = a2;
        }
    }
}

// grad_image = s (a sgn(x - y) - b ((w * P) + 2 x (w * Q) + y (w * R))),  a = (1 - lambda) / n, b = lambda / n from the host
__global__ __launch_bounds__(PHOTO_THREADS) void k_photo_loss_gradient(const float *__restrict__ image,
                                                                       const float *__restrict__ target, int W, int H,
                                                                       const float *__restrict__ maps, float a, float b,
                                                                       const float *__restrict__ grad_loss,
                                                                       float *__restrict__ grad_image)
{
    constexpr float g[PHOTO_TAPS] = PHOTO_ROW;
    __shared__ float s_p[3][PHOTO_HALO * PHOTO_STRIDE];
    __shared__ float s_h[3 * PHOTO_ITEMS];
    const int tid = threadIdx.x, tx = tid & (PHOTO_T - 1), ty = tid / PHOTO_T;
    const size_t hw = (size_t)W * (size_t)H, n = hw * (size_t)gridDim.z, off = (size_t)blockIdx.z * hw;
    const int x0 = (int)blockIdx.x * PHOTO_T, y0 = (int)blockIdx.y * PHOTO_T;
    const float s = grad_loss ? *grad_loss : 1.0f;
#pragma unroll
    for (int q = 0; q < 3; ++q) photo_load_halo(maps + (size_t)q * n + off, W, H, x0, y0, s_p[q]);
    __syncthreads();
    for (int i = tid; i < PHOTO_ITEMS; i += PHOTO_THREADS) {
        const int r = i / PHOTO_T, c = i & (PHOTO_T - 1);
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll
        for (int k = 0; k < PHOTO_TAPS; ++k) {
            a0 += g[k] * s_p[0][r * PHOTO_STRIDE + c + k];
            a1 += g[k] * s_p[1][r * PHOTO_STRIDE + c + k];
            a2 += g[k] * s_p[2][r * PHOTO_STRIDE + c + k];
        }
        s_h[i] = a0;
        s_h[PHOTO_ITEMS + i] = a1;
        s_h[2 * PHOTO_ITEMS + i] = a2;
    }
    __syncthreads();
    const int gx = x0 + tx, gy = y0 + ty;
    if (gx >= W || gy >= H) return;
    const float cP = photo_down(s_h, tx, ty), cQ = photo_down(s_h + PHOTO_ITEMS, tx, ty);
    const float cR = photo_down(s_h + 2 * PHOTO_ITEMS, tx, ty);
    const size_t at = off + (size_t)gy * (size_t)W + (size_t)gx;
    const float x = image[at], y = target[at];
    const float sg = x > y ? 1.0f : x < y ? -1.0f : 0.0f;
    const float dm = (cP + (2.0f * x) * cQ) + y * cR;
    grad_image[at] = s * (a * sg - b * dm);
}

// vp_splat.h -- tile-based Gaussian splatting of D-channel features (the reference's stage 5.2, gsplat's classic forward pass)
// with a fused argmax label / softmax-confidence epilogue.  Included by voxproj.hip only.
#pragma once

#include <type_traits>

namespace {

// ------------------------------------------------------------------------------------------------
// The contract (INTEGRATION.md "Gaussian splatting"; tests/splat_reference.py is its float64 statement):
//
// k_splat_project   one thread per Gaussian.  Depth z = ((r20 mx + r21 my) + r22 mz) + t2 in fp32 (no contraction: the
//   Makefile's -ffp-contract=off), culled when z < near or z > far.  The rest in float64 (splat_chain, which the geometry
//   backward differentiates), rounded to fp32 once at the end:
//   Sigma = M M^T with M = R(q/|q|) diag(s), Sigma_c = R_w Sigma R_w^T, the clamped EWA Jacobian, Sigma2 = J Sigma_c J^T +
//   eps2d I, conic = Sigma2^-1 (culled when det <= 0), mean2d = (fx px/z + cx, fy py/z + cy).  Float64 here keeps the fp32
//   records within one rounding of the float64 oracle's values, so the blend's decisions differ from it only within the
//   oracle's fragile band.  Opacity below 1/255, a zero quaternion or a box off the image: no tiles.  A non-finite mean /
//   quaternion / scale / opacity culls the Gaussian and adds 1 to *n_nonfinite.
//   Support box: sigma <= ln(255 o) holds inside |dx| <= sqrt(2 ln(255 o) Sigma2_00) (likewise y); the pixel range adds one
//   pixel on each side, clipped to the image, and its 16x16 tiles are the Gaussian's tiles.
// splat_sort        the tile binning of vp_tilebin.h with 64-bit keys tile << 32 | bits(z) (z > 0, so the bits order like the
//   floats): each tile's run is in (z, index) order.  A Gaussian without tiles has no key, and its record is not read.
// k_splat_blend<DT> one 256-thread workgroup per 16x16 tile, one pixel per thread, DT >= D accumulators in registers.  The
//   tile's run is staged through LDS in batches of SPLAT_BATCH(DT) Gaussians (records, then the feature rows zero-padded to
//   DT).  Per visited pair: sigma, one exp, the 1/255 and 1e-4 tests (splat_pair, the one statement of them) and DT FMAs
//   (splat_blend_batch).  A pixel stops at the first Gaussian that would take T to <= 1e-4 (that one is not added); the
//   workgroup leaves when every pixel has stopped (__syncthreads_count).  No atomics: each pixel's sum is in the sorted
//   order, so images are bit-identical run to run.  The kernel stages a batch itself (an s_id array and a barrier between
//   the records and the rows), not through the backward's splat_stage: that would change its LDS.
//   Epilogue: label = argmax over the D channels (lowest index on ties), confidence = softmax top-1 minus top-2
//   = (1 - exp(m2 - m1)) / sum_c exp(f_c - m1) (1 when D = 1), alpha = 1 - T; logits planar [D, H, W].  Only the outputs
//   whose pointer is non-NULL are written.
// k_splat_blend<DT, true> (vp_splat_rasterize_loss) is the same blend with a softmax cross-entropy epilogue: per pixel
//   l = (m + logf(sum_c expf(C_c - m))) - C_t from its accumulators (m and the sum are the confidence's), weight w (0 when
//   the target is outside [0, D)); pixel_loss = w l; {w l, w} go through the tree and the ordered sum of vp_reduce.h: slot
//   16 ty + tx of a tile is its pixel (tx, ty), zeros outside the image; one pair per tile, tiles in row-major index.  The tree
//   runs in the feature rows' LDS; the ordered sum is guarded by the device total like every kernel after the scan.
// Every kernel after the scan reads the device total first, as vp_tilebin.h states it.
// ------------------------------------------------------------------------------------------------
constexpr int SPLAT_TILE = TILE_PX;
constexpr int SPLAT_THREADS = SPLAT_TILE * SPLAT_TILE;
constexpr int SPLAT_MAX_D = 64;

__host__ __device__ constexpr int splat_batch(int DT) { return DT <= 32 ? 256 : 128; }   // LDS: 41 KiB at DT 32, 37 KiB at 64

struct SplatCam {
    float r[12];                 // world -> camera [R | t], row-major 3 x 4
    float fx, fy, cx, cy, near_z, far_z, eps2d;
    int W, H, tiles_x;
};

struct SplatRec {                // 32 bytes per Gaussian
    float mx, my, A, B;          // mean2d and the conic's first two terms
    float C, o, z;               // conic's third term, opacity, fp32 depth (the sort key)
    int pad;
};

// The float64 chain from a Gaussian and the camera to its screen-space covariance, written once: k_splat_project takes the
// record from it and k_splat_geom_chain differentiates it, so both see the same intermediates.  Rq = R(q / |q|), Rw the
// camera's rotation, p the camera-space mean, S = Sigma_c = V V^T with V = R_w R_q diag(s), u = p.xy / p.z and cu its clamp
// to the widened frustum, J the EWA Jacobian at the clamped point, JS = J S, Sigma2 = [[s00, s01], [s01, s11]] = J S J^T +
// eps2d I and its determinant.  False (nothing usable filled) for a zero quaternion.
struct SplatChain {
    double qi, w, x, y, zq;      // 1 / |q| and the unit quaternion
    double Rq[3][3], Rw[3][3], s[3], p[3], S[3][3];
    double limxp, limxn, limyp, limyn, ux, uy, cux, cuy;
    double J[2][3], JS[2][3], s00, s01, s11, det;
};

__device__ inline double splat_quat_norm2(float qw, float qx, float qy, float qz)
{
    return (double)qw * qw + (double)qx * qx + (double)qy * qy + (double)qz * qz;
}

__device__ inline void splat_chain(float mx, float my, float mz, float qw, float qx, float qy, float qz, float sx, float sy,
                                   float sz, const SplatCam &cam, SplatChain &ch)
{
    const float *r = cam.r;
    const double qi = 1.0 / sqrt(splat_quat_norm2(qw, qx, qy, qz)), w = qw * qi, x = qx * qi, y = qy * qi, zq = qz * qi;
    ch.qi = qi; ch.w = w; ch.x = x; ch.y = y; ch.zq = zq;
    const double Rq[3][3] = {{1.0 - 2.0 * (y * y + zq * zq), 2.0 * (x * y - w * zq), 2.0 * (x * zq + w * y)},
                             {2.0 * (x * y + w * zq), 1.0 - 2.0 * (x * x + zq * zq), 2.0 * (y * zq - w * x)},
                             {2.0 * (x * zq - w * y), 2.0 * (y * zq + w * x), 1.0 - 2.0 * (x * x + y * y)}};
    const double s[3] = {sx, sy, sz};
    double M[3][3], V[3][3];
    double (&Rw)[3][3] = ch.Rw, (&p)[3] = ch.p, (&S)[3][3] = ch.S, (&J)[2][3] = ch.J, (&JS)[2][3] = ch.JS;
    for (int a = 0; a < 3; ++a) {
        ch.s[a] = s[a];
        for (int c = 0; c < 3; ++c) {
            ch.Rq[a][c] = Rq[a][c];
            M[a][c] = Rq[a][c] * s[c];
            Rw[a][c] = r[4 * a + c];
        }
    }
    for (int a = 0; a < 3; ++a) p[a] = Rw[a][0] * mx + Rw[a][1] * my + Rw[a][2] * mz + (double)r[4 * a + 3];
    // V = R_w M, Sigma_c = V V^T
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) V[a][c] = Rw[a][0] * M[0][c] + Rw[a][1] * M[1][c] + Rw[a][2] * M[2][c];
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) S[a][c] = V[a][0] * V[c][0] + V[a][1] * V[c][1] + V[a][2] * V[c][2];
    const double zd = p[2], fx = cam.fx, fy = cam.fy, cx = cam.cx, cy = cam.cy;
    ch.limxp = (cam.W - cx) / fx + 0.3 * (0.5 * cam.W) / fx;
    ch.limxn = cx / fx + 0.3 * (0.5 * cam.W) / fx;
    ch.limyp = (cam.H - cy) / fy + 0.3 * (0.5 * cam.H) / fy;
    ch.limyn = cy / fy + 0.3 * (0.5 * cam.H) / fy;
    ch.ux = p[0] / zd;
    ch.uy = p[1] / zd;
    ch.cux = fmin(fmax(ch.ux, -ch.limxn), ch.limxp);
    ch.cuy = fmin(fmax(ch.uy, -ch.limyn), ch.limyp);
    const double tx = zd * ch.cux, ty = zd * ch.cuy;
    J[0][0] = fx / zd; J[0][1] = 0.0; J[0][2] = -fx * tx / (zd * zd);
    J[1][0] = 0.0; J[1][1] = fy / zd; J[1][2] = -fy * ty / (zd * zd);
    for (int a = 0; a < 2; ++a)
        for (int c = 0; c < 3; ++c) JS[a][c] = J[a][0] * S[0][c] + J[a][1] * S[1][c] + J[a][2] * S[2][c];
    ch.s00 = JS[0][0] * J[0][0] + JS[0][1] * J[0][1] + JS[0][2] * J[0][2] + cam.eps2d;
    ch.s01 = JS[0][0] * J[1][0] + JS[0][1] * J[1][1] + JS[0][2] * J[1][2];
    ch.s11 = JS[1][0] * J[1][0] + JS[1][1] * J[1][1] + JS[1][2] * J[1][2] + cam.eps2d;
    ch.det = ch.s00 * ch.s11 - ch.s01 * ch.s01;
}

__global__ __launch_bounds__(256) void k_splat_project(const float *__restrict__ means, const float *__restrict__ quats,
                                                       const float *__restrict__ scales, const float *__restrict__ opac,
                                                       long long n, SplatCam cam, SplatRec *__restrict__ rec,
                                                       int4 *__restrict__ box, int *__restrict__ count, int *n_nonfinite)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int cnt = 0;
    SplatRec g = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0};
    int4 b = make_int4(0, 0, -1, -1);
    const float mx = means[3 * i], my = means[3 * i + 1], mz = means[3 * i + 2];
    const float qw = quats[4 * i], qx = quats[4 * i + 1], qy = quats[4 * i + 2], qz = quats[4 * i + 3];
    const float sx = scales[3 * i], sy = scales[3 * i + 1], sz = scales[3 * i + 2], o = opac[i];
    const bool finite = isfinite(mx) && isfinite(my) && isfinite(mz) && isfinite(qw) && isfinite(qx) && isfinite(qy) &&
                        isfinite(qz) && isfinite(sx) && isfinite(sy) && isfinite(sz) && isfinite(o);
    if (!finite && n_nonfinite) atomicAdd(n_nonfinite, 1);
    const float *r = cam.r;
    const float z = ((r[8] * mx + r[9] * my) + r[10] * mz) + r[11];
    if (finite && z >= cam.near_z && z <= cam.far_z && splat_quat_norm2(qw, qx, qy, qz) > 0.0 && (double)o >= 1.0 / 255.0) {
        SplatChain ch;
        splat_chain(mx, my, mz, qw, qx, qy, qz, sx, sy, sz, cam, ch);
        const double s00 = ch.s00, s01 = ch.s01, s11 = ch.s11, det = ch.det;
        const double mxd = (double)cam.fx * ch.ux + (double)cam.cx, myd = (double)cam.fy * ch.uy + (double)cam.cy;
        if (det > 0.0 && isfinite(det) && isfinite(mxd) && isfinite(myd)) {
            const double ext = 2.0 * fmax(log(255.0 * (double)o), 0.0);
            const double rx = sqrt(ext * s00), ry = sqrt(ext * s11);
            // pixel j's sample is j + 0.5: |j + 0.5 - mx| <= rx, widened by one pixel each side
            const double jlo = floor(mxd - rx - 1.5), jhi = ceil(mxd + rx + 0.5);
            const double ilo = floor(myd - ry - 1.5), ihi = ceil(myd + ry + 0.5);
            if (jhi >= 0.0 && ilo <= cam.H - 1.0 && ihi >= 0.0 && jlo <= cam.W - 1.0) {
                b.x = (int)fmax(jlo, 0.0) / SPLAT_TILE;
                b.y = (int)fmax(ilo, 0.0) / SPLAT_TILE;
                b.z = (int)fmin(jhi, cam.W - 1.0) / SPLAT_TILE;
                b.w = (int)fmin(ihi, cam.H - 1.0) / SPLAT_TILE;
                cnt = (b.z - b.x + 1) * (b.w - b.y + 1);
                g.mx = (float)mxd;
                g.my = (float)myd;
                g.A = (float)(s11 / det);
                g.B = (float)(-s01 / det);
                g.C = (float)(s00 / det);
                g.o = o;
                g.z = z;
            }
        }
    }
    if (!cnt) b = make_int4(0, 0, -1, -1);
    rec[i] = g;
    box[i] = b;
    count[i] = cnt;
}

// What the loss variants of the blend kernels read and write besides the images (vp_splat_rasterize_loss,
// vp_splat_loss_backward); all NULL / 0 in the plain variants, which never look at it.
struct SplatLoss {
    const int *target;           // [H,W]; valid when 0 <= target < D
    const float *weight;         // [H,W] or NULL (1)
    float *pixel_loss;           // forward: [H,W] or NULL
    double2 *tile_sums;          // forward: {sum w l, sum w} per tile
    const double *stats;         // backward, MEAN: {sum w l, sum w}
    const float *grad_loss;      // backward: [1] or NULL (1)
    int mean;                    // backward: VP_LOSS_MEAN
};

// The loss's upstream gradient of one pixel, in place: c[] holds the pixel's D blended logits (the forward's bits) and
// becomes G[c] = sw (expf(C_c - m) / sum - [c == t]), 0 past D; sw = s w_p, 0 on an ignored pixel.  One function for the
// replay and the saved arm of the backward: the same fp32 operations, so the same bits.
template <int DT>
__device__ inline void splat_loss_grad(float (&c)[DT], int D, int t, float sw)
{
    float m = c[0];
#pragma unroll
    for (int k = 1; k < DT; ++k)
        if (k < D && c[k] > m) m = c[k];
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < DT; ++k)
        if (k < D) {
            c[k] = expf(c[k] - m);
            s += c[k];
        }
#pragma unroll
    for (int k = 0; k < DT; ++k) c[k] = k < D && sw != 0.0f ? sw * (c[k] / s - (k == t ? 1.0f : 0.0f)) : 0.0f;
}

// the scale s of the loss's gradient, read on the device: grad_loss (1 when NULL), over sum w for MEAN (0 when sum w = 0)
__device__ inline float splat_loss_scale(const SplatLoss &ls)
{
    const float g = ls.grad_loss ? *ls.grad_loss : 1.0f;
    if (!ls.mean) return g;
    const double sw = ls.stats[1];
    return sw > 0.0 ? (float)((double)g / sw) : 0.0f;
}

// One (pixel, Gaussian) pair of the blend: what every sweep over a tile's run decides, and with which values.  ga = (mx,
// my, A, B) and gb = (C, o) are the staged record, (sx, sy) the pixel's sample point, T the transmittance in front of the
// Gaussian.  A pair is skipped (it contributes nothing: false), or it would take T to <= 1e-4, so the pixel ends before it
// (true), or it is blended with weight a T and leaves Tn: then add(p) runs, and the result is false.  The forward and the
// three backward sweeps all call this, so a replayed decision is the forward's by construction.  The blended case is a
// callback, not a third result: the compiler keeps a three-valued result in a register and branches on it again in the
// hot loop.
struct SplatPair {
    float e, raw, a, Tn;         // e^-sigma, o e^-sigma, the clamped alpha, T (1 - a)
};

template <class Add>
__device__ inline bool splat_pair(const float4 ga, const float2 gb, float sx, float sy, float T, Add &&add)
{
    const float dx = ga.x - sx, dy = ga.y - sy;
    const float sigma = 0.5f * (ga.z * dx * dx + gb.x * dy * dy) + ga.w * dx * dy;
    if (sigma < 0.0f) return false;
    SplatPair p;
    p.e = __expf(-sigma);
    p.raw = gb.y * p.e;
    p.a = fminf(0.999f, p.raw);
    if (p.a < 1.0f / 255.0f) return false;
    p.Tn = T * (1.0f - p.a);
    if (p.Tn <= 1e-4f) return true;
    add(p);
    return false;
}

// The forward's accumulation over one staged batch of nb Gaussians: acc += a T f per added pair, in the batch's order.
// k_splat_blend and the loss backward's replay both blend through this function: the replayed logits are the forward's bits.
template <int DT>
__device__ inline void splat_blend_batch(const float4 *s_ga, const float2 *s_gb, const float *s_f, int nb, float sx, float sy,
                                         float (&acc)[DT], float &T, bool &done)
{
    if (done) return;
    for (int k = 0; k < nb; ++k) {
        done = splat_pair(s_ga[k], s_gb[k], sx, sy, T, [&](const SplatPair &p) {
            const float wgt = p.a * T;
            const float *f = s_f + k * DT;
#pragma unroll
            for (int c = 0; c < DT; ++c) acc[c] = fmaf(f[c], wgt, acc[c]);
            T = p.Tn;
        });
        if (done) break;
    }
}

template <int DT, bool LOSS = false>
__global__ __launch_bounds__(SPLAT_THREADS) void k_splat_blend(
    const SplatRec *__restrict__ rec, const int *__restrict__ vals, const longlong2 *__restrict__ ranges,
    const long long *total_p, long long capacity, const float *__restrict__ feats, int D, long long stride, int W, int H,
    int *__restrict__ labels, float *__restrict__ confidence, float *__restrict__ alpha_out, float *__restrict__ logits,
    SplatLoss ls)
{
    constexpr int NB = splat_batch(DT);
    __shared__ float4 s_ga[NB];              // mx, my, A, B
    __shared__ float2 s_gb[NB];              // C, o
    __shared__ int s_id[NB];
    __shared__ __attribute__((aligned(16))) float s_f[NB * DT];   // feature rows, zero past D; the loss's tile sums at the end
    static_assert(NB * DT * sizeof(float) >= 2 * SPLAT_THREADS * sizeof(double), "the tile sums reuse the feature rows' LDS");
    if (*total_p > capacity) return;
    const int tid = threadIdx.x;
    const int px = blockIdx.x * SPLAT_TILE + (tid & (SPLAT_TILE - 1)), py = blockIdx.y * SPLAT_TILE + tid / SPLAT_TILE;
    const bool inside = px < W && py < H;
    const float sx = px + 0.5f, sy = py + 0.5f;
    const longlong2 rg = ranges[(long long)blockIdx.y * gridDim.x + blockIdx.x];
    float acc[DT];
#pragma unroll
    for (int c = 0; c < DT; ++c) acc[c] = 0.0f;
    float T = 1.0f;
    bool done = !inside;
    for (long long b0 = rg.x; b0 < rg.y; b0 += NB) {
        if (__syncthreads_count(done) == SPLAT_THREADS) break;      // also keeps the LDS of the last batch until all read it
        const int nb = (int)(rg.y - b0 < NB ? rg.y - b0 : NB);
        for (int k = tid; k < nb; k += SPLAT_THREADS) {
            const int g = vals[b0 + k];
            const SplatRec r = rec[g];
            s_id[k] = g;
            s_ga[k] = make_float4(r.mx, r.my, r.A, r.B);
            s_gb[k] = make_float2(r.C, r.o);
        }
        __syncthreads();
        for (int e = tid; e < nb * DT; e += SPLAT_THREADS) {
            const int k = e / DT, c = e % DT;
            s_f[e] = c < D ? feats[(long long)s_id[k] * stride + c] : 0.0f;
        }
        __syncthreads();
        splat_blend_batch<DT>(s_ga, s_gb, s_f, nb, sx, sy, acc, T, done);
    }
    if (!LOSS && !inside) return;
    const long long pix = (long long)py * W + px, hw = (long long)H * W;
    double sums[2] = {0.0, 0.0};              // LOSS: this pixel's {w l, w}
    if (inside) {
        float m1 = acc[0];
        int lab = 0;
#pragma unroll
        for (int c = 1; c < DT; ++c)
            if (c < D && acc[c] > m1) {
                m1 = acc[c];
                lab = c;
            }
        if (!LOSS || labels) labels[pix] = lab;
        float m2 = -INFINITY, s = 0.0f;
        if (confidence || LOSS) {
#pragma unroll
            for (int c = 0; c < DT; ++c)
                if (c < D) {
                    if (c != lab && acc[c] > m2) m2 = acc[c];
                    s += expf(acc[c] - m1);
                }
        }
        if (confidence) confidence[pix] = D == 1 ? 1.0f : (1.0f - expf(m2 - m1)) / s;
        if (alpha_out) alpha_out[pix] = 1.0f - T;
        if (logits) {
#pragma unroll
            for (int c = 0; c < DT; ++c)
                if (c < D) logits[c * hw + pix] = acc[c];
        }
        if constexpr (LOSS) {
            // l = (m + logf(sum_c expf(C_c - m))) - C_t: m1 is the maximum and s the confidence's sum, channels ascending
            const int t = ls.target[pix];
            const bool valid = t >= 0 && t < D;
            const float w = valid ? (ls.weight ? ls.weight[pix] : 1.0f) : 0.0f;
            float ct = 0.0f;
#pragma unroll
            for (int c = 0; c < DT; ++c)
                if (c == t) ct = acc[c];
            const float wl = w != 0.0f ? w * ((m1 + logf(s)) - ct) : 0.0f;     // weight 0 contributes nothing, whatever l is
            if (ls.pixel_loss) ls.pixel_loss[pix] = wl;
            sums[0] = (double)wl;
            sums[1] = (double)w;
        }
    }
    if constexpr (LOSS) {
        block_tree_sum<SPLAT_THREADS>(sums, (double *)s_f);          // the blend is over: the feature rows become the tree's
        if (tid == 0) ls.tile_sums[(long long)blockIdx.y * gridDim.x + blockIdx.x] = make_double2(sums[0], sums[1]);
    }
}

// ------------------------------------------------------------------------------------------------
// The backward (vp_splat_rasterize_backward): gradients of the logits and alpha with respect to the features f and the
// activated opacities o, through the branch the forward took.  It reads what vp_splat_rasterize left in the workspace (rec,
// box, count, offs, the sorted values, the tile ranges, the device total) and writes per-(tile, Gaussian) partials of D + 1
// floats into its own scratch, at the Gaussian's emission slot for the tile:  slot = offs[g] - count[g] +
// (ty - b.y)(b.z - b.x + 1) + (tx - b.x), the position k_tile_emit gave the pair.  Every slot of [0, total) is written
// exactly once (a tile's run holds each of its pairs once): no zero fill, no second sort, no atomics.
//
// k_splat_blend_backward<DT>  one 256-thread workgroup per 16x16 tile, pixel per thread; the tile's upstream gradient G
//   [256 x DT] in registers (the thread's own pixel) and in LDS (for the product).
//   Every sweep stages a batch with splat_stage and takes each pair's decision and values from splat_pair, the function the
//   forward calls: a replayed decision is the forward's by construction.
//   Sweep 1 keeps per pixel T_final and CG = sum_k w_k (f_k . G_p) in sorted order.
//   Sweep 2 replays them again in batches of splat_bwd_batch(DT) Gaussians; per added Gaussian: w = a T, the running prefix
//   P += w (f . G_p) and the behind-sum S . G_p = CG - P (exactly 0 after the last added Gaussian, since both are the same
//   fp32 sequence; its error is a few ulp of sum_k w_k |f_k . G_p|), then
//     dL/da = T (f . G_p) - (S . G_p) / (1 - a) + G_alpha T_final / (1 - a),   Q = dL/da * (o e^-sigma < 0.999 ? e^-sigma : 0).
//   W[k][p] = w and Q[k][p] go to LDS (0 where the pixel did not add Gaussian k, and from its stop on).  Then
//   partial_f[k][c] = sum_p W[k][p] G[p][c] (thread = (channel, group of Gaussians), p ascending, 4 pixels per step) and
//   partial_o[k] = sum_p Q[k][p] (fixed segment sums, then a fixed xor tree).  Once every pixel has stopped, the rest of
//   the run gets zero partials.
// k_splat_grad_reduce<GS, GEOM>  GS = 16, 32 or 64 lanes per Gaussian, lane = channel (channel D: the opacity; GEOM: then the
//   five screen sums), grid-stride over the Gaussians: its count[g] contiguous slots summed in ascending order.  Gaussians
//   without tiles (culled) get rows of exactly 0.
// k_splat_blend_backward<DT, true> (vp_splat_rasterize_backward_geometry) is the same sweep with rows of D + 1 + 5 floats: the
//   five screen-space sums of q = dL/da o e^-sigma (0 at the clamp) follow the opacity's,
//     g_mx = -sum q (A dx + B dy), g_my = -sum q (B dx + C dy), g_A = -sum q dx^2 / 2, g_B = -sum q dx dy, g_C = -sum q dy^2 / 2.
//   They need no LDS of their own: the thread that sums a segment of Q[k][.] recomputes dx, dy of those pixels from the
//   record (the sweep's own fp32 expressions) and carries five more running sums through the same segment and xor tree.
//   The features' and the opacity's partials are computed exactly as without GEOM: bit-identical gradients.
// The LDS product was kept against a wave-shuffle reduction of the same sweep (profiles/r09_splat_backward_ab.log): the
// shuffles' butterfly costs more VALU issue at D = 32 than the product's LDS traffic.
// k_splat_blend_backward<DT, GEOM, true> (vp_splat_loss_backward) computes its upstream gradient instead of loading it:
//   G = s w (softmax(C) - onehot(target)) per pixel (splat_loss_grad), with C either read from the logits image the forward
//   wrote (saved) or blended again in a sweep 0 before sweep 1 (replay: splat_blend_batch, the forward's own accumulation,
//   with gr[] as the accumulators, so the two arms give the same bits).  s is read on the device (splat_loss_scale).  No
//   LDS is added.
// Both kernels write nothing when the device total exceeds the capacity (the reduce raises *status).
// ------------------------------------------------------------------------------------------------
// Gaussians per backward batch.  LDS: G (256 DT) + W and Q (2 NB 260) + features (NB DT) floats = 100 KiB at DT 32 and 64
__host__ __device__ constexpr int splat_bwd_batch(int DT) { return DT <= 32 ? 32 : 16; }
constexpr int SPLAT_SCREEN = 5;                    // screen-space sums per Gaussian: mean2d (x, y) and the conic (A, B, C)
constexpr int SPLAT_BWD_ROW = SPLAT_THREADS + 4;   // W / Q row stride: row k starts k 16-byte slots further round the banks

__device__ inline long long splat_slot(const long long *__restrict__ offs, const int *__restrict__ count,
                                       const int4 *__restrict__ box, int g)
{
    const int4 b = box[g];
    return offs[g] - count[g] + (long long)((int)blockIdx.y - b.y) * (b.z - b.x + 1) + ((int)blockIdx.x - b.x);
}

// Stage one batch of a tile's run for a backward sweep: the records and the feature rows (zero past D) of the nb Gaussians
// from b0 on, with SLOTS also their partial rows' slots (sweep 2 alone writes partials); then the barrier.
template <int DT, bool SLOTS>
__device__ inline void splat_stage(const SplatRec *__restrict__ rec, const int4 *__restrict__ box, const int *__restrict__ count,
                                   const long long *__restrict__ offs, const int *__restrict__ vals, long long b0, int nb,
                                   const float *__restrict__ feats, int D, long long stride, float4 *s_ga, float2 *s_gb,
                                   long long *s_slot, float *s_f)
{
    const int tid = threadIdx.x;
    for (int k = tid; k < nb; k += SPLAT_THREADS) {
        const int g = vals[b0 + k];
        const SplatRec r = rec[g];
        s_ga[k] = make_float4(r.mx, r.my, r.A, r.B);
        s_gb[k] = make_float2(r.C, r.o);
        if constexpr (SLOTS) s_slot[k] = splat_slot(offs, count, box, g);
    }
    for (int e = tid; e < nb * DT; e += SPLAT_THREADS) {
        const int k = e / DT, c = e % DT;
        s_f[e] = c < D ? feats[(long long)vals[b0 + k] * stride + c] : 0.0f;
    }
    __syncthreads();
}

// f . G_p over the DT channels, ascending: sweeps 1 and 2 form CG and its prefix P from the same sequence
template <int DT>
__device__ inline float splat_dot(const float *f, const float (&gr)[DT])
{
    float fg = 0.0f;
#pragma unroll
    for (int c = 0; c < DT; ++c) fg = fmaf(f[c], gr[c], fg);
    return fg;
}

template <int DT, bool GEOM, bool LOSS = false>
__global__ __launch_bounds__(SPLAT_THREADS) void k_splat_blend_backward(
    const SplatRec *__restrict__ rec, const int4 *__restrict__ box, const int *__restrict__ count,
    const long long *__restrict__ offs, const int *__restrict__ vals, const longlong2 *__restrict__ ranges,
    const long long *total_p, long long capacity, const float *__restrict__ feats, int D, long long stride, int W, int H,
    const float *__restrict__ grad_logits /* LOSS: the forward's logits image, NULL = replay */,
    const float *__restrict__ grad_alpha, float *__restrict__ part, SplatLoss ls)
{
    constexpr int NB = splat_bwd_batch(DT);
    constexpr int KPT = NB * DT / SPLAT_THREADS;          // Gaussians per thread in the product
    constexpr int QSEG = SPLAT_THREADS / NB;              // threads per Gaussian in the opacity sum
    static_assert(KPT >= 1 && KPT * SPLAT_THREADS == NB * DT && QSEG * NB == SPLAT_THREADS && QSEG <= 64, "batch shape");
    __shared__ float s_G[SPLAT_THREADS * DT];
    __shared__ __attribute__((aligned(16))) float s_W[NB * SPLAT_BWD_ROW];
    __shared__ float s_Q[NB * SPLAT_BWD_ROW];
    __shared__ float4 s_ga[NB];
    __shared__ float2 s_gb[NB];
    __shared__ long long s_slot[NB];
    __shared__ float s_f[NB * DT];
    if (*total_p > capacity) return;
    const int tid = threadIdx.x;
    const int px = blockIdx.x * SPLAT_TILE + (tid & (SPLAT_TILE - 1)), py = blockIdx.y * SPLAT_TILE + tid / SPLAT_TILE;
    const bool inside = px < W && py < H;
    const float sx = px + 0.5f, sy = py + 0.5f;
    const long long pix = (long long)py * W + px, hw = (long long)H * W;
    const longlong2 rg = ranges[(long long)blockIdx.y * gridDim.x + blockIdx.x];
    const int D1 = D + (GEOM ? 1 + SPLAT_SCREEN : 1);    // floats per partial row
    // the pixel's upstream gradient; LOSS: first its logits C, read back (saved) or blended again (replay)
    float gr[DT];
#pragma unroll
    for (int c = 0; c < DT; ++c) gr[c] = grad_logits && inside && c < D ? grad_logits[c * hw + pix] : 0.0f;
    if constexpr (LOSS) {
        int t = -1;
        float sw = 0.0f;
        if (inside) {
            t = ls.target[pix];
            if (t >= 0 && t < D) sw = splat_loss_scale(ls) * (ls.weight ? ls.weight[pix] : 1.0f);
        }
        if (!grad_logits) {
            // sweep 0: the forward's own accumulation (splat_blend_batch), gr[] as its accumulators
            float T = 1.0f;
            bool done = !inside;
            for (long long b0 = rg.x; b0 < rg.y; b0 += NB) {
                if (__syncthreads_count(done) == SPLAT_THREADS) break;
                const int nb = (int)(rg.y - b0 < NB ? rg.y - b0 : NB);
                splat_stage<DT, false>(rec, box, count, offs, vals, b0, nb, feats, D, stride, s_ga, s_gb, s_slot, s_f);
                splat_blend_batch<DT>(s_ga, s_gb, s_f, nb, sx, sy, gr, T, done);
            }
        }
        splat_loss_grad<DT>(gr, D, t, sw);       // G = s w (softmax(C) - onehot(target))
    }
#pragma unroll
    for (int c = 0; c < DT; ++c) s_G[tid * DT + c] = gr[c];
    const float ga_p = grad_alpha && inside ? grad_alpha[pix] : 0.0f;

    // sweep 1: T_final and CG
    float T = 1.0f, CG = 0.0f;
    bool done = !inside;
    for (long long b0 = rg.x; b0 < rg.y; b0 += NB) {
        if (__syncthreads_count(done) == SPLAT_THREADS) break;      // also keeps the last batch's LDS until all read it
        const int nb = (int)(rg.y - b0 < NB ? rg.y - b0 : NB);
        splat_stage<DT, false>(rec, box, count, offs, vals, b0, nb, feats, D, stride, s_ga, s_gb, s_slot, s_f);
        if (!done) {
            for (int k = 0; k < nb; ++k) {
                done = splat_pair(s_ga[k], s_gb[k], sx, sy, T, [&](const SplatPair &pr) {
                    CG = fmaf(pr.a * T, splat_dot<DT>(s_f + k * DT, gr), CG);
                    T = pr.Tn;
                });
                if (done) break;
            }
        }
    }
    const float T_final = T;

    // sweep 2: per-pixel weights and opacity terms into LDS, then the tile's partials
    T = 1.0f;
    float P = 0.0f;
    done = !inside;
    const int pc = tid % DT, pk0 = (tid / DT) * KPT;      // product: channel and first Gaussian of this thread
    const int qk = tid / QSEG, qs = tid % QSEG;           // opacity sum: Gaussian and segment of this thread
    for (long long b0 = rg.x; b0 < rg.y; b0 += NB) {
        if (__syncthreads_count(done) == SPLAT_THREADS) {
            for (long long i = b0 + tid; i < rg.y; i += SPLAT_THREADS) {
                const long long slot = splat_slot(offs, count, box, vals[i]);
                for (int c = 0; c < D1; ++c) part[slot * D1 + c] = 0.0f;
            }
            break;
        }
        const int nb = (int)(rg.y - b0 < NB ? rg.y - b0 : NB);
        splat_stage<DT, true>(rec, box, count, offs, vals, b0, nb, feats, D, stride, s_ga, s_gb, s_slot, s_f);
        for (int k = 0; k < NB; ++k) {
            float wk = 0.0f, qv = 0.0f;
            if (!done && k < nb)
                done = splat_pair(s_ga[k], s_gb[k], sx, sy, T, [&](const SplatPair &pr) {
                    const float fg = splat_dot<DT>(s_f + k * DT, gr);
                    wk = pr.a * T;
                    P = fmaf(wk, fg, P);
                    const float inv = 1.0f / (1.0f - pr.a);
                    const float dLda = T * fg - (CG - P) * inv + ga_p * T_final * inv;
                    qv = pr.raw < 0.999f ? dLda * pr.e : 0.0f;
                    T = pr.Tn;
                });
            s_W[k * SPLAT_BWD_ROW + tid] = wk;
            s_Q[k * SPLAT_BWD_ROW + tid] = qv;
        }
        __syncthreads();
        float acc[KPT];
#pragma unroll
        for (int j = 0; j < KPT; ++j) acc[j] = 0.0f;
        for (int p = 0; p < SPLAT_THREADS; p += 4) {
            const float g0 = s_G[p * DT + pc], g1 = s_G[(p + 1) * DT + pc], g2 = s_G[(p + 2) * DT + pc],
                        g3 = s_G[(p + 3) * DT + pc];
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                const float4 w = *(const float4 *)(s_W + (pk0 + j) * SPLAT_BWD_ROW + p);
                acc[j] = fmaf(w.x, g0, acc[j]);
                acc[j] = fmaf(w.y, g1, acc[j]);
                acc[j] = fmaf(w.z, g2, acc[j]);
                acc[j] = fmaf(w.w, g3, acc[j]);
            }
        }
        if (pc < D) {
#pragma unroll
            for (int j = 0; j < KPT; ++j)
                if (pk0 + j < nb) part[s_slot[pk0 + j] * D1 + pc] = acc[j];
        }
        // the opacity partial: Q[qk][.] summed in a fixed order, segments by pixel index, then the xor tree.  GEOM: the five
        // screen sums ride on it, Q[k][p] times a factor of the record and the pixel's offset (recomputed as splat_pair
        // computes it), through the same segments and tree
        float q = 0.0f, s5[SPLAT_SCREEN] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        float4 ga = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float2 gb = make_float2(0.0f, 0.0f);
        if constexpr (GEOM) {
            ga = s_ga[qk];
            gb = s_gb[qk];
        }
        for (int i = 0; i < NB; ++i) {
            const int p = qs * NB + i;
            const float v = s_Q[qk * SPLAT_BWD_ROW + p];
            q += v;
            if constexpr (GEOM) {
                const float dx = ga.x - ((int)blockIdx.x * SPLAT_TILE + (p & (SPLAT_TILE - 1)) + 0.5f);
                const float dy = ga.y - ((int)blockIdx.y * SPLAT_TILE + p / SPLAT_TILE + 0.5f);
                s5[0] += v * (ga.z * dx + ga.w * dy);
                s5[1] += v * (ga.w * dx + gb.x * dy);
                s5[2] += v * (0.5f * dx * dx);
                s5[3] += v * (dx * dy);
                s5[4] += v * (0.5f * dy * dy);
            }
        }
        // six butterflies step by step, not lanes_sum_down one after the other: the steps of one value wait on each other
#pragma unroll
        for (int m = QSEG / 2; m >= 1; m /= 2) {
            q += __shfl_xor(q, m);
            if constexpr (GEOM) {
#pragma unroll
                for (int j = 0; j < SPLAT_SCREEN; ++j) s5[j] += __shfl_xor(s5[j], m);
            }
        }
        if (qs == 0 && qk < nb) {
            float *row = part + s_slot[qk] * D1 + D;
            row[0] = q;
            if constexpr (GEOM) {
#pragma unroll
                for (int j = 0; j < SPLAT_SCREEN; ++j) row[1 + j] = -gb.y * s5[j];      // q = Q o, and the sums' sign
            }
        }
    }
}

// lanes per Gaussian in the reduce: the smallest of 16, 32, 64 that holds D + 1 channels (D = 64: lane c and c + 64)
inline int splat_reduce_group(int D) { return D + 1 <= 16 ? 16 : D + 1 <= 32 ? 32 : 64; }

// The kernels are instantiated for DT = 8, 16, 32, 64 accumulators (the smallest that holds D) and for reduce groups of
// 16, 32, 64 lanes (with_step, vp_common.h).

// GS lanes per Gaussian, grid-stride over the Gaussians; each lane sums its channel over the Gaussian's count[g] contiguous
// slots in ascending order, four loads in flight.  GEOM: rows of D + 1 + SPLAT_SCREEN floats, and the five screen sums of a
// Gaussian with tiles are also written back into its first slot's row, where k_splat_geom_chain reads them (the reduce has
// no per-Gaussian scratch of its own: the size function knows the capacity, not N).  Each channel of a Gaussian's rows is
// read and written by one lane only.
template <int GS, bool GEOM>
__global__ __launch_bounds__(256) void k_splat_grad_reduce(const int *__restrict__ count, const long long *__restrict__ offs,
                                                           long long n, const long long *total_p, long long capacity,
                                                           float *part, int D, float *__restrict__ grad_f,
                                                           float *__restrict__ grad_o, float *__restrict__ grad_s, int *status)
{
    if (*total_p > capacity) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && status) *status = 1;
        return;
    }
    constexpr int GPB = 256 / GS;                       // Gaussians per workgroup and round
    const int D1 = D + 1 + (GEOM ? SPLAT_SCREEN : 0), lane = threadIdx.x % GS;
    const long long step = (long long)gridDim.x * GPB;
    for (long long g = (long long)blockIdx.x * GPB + threadIdx.x / GS; g < n; g += step) {
        const long long s1 = offs[g], s0 = s1 - count[g];
        for (int c = lane; c < D1; c += GS) {
            float *p = part + c;
            float s = 0.0f;
            long long k = s0;
            for (; k + 4 <= s1; k += 4) {
                const float a0 = p[k * D1], a1 = p[(k + 1) * D1], a2 = p[(k + 2) * D1], a3 = p[(k + 3) * D1];
                s += a0;
                s += a1;
                s += a2;
                s += a3;
            }
            for (; k < s1; ++k) s += p[k * D1];
            if (c < D) {
                if (grad_f) grad_f[g * D + c] = s;
            } else if (c == D) {
                if (grad_o) grad_o[g] = s;
            } else if constexpr (GEOM) {
                if (grad_s) grad_s[g * SPLAT_SCREEN + (c - D - 1)] = s;
                if (s1 > s0) p[s0 * D1] = s;
            }
        }
    }
}

// The adjoint of k_splat_project's float64 chain, one thread per Gaussian: the five screen sums (fp32, from the first slot's
// row) to grad_means / grad_quats / grad_scales, rounded to fp32 once.  The forward's intermediates come from splat_chain, the
// function k_splat_project calls.  With X = conic, GX = [[g_A, g_B/2], [g_B/2, g_C]]:
//   G_Sigma2 = -X GX X,  G_S = J^T G_Sigma2 J,  G_J = 2 G_Sigma2 J S,  Hl = U^T G_S U with U = R_w R(n), n = q / |q|
//   (dL/dSigma in the Gaussian's own frame, where Sigma = diag(s^2)):  grad_s[c] = 2 s_c Hl_cc;  a rotation R -> R exp([d]x)
//   gives dL/dd = 2 (Hl_12 (s1^2 - s2^2), Hl_02 (s2^2 - s0^2), Hl_01 (s0^2 - s1^2)): exactly 0 between equal scales;
//   n -> n (1, d/2) turns it into grad_q = 2 E(n) dL/dd / |q|, tangent to the sphere and so orthogonal to q,
//   J02 = -fx clamp(ux) / z: the clamp passes d/dux only strictly inside its range, d/dz on both branches,
//   mean2d = f u + c with the unclamped u = p / z, grad_m = R_w^T G_p.
// The fp32 depth, the culls and the support box carry no gradient; neither does the camera.  A Gaussian without tiles, or
// whose five sums are all 0, gets rows of exactly 0.
__global__ __launch_bounds__(256) void k_splat_geom_chain(const float *__restrict__ means, const float *__restrict__ quats,
                                                          const float *__restrict__ scales, long long n, SplatCam cam,
                                                          const int *__restrict__ count, const long long *__restrict__ offs,
                                                          const long long *total_p, long long capacity,
                                                          const float *__restrict__ part, int D, float *__restrict__ grad_m,
                                                          float *__restrict__ grad_q, float *__restrict__ grad_sc)
{
    if (*total_p > capacity) return;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double gm[3] = {0.0, 0.0, 0.0}, gq[4] = {0.0, 0.0, 0.0, 0.0}, gsc[3] = {0.0, 0.0, 0.0};
    const int cnt = count[i];
    const float *row = part + (offs[i] - cnt) * (long long)(D + 1 + SPLAT_SCREEN) + D + 1;
    double g5[SPLAT_SCREEN] = {0.0, 0.0, 0.0, 0.0, 0.0};
    bool any = false;
    if (cnt > 0)
        for (int j = 0; j < SPLAT_SCREEN; ++j) {
            g5[j] = row[j];
            any |= g5[j] != 0.0;
        }
    if (any) {
        SplatChain ch;
        splat_chain(means[3 * i], means[3 * i + 1], means[3 * i + 2], quats[4 * i], quats[4 * i + 1], quats[4 * i + 2],
                    quats[4 * i + 3], scales[3 * i], scales[3 * i + 1], scales[3 * i + 2], cam, ch);
        const double qi = ch.qi, w = ch.w, x = ch.x, y = ch.y, zq = ch.zq, zd = ch.p[2], fx = cam.fx, fy = cam.fy;
        const double ux = ch.ux, uy = ch.uy, cux = ch.cux, cuy = ch.cuy, iz2 = 1.0 / (zd * zd);
        const double (&Rq)[3][3] = ch.Rq, (&Rw)[3][3] = ch.Rw, (&s)[3] = ch.s, (&J)[2][3] = ch.J, (&JS)[2][3] = ch.JS;
        const double s00 = ch.s00, s01 = ch.s01, s11 = ch.s11, det = ch.det;
        const double A = s11 / det, B = -s01 / det, C = s00 / det;
        const double gA = g5[2], hB = 0.5 * g5[3], gC = g5[4];
        const double y00 = gA * A + hB * B, y01 = gA * B + hB * C, y10 = hB * A + gC * B, y11 = hB * B + gC * C;
        const double z01 = -(A * y01 + B * y11);
        const double GZ[2][2] = {{-(A * y00 + B * y10), z01}, {z01, -(B * y01 + C * y11)}};
        double GJ[2][3], ZJ[2][3], GS[3][3], U[3][3], GU[3][3];
        for (int a = 0; a < 2; ++a)
            for (int c = 0; c < 3; ++c) {
                GJ[a][c] = 2.0 * (GZ[a][0] * JS[0][c] + GZ[a][1] * JS[1][c]);
                ZJ[a][c] = GZ[a][0] * J[0][c] + GZ[a][1] * J[1][c];
            }
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) {
                GS[a][c] = J[0][a] * ZJ[0][c] + J[1][a] * ZJ[1][c];
                U[a][c] = Rw[a][0] * Rq[0][c] + Rw[a][1] * Rq[1][c] + Rw[a][2] * Rq[2][c];
            }
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) GU[a][c] = GS[a][0] * U[0][c] + GS[a][1] * U[1][c] + GS[a][2] * U[2][c];
        // Hl = U^T G_S U, dL/dSigma in the Gaussian's own frame (symmetric: the entries used are computed once)
#define VP_HL(i, j) (U[0][i] * GU[0][j] + U[1][i] * GU[1][j] + U[2][i] * GU[2][j])
        for (int c = 0; c < 3; ++c) gsc[c] = 2.0 * s[c] * VP_HL(c, c);
        const double gd[3] = {2.0 * VP_HL(1, 2) * ((s[1] - s[2]) * (s[1] + s[2])), 2.0 * VP_HL(0, 2) * ((s[2] - s[0]) * (s[2] + s[0])),
                              2.0 * VP_HL(0, 1) * ((s[0] - s[1]) * (s[0] + s[1]))};
#undef VP_HL
        gq[0] = 2.0 * qi * (-x * gd[0] - y * gd[1] - zq * gd[2]);
        gq[1] = 2.0 * qi * (w * gd[0] - zq * gd[1] + y * gd[2]);
        gq[2] = 2.0 * qi * (zq * gd[0] + w * gd[1] - x * gd[2]);
        gq[3] = 2.0 * qi * (-y * gd[0] + x * gd[1] + w * gd[2]);
        const double g_ux = g5[0] * fx + (ux > -ch.limxn && ux < ch.limxp ? -GJ[0][2] * fx / zd : 0.0);
        const double g_uy = g5[1] * fy + (uy > -ch.limyn && uy < ch.limyp ? -GJ[1][2] * fy / zd : 0.0);
        const double g_z = (-GJ[0][0] * fx + GJ[0][2] * fx * cux - GJ[1][1] * fy + GJ[1][2] * fy * cuy) * iz2 -
                           (g_ux * ux + g_uy * uy) / zd;
        const double gp[3] = {g_ux / zd, g_uy / zd, g_z};
        for (int c = 0; c < 3; ++c) gm[c] = Rw[0][c] * gp[0] + Rw[1][c] * gp[1] + Rw[2][c] * gp[2];
    }
    if (grad_m)
        for (int c = 0; c < 3; ++c) grad_m[3 * i + c] = (float)gm[c];
    if (grad_q)
        for (int c = 0; c < 4; ++c) grad_q[4 * i + c] = (float)gq[c];
    if (grad_sc)
        for (int c = 0; c < 3; ++c) grad_sc[3 * i + c] = (float)gsc[c];
}

// bytes of the geometry backward's scratch: one partial row of D + 1 + SPLAT_SCREEN floats per intersection
inline size_t splat_geom_bytes(long long capacity, int D)
{
    return align256((size_t)(capacity > 0 ? capacity : 1) * (size_t)(D + 1 + SPLAT_SCREEN) * sizeof(float));
}

// bytes of the backward's scratch: one partial row of D + 1 floats per intersection
inline size_t splat_bwd_bytes(long long capacity, int D)
{
    return align256((size_t)(capacity > 0 ? capacity : 1) * (size_t)(D + 1) * sizeof(float));
}

// workspace of one (N, W, H, capacity): the tile bins with the records after `total`
struct SplatLayout : TileBins<unsigned long long> {
    SplatRec *rec;
};

inline bool splat_layout(char *base, long long n, int W, int H, long long capacity, SplatLayout &l)
{
    return tile_layout(base, n, W, H, capacity, l, [&](Sections &s, int at) {
        if (at == 0) s.place(l.rec, (size_t)n * sizeof(SplatRec));
    });
}

// the tile sort of the projected Gaussians: the key's low word is the record's depth
inline int splat_sort(const SplatLayout &l, long long n, long long capacity, int *status, hipStream_t stream)
{
    return tile_sort(l, &l.rec->z, (int)(sizeof(SplatRec) / sizeof(float)), n, capacity, status, stream);
}

}  // namespace

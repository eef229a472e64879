// vp_lift.h -- lifting a 2D feature map onto the Gaussians: the transpose of the splatter, as a product on the matrix cores
// (vp_splat_lift).  Included by voxproj.hip only, after vp_splat.h, whose records, sort, slots and blend step it reuses.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// sum[g, c] += sum_p m_p w_g(p) feat[p, c]   and   wsum[g] += sum_p m_p w_g(p)   over the pixels p of one view, with
// w_g(p) = a T the weight the forward blended Gaussian g into pixel p with (splat_pair: the forward's decisions and values)
// and m_p the caller's pixel weight (1 without a map).  Per 16x16 tile this is the product  W [Gaussians x 256 pixels] .
// F [256 pixels x C], which the blend backward forms with scalar FMAs for <= 64 fp32 channels; here the map stays fp16 and
// channels-last, and the product runs as v_mfma_f32_16x16x32_f16 with the pixels as the k dimension.
//
// Channels are processed in passes of CC = lift_chunk(C) (16 when C <= 16, else 64), each pass one sweep and one reduce
// launch over the same scratch: a partial row of CC floats per intersection, and one float per intersection for the weight
// (first pass only).  The weights are recomputed in every pass (one exp per pair: less than writing them out and back).
//
// k_splat_lift<CC>  one 256-thread workgroup per tile.
//   1. m_p of the thread's pixel (0 outside the image, and when not > 0), the tile's maximum and from it the power of two
//      2^e >= max m: the staged weight is (m_p 2^-e)(a T) 2^15 < 2^15, so it cannot overflow binary16 whatever the scale of
//      the map's weights, and the accumulators are scaled back by 2^(e - 15).  Powers of two: every scaling is exact.
//   2. The tile's [256 x CC] chunk of the map into LDS, transposed to [channel][pixel] binary16 (an MFMA lane reads eight
//      consecutive k of one column): 16-byte loads along the channels where C, the pixel stride and the base allow
//      (VEC), single elements otherwise.  A pixel with m_p = 0 (masked, or outside the image) and a channel past C are
//      staged as zeros whatever the map holds, so a masked NaN never reaches the product.
//   3. The tile's run in batches of LIFT_NB = 16 Gaussians through splat_stage (no feature rows: D = 0).  Thread = pixel:
//      splat_pair per Gaussian, v = (m_p 2^-e) (a T) 2^15 in fp32 split into hi = f16(v), lo = f16(v - hi): hi + lo carries
//      22 bits of v (lo is subnormal below 2^-14: its absolute error is then 2^-25, i.e. 2^-40 max m in the weight's
//      units, a relative 2^-18 of the smallest weight (1/255) 1e-4 at the tile's largest m_p).  0 where the pixel did not
//      add the Gaussian, and from its stop on.
//   4. Wavefront w forms the [16 x 16] output tiles w, w + 4, .. of the batch: eight k-steps of 32 pixels, one MFMA for hi
//      and one for lo into separate accumulators (two independent chains), summed and scaled at the end.  A operand: lane
//      l reads 16 bytes of row (Gaussian) l & 15 at pixels 32 s + 8 (l >> 4); B operand: the same bytes of channel row
//      l & 15.  Rows are LIFT_ROW = 264 halves apart (528 bytes: 16 rows start 4 banks apart, a conflict-free b128 read).
//      The accumulator has the channel on the lane (l & 15) and Gaussians 4 (l >> 4) + i in its registers: 16 lanes write
//      64 contiguous bytes of a partial row.
//   5. First pass: the weight partial sum_p (hi + lo) per Gaussian in fp32, 16 lanes per Gaussian over fixed segments of 16
//      pixels, then a fixed xor tree (as the backward sums its opacity terms).
//   Once every pixel has stopped, the rest of the run gets zero partials, as in the backward.  A tile whose pixels all
//   have m_p = 0 writes zeros for its whole run.
// k_splat_lift_reduce<CC>  CC lanes per Gaussian, lane = channel, grid-stride: the Gaussian's count[g] contiguous slots
//   summed in ascending order, then sum[g, c0 + c] += s.  A sum of exactly 0 is not added: a culled Gaussian's row, and one
//   that no pixel added, keep their bits (also a -0).  The last lane sums the weight partials in the first pass.
// No atomics anywhere: every sum has a fixed order, results are bit-identical run to run.
// Both kernels write nothing when the device total exceeds the capacity (the reduce raises *status).
// ------------------------------------------------------------------------------------------------
constexpr int LIFT_NB = 16;                        // Gaussians per batch: one MFMA row tile
constexpr int LIFT_ROW = SPLAT_THREADS + 8;        // halves per LDS row of 256 pixels
constexpr int LIFT_MAX_C = 4096;
constexpr int LIFT_SHIFT = 15;                     // the staged weight's scale 2^15

typedef _Float16 lift_h8 __attribute__((ext_vector_type(8)));
typedef float lift_f4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int lift_chunk(int C) { return C <= 16 ? 16 : 64; }

// bytes of the lift's scratch: a partial row of lift_chunk(C) floats and one weight partial per intersection
inline size_t lift_part_bytes(long long capacity, int C)
{
    return align256((size_t)(capacity > 0 ? capacity : 1) * (size_t)lift_chunk(C) * sizeof(float));
}

inline size_t lift_bytes(long long capacity, int C)
{
    return lift_part_bytes(capacity, C) + align256((size_t)(capacity > 0 ? capacity : 1) * sizeof(float));
}

template <int CC, bool VEC>
__global__ __launch_bounds__(SPLAT_THREADS) void k_splat_lift(
    const SplatRec *__restrict__ rec, const int4 *__restrict__ box, const int *__restrict__ count,
    const long long *__restrict__ offs, const int *__restrict__ vals, const longlong2 *__restrict__ ranges,
    const long long *total_p, long long capacity, const _Float16 *__restrict__ feats, int C, long long pix_stride, int c0,
    const float *__restrict__ pixel_weight, int W, int H, float *__restrict__ part,
    float *__restrict__ wpart /* the first pass's weight partials, NULL in the others */)
{
    constexpr int NB = LIFT_NB, NT = CC / 16, QSEG = SPLAT_THREADS / NB;
    static_assert(NB == 16 && QSEG == 16 && CC % 16 == 0, "batch shape");
    __shared__ __attribute__((aligned(16))) _Float16 s_F[CC * LIFT_ROW];
    __shared__ __attribute__((aligned(16))) _Float16 s_Wh[NB * LIFT_ROW];
    __shared__ __attribute__((aligned(16))) _Float16 s_Wl[NB * LIFT_ROW];
    __shared__ float s_m[SPLAT_THREADS];
    __shared__ float s_max[SPLAT_THREADS / 64];
    __shared__ float4 s_ga[NB];
    __shared__ float2 s_gb[NB];
    __shared__ long long s_slot[NB];
    __shared__ float s_f[NB];                 // splat_stage's feature rows: none here (D = 0), it writes NB zeros
    if (*total_p > capacity) return;
    const longlong2 rg = ranges[(long long)blockIdx.y * gridDim.x + blockIdx.x];
    if (rg.x >= rg.y) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 4, r = lane & 15;
    const int px = blockIdx.x * SPLAT_TILE + (tid & (SPLAT_TILE - 1)), py = blockIdx.y * SPLAT_TILE + tid / SPLAT_TILE;
    const bool inside = px < W && py < H;
    const float sx = px + 0.5f, sy = py + 0.5f;
    const int cv = C - c0 < CC ? C - c0 : CC;              // channels of this pass

    // 1. the pixel's weight, and the tile's power-of-two scale
    float m = inside ? (pixel_weight ? pixel_weight[(long long)py * W + px] : 1.0f) : 0.0f;
    if (!(m > 0.0f)) m = 0.0f;
    float mmax = lanes_max<64>(m);
    if (lane == 0) s_max[wave] = mmax;
    __syncthreads();
    mmax = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    int ex = 0;
    if (mmax > 0.0f) frexpf(mmax, &ex);                     // mmax = f 2^ex with f in [0.5, 1)
    const float msc = ldexpf(m, LIFT_SHIFT - ex), back = ldexpf(1.0f, ex - LIFT_SHIFT);
    s_m[tid] = m;
    __syncthreads();

    // 2. the map's chunk, transposed; skipped by a tile without a weighted pixel (it only writes zeros below)
    if (mmax > 0.0f) {
        const long long gx0 = (long long)blockIdx.x * SPLAT_TILE, gy0 = (long long)blockIdx.y * SPLAT_TILE;
        if constexpr (VEC) {
            constexpr int PARTS = CC / 8;
            for (int e = tid; e < SPLAT_THREADS * PARTS; e += SPLAT_THREADS) {
                const int p = e / PARTS, c = (e % PARTS) * 8;
                lift_h8 v = {};
                if (c < cv && s_m[p] != 0.0f)                 // VEC: C % 8 == 0, so the eight channels are all below C
                    v = *(const lift_h8 *)(feats + ((gy0 + p / SPLAT_TILE) * W + gx0 + (p & (SPLAT_TILE - 1))) * pix_stride +
                                           c0 + c);
#pragma unroll
                for (int j = 0; j < 8; ++j) s_F[(c + j) * LIFT_ROW + p] = v[j];
            }
        } else {
            for (int e = tid; e < SPLAT_THREADS * CC; e += SPLAT_THREADS) {
                const int p = e / CC, c = e % CC;
                _Float16 v = (_Float16)0.0f;
                if (c < cv && s_m[p] != 0.0f)
                    v = feats[((gy0 + p / SPLAT_TILE) * W + gx0 + (p & (SPLAT_TILE - 1))) * pix_stride + c0 + c];
                s_F[c * LIFT_ROW + p] = v;
            }
        }
    }

    // 3. - 5. the run in batches
    float T = 1.0f;
    bool done = m == 0.0f;
    const int qk = tid / QSEG, qs = tid % QSEG;             // weight sum: Gaussian and segment of this thread
    for (long long b0 = rg.x; b0 < rg.y; b0 += NB) {
        if (__syncthreads_count(done) == SPLAT_THREADS) {   // also orders the map's LDS writes before the first product
            for (long long i = b0 + tid; i < rg.y; i += SPLAT_THREADS) {
                const long long slot = splat_slot(offs, count, box, vals[i]);
                for (int c = 0; c < cv; ++c) part[slot * CC + c] = 0.0f;
                if (wpart) wpart[slot] = 0.0f;
            }
            break;
        }
        const int nb = (int)(rg.y - b0 < NB ? rg.y - b0 : NB);
        splat_stage<1, true>(rec, box, count, offs, vals, b0, nb, nullptr, 0, 0, s_ga, s_gb, s_slot, s_f);
        for (int k = 0; k < NB; ++k) {
            float wk = 0.0f;
            if (!done && k < nb)
                done = splat_pair(s_ga[k], s_gb[k], sx, sy, T, [&](const SplatPair &pr) {
                    wk = pr.a * T;
                    T = pr.Tn;
                });
            const float v = wk * msc;
            const _Float16 hi = (_Float16)v;
            s_Wh[k * LIFT_ROW + tid] = hi;
            s_Wl[k * LIFT_ROW + tid] = (_Float16)(v - (float)hi);
        }
        __syncthreads();
        for (int t = wave; t < NT; t += SPLAT_THREADS / 64) {
            if (t * 16 >= cv) break;
            lift_f4 acc_h = {}, acc_l = {};
            const _Float16 *wh = s_Wh + r * LIFT_ROW + 8 * h, *wl = s_Wl + r * LIFT_ROW + 8 * h;
            const _Float16 *fb = s_F + (t * 16 + r) * LIFT_ROW + 8 * h;
#pragma unroll
            for (int s = 0; s < SPLAT_THREADS / 32; ++s) {
                const lift_h8 b = *(const lift_h8 *)(fb + 32 * s);
                acc_h = __builtin_amdgcn_mfma_f32_16x16x32_f16(*(const lift_h8 *)(wh + 32 * s), b, acc_h, 0, 0, 0);
                acc_l = __builtin_amdgcn_mfma_f32_16x16x32_f16(*(const lift_h8 *)(wl + 32 * s), b, acc_l, 0, 0, 0);
            }
            const int c = t * 16 + r;
            if (c < cv) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (4 * h + i < nb) part[s_slot[4 * h + i] * CC + c] = (acc_h[i] + acc_l[i]) * back;
            }
        }
        if (wpart) {
            float q = 0.0f;
            for (int i = 0; i < NB; ++i) {
                const int p = qs * NB + i;
                q += (float)s_Wh[qk * LIFT_ROW + p] + (float)s_Wl[qk * LIFT_ROW + p];
            }
            q = lanes_sum_down<QSEG>(q);
            if (qs == 0 && qk < nb) wpart[s_slot[qk]] = q * back;
        }
    }
}

template <int CC>
__global__ __launch_bounds__(256) void k_splat_lift_reduce(const int *__restrict__ count, const long long *__restrict__ offs,
                                                           long long n, const long long *total_p, long long capacity,
                                                           const float *__restrict__ part, const float *__restrict__ wpart,
                                                           int cv, int c0, float *__restrict__ sum, long long sum_stride,
                                                           float *__restrict__ wsum, int *status)
{
    if (*total_p > capacity) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && status) *status = 1;
        return;
    }
    constexpr int GPB = 256 / CC;                       // Gaussians per workgroup and round
    const int lane = threadIdx.x % CC;
    const long long step = (long long)gridDim.x * GPB;
    for (long long g = (long long)blockIdx.x * GPB + threadIdx.x / CC; g < n; g += step) {
        const long long s1 = offs[g], s0 = s1 - count[g];
        if (lane < cv) {
            const float *p = part + lane;
            float s = 0.0f;
            long long k = s0;
            for (; k + 4 <= s1; k += 4) {
                const float a0 = p[k * CC], a1 = p[(k + 1) * CC], a2 = p[(k + 2) * CC], a3 = p[(k + 3) * CC];
                s += a0;
                s += a1;
                s += a2;
                s += a3;
            }
            for (; k < s1; ++k) s += p[k * CC];
            if (s != 0.0f) sum[g * sum_stride + c0 + lane] += s;
        }
        if (wpart && lane == CC - 1) {
            float s = 0.0f;
            for (long long k = s0; k < s1; ++k) s += wpart[k];
            if (s != 0.0f) wsum[g] += s;
        }
    }
}

}  // namespace

// vp_splat_render.h -- rendering wide per-Gaussian feature rows into a view: the splatter's forward for up to 4096 channels,
// as a product on the matrix cores (vp_splat_render).  Included by voxproj.hip only, after vp_splat.h and vp_lift.h, whose
// records, sort, blend step and staged-weight format it reuses.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// out[p, c] = sum_g w_g(p) row[g, c]  over the Gaussians g of the pixel's tile run, with w_g(p) = a T the weight the forward
// blends with (splat_pair: its decisions and values).  Per 16x16 tile this is the product  W^T [256 pixels x Gaussians] .
// F [Gaussians x C]; it runs as v_mfma_f32_16x16x32_f16 with the Gaussians as the k dimension, RENDER_NB = 32 per batch (one
// k-step).  The accumulators stay in registers for the whole run and are written once: no partial rows, no reduce launch, no
// scratch beyond the splat workspace.
//
// Channels are processed in passes of CC = 16 NT (render_chunk(C): 16 when C <= 16, else 64), one launch each; the weights
// are recomputed in every pass (one exp per pair).  A 128-channel pass (NT = 8) was built and measured: its 128 accumulator
// registers leave one wavefront per SIMD where NT = 4 has two, and at C = 512 four such passes took 3.04 ms against 2.69 ms
// for eight 64-channel passes (profiles/HISTORY.md, r19), so it is not instantiated.
//
// k_splat_render<NT, F32, VEC, OUT16>  one 256-thread workgroup per tile, thread = pixel for the weights.
//   Wavefront w owns the tile's pixel rows 4 w .. 4 w + 3 (its own threads' pixels): four M tiles of 16 pixels, times NT
//   N tiles of 16 channels: 16 NT accumulator registers.  The pixel is the A operand's row and the channel the B operand's
//   column, so the accumulator has the channel on the lane (l & 15) and pixels 4 (l >> 4) + i of its M tile in its registers:
//   16 lanes write 16 consecutive channels of one pixel.
//   Per batch:
//   1. the early exit once every pixel of the tile has stopped (the forward's);
//   2. the batch's rows, gathered by the run's sorted indices, into LDS transposed to [channel][k] binary16 (an MFMA lane
//      reads eight consecutive k of one column): 16-byte loads along the channels where C, the row stride and the base allow
//      (VEC), single elements otherwise.  A k past the batch's end and a channel past C are staged as zeros.
//      fp16 rows are the B operand as they stand.  fp32 rows (F32) are staged as hi + lo of f 2^-e_c, with 2^e_c > the
//      largest |f| of the channel's column in this batch (an integer maximum over the bit patterns in LDS: no order
//      dependence): every finite fp32 is representable, every scaling is a power of two, and a small channel beside a large
//      one keeps its own 22 bits.  The batch's product is formed in a fresh accumulator, scaled by 2^(e_c - 15) and then
//      added, so batches with different scales meet in fp32.  hi.hi + lo.hi + hi.lo: the lo.lo term is below 2^-22 of the
//      column's maximum and is dropped.
//   3. splat_stage (D = 0) for the records; thread = pixel: splat_pair per Gaussian, v = (a T) 2^15 split into
//      hi = f16(v), lo = f16(v - hi) as the lift stages it, 0 where the pixel did not add the Gaussian and from its stop on,
//      as row `pixel` of s_Wh / s_Wl (k contiguous: the A operand's 16 bytes).
//   4. the products.  Rows are RENDER_ROW = 40 halves apart (80 bytes): the 16 rows of an operand's b128 read start on
//      distinct multiples of 4 banks, and the 8 rows of a weight row's b128 write likewise.  The gather's transposing stores
//      in 2. are the expensive LDS access: eight 2-byte stores per 16-byte load, 80 bytes apart, and the lanes of one store
//      that hold the same k fall on one bank (rows eight channels apart are 160 dwords apart).  A variant that stores 32
//      different k per wavefront (k = e % 32: two to four lanes per bank, 32-byte row segments per load) measured 2.732 ms
//      against 2.694 at C = 512 (profiles/HISTORY.md, r19): the conflicts do not bound the kernel, the mapping stays.
//   At the end every pixel inside the image gets its cv channels (zeros when the run is empty: a tile without Gaussians
//   still writes), as fp32 or rounded once to binary16, and in the first pass alpha = 1 - T, the forward's chain.
// No atomics on floats, every sum has a fixed order: results are bit-identical run to run.  Nothing is written when the
// device total exceeds the capacity (*status is raised).
// ------------------------------------------------------------------------------------------------
constexpr int RENDER_NB = 32;                      // Gaussians per batch: one MFMA k-step
constexpr int RENDER_ROW = RENDER_NB + 8;          // halves per LDS row of 32 k
constexpr int RENDER_MAX_C = 4096;

__host__ __device__ constexpr int render_chunk(int C) { return C <= 16 ? 16 : 64; }

template <int NT, bool F32, bool VEC, bool OUT16>
__global__ __launch_bounds__(SPLAT_THREADS) void k_splat_render(
    const SplatRec *__restrict__ rec, const int4 *__restrict__ box, const int *__restrict__ count,
    const long long *__restrict__ offs, const int *__restrict__ vals, const longlong2 *__restrict__ ranges,
    const long long *total_p, long long capacity, const void *__restrict__ rows_, int C, long long row_stride, int c0, int W,
    int H, void *__restrict__ out_, long long pix_stride, float *__restrict__ alpha /* first pass only */, int *status)
{
    constexpr int NB = RENDER_NB, CC = 16 * NT, ROW = RENDER_ROW;
    constexpr int EPL = F32 ? 4 : 8;                                  // elements per 16-byte load
    constexpr int ITEMS = VEC ? NB * CC / EPL : NB * CC;              // loads per batch
    constexpr int PER = (ITEMS + SPLAT_THREADS - 1) / SPLAT_THREADS;  // loads per thread
    constexpr int VPL = VEC ? EPL : 1;                                // values per load
    __shared__ __attribute__((aligned(16))) _Float16 s_Fh[CC * ROW];
    __shared__ __attribute__((aligned(16))) _Float16 s_Fl[F32 ? CC * ROW : 8];
    __shared__ __attribute__((aligned(16))) _Float16 s_Wh[SPLAT_THREADS * ROW];
    __shared__ __attribute__((aligned(16))) _Float16 s_Wl[SPLAT_THREADS * ROW];
    __shared__ unsigned s_cmax[F32 ? CC : 1];   // fp32 rows: the bit pattern of the column's largest |f| in this batch
    __shared__ float4 s_ga[NB];
    __shared__ float2 s_gb[NB];
    __shared__ float s_f[NB];                   // splat_stage's feature rows: none here (D = 0), it writes NB zeros
    if (*total_p > capacity) {
        if (status && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *status = 1;
        return;
    }
    const longlong2 rg = ranges[(long long)blockIdx.y * gridDim.x + blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 4, r = lane & 15;
    const int px = blockIdx.x * SPLAT_TILE + (tid & (SPLAT_TILE - 1)), py = blockIdx.y * SPLAT_TILE + tid / SPLAT_TILE;
    const bool inside = px < W && py < H;
    const float sx = px + 0.5f, sy = py + 0.5f;
    const int cv = C - c0 < CC ? C - c0 : CC;              // channels of this pass

    lift_f4 acc[4][NT];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[m][t] = lift_f4{0.0f, 0.0f, 0.0f, 0.0f};

    float T = 1.0f;
    bool done = !inside;
    for (long long b0 = rg.x; b0 < rg.y; b0 += NB) {
        // 1. also keeps the LDS of the last batch until every wavefront has read it
        if (__syncthreads_count(done) == SPLAT_THREADS) break;
        const int nb = (int)(rg.y - b0 < NB ? rg.y - b0 : NB);

        // 2. the rows
        if constexpr (!F32) {
            const _Float16 *rows = (const _Float16 *)rows_;
#pragma unroll
            for (int it = 0; it < PER; ++it) {
                const int e = tid + it * SPLAT_THREADS;
                if (ITEMS % SPLAT_THREADS != 0 && e >= ITEMS) break;
                if constexpr (VEC) {
                    constexpr int PARTS = CC / 8;
                    const int k = e / PARTS, c = (e % PARTS) * 8;
                    lift_h8 v = {};
                    if (k < nb && c < cv)                  // VEC: C % 8 == 0, so the eight channels are all below C
                        v = *(const lift_h8 *)(rows + (long long)vals[b0 + k] * row_stride + c0 + c);
#pragma unroll
                    for (int j = 0; j < 8; ++j) s_Fh[(c + j) * ROW + k] = v[j];
                } else {
                    const int k = e / CC, c = e % CC;
                    _Float16 v = (_Float16)0.0f;
                    if (k < nb && c < cv) v = rows[(long long)vals[b0 + k] * row_stride + c0 + c];
                    s_Fh[c * ROW + k] = v;
                }
            }
            splat_stage<1, false>(rec, box, count, offs, vals, b0, nb, nullptr, 0, 0, s_ga, s_gb, nullptr, s_f);
        } else {
            const float *rows = (const float *)rows_;
            float fv[PER][VPL];
            if (tid < CC) s_cmax[tid] = 0u;
#pragma unroll
            for (int it = 0; it < PER; ++it) {
                const int e = tid + it * SPLAT_THREADS;
#pragma unroll
                for (int j = 0; j < VPL; ++j) fv[it][j] = 0.0f;
                if (ITEMS % SPLAT_THREADS != 0 && e >= ITEMS) continue;
                if constexpr (VEC) {
                    constexpr int PARTS = CC / 4;
                    const int k = e / PARTS, c = (e % PARTS) * 4;
                    if (k < nb && c < cv) {               // VEC: C % 4 == 0
                        const float4 v = *(const float4 *)(rows + (long long)vals[b0 + k] * row_stride + c0 + c);
                        fv[it][0] = v.x; fv[it][1] = v.y; fv[it][2] = v.z; fv[it][3] = v.w;
                    }
                } else {
                    const int k = e / CC, c = e % CC;
                    if (k < nb && c < cv) fv[it][0] = rows[(long long)vals[b0 + k] * row_stride + c0 + c];
                }
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < PER; ++it) {
                const int e = tid + it * SPLAT_THREADS;
                if (ITEMS % SPLAT_THREADS != 0 && e >= ITEMS) continue;
                const int c = VEC ? (e % (CC / 4)) * 4 : e % CC;
#pragma unroll
                for (int j = 0; j < VPL; ++j) {
                    const unsigned u = __float_as_uint(fv[it][j]) & 0x7fffffffu;
                    if (u) atomicMax(&s_cmax[c + j], u);
                }
            }
            splat_stage<1, false>(rec, box, count, offs, vals, b0, nb, nullptr, 0, 0, s_ga, s_gb, nullptr, s_f);
#pragma unroll
            for (int it = 0; it < PER; ++it) {
                const int e = tid + it * SPLAT_THREADS;
                if (ITEMS % SPLAT_THREADS != 0 && e >= ITEMS) continue;
                const int k = VEC ? e / (CC / 4) : e / CC, c = VEC ? (e % (CC / 4)) * 4 : e % CC;
#pragma unroll
                for (int j = 0; j < VPL; ++j) {
                    int ex = 0;
                    frexpf(__uint_as_float(s_cmax[c + j]), &ex);       // max = f 2^ex with f in [0.5, 1); 0 gives ex = 0
                    const float v = ldexpf(fv[it][j], -ex);
                    const _Float16 hi = (_Float16)v;
                    s_Fh[(c + j) * ROW + k] = hi;
                    s_Fl[(c + j) * ROW + k] = (_Float16)(v - (float)hi);
                }
            }
        }

        // 3. the weights of this thread's pixel
#pragma unroll 1
        for (int k8 = 0; k8 < NB; k8 += 8) {
            lift_h8 vh, vl;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k8 + j;
                float wk = 0.0f;
                if (!done && k < nb)
                    done = splat_pair(s_ga[k], s_gb[k], sx, sy, T, [&](const SplatPair &pr) {
                        wk = pr.a * T;
                        T = pr.Tn;
                    });
                const float v = ldexpf(wk, LIFT_SHIFT);
                const _Float16 hi = (_Float16)v;
                vh[j] = hi;
                vl[j] = (_Float16)(v - (float)hi);
            }
            *(lift_h8 *)(s_Wh + tid * ROW + k8) = vh;
            *(lift_h8 *)(s_Wl + tid * ROW + k8) = vl;
        }
        __syncthreads();

        // 4. the products
        lift_h8 ah[4], al[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int row = wave * 64 + m * 16 + r;
            ah[m] = *(const lift_h8 *)(s_Wh + row * ROW + 8 * h);
            al[m] = *(const lift_h8 *)(s_Wl + row * ROW + 8 * h);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t * 16 >= cv) break;
            const lift_h8 bh = *(const lift_h8 *)(s_Fh + (t * 16 + r) * ROW + 8 * h);
            if constexpr (!F32) {
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[m], bh, acc[m][t], 0, 0, 0);
                    acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[m], bh, acc[m][t], 0, 0, 0);
                }
            } else {
                const lift_h8 bl = *(const lift_h8 *)(s_Fl + (t * 16 + r) * ROW + 8 * h);
                int ex = 0;
                frexpf(__uint_as_float(s_cmax[t * 16 + r]), &ex);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    lift_f4 d = {0.0f, 0.0f, 0.0f, 0.0f};
                    d = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[m], bh, d, 0, 0, 0);
                    d = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[m], bl, d, 0, 0, 0);
                    d = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[m], bh, d, 0, 0, 0);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[m][t][i] += ldexpf(d[i], ex - LIFT_SHIFT);
                }
            }
        }
    }

    // every pixel of the image is written, also by a tile whose run is empty
    if (alpha && inside) alpha[(long long)py * W + px] = 1.0f - T;
    const float back = F32 ? 1.0f : 1.0f / (float)(1 << LIFT_SHIFT);   // fp32 rows: every batch was scaled back as it was added
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const long long oy = (long long)blockIdx.y * SPLAT_TILE + wave * 4 + m;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long ox = (long long)blockIdx.x * SPLAT_TILE + 4 * h + i;
            if (oy >= H || ox >= W) continue;
            const long long o = (oy * W + ox) * pix_stride + c0 + r;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (t * 16 + r >= cv) break;
                const float v = acc[m][t][i] * back;
                if constexpr (OUT16)
                    ((_Float16 *)out_)[o + t * 16] = (_Float16)v;
                else
                    ((float *)out_)[o + t * 16] = v;
            }
        }
    }
}

}  // namespace

// vp_render.h -- the projector's transpose: copy, for every pixel, the row of the voxel its ray hits first
// (k_render_walk / k_render_small).  Included by voxproj.hip only.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// dst[p, :] = rows[ids[p], :] for 0 < ids[p] < n_rows, zeros otherwise.
//
// The forward call adds the feature row of pixel p into row ids[p]; its adjoint reads row ids[p] back into pixel p.  ID 0 is
// a miss (row 0 receives no pixel in the forward, so zeros -- not rows[0] -- is the exact adjoint); an ID outside [0, n_rows)
// is never read: the pixel gets zeros and adds 1 to the optional bad_ids counter.  The bounds test precedes every load.
//
// The pixels are one flat stream: dst rows of consecutive pixels are contiguous whatever the image shape.  One wavefront owns
// a tile of 64 consecutive pixels; each lane loads one ID (one 256-byte load per tile).
//
// k_render_walk: the wavefront walks its 64 pixels with the ID made wave-uniform (readlane), so a row's address is scalar and
//   its C channels are moved by the 64 lanes together, VEC floats per lane per slot, K slots = 64*VEC*K channels per pass
//   (VEC = 4: dwordx4 per lane; 8: two dwordx4 loads -> one 16-byte store of 8 halves; 1: one dword, any C / alignment).  A
//   pixel whose ID repeats the previous pixel's takes the registers already loaded -- runs of one voxel along an image row
//   are tens of pixels on close-ups, so the kernel reads about one row per run and becomes a write stream.  The walk goes
//   UNR pixels at a time: the rows of up to UNR new IDs are requested before any of them is stored.
// k_render_small: C < 64, any alignment: the tile's 64*C contiguous dst elements are dealt to the lanes in order,
//   the pixel of an element found by a 32-bit division, its ID by a lane permute (full lanes for RGB-sized rows).
//
// dst is written with non-temporal stores: nothing reads it back soon, and keeping it out of the caches leaves them to the rows
// (R2, 60 views, fp32: 13.8 -> 12.0 ms; fp16 7.64 -> 7.00 ms; the trajectory legs, one row per long run, unchanged; 8 pixels per
// walk step instead of 4: within 1 %, fp16 5 %, not adopted -- profiles/r07_render_ab.log).
// Rounding to float16 is round-to-nearest-even (v_cvt_f16_f32 = __float2half_rn = torch's .half()); fp32 rows are copied
// bit for bit (NaN payloads, -0.0 and denormals included: no arithmetic touches them).
// ------------------------------------------------------------------------------------------------
#ifndef VP_RENDER_UNR
#define VP_RENDER_UNR 4
#endif
constexpr int RENDER_UNR = VP_RENDER_UNR;

// dst stores: non-temporal (default) or plain (-DVP_RENDER_PLAIN_STORES, the A/B arm)
template <typename T> __device__ __forceinline__ void render_st(T *p, T v)
{
#ifdef VP_RENDER_PLAIN_STORES
    *p = v;
#else
    __builtin_nontemporal_store(v, p);
#endif
}

template <typename T> __device__ __forceinline__ T render_cvt(float v);
template <> __device__ __forceinline__ float render_cvt<float>(float v) { return v; }
template <> __device__ __forceinline__ _Float16 render_cvt<_Float16>(float v) { return (_Float16)v; }

// IDs of the tile at `base` (pixels past the end read as 0 and are never stored) and the tile's out-of-range IDs counted
__device__ __forceinline__ int render_tile_ids(const int *__restrict__ ids, long long base, long long n_pixels, long long n_rows,
                                               int *bad_ids, int lane, int &np)
{
    const long long left = n_pixels - base;
    np = left < 64 ? (int)left : 64;
    int id = lane < np ? ids[base + lane] : 0;
    const bool bad = id < 0 || (long long)id >= n_rows;
    const unsigned long long m = __ballot(bad);
    if (m != 0ull) {
        if (bad_ids && lane == 0) atomicAdd(bad_ids, __popcll(m));
        if (bad) id = 0;            // from here on an out-of-range ID is a miss: zeros, no load
    }
    return id;
}

template <int VEC, int K, typename TO>
__global__ __launch_bounds__(256) void k_render_walk(const int *__restrict__ ids, long long n_pixels, const float *__restrict__ rows,
                                                     long long n_rows, int C, TO *__restrict__ dst, int *bad_ids)
{
    static_assert(VEC == 1 || VEC == 4 || VEC == 8, "lane width");
    static_assert(VEC != 8 || sizeof(TO) == 2, "8 channels per lane: float16 destination");
    using LD = typename std::conditional<VEC == 1, float, float4>::type;   // what one load moves
    constexpr int NL = VEC == 8 ? 2 : 1;                                   // loads per slot
    constexpr int LW = VEC == 1 ? 1 : 4;                                   // floats per load
    const int lane = threadIdx.x & 63;
    const long long n_tiles = (n_pixels + 63) / 64;
    for (long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); tile < n_tiles; tile += (long long)gridDim.x * 4) {
        const long long base = tile * 64;
        int np;
        const int idv = render_tile_ids(ids, base, n_pixels, n_rows, bad_ids, lane, np);
        for (int cb = 0; cb < C; cb += 64 * VEC * K) {
            LD cur[K][NL];               // registers of the previous pixel's row
            int prev = 0;
#pragma unroll
            for (int k = 0; k < K; k++)
#pragma unroll
                for (int h = 0; h < NL; h++) cur[k][h] = LD{};
            for (int j0 = 0; j0 < np; j0 += RENDER_UNR) {
                int id[RENDER_UNR];
                LD r[RENDER_UNR][K][NL];
                // the rows of the new IDs among the next UNR pixels, all requested before the first store
#pragma unroll
                for (int u = 0; u < RENDER_UNR; u++) {
                    id[u] = j0 + u < np ? __builtin_amdgcn_readlane(idv, j0 + u) : 0;     // wave-uniform
                    const int before = u == 0 ? prev : id[u - 1];
                    if (id[u] != 0 && id[u] != before) {
                        const float *src = rows + (long long)id[u] * C + cb;
#pragma unroll
                        for (int k = 0; k < K; k++) {
                            const int ch = (k * 64 + lane) * VEC;
#pragma unroll
                            for (int h = 0; h < NL; h++)
                                r[u][k][h] = cb + ch < C ? *reinterpret_cast<const LD *>(src + ch + h * LW) : LD{};
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < RENDER_UNR; u++) {
                    if (j0 + u >= np) break;
                    const int before = u == 0 ? prev : id[u - 1];
#pragma unroll
                    for (int k = 0; k < K; k++)
#pragma unroll
                        for (int h = 0; h < NL; h++) {
                            if (id[u] == 0) cur[k][h] = LD{};
                            else if (id[u] != before) cur[k][h] = r[u][k][h];
                        }
                    prev = id[u];
                    TO *out = dst + (base + j0 + u) * C + cb;
#pragma unroll
                    for (int k = 0; k < K; k++) {
                        const int ch = (k * 64 + lane) * VEC;
                        if (cb + ch >= C) continue;
                        if constexpr (VEC == 1) {
                            render_st(out + ch, render_cvt<TO>(cur[k][0]));
                        } else if constexpr (VEC == 4) {
                            static_assert(VEC != 4 || sizeof(TO) == 4, "4 channels per lane: float32 destination");
                            typedef float v4f __attribute__((ext_vector_type(4)));
                            const float4 a = cur[k][0];
                            const v4f v = {a.x, a.y, a.z, a.w};
                            render_st(reinterpret_cast<v4f *>(out + ch), v);
                        } else {
                            typedef _Float16 v8h __attribute__((ext_vector_type(8)));
                            const float4 a = cur[k][0], b = cur[k][1];
                            const v8h v = {(_Float16)a.x, (_Float16)a.y, (_Float16)a.z, (_Float16)a.w,
                                           (_Float16)b.x, (_Float16)b.y, (_Float16)b.z, (_Float16)b.w};
                            render_st(reinterpret_cast<v8h *>(out + ch), v);
                        }
                    }
                }
            }
        }
    }
}

template <typename TO>
__global__ __launch_bounds__(256) void k_render_small(const int *__restrict__ ids, long long n_pixels, const float *__restrict__ rows,
                                                      long long n_rows, int C, TO *__restrict__ dst, int *bad_ids)
{
    const int lane = threadIdx.x & 63;
    const long long n_tiles = (n_pixels + 63) / 64;
    for (long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); tile < n_tiles; tile += (long long)gridDim.x * 4) {
        const long long base = tile * 64;
        int np;
        const int idv = render_tile_ids(ids, base, n_pixels, n_rows, bad_ids, lane, np);
        const unsigned n_el = (unsigned)np * (unsigned)C;        // < 64 * 64
        TO *out = dst + base * C;
        for (unsigned e = lane; e < (n_el + 63) / 64 * 64; e += 64) {
            const unsigned j = e / (unsigned)C, c = e - j * (unsigned)C;
            const int id = __shfl(idv, (int)(j & 63));           // every lane takes part in the permute
            if (e < n_el) render_st(out + e, render_cvt<TO>(id != 0 ? rows[(long long)id * C + c] : 0.0f));
        }
    }
}

}  // namespace

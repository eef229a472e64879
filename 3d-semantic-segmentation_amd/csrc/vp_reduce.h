// vp_reduce.h -- the fixed-order sums every loss family ends in, and the lane butterflies.  Device code; included by
// voxproj.hip only, before the family headers.
//
// The two-step float64 sum.  A statistic is a sum over elements (pixels, samples); float64 addition is not associative, so
// the order is part of the contract (include/voxproj.h states it per call), and it is written here once:
//   step 1  block_tree_sum: a workgroup's threads hold one slot each (a thread without an element holds zeros); the slots are
//           added by a halving tree, slot t += slot t + h for h = THREADS / 2, .., 1.  One partial per workgroup.
//   step 2  k_ordered_sum: the partials are added one by one in ascending index, by thread 0 of one workgroup.
// What a slot is, and which element a thread holds, is the family's business.  No atomics: the same bits on every run.
#pragma once

namespace {

// Butterflies over a group of G consecutive lanes, G a power of two up to 64: every lane of the group ends with the same bits
// (a + b = b + a in every step).  The order of the masks is part of a float sum's bits, so the sum names it: _up takes the
// masks 1, 2, .., G / 2, _down takes G / 2, .., 1.  A maximum is the same in any order.  G is a template argument where the
// caller knows it, an argument where it is a run-time value (the neighbour KL's lanes per row).
template <int G, typename T> __device__ __forceinline__ T lanes_sum_up(T v)
{
#pragma unroll
    for (int m = 1; m < G; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

template <int G, typename T> __device__ __forceinline__ T lanes_sum_down(T v)
{
#pragma unroll
    for (int m = G / 2; m >= 1; m /= 2) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ float lanes_sum_down(float v, int G)
{
    for (int m = G >> 1; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

template <int G> __device__ __forceinline__ float lanes_max(float v)
{
#pragma unroll
    for (int m = G / 2; m >= 1; m /= 2) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}

__device__ __forceinline__ float lanes_max(float v, int G)
{
    for (int m = G >> 1; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}

// Step 1.  Every thread of the workgroup calls it with its NV values and gets the NV totals back.  red holds NV * THREADS
// doubles of the caller's LDS, slot t in red[NV t .. NV t + NV - 1].  The barrier before the first write lets the caller pass
// LDS it was reading a moment ago, and call again on the same buffer.  A workgroup larger than THREADS may call it: the
// threads from THREADS on take part in the barriers only, their values are not read.
template <int THREADS, int NV> __device__ __forceinline__ void block_tree_sum(double (&v)[NV], double *red)
{
    static_assert(THREADS >= 64 && (THREADS & (THREADS - 1)) == 0, "a halving tree");
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < THREADS) {
#pragma unroll
        for (int j = 0; j < NV; ++j) red[NV * tid + j] = v[j];
    }
    __syncthreads();
    for (int h = THREADS / 2; h >= 1; h /= 2) {
        if (tid < h) {
#pragma unroll
            for (int j = 0; j < NV; ++j) red[NV * tid + j] += red[NV * (tid + h) + j];
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = red[j];
}

template <int THREADS> __device__ __forceinline__ double block_tree_sum(double v, double *red)
{
    double a[1] = {v};
    block_tree_sum<THREADS, 1>(a, red);
    return a[0];
}

// Step 2.  out[j] = partials[j] + partials[NV + j] + partials[2 NV + j] + .., left to right, for j < NV.  One workgroup of
// STAGE threads: they stage STAGE partials at a time in LDS, thread 0 adds them in order (unrolled: the LDS reads run ahead of
// the dependent additions).  guard, when not NULL: a value above guard_max writes nothing (the splatter's device total
// against its capacity).
template <int NV, int STAGE>
__global__ __launch_bounds__(STAGE) void k_ordered_sum(const double *__restrict__ partials, long long n, const long long *guard,
                                                       long long guard_max, double *__restrict__ out)
{
    __shared__ double s_part[NV * STAGE];
    if (guard && *guard > guard_max) return;
    const int tid = threadIdx.x;
    double a[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) a[j] = 0.0;
    for (long long b0 = 0; b0 < n; b0 += STAGE) {
        const int nb = (int)(n - b0 < STAGE ? n - b0 : STAGE);
        __syncthreads();
        for (int i = tid; i < NV * nb; i += STAGE) s_part[i] = partials[NV * b0 + i];
        __syncthreads();
        if (tid == 0)
#pragma unroll 8
            for (int k = 0; k < nb; ++k) {
#pragma unroll
                for (int j = 0; j < NV; ++j) a[j] += s_part[NV * k + j];
            }
    }
    if (tid == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) out[j] = a[j];
    }
}

}  // namespace

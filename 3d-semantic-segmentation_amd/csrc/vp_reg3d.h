// vp_reg3d.h -- the 3D neighbourhood regulariser: the KL divergence between a row's class distribution and those of its
// nearest neighbours in space (vp_neighbor_kl), and its gradient with respect to the logits (vp_neighbor_kl_gradient).
// include/voxproj.h states the contract, tests/reg3d_reference.py states it in float64.  Included by voxproj.hip only.
//
// k counts the point itself, as in the reference's loss_cls_3d (its cdist against the full set returns the point first, at
// distance 0, with a KL term of exactly 0): the neighbour table holds the k - 1 others, the mean divides by k.
//
// Lane layout.  P runs from a handful (prompts) to 256 (codes).  A row is served by a group of G consecutive lanes, G a power
// of two in [4, 64], lane l of the group holding channels l, l + G, ... (CPL of them at most, a template parameter: 1, 2 or
// 4); a wavefront serves 64 / G rows, a workgroup 256 / G.  Measured on the MI355X at 1 000 000 rows, k = 5, every layout the
// lanes switch allows (profiles/r23_reg3d_lanes.jsonl): the kernels are gather-bound and the narrowest group wins or ties at
// every P -- forward plus gradient at P = 40: 1.14 / 1.44 / 1.86 ms with 16 / 32 / 64 lanes, at P = 3: 0.35 ms with 4 lanes
// against 1.81 with 64 -- except that at P = 13 and 16 eight lanes with two channels beat four with four by 4 - 6 %.  So
// kl_pick_lanes takes the smallest power of two G with 4 G >= P, and 8 where P is in 9..16; the variants it can pick are
// (G, CPL) = (4,1) P <= 4, (4,2) P <= 8, (8,2) P <= 16, (8,4) P <= 32, (16,4) P <= 64, (32,4) P <= 128, (64,4) P <= 256 (CPL 4
// also serves three channels per lane).  Sums over a row's channels: per lane in ascending channel order, then a butterfly
// over the group, masks descending from G / 2 (lanes_sum_down, vp_reduce.h).
//
//   k_kl_lse       row_lse[i] = max + logf(sum expf(z - max)) for every row.
//   k_kl_forward   a group per sample position: p_s = expf(z_s - lse_s) and logf(p_s + eps) stay in registers, the k - 1
//                  neighbour rows are gathered one after the other; sample_loss[s] = sum_j sum_c p_sc (log(p_sc + eps) -
//                  log(p_jc + eps)), unscaled.
//   k_kl_sum1/2    the per-sample sums in float64: 256 workgroups over consecutive stretches of ceil(S / 256) samples (slot t:
//                  the stretch's samples t, t + 256, .. added in ascending order; the tree of vp_reduce.h), then the 256
//                  partial sums in ascending order.  No atomics: the same bits on every run.
//   k_kl_gradient  a group per ROW: the row gathers what it receives as a sample (its own neighbours, through the sample list
//                  of the row) and as a neighbour (through the reversed table, CSR over rows), in that fixed order, then
//                  goes through the softmax: dz = p (g - <g, p>).  Every row of grad_logits is written, zeros included.
//                  A row with a long reversed list keeps only its own group busy; the loop over the list is unrolled by four
//                  so that four gathered rows are in flight.
// Every index read from a table is checked against its range before it is used as an address.
#pragma once

namespace {

constexpr int KL_THREADS = 256;
constexpr int KL_MAX_P = VP_NEIGHBOR_KL_MAX_P;
constexpr int KL_MAX_K = VP_NEIGHBOR_KL_MAX_K;
constexpr int KL_PARTS = 256;
constexpr float KL_EPS = 1e-10f;

static inline int kl_pick_lanes(int P)
{
    int G = 4;
    while (4 * G < P && G < 64) G *= 2;
    return (P > 8 && G < 8) ? 8 : G;
}

template <int CPL>
__global__ __launch_bounds__(KL_THREADS) void k_kl_lse(const float *__restrict__ z, long long stride, long long N, int P, int G,
                                                       float *__restrict__ row_lse)
{
    const long long row = ((long long)blockIdx.x * KL_THREADS + threadIdx.x) / G;
    const int l = threadIdx.x & (G - 1);
    const bool active = row < N;
    float v[CPL], m = -INFINITY;
#pragma unroll
    for (int u = 0; u < CPL; ++u) {
        const int c = l + u * G;
        v[u] = (active && c < P) ? z[row * stride + c] : -INFINITY;
        m = fmaxf(m, v[u]);
    }
    m = lanes_max(m, G);
    float s = 0.0f;
#pragma unroll
    for (int u = 0; u < CPL; ++u)
        if (active && l + u * G < P) s += expf(v[u] - m);
    s = lanes_sum_down(s, G);
    if (active && l == 0) row_lse[row] = m + logf(s);
}

template <int CPL>
__global__ __launch_bounds__(KL_THREADS) void k_kl_forward(const float *__restrict__ z, long long stride, long long N, int P,
                                                           int G, const int *__restrict__ samples, long long S,
                                                           const int *__restrict__ nbr, int km1,
                                                           const float *__restrict__ row_lse, float *__restrict__ sl)
{
    const long long sp = ((long long)blockIdx.x * KL_THREADS + threadIdx.x) / G;
    const int l = threadIdx.x & (G - 1);
    long long row = sp < S ? (samples ? (long long)samples[sp] : sp) : -1;
    const bool active = row >= 0 && row < N;
    float ps[CPL], lps[CPL], acc = 0.0f;
    if (active) {
        const float lse = row_lse[row];
#pragma unroll
        for (int u = 0; u < CPL; ++u) {
            const int c = l + u * G;
            ps[u] = c < P ? expf(z[row * stride + c] - lse) : 0.0f;
            lps[u] = logf(ps[u] + KL_EPS);
        }
#pragma unroll 2
        for (int j = 0; j < km1; ++j) {
            const long long nb = nbr[sp * km1 + j];
            if (nb < 0 || nb >= N) continue;
            const float lj = row_lse[nb];
#pragma unroll
            for (int u = 0; u < CPL; ++u) {
                const int c = l + u * G;
                if (c < P) {
                    const float pj = expf(z[nb * stride + c] - lj);
                    acc += ps[u] * (lps[u] - logf(pj + KL_EPS));
                }
            }
        }
    }
    acc = lanes_sum_down(acc, G);
    if (sp < S && l == 0) sl[sp] = acc;
}

__global__ __launch_bounds__(KL_THREADS) void k_kl_sum1(const float *__restrict__ sl, long long S, double *__restrict__ part)
{
    __shared__ double red[KL_THREADS];
    const long long per = (S + KL_PARTS - 1) / KL_PARTS, lo = min(S, blockIdx.x * per), hi = min(S, lo + per);
    double s = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += KL_THREADS) s += (double)sl[i];
    s = block_tree_sum<KL_THREADS>(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ void k_kl_sum2(const double *__restrict__ part, long long S, double *__restrict__ stats)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int b = 0; b < KL_PARTS; ++b) s += part[b];
    stats[0] = s;
    stats[1] = (double)S;
}

template <int CPL>
__global__ __launch_bounds__(KL_THREADS) void k_kl_gradient(const float *__restrict__ z, long long stride, long long N, int P,
                                                            int G, const int *__restrict__ samples, long long S,
                                                            const int *__restrict__ nbr, int km1,
                                                            const float *__restrict__ row_lse, const int *__restrict__ rev_start,
                                                            const int *__restrict__ rev_entry, const int *__restrict__ smp_start,
                                                            const int *__restrict__ smp_entry, double coef64,
                                                            const float *__restrict__ grad_loss, float *__restrict__ grad,
                                                            long long gstride)
{
    const long long row = ((long long)blockIdx.x * KL_THREADS + threadIdx.x) / G;
    const int l = threadIdx.x & (G - 1);
    const bool active = row < N;
    float p[CPL], a[CPL], lp[CPL], r[CPL], g[CPL];
#pragma unroll
    for (int u = 0; u < CPL; ++u) p[u] = a[u] = lp[u] = r[u] = g[u] = 0.0f;
    if (active) {
        const float lse = row_lse[row];
#pragma unroll
        for (int u = 0; u < CPL; ++u) {
            const int c = l + u * G;
            p[u] = c < P ? expf(z[row * stride + c] - lse) : 0.0f;
            a[u] = p[u] + KL_EPS;
            lp[u] = logf(a[u]);
            r[u] = p[u] / a[u];
        }
        // as a sample: the positions of the sample list that name this row, ascending
        const long long tb = samples ? smp_start[row] : row, te = samples ? smp_start[row + 1] : min(row + 1, S);
        for (long long t = tb; t < te; ++t) {
            const long long sp = samples ? (long long)smp_entry[t] : t;
            if (sp < 0 || sp >= S) continue;
#pragma unroll 2
            for (int j = 0; j < km1; ++j) {
                const long long nb = nbr[sp * km1 + j];
                if (nb < 0 || nb >= N) continue;
                const float lj = row_lse[nb];
#pragma unroll
                for (int u = 0; u < CPL; ++u) {
                    const int c = l + u * G;
                    if (c < P) {
                        const float pj = expf(z[nb * stride + c] - lj);
                        g[u] += (lp[u] - logf(pj + KL_EPS)) + r[u];
                    }
                }
            }
        }
        // as a neighbour: the entries of the table that name this row, ascending
        const long long eb = rev_start[row], ee = rev_start[row + 1];
#pragma unroll 4
        for (long long t = eb; t < ee; ++t) {
            const long long e = rev_entry[t];
            if (e < 0 || e >= S * km1) continue;
            const long long sp = e / km1;
            const long long srow = samples ? (long long)samples[sp] : sp;
            if (srow < 0 || srow >= N) continue;
            const float ls = row_lse[srow];
#pragma unroll
            for (int u = 0; u < CPL; ++u) {
                const int c = l + u * G;
                if (c < P) {
                    const float psv = expf(z[srow * stride + c] - ls);
                    g[u] -= psv / a[u];
                }
            }
        }
    }
    float dot = 0.0f;
#pragma unroll
    for (int u = 0; u < CPL; ++u) dot += g[u] * p[u];
    dot = lanes_sum_down(dot, G);
    if (!active) return;
    float coef = (float)coef64;
    if (grad_loss) coef *= grad_loss[0];
#pragma unroll
    for (int u = 0; u < CPL; ++u) {
        const int c = l + u * G;
        if (c < P) grad[row * gstride + c] = coef * (p[u] * (g[u] - dot));
    }
}

// channels per lane of a group of G lanes; the kernels are instantiated for 1, 2 and 4
static inline int kl_cpl(int P, int G) { return (P + G - 1) / G; }

}  // namespace

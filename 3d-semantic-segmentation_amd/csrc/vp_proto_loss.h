// vp_proto_loss.h -- the prototype-contrastive loss of a rendered identity image against a per-view instance mask, and its
// gradient image (include/voxproj.h states the contract; tests/proto_loss_reference.py in float64).
//
// The image is planar [D,n]: a thread owns a pixel, its D channels are D coalesced loads, and the normalised row s lives in
// registers (DP = 16, 32 or 64 of them, channels at or beyond D read as zeros).  Everything per id lives on chip.  A sum
// over pixels is taken without float atomics: a workgroup walks its tiles of 256 pixels (tile = b, b + G, ...), compacts the
// tile's samples in ascending pixel order into LDS, and every accumulator has ONE owner thread that adds the samples in that
// order; the workgroups' partial sums are then added in one fixed shape by a combine kernel.
//
//   k_proto_sums     read 1: r, s; S[id][c] += m s_c (owner of (id mod 16, c mod 16) scans the tile), n[id] += m (integer
//                    atomics in LDS), sum (r - 1)^2 over every pixel in float64.
//   k_proto_means    n_k, u_k = S_k / n_k, the norm statistic (the workgroups' sums in a fixed shape: 16 chunks of 48, see below).
//   k_proto_spread   read 2 (samples of active ids only): d = m |s - u_id|; thread t owns id t and scans the tile.
//   k_proto_temps    phi_k, the active list (ascending id), the table u_k / phi_k by slot, K and sum n.
//   k_proto_loss     read 3 (samples only): z_k = s . u_k / phi_k with the table read through uniform addresses, l, own_prob;
//                    then T[k][c] += sum_p (m q_pk) s_pc as a 16 x 16 block per step: 256 threads, one output each, over the
//                    compacted samples of the tile held in two [256][17] LDS tiles (q recomputed per block of 16 slots).
//   k_proto_protos   g_k / n_k = T_k / phi_k / n_k by slot, the loss statistic.
//   k_proto_gradient one read, one write: sum_k q_k u'_k + g_c / n_c in one loop over the table (the own id's 1 - P taken as
//                    (sum of the others + 1e-6) / den), the norm term, every element written.
#pragma once

constexpr int PROTO_MAX_D = 64;
constexpr int PROTO_IDS = VP_PROTO_MAX_IDS;
constexpr int PROTO_THREADS = 256;        // = pixels per tile = ids
constexpr int PROTO_GRID = 768;           // workgroups of the three reads, at most (a constant: the order of a sum is fixed)
constexpr int PROTO_CHUNKS = 16;          // a combine adds 16 chunks of 48 workgroups side by side, then the chunks in order
constexpr int PROTO_CHUNK = PROTO_GRID / PROTO_CHUNKS;
constexpr int PROTO_COMBINE = 64 * PROTO_CHUNKS;   // threads of a combine kernel
constexpr int PROTO_PAD = 17;             // row stride of the two sample tiles: 16 values, conflict-free writes
static_assert(PROTO_IDS == PROTO_THREADS, "thread t owns id t");
static_assert(PROTO_CHUNK * PROTO_CHUNKS == PROTO_GRID && PROTO_COMBINE == 1024, "16 chunks of 48 workgroups");

struct ProtoHeader {
    int K;                                // active ids
    int pad[63];
};
static_assert(sizeof(ProtoHeader) == 256, "the header is 256 bytes");

struct ProtoWs {
    ProtoHeader *hdr;
    unsigned long long *n_id;             // [256] by id: sum of m over the id's samples
    int *slot_of_id;                      // [256] by id: its slot in the active list, -1 when not active
    float *inv_phi;                       // [256] by slot
    float *n_slot;                        // [256] by slot
    float *u_id;                          // [256][D] by id
    float *utab;                          // [256][D] by slot: u_k / phi_k
    float *gn;                            // [256][D] by slot: g_k / n_k
    double *norm_part, *loss_part;        // [G]
    unsigned long long *cnt_part;         // [G][256]
    float *a_part;                        // [G][256]
    float *s_part;                        // [G][256][D]: S partials, then T partials
    size_t bytes;
};

__host__ __device__ static inline long long proto_tiles(long long n) { return (n + PROTO_THREADS - 1) / PROTO_THREADS; }
static inline int proto_grid(long long n) { return (int)std::min<long long>(proto_tiles(n), PROTO_GRID); }

static inline ProtoWs proto_carve(void *workspace, int D, long long n)
{
    const size_t G = (size_t)proto_grid(n);
    char *p = (char *)workspace;
    size_t off = 0;
    auto take = [&](size_t bytes) { char *q = p + off; off += align256(bytes); return q; };
    ProtoWs w;
    w.hdr = (ProtoHeader *)take(sizeof(ProtoHeader));
    w.n_id = (unsigned long long *)take(PROTO_IDS * sizeof(unsigned long long));
    w.slot_of_id = (int *)take(PROTO_IDS * sizeof(int));
    w.inv_phi = (float *)take(PROTO_IDS * sizeof(float));
    w.n_slot = (float *)take(PROTO_IDS * sizeof(float));
    w.u_id = (float *)take((size_t)PROTO_IDS * D * sizeof(float));
    w.utab = (float *)take((size_t)PROTO_IDS * D * sizeof(float));
    w.gn = (float *)take((size_t)PROTO_IDS * D * sizeof(float));
    w.norm_part = (double *)take(G * sizeof(double));
    w.loss_part = (double *)take(G * sizeof(double));
    w.cnt_part = (unsigned long long *)take(G * PROTO_IDS * sizeof(unsigned long long));
    w.a_part = (float *)take(G * PROTO_IDS * sizeof(float));
    w.s_part = (float *)take(G * PROTO_IDS * D * sizeof(float));
    w.bytes = off;
    return w;
}

// is pixel p drawn, with an id that can be a sample's?  m = its multiplicity
__device__ __forceinline__ bool proto_sample(const int *__restrict__ ids, const int *__restrict__ count, long long p,
                                             int ignore_id, int &id, float &m, int *cnt = nullptr)
{
    const int c = count ? count[p] : 1;
    id = ids[p];
    m = (float)c;
    if (cnt) *cnt = c;
    return c > 0 && id >= 0 && id < PROTO_IDS && id != ignore_id;
}

// s = f / (r + 1e-6) in registers, channels at or beyond D as zeros; returns r
template <int DP>
__device__ __forceinline__ float proto_load(const float *__restrict__ image, long long n, long long p, int D, float (&s)[DP])
{
    float ss = 0.0f;
#pragma unroll
    for (int c = 0; c < DP; ++c) {
        s[c] = c < D ? image[(size_t)c * (size_t)n + (size_t)p] : 0.0f;
        ss += s[c] * s[c];
    }
    const float r = sqrtf(ss), den = r + 1e-6f;
#pragma unroll
    for (int c = 0; c < DP; ++c) s[c] = s[c] / den;
    return r;
}

// z = s . row, row at a uniform address
template <int DP> __device__ __forceinline__ float proto_dot(const float (&s)[DP], const float *__restrict__ row, int D)
{
    float z = 0.0f;
#pragma unroll
    for (int c = 0; c < DP; ++c)
        if (c < D) z += s[c] * row[c];
    return z;
}

// The tile's samples in ascending pixel order: the sample's slot, nv = how many.  Two barriers: woff may be written again at once.
template <int WAVES = PROTO_THREADS / 64> __device__ __forceinline__ int proto_compact(bool valid, int *woff, int &nv)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long b = __ballot(valid);
    if (lane == 0) woff[w] = __popcll(b);
    __syncthreads();
    int off = 0;
    nv = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
        const int ci = woff[i];
        if (i < w) off += ci;
        nv += ci;
    }
    __syncthreads();
    return off + __popcll(b & ((1ull << lane) - 1ull));
}

template <int DP>
__global__ __launch_bounds__(PROTO_THREADS) void k_proto_sums(const float *__restrict__ image, int D, long long n,
                                                              const int *__restrict__ ids, const int *__restrict__ count,
                                                              int ignore_id, float *__restrict__ s_part,
                                                              unsigned long long *__restrict__ cnt_part,
                                                              double *__restrict__ norm_part)
{
    extern __shared__ float proto_acc[];                              // [256][D]
    __shared__ unsigned long long s_cnt[PROTO_IDS];
    __shared__ float s_tile[PROTO_THREADS * PROTO_PAD];
    __shared__ int s_id[PROTO_THREADS];
    __shared__ int s_woff[PROTO_THREADS / 64];
    __shared__ double s_red[PROTO_THREADS];
    const int tid = threadIdx.x, cl = tid & 15, j = tid >> 4;
    for (int i = tid; i < PROTO_IDS * D; i += PROTO_THREADS) proto_acc[i] = 0.0f;
    s_cnt[tid] = 0ull;
    __syncthreads();
    double nrm = 0.0;
    const long long tiles = proto_tiles(n);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long p = tile * PROTO_THREADS + tid;
        float s[DP];
        int id = -1, cnt = 0;
        float m = 0.0f;
        bool valid = false;
        if (p < n) {
            const float r = proto_load<DP>(image, n, p, D, s);
            const float e = r - 1.0f;
            nrm += (double)(e * e);
            valid = proto_sample(ids, count, p, ignore_id, id, m, &cnt);
        }
        int nv;
        const int slot = proto_compact(valid, s_woff, nv);
        if (nv == 0) continue;
        if (valid) {
            s_id[slot] = id;
            atomicAdd(&s_cnt[id], (unsigned long long)cnt);
        }
#pragma unroll
        for (int cc = 0; cc < DP / 16; ++cc) {
            if (cc * 16 < D) {                                        // uniform
                if (valid) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) s_tile[slot * PROTO_PAD + e] = m * s[cc * 16 + e];
                }
                __syncthreads();
                const int c = cc * 16 + cl;
                if (c < D)
                    for (int q = 0; q < nv; ++q) {
                        const int k = s_id[q];
                        if ((k & 15) == j) proto_acc[k * D + c] += s_tile[q * PROTO_PAD + cl];
                    }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    const size_t b = blockIdx.x;
    cnt_part[b * PROTO_IDS + tid] = s_cnt[tid];
    for (int i = tid; i < PROTO_IDS * D; i += PROTO_THREADS)
        s_part[b * PROTO_IDS * D + i] = proto_acc[i];
    const double tot = block_tree_sum<PROTO_THREADS>(nrm, s_red);
    if (tid == 0) norm_part[b] = tot;
}

// The fixed shape of every combine over the G <= 768 workgroups: chunk j = 0 .. 15 adds workgroups 48 j .. 48 j + 47 in
// ascending order (16 chunks side by side, their loads independent of each other), then the 16 chunk sums are added in
// ascending j.  The shape does not depend on G: a workgroup at or beyond G adds nothing.

// row [G][256][D] of slot / id k: thread (j = tid / 64, c = tid % 64); the sum is in the threads with j = 0
__device__ __forceinline__ float proto_row_sum(const float *__restrict__ part, int k, int D, int G, float *red)
{
    const int tid = threadIdx.x, c = tid & 63, j = tid >> 6;
    float a = 0.0f;
    if (c < D) {
        const int b0 = j * PROTO_CHUNK, b1 = min(b0 + PROTO_CHUNK, G);
#pragma unroll 8
        for (int b = b0; b < b1; ++b) a += part[((size_t)b * PROTO_IDS + k) * D + c];
    }
    red[tid] = a;
    __syncthreads();
    float t = 0.0f;
    if (j == 0)
        for (int i = 0; i < PROTO_CHUNKS; ++i) t += red[i * 64 + c];
    __syncthreads();
    return t;
}

// one float64 per workgroup: the tree of vp_reduce.h over 1024 slots (slot b = workgroup b, zeros beyond G)
__device__ __forceinline__ double proto_part_sum(const double *__restrict__ part, int G, double *red)
{
    const int tid = threadIdx.x;
    return block_tree_sum<PROTO_COMBINE>(tid < G ? part[tid] : 0.0, red);
}
static_assert(PROTO_GRID <= PROTO_COMBINE, "one slot per workgroup");

// one workgroup per id: S and n in the combine's shape, u = S / n; block 0 also adds the norm partials
__global__ __launch_bounds__(PROTO_COMBINE) void k_proto_means(int D, int G, const float *__restrict__ s_part,
                                                               const unsigned long long *__restrict__ cnt_part,
                                                               const double *__restrict__ norm_part,
                                                               unsigned long long *__restrict__ n_id, float *__restrict__ u_id,
                                                               double *__restrict__ stats)
{
    __shared__ double s_red[PROTO_COMBINE];
    __shared__ unsigned long long s_n;
    const int k = blockIdx.x, tid = threadIdx.x, c = tid & 63;
    if (tid == 0) s_n = 0ull;
    __syncthreads();
    if (tid < G) {                                                    // integers: any order
        const unsigned long long cb = cnt_part[(size_t)tid * PROTO_IDS + k];
        if (cb) atomicAdd(&s_n, cb);
    }
    const float S = proto_row_sum(s_part, k, D, G, (float *)s_red);   // its barriers publish s_n as well
    const unsigned long long nk = s_n;
    if (tid < 64 && c < D) u_id[k * D + c] = nk ? S / (float)nk : 0.0f;
    if (tid == 0) n_id[k] = nk;
    if (k == 0) {
        const double t = proto_part_sum(norm_part, G, s_red);
        if (tid == 0) stats[2] = t;
    }
}

template <int DP>
__global__ __launch_bounds__(PROTO_THREADS) void k_proto_spread(const float *__restrict__ image, int D, long long n,
                                                                const int *__restrict__ ids, const int *__restrict__ count,
                                                                int ignore_id, int min_count,
                                                                const unsigned long long *__restrict__ n_id,
                                                                const float *__restrict__ u_id, float *__restrict__ a_part)
{
    __shared__ float s_d[PROTO_THREADS];
    __shared__ int s_id[PROTO_THREADS];
    __shared__ int s_woff[PROTO_THREADS / 64];
    const int tid = threadIdx.x;
    float a = 0.0f;
    const long long tiles = proto_tiles(n);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long p = tile * PROTO_THREADS + tid;
        int id = -1;
        float m = 0.0f, d = 0.0f;
        bool valid = false;
        if (p < n) valid = proto_sample(ids, count, p, ignore_id, id, m) && n_id[id] > (unsigned long long)min_count;
        if (valid) {
            float s[DP];
            proto_load<DP>(image, n, p, D, s);
            const float *u = u_id + id * D;
            float dd = 0.0f;
#pragma unroll
            for (int c = 0; c < DP; ++c)
                if (c < D) {
                    const float t = s[c] - u[c];
                    dd += t * t;
                }
            d = m * sqrtf(dd);
        }
        int nv;
        const int slot = proto_compact(valid, s_woff, nv);
        if (nv == 0) continue;
        if (valid) {
            s_id[slot] = id;
            s_d[slot] = d;
        }
        __syncthreads();
        for (int q = 0; q < nv; ++q)
            if (s_id[q] == tid) a += s_d[q];
        __syncthreads();
    }
    a_part[(size_t)blockIdx.x * PROTO_IDS + tid] = a;
}

// one workgroup: thread (j = tid / 256, id t = tid % 256) adds a quarter of the workgroups' spreads of id t, four of the 16
// chunks in ascending order; then threads 0 .. 255, one per id: the temperature, the active list in ascending id, the table
// u / phi by slot, K and sum n
__global__ __launch_bounds__(PROTO_COMBINE) void k_proto_temps(int D, int G, int min_count, float phi_scale, float phi_min,
                                                               float phi_max, const float *__restrict__ a_part,
                                                               const unsigned long long *__restrict__ n_id,
                                                               const float *__restrict__ u_id, ProtoHeader *__restrict__ hdr,
                                                               int *__restrict__ slot_of_id, float *__restrict__ inv_phi,
                                                               float *__restrict__ n_slot, float *__restrict__ utab,
                                                               double *__restrict__ stats)
{
    __shared__ int s_woff[PROTO_COMBINE / 64];
    __shared__ double s_red[PROTO_THREADS];
    __shared__ float s_a[PROTO_COMBINE];
    const int tid = threadIdx.x, t = tid & (PROTO_IDS - 1), q = tid / PROTO_IDS;
    const unsigned long long nk = n_id[t];
    const bool active = tid < PROTO_IDS && nk > (unsigned long long)min_count;
    {
        float a = 0.0f;
        const int b0 = q * (PROTO_GRID / 4), b1 = min(b0 + PROTO_GRID / 4, G);
#pragma unroll 8
        for (int b = b0; b < b1; ++b) a += a_part[(size_t)b * PROTO_IDS + t];
        s_a[tid] = a;
    }
    __syncthreads();
    const float A = ((s_a[t] + s_a[PROTO_IDS + t]) + s_a[2 * PROTO_IDS + t]) + s_a[3 * PROTO_IDS + t];
    int K;
    const int slot = proto_compact<PROTO_COMBINE / 64>(active, s_woff, K);
    if (tid < PROTO_IDS) slot_of_id[tid] = active ? slot : -1;
    if (active) {
        const float nf = (float)nk;
        float phi = phi_scale * A / (nf * logf(nf + 10.0f));
        phi = fminf(fmaxf(phi, phi_min), phi_max);
        inv_phi[slot] = 1.0f / phi;
        n_slot[slot] = nf;
        for (int c = 0; c < D; ++c) utab[slot * D + c] = u_id[tid * D + c] / phi;
    }
    const double tot = block_tree_sum<PROTO_THREADS>(active ? (double)nk : 0.0, s_red);  // integers below 2^53: exact
    if (tid == 0) {
        hdr->K = K;
        stats[1] = (double)K;
        stats[3] = tot;
    }
}

template <int DP>
__global__ __launch_bounds__(PROTO_THREADS) void k_proto_loss(const float *__restrict__ image, int D, long long n,
                                                              const int *__restrict__ ids, const int *__restrict__ count,
                                                              const ProtoHeader *__restrict__ hdr,
                                                              const int *__restrict__ slot_of_id, const float *__restrict__ utab,
                                                              float *__restrict__ pixel_loss, float *__restrict__ own_prob,
                                                              float *__restrict__ t_part, double *__restrict__ loss_part)
{
    extern __shared__ float proto_acc[];                              // T [K][D]
    __shared__ float s_tile[PROTO_THREADS * PROTO_PAD];               // s, 16 channels of every sample
    __shared__ float s_q[PROTO_THREADS * PROTO_PAD];                  // m q, 16 slots of every sample
    __shared__ int s_woff[PROTO_THREADS / 64];
    __shared__ double s_red[PROTO_THREADS];
    const int tid = threadIdx.x, cl = tid & 15, kl = tid >> 4;
    const int K = hdr->K;
    for (int i = tid; i < K * D; i += PROTO_THREADS) proto_acc[i] = 0.0f;
    __syncthreads();
    double lsum = 0.0;
    const long long tiles = proto_tiles(n);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long p = tile * PROTO_THREADS + tid;
        float s[DP];
        int id = -1, own = -1;
        float m = 0.0f, den = 1.0f, rest = 0.0f, ml = 0.0f, prob = 0.0f;
        bool valid = false;
        if (p < n) {
            valid = proto_sample(ids, count, p, -1, id, m);
            if (valid) {
                own = slot_of_id[id];                                 // -1 for the ignored id and for an id that is not active
                valid = own >= 0;
            }
        }
        if (valid) {
            proto_load<DP>(image, n, p, D, s);
            float zown = 0.0f, others = 0.0f;                         // others: the other ids' e^z, kept apart for q below
            for (int k = 0; k < K; ++k) {
                const float z = proto_dot<DP>(s, utab + k * D, D);
                if (k == own) zown = z;
                else others += expf(z);
            }
            rest = others + 1e-6f;
            den = (others + expf(zown)) + 1e-6f;
            ml = m * (logf(den) - zown);
            prob = expf(zown) / den;
            lsum += (double)ml;
        }
        if (p < n) {
            if (pixel_loss) pixel_loss[p] = ml;
            if (own_prob) own_prob[p] = prob;
        }
        int nv;
        const int slot = proto_compact(valid, s_woff, nv);
        if (nv == 0) continue;
#pragma unroll
        for (int cc = 0; cc < DP / 16; ++cc) {
            if (cc * 16 < D) {                                        // uniform
                if (valid) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) s_tile[slot * PROTO_PAD + e] = s[cc * 16 + e];
                }
                for (int kc = 0; kc < K; kc += 16) {
                    if (valid)
                        for (int e = 0; e < 16; ++e) {
                            const int k = kc + e;
                            float q = 0.0f;
                            // q = P - [k = c]; for the own id 1 - P = rest / den has no cancellation where P is close to 1
                            if (k < K) q = m * (k == own ? -(rest / den) : expf(proto_dot<DP>(s, utab + k * D, D)) / den);
                            s_q[slot * PROTO_PAD + e] = q;
                        }
                    __syncthreads();
                    const int k = kc + kl, c = cc * 16 + cl;
                    if (k < K && c < D) {
                        float a = 0.0f;
                        for (int q = 0; q < nv; ++q) a += s_q[q * PROTO_PAD + kl] * s_tile[q * PROTO_PAD + cl];
                        proto_acc[k * D + c] += a;
                    }
                    __syncthreads();
                }
            }
        }
    }
    __syncthreads();
    const size_t b = blockIdx.x;
    for (int i = tid; i < K * D; i += PROTO_THREADS) t_part[b * PROTO_IDS * D + i] = proto_acc[i];
    const double tot = block_tree_sum<PROTO_THREADS>(lsum, s_red);
    if (tid == 0) loss_part[b] = tot;
}

// one workgroup per slot: T in the combine's shape, g_k / n_k; block 0 also adds the loss partials
__global__ __launch_bounds__(PROTO_COMBINE) void k_proto_protos(int D, int G, const ProtoHeader *__restrict__ hdr,
                                                                const float *__restrict__ t_part,
                                                                const double *__restrict__ loss_part,
                                                                const float *__restrict__ inv_phi, const float *__restrict__ n_slot,
                                                                float *__restrict__ gn, double *__restrict__ stats)
{
    __shared__ double s_red[PROTO_COMBINE];
    const int k = blockIdx.x, tid = threadIdx.x, c = tid & 63;
    if (k == 0) {
        const double t = proto_part_sum(loss_part, G, s_red);
        if (tid == 0) stats[0] = t;
        __syncthreads();
    }
    if (k >= hdr->K) return;                                          // uniform
    const float T = proto_row_sum(t_part, k, D, G, (float *)s_red);
    if (tid < 64 && c < D) gn[k * D + c] = T * inv_phi[k] / n_slot[k];
}

template <int DP>
__global__ __launch_bounds__(PROTO_THREADS) void k_proto_gradient(const float *__restrict__ image, int D, long long n,
                                                                  const int *__restrict__ ids, const int *__restrict__ count,
                                                                  const ProtoHeader *__restrict__ hdr,
                                                                  const int *__restrict__ slot_of_id,
                                                                  const float *__restrict__ utab, const float *__restrict__ gn,
                                                                  float weight_contrast, float weight_norm,
                                                                  const float *__restrict__ grad_loss, float *__restrict__ grad)
{
    const long long p = (long long)blockIdx.x * PROTO_THREADS + threadIdx.x;
    if (p >= n) return;
    const int K = hdr->K;
    const float gl = grad_loss ? *grad_loss : 1.0f;
    const float wc = K > 0 ? weight_contrast / (float)K : 0.0f;
    const float wn = weight_norm / (float)n;
    float s[DP], a[DP];
    const float r = proto_load<DP>(image, n, p, D, s);
#pragma unroll
    for (int c = 0; c < DP; ++c) a[c] = 0.0f;
    int id, own = -1;
    float m;
    if (K > 0 && proto_sample(ids, count, p, -1, id, m)) own = slot_of_id[id];
    if (own >= 0) {
        // sum_k q_k u'_k = (sum_{k != c} e_k u'_k - (sum_{k != c} e_k + 1e-6) u'_c) / den: the own id's 1 - P without cancellation
        float others = 0.0f, eown = 0.0f;
        for (int k = 0; k < K; ++k) {
            const float *row = utab + k * D;
            const float e = expf(proto_dot<DP>(s, row, D));
            if (k == own) {
                eown = e;
                continue;
            }
            others += e;
#pragma unroll
            for (int c = 0; c < DP; ++c)
                if (c < D) a[c] += e * row[c];
        }
        const float rest = others + 1e-6f, den = (others + eown) + 1e-6f;
        const float *urow = utab + own * D, *grow = gn + own * D;
        const float wm = wc * m;
#pragma unroll
        for (int c = 0; c < DP; ++c)
            if (c < D) a[c] = wm * ((a[c] - rest * urow[c]) / den + grow[c]);
    }
    const float rd = r + 1e-6f;
    const float nt = r > 0.0f ? wn * (2.0f * (r - 1.0f) / r) : 0.0f;
#pragma unroll
    for (int c = 0; c < DP; ++c)
        if (c < D) {
            const size_t at = (size_t)c * (size_t)n + (size_t)p;
            grad[at] = gl * (a[c] / rd + nt * image[at]);
        }
}


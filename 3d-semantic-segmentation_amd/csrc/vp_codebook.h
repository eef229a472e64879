// vp_codebook.h -- a code book of global instance labels against a rendered identity image and one view's instance mask:
// the id-by-code score matrix of the linear assignment (k_codebook_assoc, k_codebook_score) and the cross-entropy /
// clustering loss with its two code-book gradients (k_codebook_loss, k_codebook_finish).  include/voxproj.h states the
// contract, tests/codebook_reference.py states it in float64.  Included by voxproj.hip only.
//
// A workgroup is four wavefronts and walks tiles of 64 consecutive pixels, 16 per wavefront.  The code book lives in LDS
// (Kpad x DP floats, K and D rounded up to 16, the padding zeros, channel index XOR-swizzled by the code so that the 16 codes
// of a B operand fall on distinct banks).  Logits: 16 pixels x D x 16 codes is one accumulator tile of
// v_mfma_f32_16x16x4_f32, D / 4 steps, 16 code tiles: lane (r = lane & 15, h = lane >> 4) feeds pixel r, channel 4 s + h as
// A and code 16 t + r, channel 4 s + h as B, and receives code 16 t + r of pixels 4 h + i in register i of tile t -- the
// layout of k_query.  A pixel's whole softmax therefore stays in 64 registers: the maximum and the sum are 16 values on the
// lane, then a butterfly over the 16 lanes of the group (commutative steps: every lane of the group ends with the same bits).
// Codes at or beyond K are -inf before the maximum and never enter the sum.
//
// Sums over pixels, all without float atomics:
//   score      the probabilities of a tile go to LDS [64][256]; thread k owns code k and walks the 64 pixels in ascending order
//              with the running sum of the current id in a register, added to the workgroup's own row [id][k] in the workspace
//              when the id changes (the first touch of a row stores instead of adding: nothing is zeroed beforehand).
//              k_codebook_score adds the workgroups' rows in float64 in ascending workgroup order.
//   grad_cls   Q^T F on the matrix cores with the pixels as the k dimension: wavefront w owns code tiles 4 w .. 4 w + 3, the
//              accumulators (four code tiles x D / 16 channel blocks) stay in registers over all tiles of the workgroup.  Q
//              goes through LDS 32 pixels at a time, F [64][D] once per tile.
//   grad_cluster  the same product with Q replaced by the 0 / 1 matrix [v_p = k] and F by (B_v - s_p) / |s_p - B_v|.
//   The workgroups' [K][D] partial sums and float64 statistics are added in ascending workgroup order by k_codebook_finish.
// Workgroup b of G takes the consecutive tiles b T .. (b + 1) T - 1, T = ceil(tiles / 256), G = ceil(tiles / T) <= 256: masks
// are spatially coherent, so consecutive tiles keep the runs of one id long and the rows a workgroup touches few.
#pragma once

constexpr int CB_MAX_D = 64;
constexpr int CB_IDS = VP_PROTO_MAX_IDS;
constexpr int CB_MAX_K = VP_CODEBOOK_MAX_CODES;
constexpr int CB_THREADS = 256;
constexpr int CB_TILE = 64;               // pixels per tile: 16 per wavefront
constexpr int CB_GRID = 256;              // workgroups at most (one table of 256 x K floats each)
constexpr int CB_QS = 260;                // row stride of the probability tile: rows 4 h + i fall 16 banks apart
constexpr int CB_FS = 68;                 // row stride of the row tiles: the same, for 64 channels
constexpr int CB_QROWS = 32;              // pixels of the loss kernel's Q tile
static_assert(CB_IDS == 256 && CB_MAX_K == 256 && CB_THREADS == 256, "thread k owns code k, thread l id l");

typedef float cb_f4 __attribute__((ext_vector_type(4)));

struct CbPlan {
    long long n, tiles, per;              // pixels, tiles of 64, tiles per workgroup
    int G;                                // workgroups
};

static inline CbPlan cb_plan(int W, int H)
{
    CbPlan p;
    p.n = (long long)W * H;
    p.tiles = (p.n + CB_TILE - 1) / CB_TILE;
    p.per = (p.tiles + CB_GRID - 1) / CB_GRID;
    p.G = (int)((p.tiles + p.per - 1) / p.per);
    return p;
}

struct CbWs {
    float *tab;                           // [G][256][K]   assoc: the workgroups' score rows
    int *touched, *cnt;                   // [G][256]      assoc: which rows hold a sum, pixels per id
    float *gcls, *gclu;                   // [G][K][D]     loss: the workgroups' gradient sums
    double *dpart;                        // [G][4]        loss: cross-entropy, distance, participating, mismatches
    size_t bytes;
};

static inline CbWs cb_carve(void *workspace, int D, int K, int G)
{
    char *p = (char *)workspace;
    size_t off = 0;
    auto take = [&](size_t bytes) { char *q = p + off; off += align256(bytes); return q; };
    CbWs w;
    w.tab = (float *)take((size_t)G * CB_IDS * K * sizeof(float));
    w.touched = (int *)take((size_t)G * CB_IDS * sizeof(int));
    w.cnt = (int *)take((size_t)G * CB_IDS * sizeof(int));
    w.gcls = (float *)take((size_t)G * K * D * sizeof(float));
    w.gclu = (float *)take((size_t)G * K * D * sizeof(float));
    w.dpart = (double *)take((size_t)G * 4 * sizeof(double));
    w.bytes = off;
    return w;
}

__host__ __device__ static inline int cb_kpad(int K) { return (K + 15) / 16 * 16; }
static inline size_t cb_assoc_lds(int DP, int K) { return ((size_t)cb_kpad(K) * DP + (size_t)CB_TILE * CB_QS) * sizeof(float); }
static inline size_t cb_loss_lds(int DP, int K)
{
    return ((size_t)cb_kpad(K) * DP + (size_t)CB_QROWS * CB_QS + 2 * (size_t)CB_TILE * CB_FS) * sizeof(float);
}

// where channel ch of code k lives in the LDS code book
template <int DP> __device__ __forceinline__ int cb_at(int k, int ch) { return k * DP + (ch ^ (4 * ((k & 15) / (64 / DP)))); }

// the code book into LDS, zeros in the padding
template <int DP> __device__ __forceinline__ void cb_stage(const float *__restrict__ codebook, int K, int D, float *s_B)
{
    const int total = cb_kpad(K) * DP;
    for (int i = threadIdx.x; i < total; i += CB_THREADS) {
        const int k = i / DP, ch = i % DP;
        s_B[cb_at<DP>(k, ch)] = (k < K && ch < D) ? codebook[(size_t)k * D + ch] : 0.0f;
    }
}

// pixel p's channels 4 s + h (zeros at or beyond D and for a pixel past the image)
template <int DP>
__device__ __forceinline__ void cb_load(const float *__restrict__ image, long long n, long long p, int D, int h, float (&a)[DP / 4])
{
#pragma unroll
    for (int s = 0; s < DP / 4; ++s) {
        const int ch = 4 * s + h;
        a[s] = (p < n && ch < D) ? image[(size_t)ch * (size_t)n + (size_t)p] : 0.0f;
    }
}

template <int DP>
__device__ __forceinline__ void cb_logits(const float (&a)[DP / 4], const float *s_B, int D, int ntile, int r, int h, cb_f4 (&acc)[16])
{
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        acc[t] = cb_f4{0.0f, 0.0f, 0.0f, 0.0f};
        if (t < ntile) {                                              // uniform
#pragma unroll
            for (int s = 0; s < DP / 4; ++s)
                if (4 * s < D)                                        // uniform
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], s_B[cb_at<DP>(16 * t + r, 4 * s + h)], acc[t], 0, 0, 0);
        }
    }
}

// acc: the logits on entry, the probabilities on return (exact zeros at or beyond K).  mx: the maximum, sum: of
// expf(z - mx), arg: the lowest code at the maximum, zv: the logit of code v[i] (-inf when v[i] is no code).
__device__ __forceinline__ void cb_softmax(cb_f4 (&acc)[16], int K, int ntile, int r, const int (&v)[4], float (&mx)[4],
                                           float (&sum)[4], int (&arg)[4], float (&zv)[4])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        mx[i] = -INFINITY;
        zv[i] = -INFINITY;
        arg[i] = 0x7fffffff;
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        if (t < ntile) {
            const int k = 16 * t + r;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float z = k < K ? acc[t][i] : -INFINITY;
                acc[t][i] = z;
                if (z > mx[i]) {
                    mx[i] = z;
                    arg[i] = k;
                }
                if (k == v[i]) zv[i] = z;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const float m2 = __shfl_xor(mx[i], o);
            const int a2 = __shfl_xor(arg[i], o);
            if (m2 > mx[i] || (m2 == mx[i] && a2 < arg[i])) {
                mx[i] = m2;
                arg[i] = a2;
            }
            zv[i] = fmaxf(zv[i], __shfl_xor(zv[i], o));
        }
        sum[i] = 0.0f;
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        if (t < ntile) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float e = expf(acc[t][i] - mx[i]);              // -inf: 0
                acc[t][i] = e;
                sum[i] += e;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sum[i] = lanes_sum_up<16>(sum[i]);
        const float inv = 1.0f / sum[i];
#pragma unroll
        for (int t = 0; t < 16; ++t)
            if (t < ntile) acc[t][i] *= inv;
    }
}

__device__ __forceinline__ bool cb_valid(int id, int ignore_id) { return id >= 0 && id < CB_IDS && id != ignore_id; }

template <int DP>
__global__ __launch_bounds__(CB_THREADS) void k_codebook_assoc(const float *__restrict__ image, int D, long long n,
                                                               const int *__restrict__ ids, int ignore_id,
                                                               const float *__restrict__ codebook, int K, long long tiles,
                                                               long long per, float *__restrict__ tab, int *__restrict__ touched,
                                                               int *__restrict__ cnt_part, int *__restrict__ pred)
{
    extern __shared__ float cb_lds[];
    __shared__ int s_id[CB_TILE];
    __shared__ int s_cnt[CB_IDS];
    __shared__ int s_touch[4 * CB_IDS];                               // a copy per wavefront: read and set without a barrier
    float *s_B = cb_lds, *s_P = cb_lds + cb_kpad(K) * DP;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, h = lane >> 4;
    const int ntile = cb_kpad(K) / 16;
    cb_stage<DP>(codebook, K, D, s_B);
    s_cnt[tid] = 0;
    for (int i = tid; i < 4 * CB_IDS; i += CB_THREADS) s_touch[i] = 0;
    __syncthreads();
    float *mytab = tab + (size_t)blockIdx.x * CB_IDS * K;
    int *flag = s_touch + w * CB_IDS;
    int cur = -1;
    float run = 0.0f;
    auto flush = [&]() {
        float *at = mytab + (size_t)cur * K + tid;
        const float prev = flag[cur] ? *at : 0.0f;                    // the same in every lane of the wavefront
        *at = prev + run;
        flag[cur] = 1;
    };
    const long long t0 = (long long)blockIdx.x * per, t1 = min(t0 + per, tiles);
    for (long long tile = t0; tile < t1; ++tile) {
        const long long base = tile * CB_TILE + 16 * w;
        float a[DP / 4];
        cb_load<DP>(image, n, base + r, D, h, a);
        cb_f4 acc[16];
        cb_logits<DP>(a, s_B, D, ntile, r, h, acc);
        const int none[4] = {-1, -1, -1, -1};
        float mx[4], sum[4], zv[4];
        int arg[4];
        cb_softmax(acc, K, ntile, r, none, mx, sum, arg, zv);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long p = base + 4 * h + i;
            if (r == i) {                                             // one lane of the group per pixel
                const int id = p < n ? ids[p] : -1;
                const bool valid = p < n && cb_valid(id, ignore_id);
                s_id[16 * w + 4 * h + i] = valid ? id : -1;
                if (valid) atomicAdd(&s_cnt[id], 1);
                if (pred && p < n) pred[p] = valid ? min(arg[i], K - 1) : -1;
            }
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (t < ntile) s_P[(16 * w + 4 * h + i) * CB_QS + 16 * t + r] = acc[t][i];
        }
        __syncthreads();
        if (tid < K) {
            for (int q = 0; q < CB_TILE; ++q) {
                const int id = s_id[q];
                if (id < 0) continue;
                if (id != cur) {
                    if (cur >= 0) flush();
                    cur = id;
                    run = 0.0f;
                }
                run += s_P[q * CB_QS + tid];
            }
        }
        __syncthreads();
    }
    if (tid < K && cur >= 0) flush();
    __syncthreads();
    cnt_part[(size_t)blockIdx.x * CB_IDS + tid] = s_cnt[tid];
    touched[(size_t)blockIdx.x * CB_IDS + tid] = s_touch[tid];        // wavefront 0 owns code 0: it saw every flush
}

// one workgroup per id l, thread k: score[l][k] = the workgroups' rows added in float64 in ascending order
__global__ __launch_bounds__(CB_THREADS) void k_codebook_score(int K, int G, const float *__restrict__ tab,
                                                               const int *__restrict__ touched, const int *__restrict__ cnt_part,
                                                               double *__restrict__ score, int *__restrict__ id_pixels)
{
    __shared__ int s_t[CB_GRID];
    __shared__ int s_n;
    const int l = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_n = 0;
    s_t[tid] = tid < G ? touched[(size_t)tid * CB_IDS + l] : 0;
    __syncthreads();
    if (tid < G) {                                                    // integers: any order
        const int c = cnt_part[(size_t)tid * CB_IDS + l];
        if (c) atomicAdd(&s_n, c);
    }
    if (tid < K) {
        double s = 0.0;
        for (int b = 0; b < G; ++b)
            if (s_t[b]) s += (double)tab[((size_t)b * CB_IDS + l) * K + tid];
        score[(size_t)l * K + tid] = s;
    }
    __syncthreads();
    if (tid == 0) id_pixels[l] = s_n;
}

template <int DP>
__global__ __launch_bounds__(CB_THREADS) void k_codebook_loss(const float *__restrict__ image, int D, long long n,
                                                              const int *__restrict__ ids, int ignore_id,
                                                              const float *__restrict__ conf, float conf_min,
                                                              const float *__restrict__ codebook, int K,
                                                              const int *__restrict__ assign, long long tiles, long long per,
                                                              float *__restrict__ gcls_part, float *__restrict__ gclu_part,
                                                              double *__restrict__ dpart, float *__restrict__ pixel_loss)
{
    constexpr int DB = DP / 16;
    extern __shared__ float cb_lds[];
    __shared__ int s_v[CB_TILE];
    __shared__ int s_assign[CB_IDS];
    __shared__ double s_red[CB_THREADS];
    const int kpad = cb_kpad(K);
    float *s_B = cb_lds, *s_Q = s_B + kpad * DP, *s_F = s_Q + CB_QROWS * CB_QS, *s_W = s_F + CB_TILE * CB_FS;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, h = lane >> 4;
    const int ntile = kpad / 16;
    cb_stage<DP>(codebook, K, D, s_B);
    {
        const int v = assign[tid];
        s_assign[tid] = v >= 0 && v < K ? v : -1;
    }
    __syncthreads();
    cb_f4 gc[4][DB], gk[4][DB];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int cc = 0; cc < DB; ++cc) gc[tt][cc] = gk[tt][cc] = cb_f4{0.0f, 0.0f, 0.0f, 0.0f};
    double ce_sum = 0.0, dist_sum = 0.0;
    int n_part = 0, n_mis = 0;
    const long long t0 = (long long)blockIdx.x * per, t1 = min(t0 + per, tiles);
    for (long long tile = t0; tile < t1; ++tile) {
        const long long base = tile * CB_TILE + 16 * w;
        float a[DP / 4];
        {   // pixel r of the wavefront: the row tile, the clustering term
            const long long p = base + r;
            cb_load<DP>(image, n, p, D, h, a);
            int v = -1;
            if (p < n) {
                const int id = ids[p];
                if (cb_valid(id, ignore_id) && (!conf || conf[p] > conf_min)) v = s_assign[id];
            }
            const bool part = v >= 0;
            float ss = 0.0f;
#pragma unroll
            for (int s = 0; s < DP / 4; ++s) ss += a[s] * a[s];
            ss += __shfl_xor(ss, 16);
            ss += __shfl_xor(ss, 32);
            const float den = sqrtf(ss) + 1e-6f;
            float d[DP / 4], dd = 0.0f;
#pragma unroll
            for (int s = 0; s < DP / 4; ++s) {
                d[s] = a[s] / den - s_B[cb_at<DP>(part ? v : 0, 4 * s + h)];   // padding: 0 - 0
                dd += d[s] * d[s];
            }
            dd += __shfl_xor(dd, 16);
            dd += __shfl_xor(dd, 32);
            const float dist = sqrtf(dd);
#pragma unroll
            for (int s = 0; s < DP / 4; ++s) {
                s_F[(16 * w + r) * CB_FS + 4 * s + h] = a[s];
                s_W[(16 * w + r) * CB_FS + 4 * s + h] = (part && dist > 0.0f) ? -d[s] / dist : 0.0f;
            }
            if (h == 0) {
                s_v[16 * w + r] = v;
                if (part) dist_sum += (double)dist;
            }
        }
        cb_f4 acc[16];
        cb_logits<DP>(a, s_B, D, ntile, r, h, acc);
        int vc[4];
        bool okc[4], confc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {                                 // pixels 4 h + i: the same loads in the 16 lanes of a group
            const long long p = base + 4 * h + i;
            vc[i] = -1;
            okc[i] = p < n;
            confc[i] = false;
            if (p < n) {
                const int id = ids[p];
                if (cb_valid(id, ignore_id)) {
                    vc[i] = s_assign[id];
                    confc[i] = !conf || conf[p] > conf_min;
                }
            }
        }
        float mx[4], sum[4], zv[4];
        int arg[4];
        cb_softmax(acc, K, ntile, r, vc, mx, sum, arg, zv);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool part = vc[i] >= 0 && confc[i];
            const float ce = part ? (mx[i] + logf(sum[i])) - zv[i] : 0.0f;
            if (r == i) {
                if (part) {
                    ce_sum += (double)ce;
                    ++n_part;
                }
                if (vc[i] >= 0 && arg[i] != vc[i]) ++n_mis;
                if (pixel_loss && okc[i]) pixel_loss[base + 4 * h + i] = ce;
            }
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (t < ntile) acc[t][i] = part ? acc[t][i] - (16 * t + r == vc[i] ? 1.0f : 0.0f) : 0.0f;
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if ((w >> 1) == half) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int t = 0; t < 16; ++t)
                        if (t < ntile) s_Q[(16 * (w & 1) + 4 * h + i) * CB_QS + 16 * t + r] = acc[t][i];
            }
            __syncthreads();
            // pixels 16 j + 4 h + i of the half are the four k of one step, h on the lane: A from s_Q, B from the row tiles
#pragma unroll
            for (int j = 0; j < 2; ++j) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = 16 * j + 4 * h + i, pix = CB_QROWS * half + row;
                    const int vq = s_v[pix];
                    float bf[DB], bw[DB];
#pragma unroll
                    for (int cc = 0; cc < DB; ++cc) {
                        bf[cc] = s_F[pix * CB_FS + 16 * cc + r];
                        bw[cc] = s_W[pix * CB_FS + 16 * cc + r];
                    }
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const int t = 4 * w + tt;
                        if (t < ntile) {                              // uniform in the wavefront
                            const float aq = s_Q[row * CB_QS + 16 * t + r];
                            const float a1 = vq == 16 * t + r ? 1.0f : 0.0f;
#pragma unroll
                            for (int cc = 0; cc < DB; ++cc)
                                if (16 * cc < D) {
                                    gc[tt][cc] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq, bf[cc], gc[tt][cc], 0, 0, 0);
                                    gk[tt][cc] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bw[cc], gk[tt][cc], 0, 0, 0);
                                }
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
    // register i of an accumulator: code 16 t + 4 h + i, channel 16 cc + r
    const size_t b = blockIdx.x;
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int cc = 0; cc < DB; ++cc)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = 16 * (4 * w + tt) + 4 * h + i, c = 16 * cc + r;
                if (k < K && c < D) {
                    gcls_part[(b * K + k) * D + c] = gc[tt][cc][i];
                    gclu_part[(b * K + k) * D + c] = gk[tt][cc][i];
                }
            }
    // four trees of one value on one buffer, not one tree of four: the kernel's LDS stays what it was
    const double s0 = block_tree_sum<CB_THREADS>(ce_sum, s_red), s1 = block_tree_sum<CB_THREADS>(dist_sum, s_red);
    const double s2 = block_tree_sum<CB_THREADS>((double)n_part, s_red);                      // integers: exact
    const double s3 = block_tree_sum<CB_THREADS>((double)n_mis, s_red);
    if (tid == 0) {
        dpart[b * 4 + 0] = s0;
        dpart[b * 4 + 1] = s1;
        dpart[b * 4 + 2] = s2;
        dpart[b * 4 + 3] = s3;
    }
}

// element e of the two [K][D] gradients: the workgroups' sums in float64 in ascending order; the last workgroup adds the
// statistics the same way
__global__ __launch_bounds__(CB_THREADS) void k_codebook_finish(int KD, int G, const float *__restrict__ gcls_part,
                                                                const float *__restrict__ gclu_part,
                                                                const double *__restrict__ dpart, float *__restrict__ grad_cls,
                                                                float *__restrict__ grad_cluster, double *__restrict__ stats)
{
    const int tid = threadIdx.x;
    if (blockIdx.x == gridDim.x - 1) {
        if (tid < 4) {
            double s = 0.0;
            for (int b = 0; b < G; ++b) s += dpart[(size_t)b * 4 + tid];
            stats[tid] = s;
        }
        return;
    }
    const int e = blockIdx.x * CB_THREADS + tid;
    if (e >= KD) return;
    double s = 0.0, t = 0.0;
#pragma unroll 8
    for (int b = 0; b < G; ++b) {
        s += (double)gcls_part[(size_t)b * KD + e];
        t += (double)gclu_part[(size_t)b * KD + e];
    }
    grad_cls[e] = (float)s;
    grad_cluster[e] = (float)t;
}

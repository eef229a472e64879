// vp_eval.h -- scoring label maps against ground truth: confusion matrix, boundary band, boundary counts.  Everything here
// is an integer, so every result is exact and independent of the order the atomics arrive in.
//
// Boundary band.  band[y,x] = 0 iff the (2r+1)^2 window round (x,y) lies inside the image and holds one label.  "All equal"
// over a square window is separable, and over a run of equal labels it is a question of run lengths, not of a window scan:
//   k_eval_row_ok    ok[y,x] = the run of labels equal to labels[y,x] in row y reaches at least r pixels to either side
//                    (the image edge ends a run, so a window that leaves the image sideways is never ok)
//   k_eval_col_band  band[y,x] = 0 iff the run, in column x, of rows that are ok and carry labels[y,x] reaches at least r
//                    rows up and down
// Both are O(1) per pixel for every r.  A row (column) is cut into segments that are swept forward and backward; a sweep
// starts r + 1 pixels before its segment, pretending a break there: a run that long is long enough whatever lies before it,
// so segments need nothing from each other and r may exceed the segment, W, H or all three.
//
// Scores.  k_eval_scores<true>  (P <= EVAL_LDS_P): the confusion of a workgroup's pixels in an LDS histogram of P*P u32,
//                               flushed with one 64-bit atomic per non-zero cell
//          k_eval_scores<false> (P up to 256, P*P u32 would not fit): a wavefront groups its 64 keys by ballot and holds the
//                               last key's count in registers across batches, so a constant region costs no atomic at all
// Both count the skipped pixels and, when the two bands are given, the boundary intersections and unions per class (LDS).
#pragma once

constexpr int EVAL_MAX_P = 256;
constexpr int EVAL_MAX_RADIUS = 4096;
constexpr int EVAL_LDS_P = 64;            // P*P u32 = 16 KiB of LDS at most
constexpr int EVAL_ROW_SEG = 256;         // least pixels per row segment (a multiple of 64)
constexpr int EVAL_COL_SEG = 64;          // least rows per column segment
constexpr int EVAL_SCORE_BLOCKS = 2048;   // grid-stride beyond

static inline int eval_round64(int v) { return (v + 63) / 64 * 64; }
// pixels per row segment / rows per column segment: at least the halo, so a sweep reads at most ~3x its segment
static inline int eval_row_seg(int radius) { return std::max(EVAL_ROW_SEG, eval_round64(radius + 1)); }
static inline int eval_col_seg(int radius) { return std::max(EVAL_COL_SEG, radius + 1); }

// one wavefront per (row, segment); lane = pixel of a 64-pixel chunk; the breaks of a chunk are one ballot
__global__ __launch_bounds__(256) void k_eval_row_ok(const int *__restrict__ labels, int W, int H, int radius, int seg, int nseg,
                                                     unsigned char *__restrict__ ok)
{
    const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (long long)H * nseg) return;
    const int lane = threadIdx.x & 63;
    const int y = (int)(item / nseg);
    const int x0 = (int)(item % nseg) * seg, x1 = min(W, x0 + seg);
    const int need = radius + 1, halo = (need + 63) / 64 * 64;
    const int *row = labels + (long long)y * W;
    unsigned char *okr = ok + (long long)y * W;

    // forward: start of the run each pixel is in -> long enough to the left?
    const int xs = max(0, x0 - halo);
    int start = xs;
    for (int b = xs; b < x1; b += 64) {
        const int x = b + lane;
        const bool in = x < x1;
        const int v = in ? row[x] : 0;
        const int pv = (in && x > xs) ? row[x - 1] : 0;
        const unsigned long long brk = __ballot(in && (x == xs || v != pv));
        const unsigned long long upto = brk & (~0ull >> (63 - lane));
        const int st = upto ? b + 63 - __clzll((long long)upto) : start;
        if (in && x >= x0) okr[x] = (x - st + 1 >= need) ? 1 : 0;
        if (brk) start = b + 63 - __clzll((long long)brk);
    }
    // backward: end of the run -> long enough to the right?  (the same lane wrote okr[x] above)
    const int xe = min(W, x1 + halo);
    int end = xe - 1;
    for (int b = x0 + (xe - 1 - x0) / 64 * 64; b >= x0; b -= 64) {
        const int x = b + lane;
        const bool in = x < xe;
        const int v = in ? row[x] : 0;
        const int nv = (in && x + 1 < xe) ? row[x + 1] : 0;
        const unsigned long long brk = __ballot(in && (x == xe - 1 || v != nv));
        const unsigned long long from = brk >> lane;
        const int en = from ? x + __ffsll((long long)from) - 1 : end;
        if (in && x < x1 && en - x + 1 < need) okr[x] = 0;
        if (brk) end = b + __ffsll((long long)brk) - 1;
    }
}

// one lane per (column, segment of rows): adjacent lanes read adjacent pixels of a row
__global__ __launch_bounds__(64) void k_eval_col_band(const int *__restrict__ labels, const unsigned char *__restrict__ ok, int W,
                                                      int H, int radius, int seg, unsigned char *__restrict__ band)
{
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    const int y0 = blockIdx.y * seg, y1 = min(H, y0 + seg);
    const int need = radius + 1;
    const int ys = max(0, y0 - need), ye = min(H, y1 + need);
    // run = rows up to and including y that are ok and hold the label of row y
    int run = 0, pv = 0;
#pragma unroll 4
    for (int y = ys; y < y1; ++y) {
        const long long i = (long long)y * W + x;
        const int v = labels[i];
        run = ok[i] ? ((run > 0 && v == pv) ? run + 1 : 1) : 0;
        pv = v;
        if (y >= y0) band[i] = run < need ? 1 : 0;
    }
    run = 0;
#pragma unroll 4
    for (int y = ye - 1; y >= y0; --y) {
        const long long i = (long long)y * W + x;
        const int v = labels[i];
        run = ok[i] ? ((run > 0 && v == pv) ? run + 1 : 1) : 0;
        pv = v;
        if (y < y1 && run < need) band[i] = 1;
    }
}

template <bool LDS_CONF>
__global__ __launch_bounds__(256) void k_eval_scores(const int *__restrict__ pred, const int *__restrict__ target, long long n, int P,
                                                     const unsigned char *__restrict__ pband,
                                                     const unsigned char *__restrict__ tband, unsigned long long *confusion,
                                                     unsigned long long *skipped, unsigned long long *bnd_inter,
                                                     unsigned long long *bnd_union)
{
    __shared__ unsigned s_conf[LDS_CONF ? EVAL_LDS_P * EVAL_LDS_P : 1];
    __shared__ unsigned s_inter[EVAL_MAX_P], s_union[EVAL_MAX_P], s_skip[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const bool bnd = pband != nullptr;
    if (LDS_CONF)
        for (int k = tid; k < P * P; k += 256) s_conf[k] = 0;
    for (int k = tid; k < P; k += 256) { s_inter[k] = 0; s_union[k] = 0; }
    if (tid < 2) s_skip[tid] = 0;
    __syncthreads();

    unsigned skip_t = 0, skip_p = 0;
    int held_key = -1;            // the global path: the key whose count this wavefront still holds, and the count
    unsigned held = 0;
    const long long stride = (long long)gridDim.x * 256;
    for (long long base = (long long)blockIdx.x * 256; base < n; base += stride) {      // (uniform per workgroup)
        const long long i = base + tid;
        int key = -1;
        if (i < n) {
            const int t = target[i], p = pred[i];
            const bool tv = t >= 0 && t < P, pv = p >= 0 && p < P;
            if (!tv) skip_t++;
            else if (!pv) skip_p++;
            else key = t * P + p;
            if (bnd && tv) {
                const bool tb = tband[i] != 0, pb = pv && pband[i] != 0;
                if (p == t) {
                    if (tb && pb) atomicAdd(&s_inter[t], 1u);
                    if (tb || pb) atomicAdd(&s_union[t], 1u);
                } else {
                    if (tb) atomicAdd(&s_union[t], 1u);
                    if (pb) atomicAdd(&s_union[p], 1u);
                }
            }
        }
        if (LDS_CONF) {
            if (key >= 0) atomicAdd(&s_conf[key], 1u);
        } else {
            unsigned long long todo = __ballot(key >= 0);
            while (todo) {
                const int k = __shfl(key, __ffsll((long long)todo) - 1);
                const unsigned long long same = __ballot(key == k);
                if (k != held_key) {
                    if (held && lane == 0) atomicAdd(confusion + held_key, (unsigned long long)held);
                    held_key = k;
                    held = 0;
                }
                held += (unsigned)__popcll(same);
                todo &= ~same;
            }
        }
    }
    if (!LDS_CONF && held && lane == 0) atomicAdd(confusion + held_key, (unsigned long long)held);
    if (skip_t) atomicAdd(&s_skip[0], skip_t);
    if (skip_p) atomicAdd(&s_skip[1], skip_p);
    __syncthreads();
    if (LDS_CONF)
        for (int k = tid; k < P * P; k += 256)
            if (s_conf[k]) atomicAdd(confusion + k, (unsigned long long)s_conf[k]);
    if (bnd)
        for (int k = tid; k < P; k += 256) {
            if (s_inter[k]) atomicAdd(bnd_inter + k, (unsigned long long)s_inter[k]);
            if (s_union[k]) atomicAdd(bnd_union + k, (unsigned long long)s_union[k]);
        }
    if (tid < 2 && s_skip[tid]) atomicAdd(skipped + tid, (unsigned long long)s_skip[tid]);
}

// the band of one map into `band`, with `ok` (W*H bytes) as the row pass's scratch
static void eval_launch_band(const int *labels, int W, int H, int radius, unsigned char *band, unsigned char *ok, hipStream_t stream)
{
    const int seg = eval_row_seg(radius), nseg = (W + seg - 1) / seg;
    const long long items = (long long)H * nseg;
    hipLaunchKernelGGL(k_eval_row_ok, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, stream, labels, W, H, radius, seg, nseg, ok);
    const int cseg = eval_col_seg(radius);
    hipLaunchKernelGGL(k_eval_col_band, dim3((unsigned)((W + 63) / 64), (unsigned)((H + cseg - 1) / cseg)), dim3(64), 0, stream,
                       labels, (const unsigned char *)ok, W, H, radius, cseg, band);
}

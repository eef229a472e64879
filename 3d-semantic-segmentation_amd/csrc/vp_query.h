// vp_query.h -- text query of a per-voxel feature table: normalised dot product against P prompt embeddings, argmax label and
// softmax top-1 minus top-2 margin (k_query_text, k_query).  Included by voxproj.hip only.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// logit[r, j] = scale * (x_r / max(|x_r|, 1e-12)) . (t_j / max(|t_j|, 1e-12))   (F.normalize, eps 1e-12)
// label[r]    = argmax_j logit[r, j], lowest j on exact ties
// margin[r]   = softmax(logit[r])[label] - second-largest softmax entry   (1 when P = 1)
//
// k_query_text: one wavefront per prompt: t / max(|t|, 1e-12) (|t| summed in float64) into the workspace as a zero-padded
//   row-major [Ppad = 16*ceil(P/16)][Cpad = 32*ceil(C/32)] table, binary16 (round to nearest even) for fp16 rows, f32 for f32
//   rows.  Rows and columns of the padding are zeros, so they add nothing to any dot product.
//
// k_query: one wavefront per tile of 16 rows, four per workgroup.  A skinny GEMM [16, C] x [C, 16] per P-tile on the matrix
//   cores, the rows as the A operand straight from registers:
//   fp16 rows: v_mfma_f32_16x16x32_f16.  Lane l holds A[row l&15][k = 8(l>>4) + j] -- one 16-byte load per lane per k-step of 32
//     columns; the 16 k-steps of C = 512 (64 VGPRs) are all requested before the first MFMA, so every 128-byte line of a row is
//     asked for by two adjacent loads in flight together.  The rows go in as they are: gfx950's f16 MFMA keeps subnormal
//     inputs: test_gpu_query.py's rows of fp16 subnormals meet the float64 bound without any scaling (an earlier build
//     scaled every row into [2^14, 2^15) first, in case they were flushed; the unscaled build passes the same tests).
//   fp32 rows: v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation; no rounding of the rows).  The k order is
//     permuted so that a lane still reads 16 bytes at a time: one float4 at columns 16s + 4(l>>4) feeds the four MFMAs of slot
//     s, MFMA q taking column 16s + 4h + q of A and B alike (any k order gives the same sum; the text is read in the same order).
//   The B operand (16 prompts x one chunk of 512 f16 / 256 f32 columns, 16 KiB) is staged in LDS once per workgroup and
//   P-tile, rows padded by 16 bytes so that the 16 prompt rows of a ds_read_b128 fall on distinct banks.  Each tile is
//   requested into registers one step ahead (the first before the rows), so its latency hides behind the rows' or behind the
//   previous tile's MFMAs (fp16, 16 M rows: 6.7 -> 4.8 ms at P = 13 with the single-chunk variant; every wavefront reading
//   the text from L2 itself, without LDS and barriers, was slower at every P: profiles/r07_query_ab.log).
//   C above the chunk (fp16 C > 512, fp32 C > 256): the norm is taken in a first pass over the chunks and the row is
//   re-read chunk by chunk for every P-tile (from L1/L2: one wavefront's 16 rows are at most 128 KiB).
//   |x|^2 is summed in f32 (fp16 squares, subnormals included, are normal f32 numbers).
//
//   The accumulator tile has the prompt on the lane (col = l&15) and rows 4(l>>4) + i in its four registers.  Each lane keeps,
//   for its four rows, a running (max, argmax, second max, sum of exp(z - max)) over the prompts j = l&15 (mod 16) of all
//   P-tiles; one butterfly over the 16 lanes of a row group merges them at the end.  The merge is commutative, so every lane
//   of a group ends with the same bits and a row's result does not depend on its position in the tile or on its neighbours.
//
//   A row with a non-finite element: label -1, logits and margin NaN, +1 to *n_nonfinite (one vector atomic per wavefront).
//   ONE: the row fits one chunk (C <= 512 fp16, <= 256 fp32), the loops over chunks compile away.
//   VEC: 16-byte row loads (C % 8 == 0 for fp16, C % 4 == 0 for fp32, 16-byte aligned rows and stride); otherwise every
//   element is loaded on its own (any C, any alignment).  Bounds are tested before every load: rows past n_rows and columns
//   past C read as zero, and only valid rows are stored.  64-bit offsets throughout.
// ------------------------------------------------------------------------------------------------
constexpr int QUERY_WAVES = 4;                    // wavefronts per workgroup (16 rows each)
constexpr int QUERY_NS = 16;                      // 16-byte slots per lane and chunk: 64 VGPRs of row data
constexpr int QUERY_LDS_ROW = 1024 / 16 + 1;      // one prompt's chunk in uint4, padded by 16 bytes
constexpr int QUERY_MAX_P = 1024;
constexpr int QUERY_MAX_C = 2048;

__host__ __device__ inline int query_ppad(int P) { return (P + 15) / 16 * 16; }
__host__ __device__ inline int query_cpad(int C) { return (C + 31) / 32 * 32; }

typedef _Float16 query_h8 __attribute__((ext_vector_type(8)));
typedef float query_f4 __attribute__((ext_vector_type(4)));

template <typename T> struct QueryTraits;
template <> struct QueryTraits<_Float16> {
    static constexpr int W = 32;                  // columns per slot (one k-step of 16x16x32)
    typedef query_h8 Slot;
};
template <> struct QueryTraits<float> {
    static constexpr int W = 16;                  // columns per slot (four k-steps of 16x16x4)
    typedef query_f4 Slot;
};

template <typename T>
__global__ __launch_bounds__(64) void k_query_text(const float *__restrict__ text, int P, int C, T *__restrict__ out)
{
    const int p = blockIdx.x, lane = threadIdx.x, Cpad = query_cpad(C);
    const float *t = text + (long long)p * C;
    double ss = 0.0;
    if (p < P)
        for (int c = lane; c < C; c += 64) ss += (double)t[c] * (double)t[c];
    ss = lanes_sum_down<64>(ss);
    const double inv = 1.0 / fmax(sqrt(ss), 1e-12);
    T *dst = out + (long long)p * Cpad;
    for (int c = lane; c < Cpad; c += 64) dst[c] = (T)((p < P && c < C) ? (float)((double)t[c] * inv) : 0.0f);
}

// row data of one slot: the 16 bytes at columns col .. col + 16/sizeof(T) - 1 of `row` (zeros past C or for a missing row)
template <typename T, bool VEC>
__device__ __forceinline__ typename QueryTraits<T>::Slot query_load(const T *__restrict__ row, bool row_ok, int col, int C)
{
    typedef typename QueryTraits<T>::Slot S;
    constexpr int E = 16 / sizeof(T);
    S v = {};
    if (VEC) {
        if (row_ok && col < C) v = *(const S *)(row + col);
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (row_ok && col + e < C) v[e] = row[col + e];
    }
    return v;
}

// this thread's 4 x 16 bytes of the B tile (prompts 16pt .. 16pt+15, columns ch*CW .. ch*CW + CW - 1 of the normalised text)
template <typename T>
__device__ __forceinline__ void query_fetch_b(const T *__restrict__ textn, int Cpad, int pt, int ch, uint4 (&v)[4])
{
    constexpr int CW = QUERY_NS * QueryTraits<T>::W, E = 16 / sizeof(T);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = threadIdx.x + q * 64 * QUERY_WAVES, pr = idx >> 6, c16 = idx & 63;
        const int col = ch * CW + c16 * E;
        v[q] = col < Cpad ? *(const uint4 *)(textn + (long long)(pt * 16 + pr) * Cpad + col) : uint4{0u, 0u, 0u, 0u};
    }
}

// running top-2 / softmax state of one row over the prompts a lane has seen
struct QueryStat {
    float m1, m2, s;
    int arg;
};

__device__ __forceinline__ void query_push(QueryStat &st, float z, int j)
{
    if (z > st.m1) {
        st.s = st.s * __expf(st.m1 - z) + 1.0f;
        st.m2 = st.m1;
        st.m1 = z;
        st.arg = j;
    } else {
        st.s += __expf(z - st.m1);
        st.m2 = fmaxf(st.m2, z);
    }
}

// merge with the state of lane `lane ^ o` (commutative: both lanes end with the same bits)
__device__ __forceinline__ void query_merge(QueryStat &st, int o)
{
    const float m1 = __shfl_xor(st.m1, o), m2 = __shfl_xor(st.m2, o), s = __shfl_xor(st.s, o);
    const int arg = __shfl_xor(st.arg, o);
    const float m = fmaxf(st.m1, m1);
    const float a = st.m1 == -INFINITY ? 0.0f : st.s * __expf(st.m1 - m);
    const float b = m1 == -INFINITY ? 0.0f : s * __expf(m1 - m);
    const bool take = m1 > st.m1 || (m1 == st.m1 && arg < st.arg);
    st.m2 = fmaxf(fmaxf(st.m2, m2), fminf(st.m1, m1));
    st.arg = take ? arg : st.arg;
    st.m1 = m;
    st.s = a + b;
}

template <typename T, bool VEC, bool ONE>
__global__ __launch_bounds__(64 * QUERY_WAVES) void k_query(const T *__restrict__ rows, long long n_rows, int C, long long stride,
                                                           const T *__restrict__ textn, int P, float scale, float *__restrict__ logits,
                                                           int *__restrict__ labels, float *__restrict__ margin, int *n_nonfinite)
{
    typedef QueryTraits<T> Tr;
    typedef typename Tr::Slot Slot;
    constexpr int W = Tr::W, E = 16 / sizeof(T);
    __shared__ uint4 lds[16 * QUERY_LDS_ROW];

    const int lane = threadIdx.x & 63, h = lane >> 4, r = lane & 15;
    const long long row0 = ((long long)blockIdx.x * QUERY_WAVES + (threadIdx.x >> 6)) * 16;
    const long long my_row = row0 + r;                       // A layout: this lane's row
    const bool row_ok = my_row < n_rows;
    const T *rp = rows + (row_ok ? my_row : 0) * stride;
    const int Cpad = query_cpad(C), n_slots = (C + W - 1) / W, n_chunks = ONE ? 1 : (n_slots + QUERY_NS - 1) / QUERY_NS;

    // the first B tile is requested before the rows, so that its latency hides behind theirs
    uint4 bnext[4];
    query_fetch_b<T>(textn, Cpad, 0, 0, bnext);

    // pass over the row: sum of squares, non-finite elements (x - x is NaN exactly for inf / NaN)
    Slot a[QUERY_NS];
    float ss = 0.0f, nf = 0.0f;
    for (int ch = 0; ch < n_chunks; ++ch) {
#pragma unroll
        for (int s = 0; s < QUERY_NS; ++s) {
            if (ch * QUERY_NS + s < n_slots) {
                a[s] = query_load<T, VEC>(rp, row_ok, (ch * QUERY_NS + s) * W + h * E, C);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const float x = (float)a[s][e];
                    ss = fmaf(x, x, ss);
                    nf += x - x;
                }
            } else {
                a[s] = Slot{};
            }
        }
    }
    ss += __shfl_xor(ss, 16); ss += __shfl_xor(ss, 32);        // the same order in every lane of the row: identical bits
    nf += __shfl_xor(nf, 16); nf += __shfl_xor(nf, 32);
    const bool bad = row_ok && !(nf == 0.0f);
    float mult = scale / fmaxf(sqrtf(ss), 1e-12f);
    if (bad) mult = __builtin_nanf("");

    {   // non-finite rows counted once (A layout, lanes 0..15)
        const unsigned long long m = __ballot(bad && h == 0);
        if (m && n_nonfinite && lane == 0) atomicAdd(n_nonfinite, (int)__popcll(m));
    }

    // C/D layout: this lane's prompt column is r, its rows 4h + i
    float mult4[4];
    bool ok4[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        mult4[i] = __shfl(mult, 4 * h + i);
        ok4[i] = row0 + 4 * h + i < n_rows;
    }
    QueryStat st[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) st[i] = QueryStat{-INFINITY, -INFINITY, 0.0f, 0};

    const int n_pt = query_ppad(P) / 16;
    for (int pt = 0; pt < n_pt; ++pt) {
        query_f4 acc0 = {}, acc1 = {};
        for (int ch = 0; ch < n_chunks; ++ch) {
            // B tile (pt, ch) from registers into LDS; the next one is requested before this one's MFMAs
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int idx = threadIdx.x + q * 64 * QUERY_WAVES;
                lds[(idx >> 6) * QUERY_LDS_ROW + (idx & 63)] = bnext[q];
            }
            __syncthreads();
            if (ch + 1 < n_chunks) query_fetch_b<T>(textn, Cpad, pt, ch + 1, bnext);
            else if (pt + 1 < n_pt) query_fetch_b<T>(textn, Cpad, pt + 1, 0, bnext);
            if (n_chunks > 1) {
#pragma unroll
                for (int s = 0; s < QUERY_NS; ++s)
                    a[s] = ch * QUERY_NS + s < n_slots ? query_load<T, VEC>(rp, row_ok, (ch * QUERY_NS + s) * W + h * E, C) : Slot{};
            }
#pragma unroll
            for (int s = 0; s < QUERY_NS; ++s) {
                if (ch * QUERY_NS + s < n_slots) {
                    const Slot b = __builtin_bit_cast(Slot, lds[r * QUERY_LDS_ROW + s * (W / E) + h]);
                    if constexpr (sizeof(T) == 2) {
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], b, acc0, 0, 0, 0);
                    } else {
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][0], b[0], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][1], b[1], acc1, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][2], b[2], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][3], b[3], acc1, 0, 0, 0);
                    }
                }
            }
        }
        const int j = pt * 16 + r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float z = (sizeof(T) == 2 ? acc0[i] : acc0[i] + acc1[i]) * mult4[i];
            if (j < P) {
                query_push(st[i], z, j);
                if (logits && ok4[i]) logits[(row0 + 4 * h + i) * P + j] = z;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) query_merge(st[i], o);

    // lane r < 4 of row group h stores row 4h + r
    const bool bad_r = __shfl(bad ? 1 : 0, 4 * h + (r & 3)) != 0;
    const long long row = row0 + 4 * h + r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (r == i && row < n_rows) {
            labels[row] = bad_r ? -1 : st[i].arg;
            if (margin) margin[row] = bad_r ? __builtin_nanf("") : P == 1 ? 1.0f : (1.0f - __expf(st[i].m2 - st[i].m1)) / st[i].s;
        }
    }
}

}  // namespace

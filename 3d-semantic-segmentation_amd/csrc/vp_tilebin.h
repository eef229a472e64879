// vp_tilebin.h -- binning primitives into the 16 x 16 pixel tiles of an image: from per-primitive tile boxes to one sorted run
// of primitive indices per tile.  Everything here is blind to what the primitive is; the Gaussian splatter (vp_splat.h) and
// the mesh rasterizer (vp_mesh.h) bring their records, their projection kernel and their tile kernel.  Included by voxproj.hip
// only, after vp_common.h and before vp_splat.h.
#pragma once

#if !__has_include(<rocprim/device/device_radix_sort.hpp>)
#error "vp_tilebin.h needs rocPRIM's headers (ROCm's include/rocprim): the tile sort is rocprim::radix_sort_pairs"
#endif
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

// ------------------------------------------------------------------------------------------------
// The contract.  A family's projection kernel leaves per primitive a tile box (x0, y0, x1, y1; 0, 0, -1, -1 without tiles)
// and its tile count.  tile_scan: the inclusive scan of the counts (rocprim, int64), then k_tile_total.
// Key: a tile index above `tile_shift<Key>` low bits.  32-bit keys (the mesh) are the tile alone: a tile's run is in index
//   order.  64-bit keys (the splatter) carry the bits of a positive fp32 depth below the tile, which order like the floats: a
//   tile's run is in (depth, index) order.
// k_tile_emit<Key>    one thread per primitive: key and value = primitive index for each tile of its box, in index order; the
//   slots [total, capacity) get the key of n_tiles (after every real tile).  rocprim::radix_sort_pairs is stable and sorts bits
//   [0, end_bit), end_bit = tile_shift<Key> + tile_bits(n_tiles): the padding key needs the bit of n_tiles too.
// k_tile_ranges<Key>  one thread per sorted key: [start, end) of every tile's run.
// Every kernel after the scan reads the device total first: a total above the workspace's capacity writes nothing (the emit
// kernel raises *status instead), so a too-small workspace never leaves a partial image.
// ------------------------------------------------------------------------------------------------
constexpr int TILE_PX = 16;

template <typename Key>
constexpr int tile_shift = 8 * (int)sizeof(Key) - 32;

// bits needed to write v
inline int tile_bits(long long v)
{
    int b = 0;
    while (b < 63 && (1LL << b) <= v) ++b;
    return b;
}

// total = the scan's last element (0 without primitives), into the workspace and, when given, the caller's int64
__global__ void k_tile_total(const long long *__restrict__ offs, long long n, long long *total, long long *n_isect)
{
    const long long t = n > 0 ? offs[n - 1] : 0;
    *total = t;
    if (n_isect) *n_isect = t;
}

// depth: primitive i's depth at depth[i * depth_stride], read only for a 64-bit key and a primitive with tiles
template <typename Key>
__global__ __launch_bounds__(256) void k_tile_emit(const float *__restrict__ depth, int depth_stride,
                                                   const int4 *__restrict__ box, const long long *__restrict__ offs,
                                                   long long n, int tiles_x, long long n_tiles, const long long *total_p,
                                                   long long capacity, Key *__restrict__ keys, int *__restrict__ vals,
                                                   int *status)
{
    const long long total = *total_p;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (total > capacity) {
        if (gid == 0 && status) *status = 1;
        return;
    }
    if (gid < n) {
        const int4 b = box[gid];
        long long k = offs[gid] - (long long)(b.z - b.x + 1) * (b.w - b.y + 1);
        if (b.z >= b.x) {
            Key low = 0;
            if constexpr (tile_shift<Key> > 0) low = __float_as_uint(depth[gid * depth_stride]);
            for (int ty = b.y; ty <= b.w; ++ty)
                for (int tx = b.x; tx <= b.z; ++tx, ++k) {
                    keys[k] = ((Key)(ty * tiles_x + tx) << tile_shift<Key>) | low;
                    vals[k] = (int)gid;
                }
        }
    }
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long k = total + gid; k < capacity; k += stride) {
        keys[k] = (Key)n_tiles << tile_shift<Key>;
        vals[k] = 0;
    }
}

template <typename Key>
__global__ __launch_bounds__(256) void k_tile_ranges(const Key *__restrict__ keys, const long long *total_p, long long capacity,
                                                     longlong2 *__restrict__ ranges)
{
    const long long total = *total_p;
    if (total > capacity) return;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long tile = (long long)(keys[i] >> tile_shift<Key>);
    const long long prev = i > 0 ? (long long)(keys[i - 1] >> tile_shift<Key>) : -1;
    if (tile != prev) {
        ranges[tile].x = i;
        if (prev >= 0) ranges[prev].y = i;
    }
    if (i == total - 1) ranges[tile].y = total;
}

// Lays the sections of a workspace one after another, each 256-byte aligned; without a base it only adds up the bytes.
struct Sections {
    char *base;
    size_t bytes = 0;
    template <typename T>
    void place(T *&p, size_t n_bytes)
    {
        p = base ? (T *)(base + bytes) : nullptr;
        bytes += align256(n_bytes);
    }
};

// The shared sections of a tile-binned workspace of one (n, W, H, capacity), as typed pointers into it.  Everything before
// `keys0` lies at an offset that does not depend on the capacity: what a projection wrote survives a regrow by copying.
template <typename Key>
struct TileBins {
    long long *total;
    int4 *box;
    int *count;
    long long *offs;
    char *scan_tmp;
    Key *keys0, *keys1;
    int *vals0, *vals1;
    char *sort_tmp;
    longlong2 *ranges;
    size_t bytes, scan_bytes, sort_bytes;
    int tiles_x, tiles_y, end_bit;

    long long n_tiles() const { return (long long)tiles_x * tiles_y; }
    dim3 tile_grid() const { return dim3((unsigned)tiles_x, (unsigned)tiles_y); }
};

// Host only: the rocprim calls with a NULL scratch pointer only report their scratch sizes (false when one fails).
// own(sections, 0) places the family's sections that follow `total`, own(sections, 1) those that follow `offs`.
template <typename Key, typename Own>
bool tile_layout(char *base, long long n, int W, int H, long long capacity, TileBins<Key> &l, Own &&own)
{
    l.tiles_x = (W + TILE_PX - 1) / TILE_PX;
    l.tiles_y = (H + TILE_PX - 1) / TILE_PX;
    l.end_bit = tile_shift<Key> + tile_bits(l.n_tiles());
    l.scan_bytes = 0;
    l.sort_bytes = 0;
    if (n > 0 && rocprim::inclusive_scan(nullptr, l.scan_bytes, (const int *)nullptr, (long long *)nullptr, (size_t)n,
                                         rocprim::plus<long long>()) != hipSuccess)
        return false;
    if (capacity > 0 && rocprim::radix_sort_pairs(nullptr, l.sort_bytes, (const Key *)nullptr, (Key *)nullptr,
                                                  (const int *)nullptr, (int *)nullptr, (size_t)capacity, 0u,
                                                  (unsigned)l.end_bit) != hipSuccess)
        return false;
    Sections s{base};
    s.place(l.total, sizeof(long long));
    own(s, 0);
    s.place(l.box, (size_t)n * sizeof(int4));
    s.place(l.count, (size_t)n * sizeof(int));
    s.place(l.offs, (size_t)n * sizeof(long long));
    own(s, 1);
    s.place(l.scan_tmp, l.scan_bytes);
    s.place(l.keys0, (size_t)capacity * sizeof(Key));
    s.place(l.keys1, (size_t)capacity * sizeof(Key));
    s.place(l.vals0, (size_t)capacity * sizeof(int));
    s.place(l.vals1, (size_t)capacity * sizeof(int));
    s.place(l.sort_tmp, l.sort_bytes);
    s.place(l.ranges, (size_t)l.n_tiles() * sizeof(longlong2));
    l.bytes = s.bytes;
    return true;
}

// the tail of a projection: the inclusive scan of the n tile counts, then the total
template <typename Key>
int tile_scan(const TileBins<Key> &l, long long n, long long *n_isect, hipStream_t stream)
{
    if (n > 0) {
        size_t tmp = l.scan_bytes;
        VP_HIP(rocprim::inclusive_scan(l.scan_tmp, tmp, (const int *)l.count, l.offs, (size_t)n, rocprim::plus<long long>(),
                                       stream));
    }
    hipLaunchKernelGGL(k_tile_total, dim3(1), dim3(1), 0, stream, (const long long *)l.offs, n, l.total, n_isect);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

// emit the keys of the n projected primitives, sort them and find every tile's run: what a tile kernel reads (vals1, ranges)
template <typename Key>
int tile_sort(const TileBins<Key> &l, const float *depth, int depth_stride, long long n, long long capacity, int *status,
              hipStream_t stream)
{
    // emit: one thread per primitive (at least one workgroup, which also pads [total, capacity) and raises the status)
    const unsigned g_emit = (unsigned)((std::max<long long>(n, 1) + 255) / 256);
    hipLaunchKernelGGL(k_tile_emit<Key>, dim3(g_emit), dim3(256), 0, stream, depth, depth_stride, (const int4 *)l.box,
                       (const long long *)l.offs, n, l.tiles_x, l.n_tiles(), (const long long *)l.total, capacity, l.keys0,
                       l.vals0, status);
    VP_HIP(hipGetLastError());
    if (capacity > 0) {
        size_t tmp = l.sort_bytes;
        VP_HIP(rocprim::radix_sort_pairs(l.sort_tmp, tmp, l.keys0, l.keys1, l.vals0, l.vals1, (size_t)capacity, 0u,
                                         (unsigned)l.end_bit, stream));
    }
    VP_HIP(hipMemsetAsync(l.ranges, 0, (size_t)l.n_tiles() * sizeof(longlong2), stream));
    if (capacity > 0) {
        hipLaunchKernelGGL(k_tile_ranges<Key>, dim3((unsigned)((capacity + 255) / 256)), dim3(256), 0, stream,
                           (const Key *)l.keys1, (const long long *)l.total, capacity, l.ranges);
        VP_HIP(hipGetLastError());
    }
    return VP_OK;
}

}  // namespace

// Mean pyramid kernel for gfx950: levels k+1 ... k+n of the OME-Zarr multiscale image from ONE read of level k.
//
// Restates generate_pyramid_levels -> downsample_block of the reference's zarr_stitcher.py:614-719 (and generate_pyramid,
// stitcher_process.py:1583-1602): every level is da.coarsen(np.mean, level, {y: 2, x: 2}, trim_excess=True) of the STORED
// level before, assigned into an integer array of the input dtype (the float64 mean of four integers is exact, the cast
// truncates):
//
//     L(l+1)[y][x] = (L(l)[2y][2x] + L(l)[2y][2x+1] + L(l)[2y+1][2x] + L(l)[2y+1][2x+1]) >> 2,
//     L(l+1) is (H_l / 2) x (W_l / 2)   (floor: a trailing odd row / column is dropped).
//
// Level shapes halve rounding down, so voxel (y, x) of level l depends only on the 2^l x 2^l block of level 0 at
// (y << l, x << l), which always lies inside level 0: a workgroup that holds a 32-row strip of the source can produce its part
// of five levels without seeing any other part of the image.
//
// Roofline: HBM.  Algorithmic traffic: the source once (1) + the levels written (1/4 + 1/16 + ... < 1/3) = 1.33 x the source
// bytes; the per-level chain reads every level it wrote again (1.67 x).
//
// Mapping: a workgroup (4 waves) owns a tile of 32 source rows x TILE_BYTES of a source row, grid-stride over (plane, strip,
// column tile).  Every lane loads 16 bytes (at whatever 2-byte phase the row has) from both rows of a row pair, all loads of the
// tile in flight at once; the horizontal pair sums are (d & 0xffff) + (d >> 16) per dword (17 bits), the vertical add makes 18,
// >> 2 gives level k+1, which goes to LDS.  Levels k+2 ... k+n are 1/16 of the data and are reduced LDS -> LDS.  Then every
// level's rows of the tile leave LDS: the stores of a row start on a 16-byte boundary of the destination (its pitch is
// arbitrary, so the boundary differs from row to row: the aligned vectors are cut from LDS dwords with v_alignbyte_b32); the few
// elements before and after the aligned body go out one by one.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "device_util.h"

using namespace sq;

namespace {

struct __attribute__((packed)) U32x4U {
    u32x4 v;
};

constexpr int MAX_LEVELS = SQ_PYRAMID_MEAN_MAX_LEVELS;   // levels per launch
constexpr int STRIP_ROWS = 1 << MAX_LEVELS;              // source rows of a tile
constexpr int TILE_BYTES = 2048;                         // bytes of a source row per tile
constexpr int THREADS = 256;
constexpr int ROW_VECS = TILE_BYTES / 16;                               // 16-byte vectors per source row of a tile
constexpr int LOADS = (STRIP_ROWS / 2) * ROW_VECS / THREADS;            // row pairs per thread
static_assert(THREADS % ROW_VECS == 0 && (STRIP_ROWS / 2) * ROW_VECS % THREADS == 0, "tile / workgroup shape");

// LDS: level j (1-based, relative to the source) of the tile has (STRIP_ROWS >> j) rows of (TILE_BYTES >> j) bytes
__host__ __device__ constexpr int lds_row_bytes(int j) { return TILE_BYTES >> j; }
__host__ __device__ constexpr int lds_level_offset(int j) {   // bytes; 16 spare bytes behind every level (the write-out reads a dword ahead)
    int off = 0;
    for (int i = 1; i < j; ++i) off += (STRIP_ROWS >> i) * (TILE_BYTES >> i) + 16;
    return off;
}
constexpr int LDS_BYTES = lds_level_offset(MAX_LEVELS + 1);

struct MeanArgs {
    const void *src;
    int64_t src_plane_stride, src_pitch;   // elements
    int32_t src_h, src_w;
    int32_t n_levels;                      // 1 .. MAX_LEVELS, none of them empty
    int32_t tiles_x;
    int64_t strips, n_tiles;               // n_tiles = n_planes * strips * tiles_x
    void *dst[MAX_LEVELS];
    int64_t dst_plane_stride[MAX_LEVELS], dst_pitch[MAX_LEVELS];
};

// Pair sums along x of one dword: uint16 -> one 17-bit sum; uint8 -> two 9-bit sums in the 16-bit halves.
template <typename T>
__device__ __forceinline__ uint32_t hsum(uint32_t d);
template <>
__device__ __forceinline__ uint32_t hsum<uint16_t>(uint32_t d) {
    return (d & 0xffffu) + (d >> 16);
}
template <>
__device__ __forceinline__ uint32_t hsum<uint8_t>(uint32_t d) {
    return (d & 0x00ff00ffu) + ((d >> 8) & 0x00ff00ffu);
}

// One dword of the next level from 8 bytes of each row of a row pair (a = upper row, b = lower row).
template <typename T>
__device__ __forceinline__ uint32_t mean2x2(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1);
template <>
__device__ __forceinline__ uint32_t mean2x2<uint16_t>(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {
    const uint32_t lo = (hsum<uint16_t>(a0) + hsum<uint16_t>(b0)) >> 2;   // 18-bit sum
    const uint32_t hi = (hsum<uint16_t>(a1) + hsum<uint16_t>(b1)) >> 2;
    return lo | (hi << 16);
}
template <>
__device__ __forceinline__ uint32_t mean2x2<uint8_t>(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {
    const uint32_t lo = ((hsum<uint8_t>(a0) + hsum<uint8_t>(b0)) >> 2) & 0x00ff00ffu;   // two 10-bit sums
    const uint32_t hi = ((hsum<uint8_t>(a1) + hsum<uint8_t>(b1)) >> 2) & 0x00ff00ffu;
    return ((lo | (lo >> 8)) & 0xffffu) | ((hi | (hi >> 8)) << 16);
}

// 16 bytes of a source row starting at element ``col``; elements at or past ``w`` read as 0 (they only reach outputs that
// are not written).
template <typename T>
__device__ __forceinline__ u32x4 load_edge(const T *row, int col, int w) {
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr int PER = 4 / (int)sizeof(T);
    u32x4 v = {0u, 0u, 0u, 0u};
    for (int e = 0; e < VEC; ++e)
        if (col + e < w) v[e / PER] |= (uint32_t)(*(const SQ_GLOBAL T *)(row + col + e)) << (8 * (int)sizeof(T) * (e % PER));
    return v;
}

// Rows [0, rows) x elements [0, cols) of one level of the tile: LDS -> destination.  One wave per row and step; lane l takes the
// l-th aligned 16-byte vector of the row.
template <typename T>
__device__ __forceinline__ void write_level(const uint8_t *lds, int row_bytes, T *dst, int64_t pitch, int rows, int cols) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < rows; r += THREADS / 64) {
        const uint8_t *lrow = lds + r * row_bytes;
        T *drow = dst + (int64_t)r * pitch;
        const int mis = (int)((reinterpret_cast<uintptr_t>(drow) / sizeof(T)) & (VEC - 1));
        const int lead = min(cols, (VEC - mis) & (VEC - 1));
        const int n_vec = (cols - lead) / VEC;
        const int tail0 = lead + n_vec * VEC;
        if (lane < lead) drow[lane] = reinterpret_cast<const T *>(lrow)[lane];
        if (lane < cols - tail0) drow[tail0 + lane] = reinterpret_cast<const T *>(lrow)[tail0 + lane];
        const int lead_bytes = lead * (int)sizeof(T);
        const uint32_t shift = (uint32_t)(lead_bytes & 3);
        const uint32_t *lw = reinterpret_cast<const uint32_t *>(lrow) + (lead_bytes >> 2);
        for (int v = lane; v < n_vec; v += 64) {
            const uint32_t *p = lw + v * 4;
            const uint32_t w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3], w4 = p[4];
            u32x4 o;
            o[0] = __builtin_amdgcn_alignbyte(w1, w0, shift);
            o[1] = __builtin_amdgcn_alignbyte(w2, w1, shift);
            o[2] = __builtin_amdgcn_alignbyte(w3, w2, shift);
            o[3] = __builtin_amdgcn_alignbyte(w4, w3, shift);
            __builtin_nontemporal_store(o, (SQ_GLOBAL u32x4 *)(drow + lead + v * VEC));
        }
    }
}

template <typename T>
__global__ __launch_bounds__(THREADS) void pyramid_mean_kernel(const MeanArgs a) {
    constexpr int VEC = 16 / (int)sizeof(T);            // source elements per 16-byte vector
    constexpr int TILE_W = TILE_BYTES / (int)sizeof(T);  // source elements per tile row
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDS_BYTES];
    const int tid = threadIdx.x;
    const int vec = tid % ROW_VECS;          // this thread's vector of the tile row
    const int rp0 = tid / ROW_VECS;          // ... and its first row pair; the others follow THREADS / ROW_VECS apart
    const T *src = static_cast<const T *>(a.src);
    for (int64_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        const int tx = (int)(t % a.tiles_x);
        const int64_t ps = t / a.tiles_x;
        const int64_t plane = ps / a.strips;
        const int y0 = (int)(ps - plane * a.strips) * STRIP_ROWS;
        const int x0 = tx * TILE_W;
        // ---- level 1 of the tile from the source, through registers
        {
            const T *sp = src + plane * a.src_plane_stride + (int64_t)y0 * a.src_pitch;
            const int col = x0 + vec * VEC;
            const bool whole = col + VEC <= a.src_w;
            u32x4 ra[LOADS], rb[LOADS];
#pragma unroll
            for (int i = 0; i < LOADS; ++i) {
                const int row = 2 * (rp0 + i * (THREADS / ROW_VECS));
                ra[i] = rb[i] = u32x4{0u, 0u, 0u, 0u};
                if (whole && y0 + row + 1 < a.src_h) {
                    const T *p = sp + (int64_t)row * a.src_pitch + col;
                    ra[i] = ((const SQ_GLOBAL U32x4U *)p)->v;
                    rb[i] = ((const SQ_GLOBAL U32x4U *)(p + a.src_pitch))->v;
                }
            }
            if (!whole && col < a.src_w) {   // the vector the row ends in: element by element
                for (int i = 0; i < LOADS; ++i) {
                    const int row = 2 * (rp0 + i * (THREADS / ROW_VECS));
                    if (y0 + row + 1 < a.src_h) {
                        const T *p = sp + (int64_t)row * a.src_pitch;
                        const u32x4 ea = load_edge<T>(p, col, a.src_w), eb = load_edge<T>(p + a.src_pitch, col, a.src_w);
                        u32x2 o;
                        o[0] = mean2x2<T>(ea[0], ea[1], eb[0], eb[1]);
                        o[1] = mean2x2<T>(ea[2], ea[3], eb[2], eb[3]);
                        *reinterpret_cast<u32x2 *>(lds + (row / 2) * lds_row_bytes(1) + vec * 8) = o;
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < LOADS; ++i) {
                    const int rp = rp0 + i * (THREADS / ROW_VECS);
                    u32x2 o;
                    o[0] = mean2x2<T>(ra[i][0], ra[i][1], rb[i][0], rb[i][1]);
                    o[1] = mean2x2<T>(ra[i][2], ra[i][3], rb[i][2], rb[i][3]);
                    *reinterpret_cast<u32x2 *>(lds + rp * lds_row_bytes(1) + vec * 8) = o;
                }
            }
        }
        __syncthreads();
        // ---- levels 2 ... n, LDS -> LDS: one dword out of 8 bytes of each row of a row pair
#pragma unroll
        for (int j = 2; j <= MAX_LEVELS; ++j) {
            if (j <= a.n_levels) {
                const uint8_t *in = lds + lds_level_offset(j - 1);
                uint8_t *out = lds + lds_level_offset(j);
                const int row_dwords = lds_row_bytes(j) / 4;
                const int n = (STRIP_ROWS >> j) * row_dwords;
                for (int i = tid; i < n; i += THREADS) {
                    const int r = i / row_dwords, c = i - r * row_dwords;
                    const u32x2 ua = *reinterpret_cast<const u32x2 *>(in + (2 * r) * lds_row_bytes(j - 1) + c * 8);
                    const u32x2 ub = *reinterpret_cast<const u32x2 *>(in + (2 * r + 1) * lds_row_bytes(j - 1) + c * 8);
                    *reinterpret_cast<uint32_t *>(out + r * lds_row_bytes(j) + c * 4) = mean2x2<T>(ua[0], ua[1], ub[0], ub[1]);
                }
                __syncthreads();
            }
        }
        // ---- every level's part of the tile: LDS -> destination
#pragma unroll
        for (int j = 1; j <= MAX_LEVELS; ++j) {
            if (j <= a.n_levels) {
                const int yj = y0 >> j, xj = x0 >> j;
                const int rows = min(STRIP_ROWS >> j, (a.src_h >> j) - yj);
                const int cols = min(TILE_W >> j, (a.src_w >> j) - xj);
                if (rows > 0 && cols > 0) {
                    T *dp = static_cast<T *>(a.dst[j - 1]) + plane * a.dst_plane_stride[j - 1] +
                            (int64_t)yj * a.dst_pitch[j - 1] + xj;
                    write_level<T>(lds + lds_level_offset(j), lds_row_bytes(j), dp, a.dst_pitch[j - 1], rows, cols);
                }
            }
        }
        __syncthreads();   // the next tile's level 1 overwrites what the write-out has just read
    }
}

}   // namespace

// One launch: levels 1 ... n (n <= MAX_LEVELS, none empty) of [n_planes, h, w].
static int launch_mean(const void *src, int64_t sps, int32_t h, int32_t w, int64_t spitch, void *const *dst, const int64_t *dps,
                       const int64_t *dpitch, int32_t n, int32_t n_planes, int32_t dtype, hipStream_t stream) {
    MeanArgs a{};
    a.src = src;
    a.src_plane_stride = sps;
    a.src_pitch = spitch;
    a.src_h = h;
    a.src_w = w;
    a.n_levels = n;
    const int tile_w = TILE_BYTES / (dtype == SQ_U16 ? 2 : 1);
    // only whole row pairs / column pairs reach level 1: a trailing odd row or column is not even read
    a.tiles_x = ((w & ~1) + tile_w - 1) / tile_w;
    a.strips = ((h & ~1) + STRIP_ROWS - 1) / STRIP_ROWS;
    a.n_tiles = (int64_t)n_planes * a.strips * a.tiles_x;
    for (int j = 0; j < n; ++j) {
        a.dst[j] = dst[j];
        a.dst_plane_stride[j] = dps[j];
        a.dst_pitch[j] = dpitch[j];
    }
    // enough workgroups to fill 256 CUs several times over; the grid stride covers the rest
    const int64_t blocks = std::min<int64_t>(a.n_tiles, 256 * 64);
    if (dtype == SQ_U16)
        pyramid_mean_kernel<uint16_t><<<dim3((unsigned)blocks), dim3(THREADS), 0, stream>>>(a);
    else
        pyramid_mean_kernel<uint8_t><<<dim3((unsigned)blocks), dim3(THREADS), 0, stream>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SQ_ERR_HIP, "sq_pyramid_mean: launch failed: %s", hipGetErrorString(e));
    return SQ_OK;
}

extern "C" int sq_pyramid_mean(const void *src_dev, int64_t src_plane_stride, int32_t src_h, int32_t src_w, int64_t src_pitch,
                               void *const *dst_dev, const int64_t *dst_plane_stride, const int64_t *dst_pitch,
                               int32_t n_levels, int32_t n_planes, int32_t dtype, void *stream_) {
    if (n_planes < 0 || src_h < 0 || src_w < 0 || src_pitch < src_w || n_levels < 0 || n_levels > 31)
        return fail(SQ_ERR_INVALID, "sq_pyramid_mean: bad sizes (planes=%d src=%dx%d pitch %lld levels=%d)", n_planes, src_h, src_w,
                    (long long)src_pitch, n_levels);
    if (dtype != SQ_U8 && dtype != SQ_U16) return fail(SQ_ERR_UNSUPPORTED, "sq_pyramid_mean: dtype %d", dtype);
    // levels that exist: level l is (src_h >> l) x (src_w >> l); the first empty one ends the pyramid
    int32_t n = 0;
    while (n < n_levels && (src_h >> (n + 1)) > 0 && (src_w >> (n + 1)) > 0) ++n;
    if (n == 0 || n_planes == 0) return SQ_OK;
    if (!src_dev || !dst_dev || !dst_plane_stride || !dst_pitch) return fail(SQ_ERR_INVALID, "sq_pyramid_mean: NULL buffer");
    if (n_planes > 1 && src_plane_stride < (int64_t)src_h * src_pitch)
        return fail(SQ_ERR_INVALID, "sq_pyramid_mean: source plane stride smaller than a plane");
    for (int32_t l = 0; l < n; ++l) {
        const int32_t lh = src_h >> (l + 1), lw = src_w >> (l + 1);
        if (!dst_dev[l]) return fail(SQ_ERR_INVALID, "sq_pyramid_mean: NULL buffer for level %d", l + 1);
        if (dst_pitch[l] < lw || (n_planes > 1 && dst_plane_stride[l] < (int64_t)lh * dst_pitch[l]))
            return fail(SQ_ERR_INVALID, "sq_pyramid_mean: level %d (%dx%d): pitch %lld / plane stride %lld too small", l + 1, lh, lw,
                        (long long)dst_pitch[l], (long long)dst_plane_stride[l]);
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // the definition composes: what one launch does not reach is made by the next launch from the last level written
    const void *src = src_dev;
    int64_t sps = src_plane_stride, spitch = src_pitch;
    int32_t h = src_h, w = src_w;
    for (int32_t l0 = 0; l0 < n; l0 += MAX_LEVELS) {
        const int32_t m = std::min<int32_t>(MAX_LEVELS, n - l0);
        const int rc = launch_mean(src, sps, h, w, spitch, dst_dev + l0, dst_plane_stride + l0, dst_pitch + l0, m, n_planes, dtype,
                                   stream);
        if (rc != SQ_OK) return rc;
        src = dst_dev[l0 + m - 1];
        sps = dst_plane_stride[l0 + m - 1];
        spitch = dst_pitch[l0 + m - 1];
        h >>= m;
        w >>= m;
    }
    return SQ_OK;
}

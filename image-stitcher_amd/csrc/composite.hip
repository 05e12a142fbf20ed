// The two kernels behind --composite (a colour quick-look PNG of every region) for gfx950:
//
//   sq_block_mean        n planes [H, W] -> n planes [ceil(H / f), ceil(W / f)], f = 2^k, k = 0 ... 8:
//                            M[Y][X] = floor(sum of the block's pixels that exist / their number)
//                        (a partial block at the bottom / right edge averages what is there; k = 0 is the identity)
//   sq_composite_render  n <= 16 such planes, a window (a, b) and a colour 0xRRGGBB each -> interleaved RGB8 [h, w, 3]:
//                            v_c = 0 where M <= a, 255 where M >= b, else floor((M - a) * 255 / (b - a))
//                            out[j] = min(255, sum_c floor(v_c * colour_c[j] / 255))
//
// They replace the reference's _save_debug_slice (stitcher.py:861-885), which min/max-normalises the first three channels of a
// host copy of the whole stack.  Integers only; the definition is the numpy restatement in tests/composite_ref.py.
//
// sq_block_mean is the hot one.  Roofline: HBM, one read of the source (the means are 4^-k of it).  Mapping: the unit of work is
// a WAVE, not a workgroup -- a task is max(f, 4) source rows x 64 lanes x 16 bytes of a row, the tasks of a plane are dealt to
// the waves in row-major order (neighbouring waves read neighbouring kilobytes of the same rows).  A lane loads 16 bytes (at
// whatever phase the row has) from 4 or 8 rows at once, sums along x inside its vector with v_sad_u8 / v_sad_u16, along y in
// 32-bit registers (65535 * 256 * 256 < 2^32), and -- from f = 16 (uint16) / 32 (uint8) up, where a block is wider than a
// lane's vector -- across the f / VEC neighbouring lanes with a butterfly.  No LDS, no barrier, no atomics, no scratch buffer:
// every mean is written once, by one lane, from one fixed order of additions.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "device_util.h"

using namespace sq;

namespace {

struct __attribute__((packed)) U32x4U {
    u32x4 v;
};

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_K = 8;
constexpr int MAX_RENDER_PLANES = 16;

struct MeanArgs {
    const void *src;
    int64_t src_plane_stride, src_pitch;   // elements
    int32_t w;                             // source columns
    int32_t y_begin, y_end;                // source rows [y_begin, y_end), y_begin a multiple of f
    int32_t tiles_x;
    uint32_t n_tasks;                      // per plane: task rows * tiles_x
    void *dst;
    int64_t dst_plane_stride, dst_pitch;   // elements
    int32_t w_out;
};

// 16 bytes of a source row starting at element ``col``; elements at or past ``w`` read as 0 (zeros add nothing to a sum).
template <typename T>
__device__ __forceinline__ u32x4 load_edge(const T *row, int col, int w) {
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr int PER = 4 / (int)sizeof(T);
    u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < VEC; ++e)
        if (col + e < w) v[e / PER] |= (uint32_t)(*(const SQ_GLOBAL T *)(row + col + e)) << (8 * (int)sizeof(T) * (e % PER));
    return v;
}

// acc[j] += the sum of elements [j * G, (j + 1) * G) of the vector, j < VEC / G (G = elements of a lane's vector per block)
template <typename T, int G>
__device__ __forceinline__ void add_vector(const u32x4 d, uint32_t *acc) {
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr int PER = 4 / (int)sizeof(T);
    constexpr int BITS = 8 * (int)sizeof(T);
    if constexpr (G >= PER) {      // whole dwords go to one block: |x - 0| summed over the dword's elements, one instruction
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t &a = acc[i * PER / G];
            if constexpr (sizeof(T) == 1)
                a = __builtin_amdgcn_sad_u8(d[i], 0u, a);
            else
                a = __builtin_amdgcn_sad_u16(d[i], 0u, a);
        }
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e / G] += (d[e / PER] >> (BITS * (e % PER))) & ((1u << BITS) - 1u);
    }
}

// NOUT consecutive means of one destination row: one vector store when the address allows it, else element by element
template <typename T, int NOUT>
__device__ __forceinline__ void store_means(T *dp, const uint32_t *v, int n_valid) {
    constexpr int BYTES = NOUT * (int)sizeof(T);
    constexpr int PER = 4 / (int)sizeof(T);
    constexpr int BITS = 8 * (int)sizeof(T);
    if constexpr (BYTES >= 4) {
        if (n_valid == NOUT && (reinterpret_cast<uintptr_t>(dp) & (BYTES - 1)) == 0) {
            uint32_t o[BYTES / 4];
#pragma unroll
            for (int i = 0; i < BYTES / 4; ++i) {
                o[i] = 0u;
#pragma unroll
                for (int e = 0; e < PER; ++e) o[i] |= v[i * PER + e] << (BITS * e);
            }
            if constexpr (BYTES == 16)
                *(SQ_GLOBAL u32x4 *)dp = u32x4{o[0], o[1], o[2], o[3]};
            else if constexpr (BYTES == 8)
                *(SQ_GLOBAL u32x2 *)dp = u32x2{o[0], o[1]};
            else
                *(SQ_GLOBAL uint32_t *)dp = o[0];
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < NOUT; ++j)
        if (j < n_valid) *(SQ_GLOBAL T *)(dp + j) = (T)v[j];
}

template <typename T, int K>
__global__ __launch_bounds__(THREADS) void block_mean_kernel(const MeanArgs a) {
    constexpr int VEC = 16 / (int)sizeof(T);          // source elements of a lane's vector
    constexpr int F = 1 << K;
    constexpr int ROWS = F > 4 ? F : 4;               // source rows of a task
    constexpr int LOADS = F >= 8 ? 8 : 4;             // 16-byte loads of a lane in flight
    constexpr int OUT_ROWS = ROWS / F;                // destination rows of a task (4, 2, 1, 1, ...)
    constexpr int G = F < VEC ? F : VEC;              // elements of a vector that belong to one block
    constexpr int NOUT = VEC / G;                     // blocks a vector spans along x
    constexpr int LPG = F > VEC ? F / VEC : 1;        // lanes that share one block along x
    constexpr int TILE_W = 64 * VEC;                  // source elements of a task row
    static_assert(OUT_ROWS == 1 || ROWS == LOADS, "several destination rows: one step of loads");
    static_assert(LPG <= 32 && K <= MAX_K, "a block lies inside one wave's kilobyte");

    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t plane = blockIdx.y;
    const T *src = static_cast<const T *>(a.src) + plane * a.src_plane_stride;
    T *dst = static_cast<T *>(a.dst) + plane * a.dst_plane_stride;
    for (uint32_t t = blockIdx.x * WAVES + wave; t < a.n_tasks; t += gridDim.x * WAVES) {
        const uint32_t ty = t / (uint32_t)a.tiles_x, tx = t - ty * (uint32_t)a.tiles_x;
        const int y0 = a.y_begin + (int)ty * ROWS;
        const int col = (int)tx * TILE_W + lane * VEC;
        const bool whole = col + VEC <= a.w;
        uint32_t acc[OUT_ROWS][NOUT];
#pragma unroll
        for (int o = 0; o < OUT_ROWS; ++o)
#pragma unroll
            for (int j = 0; j < NOUT; ++j) acc[o][j] = 0u;
        const T *rp0 = src + (int64_t)y0 * a.src_pitch;
#pragma unroll 1
        for (int s = 0; s < ROWS; s += LOADS) {
            u32x4 d[LOADS];
#pragma unroll
            for (int i = 0; i < LOADS; ++i) {
                d[i] = u32x4{0u, 0u, 0u, 0u};
                if (whole && y0 + s + i < a.y_end) d[i] = ((const SQ_GLOBAL U32x4U *)(rp0 + (int64_t)(s + i) * a.src_pitch + col))->v;
            }
            if (!whole && col < a.w) {   // the vector the row ends in: element by element
#pragma unroll
                for (int i = 0; i < LOADS; ++i)
                    if (y0 + s + i < a.y_end) d[i] = load_edge<T>(rp0 + (int64_t)(s + i) * a.src_pitch, col, a.w);
            }
#pragma unroll
            for (int i = 0; i < LOADS; ++i) add_vector<T, G>(d[i], acc[OUT_ROWS > 1 ? i / F : 0]);
        }
        if constexpr (LPG > 1) {   // the block's other lanes (every lane of the wave is here: nothing above leaves the loop)
#pragma unroll
            for (int m = 1; m < LPG; m <<= 1) acc[0][0] += (uint32_t)__shfl_xor((int)acc[0][0], m, 64);
        }
        const int x_out = (col >> K);      // this lane's first block
        if ((lane & (LPG - 1)) == 0 && x_out < a.w_out) {
            const int n_valid = min(NOUT, a.w_out - x_out);
#pragma unroll
            for (int o = 0; o < OUT_ROWS; ++o) {
                const int yb = y0 + o * F;
                if (yb < a.y_end) {
                    const uint32_t n_rows = (uint32_t)min(F, a.y_end - yb);
                    uint32_t v[NOUT];
#pragma unroll
                    for (int j = 0; j < NOUT; ++j) {
                        const uint32_t n_cols = (uint32_t)max(1, min(F, a.w - ((x_out + j) << K)));
                        const uint32_t count = n_rows * n_cols;
                        v[j] = count == (uint32_t)(F * F) ? acc[o][j] >> (2 * K) : acc[o][j] / count;
                    }
                    store_means<T, NOUT>(dst + (int64_t)(yb >> K) * a.dst_pitch + x_out, v, n_valid);
                }
            }
        }
    }
}

template <typename T, int K>
void launch_mean(const MeanArgs &a, int32_t n_planes, hipStream_t stream) {
    // enough workgroups to fill 256 CUs eight waves deep; the grid stride covers the rest
    const uint32_t blocks_x = std::max<uint32_t>(1u, std::min<uint32_t>((a.n_tasks + WAVES - 1) / WAVES,
                                                                          (uint32_t)std::max(1, 2048 / std::min(n_planes, 8))));
    block_mean_kernel<T, K><<<dim3(blocks_x, (unsigned)n_planes), dim3(THREADS), 0, stream>>>(a);
}

template <typename T>
void dispatch_mean(int k, const MeanArgs &a, int32_t n_planes, hipStream_t stream) {
    switch (k) {
        case 0: launch_mean<T, 0>(a, n_planes, stream); break;
        case 1: launch_mean<T, 1>(a, n_planes, stream); break;
        case 2: launch_mean<T, 2>(a, n_planes, stream); break;
        case 3: launch_mean<T, 3>(a, n_planes, stream); break;
        case 4: launch_mean<T, 4>(a, n_planes, stream); break;
        case 5: launch_mean<T, 5>(a, n_planes, stream); break;
        case 6: launch_mean<T, 6>(a, n_planes, stream); break;
        case 7: launch_mean<T, 7>(a, n_planes, stream); break;
        default: launch_mean<T, 8>(a, n_planes, stream); break;
    }
}

struct RenderArgs {
    const void *src;
    int64_t plane_stride, pitch;   // elements
    int32_t h, w, n;
    uint8_t *dst;
    int64_t dst_pitch;             // bytes
    int32_t lo[MAX_RENDER_PLANES], hi[MAX_RENDER_PLANES];
    uint32_t color[MAX_RENDER_PLANES];
};

template <typename T>
__global__ __launch_bounds__(THREADS) void composite_render_kernel(const RenderArgs a) {
    const int x = blockIdx.x * THREADS + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= a.w) return;
    const T *sp = static_cast<const T *>(a.src) + (int64_t)y * a.pitch + x;
    uint32_t r = 0, g = 0, b = 0;
    for (int c = 0; c < a.n; ++c) {
        const int32_t m = (int32_t)(*(const SQ_GLOBAL T *)(sp + c * a.plane_stride));
        const int32_t lo = a.lo[c], hi = a.hi[c];
        const uint32_t v = m <= lo ? 0u : (m >= hi ? 255u : (uint32_t)(m - lo) * 255u / (uint32_t)(hi - lo));
        const uint32_t col = a.color[c];
        r += v * ((col >> 16) & 0xffu) / 255u;
        g += v * ((col >> 8) & 0xffu) / 255u;
        b += v * (col & 0xffu) / 255u;
    }
    uint8_t *dp = a.dst + (int64_t)y * a.dst_pitch + 3 * (int64_t)x;
    dp[0] = (uint8_t)min(r, 255u);
    dp[1] = (uint8_t)min(g, 255u);
    dp[2] = (uint8_t)min(b, 255u);
}

}   // namespace

extern "C" int sq_block_mean(const void *planes_dev, int64_t plane_stride, int32_t h, int32_t w, int64_t pitch, int32_t n_planes,
                             int32_t dtype, int32_t k, int32_t row0, int32_t n_rows, void *dst_dev, int64_t dst_plane_stride,
                             int64_t dst_pitch, void *stream_) {
    if (dtype != SQ_U8 && dtype != SQ_U16) return fail(SQ_ERR_UNSUPPORTED, "sq_block_mean: dtype %d", dtype);
    if (k < 0 || k > MAX_K) return fail(SQ_ERR_INVALID, "sq_block_mean: k = %d is outside 0..%d", k, MAX_K);
    if (n_planes < 0 || n_planes > 65535 || h <= 0 || w <= 0 || h > (1 << 30) || w > (1 << 30) || pitch < w)
        return fail(SQ_ERR_INVALID, "sq_block_mean: bad sizes (planes=%d %dx%d pitch %lld)", n_planes, h, w, (long long)pitch);
    const int32_t f = 1 << k;
    if (row0 < 0 || n_rows < 0 || (int64_t)row0 + n_rows > h || row0 % f || (n_rows % f && row0 + n_rows != h))
        return fail(SQ_ERR_INVALID, "sq_block_mean: rows %d + %d of %d: a band starts on a multiple of %d and is a multiple of it "
                    "long, or runs to the last row", row0, n_rows, h, f);
    if (n_planes == 0 || n_rows == 0) return SQ_OK;
    const int32_t w_out = (w + f - 1) >> k, h_out = (h + f - 1) >> k;
    if (!planes_dev || !dst_dev) return fail(SQ_ERR_INVALID, "sq_block_mean: NULL buffer");
    if (dst_pitch < w_out || (n_planes > 1 && (plane_stride < (int64_t)h * pitch || dst_plane_stride < (int64_t)h_out * dst_pitch)))
        return fail(SQ_ERR_INVALID, "sq_block_mean: pitch / plane stride smaller than a row / plane");
    const int esize = dtype == SQ_U16 ? 2 : 1;
    if (reinterpret_cast<uintptr_t>(planes_dev) % esize || reinterpret_cast<uintptr_t>(dst_dev) % esize)
        return fail(SQ_ERR_INVALID, "sq_block_mean: buffers must be aligned to their element");
    MeanArgs a{};
    a.src = planes_dev;
    a.src_plane_stride = plane_stride;
    a.src_pitch = pitch;
    a.w = w;
    a.y_begin = row0;
    a.y_end = row0 + n_rows;
    const int32_t rows = std::max(f, 4), tile_w = 64 * (16 / esize);
    a.tiles_x = (w + tile_w - 1) / tile_w;
    const int64_t n_tasks = (int64_t)((n_rows + rows - 1) / rows) * a.tiles_x;
    if (n_tasks >= (1ll << 31)) return fail(SQ_ERR_UNSUPPORTED, "sq_block_mean: %lld tasks per plane", (long long)n_tasks);
    a.n_tasks = (uint32_t)n_tasks;
    a.dst = dst_dev;
    a.dst_plane_stride = dst_plane_stride;
    a.dst_pitch = dst_pitch;
    a.w_out = w_out;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (dtype == SQ_U16)
        dispatch_mean<uint16_t>(k, a, n_planes, stream);
    else
        dispatch_mean<uint8_t>(k, a, n_planes, stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SQ_ERR_HIP, "sq_block_mean: launch failed: %s", hipGetErrorString(e));
    return SQ_OK;
}

extern "C" int sq_composite_render(const void *means_dev, int64_t plane_stride, int32_t h, int32_t w, int64_t pitch,
                                   int32_t n_planes, int32_t dtype, const int32_t *windows, const uint32_t *colors,
                                   uint8_t *rgb_dev, int64_t rgb_pitch, void *stream_) {
    if (dtype != SQ_U8 && dtype != SQ_U16) return fail(SQ_ERR_UNSUPPORTED, "sq_composite_render: dtype %d", dtype);
    if (n_planes < 1 || n_planes > MAX_RENDER_PLANES)
        return fail(SQ_ERR_INVALID, "sq_composite_render: %d planes (1..%d)", n_planes, MAX_RENDER_PLANES);
    if (h <= 0 || w <= 0 || h > 65535 || w > (1 << 30) || pitch < w || rgb_pitch < 3 * (int64_t)w ||
        (n_planes > 1 && plane_stride < (int64_t)h * pitch))
        return fail(SQ_ERR_INVALID, "sq_composite_render: bad sizes (%dx%d pitch %lld, rgb pitch %lld)", h, w, (long long)pitch,
                    (long long)rgb_pitch);
    if (!means_dev || !windows || !colors || !rgb_dev) return fail(SQ_ERR_INVALID, "sq_composite_render: NULL buffer");
    if (reinterpret_cast<uintptr_t>(means_dev) % (dtype == SQ_U16 ? 2 : 1))
        return fail(SQ_ERR_INVALID, "sq_composite_render: planes must be aligned to their element");
    RenderArgs a{};
    a.src = means_dev;
    a.plane_stride = plane_stride;
    a.pitch = pitch;
    a.h = h;
    a.w = w;
    a.n = n_planes;
    a.dst = rgb_dev;
    a.dst_pitch = rgb_pitch;
    for (int32_t c = 0; c < n_planes; ++c) {
        a.lo[c] = windows[2 * c];
        a.hi[c] = windows[2 * c + 1];
        a.color[c] = colors[c] & 0xffffffu;
        if (a.lo[c] < 0 || a.hi[c] <= a.lo[c] || a.hi[c] > 65535)
            return fail(SQ_ERR_INVALID, "sq_composite_render: window %d = (%d, %d): 0 <= start < end <= 65535", c, a.lo[c], a.hi[c]);
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid((unsigned)((w + THREADS - 1) / THREADS), (unsigned)h);
    if (dtype == SQ_U16)
        composite_render_kernel<uint16_t><<<grid, dim3(THREADS), 0, stream>>>(a);
    else
        composite_render_kernel<uint8_t><<<grid, dim3(THREADS), 0, stream>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SQ_ERR_HIP, "sq_composite_render: launch failed: %s", hipGetErrorString(e));
    return SQ_OK;
}

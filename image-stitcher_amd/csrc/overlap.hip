// Overlap moments of window pairs: the exact integer sums a zero-normalised cross-correlation is formed from.
//
// Global registration (alignment.py) has to tell a pair whose phase correlation found the true offset from one that
// returned a "shift" on a blank or featureless field; skimage's error term cannot (it compares the normalised peak
// with the un-normalised amplitudes).  The host forms ncc = (n Sab - Sa Sb) / sqrt((n Saa - Sa^2)(n Sbb - Sb^2)) from
// the five sums below, for the overlap of the two FULL tiles at each pair's measured offset.
//
// One workgroup takes one band of rows of one window pair (blockIdx.y = pair, blockIdx.x = band); a band holds about
// BAND_PIXELS pixels whatever the window's shape, so a 2048 x 250 window spreads over ~32 workgroups and a 250 x 2048
// one too.  Each wave walks rows of the band, its lanes consecutive columns (windows start at any column: plain
// element loads, coalesced across the wave).  Sums are exact unsigned integers: per lane in 64-bit registers (a * b
// of two 16-bit pixels fits 32 bits), then across the wave with __shfl_xor, across the block through LDS, and one
// 64-bit atomic add per sum per block into an output the entry point zeroes on the same stream.  Integer addition
// is associative, so the result does not depend on the schedule: it equals numpy's int64 sums bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "common.h"

using namespace sq;

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int BAND_PIXELS = 16384;   // pixels of one window a workgroup reads (x 2 windows x 2 B: 64 KB for uint16)

__host__ __device__ inline int band_rows(int w) { return w > 0 ? std::max(1, BAND_PIXELS / w) : 1; }

__device__ inline unsigned long long wave_sum(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <typename T>
__global__ __launch_bounds__(THREADS) void overlap_moments_kernel(const void *const *tile_ptrs, const void *tile_base,
                                                                  int64_t tile_stride, int pitch, const sq_overlap *pairs,
                                                                  unsigned long long *out) {
    const sq_overlap p = pairs[blockIdx.y];
    const int rows = band_rows(p.w);
    const int r0 = (int)blockIdx.x * rows;
    if (p.w <= 0 || r0 >= p.h) return;       // uniform over the block: no barrier is skipped by part of it
    const int r1 = min(p.h, r0 + rows);
    const T *ref = tile_ptrs ? static_cast<const T *>(tile_ptrs[p.ref_tile]) : static_cast<const T *>(tile_base) + p.ref_tile * tile_stride;
    const T *mov = tile_ptrs ? static_cast<const T *>(tile_ptrs[p.mov_tile]) : static_cast<const T *>(tile_base) + p.mov_tile * tile_stride;
    ref += (int64_t)p.ref_y0 * pitch + p.ref_x0;
    mov += (int64_t)p.mov_y0 * pitch + p.mov_x0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;
    for (int r = r0 + wave; r < r1; r += WAVES) {
        const T *ra = ref + (int64_t)r * pitch;
        const T *rb = mov + (int64_t)r * pitch;
#pragma unroll 4
        for (int c = lane; c < p.w; c += 64) {
            const uint32_t a = ra[c], b = rb[c];
            sa += a;
            sb += b;
            saa += a * a;      // < 2^32 for 16-bit pixels
            sbb += b * b;
            sab += a * b;
        }
    }
    __shared__ unsigned long long part[WAVES][5];
    sa = wave_sum(sa);
    sb = wave_sum(sb);
    saa = wave_sum(saa);
    sbb = wave_sum(sbb);
    sab = wave_sum(sab);
    if (lane == 0) {
        part[wave][0] = sa;
        part[wave][1] = sb;
        part[wave][2] = saa;
        part[wave][3] = sbb;
        part[wave][4] = sab;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        unsigned long long s = 0;
        for (int w = 0; w < WAVES; ++w) s += part[w][threadIdx.x];
        if (s) atomicAdd(out + 5 * (int64_t)blockIdx.y + threadIdx.x, s);
    }
}

bool inside(int32_t y0, int32_t x0, int32_t h, int32_t w, int32_t tile_h, int32_t tile_w) {
    return y0 >= 0 && x0 >= 0 && (int64_t)y0 + h <= tile_h && (int64_t)x0 + w <= tile_w;
}

}  // namespace

extern "C" int sq_pair_overlap_moments(const void *const *tile_ptrs_dev, const void *tile_base_dev, int64_t tile_stride,
                                       int32_t n_tiles, int32_t tile_h, int32_t tile_w, int32_t tile_pitch, int32_t tile_dtype,
                                       const sq_overlap *pairs_dev, int32_t n_pairs, uint64_t *out_dev, void *stream_) {
    if ((!tile_ptrs_dev && !tile_base_dev) || n_tiles < 0 || tile_h <= 0 || tile_w <= 0 || tile_pitch < tile_w || n_pairs < 0 ||
        (n_pairs > 0 && (!pairs_dev || !out_dev)))
        return fail(SQ_ERR_INVALID, "sq_pair_overlap_moments: bad arguments (n_tiles=%d %dx%d pitch %d, n_pairs=%d)", n_tiles, tile_h,
                    tile_w, tile_pitch, n_pairs);
    if (tile_dtype != SQ_U8 && tile_dtype != SQ_U16) return fail(SQ_ERR_UNSUPPORTED, "sq_pair_overlap_moments: dtype %d", tile_dtype);
    if (n_pairs > 65535) return fail(SQ_ERR_UNSUPPORTED, "sq_pair_overlap_moments: more than 65535 window pairs per call");
    if (n_pairs == 0) return SQ_OK;
    hipStream_t s = static_cast<hipStream_t>(stream_);
    // the windows are validated on the host before anything is launched: read the table back (this synchronises `stream`)
    std::vector<sq_overlap> host(n_pairs);
    hipError_t e = hipMemcpyAsync(host.data(), pairs_dev, sizeof(sq_overlap) * n_pairs, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(SQ_ERR_HIP, "sq_pair_overlap_moments: reading the window table: %s", hipGetErrorString(e));
    int64_t bands = 1;
    for (int32_t i = 0; i < n_pairs; ++i) {
        const sq_overlap &p = host[i];
        if (p.ref_tile < 0 || p.ref_tile >= n_tiles || p.mov_tile < 0 || p.mov_tile >= n_tiles)
            return fail(SQ_ERR_INVALID, "sq_pair_overlap_moments: pair %d names tiles %d, %d of a table of %d", i, p.ref_tile,
                        p.mov_tile, n_tiles);
        if (p.h < 0 || p.w < 0 || !inside(p.ref_y0, p.ref_x0, p.h, p.w, tile_h, tile_w) ||
            !inside(p.mov_y0, p.mov_x0, p.h, p.w, tile_h, tile_w))
            return fail(SQ_ERR_INVALID, "sq_pair_overlap_moments: window %d (%d x %d at (%d, %d) / (%d, %d)) leaves its %d x %d tile", i,
                        p.h, p.w, p.ref_y0, p.ref_x0, p.mov_y0, p.mov_x0, tile_h, tile_w);
        if (p.h > 0 && p.w > 0) bands = std::max<int64_t>(bands, (p.h + band_rows(p.w) - 1) / band_rows(p.w));
    }
    e = hipMemsetAsync(out_dev, 0, sizeof(uint64_t) * 5 * (size_t)n_pairs, s);
    if (e != hipSuccess) return fail(SQ_ERR_HIP, "sq_pair_overlap_moments: zeroing the output: %s", hipGetErrorString(e));
    const dim3 grid((unsigned)bands, (unsigned)n_pairs);
    auto *out = reinterpret_cast<unsigned long long *>(out_dev);
    if (tile_dtype == SQ_U16)
        hipLaunchKernelGGL(overlap_moments_kernel<uint16_t>, grid, dim3(THREADS), 0, s, tile_ptrs_dev, tile_base_dev, tile_stride,
                           tile_pitch, pairs_dev, out);
    else
        hipLaunchKernelGGL(overlap_moments_kernel<uint8_t>, grid, dim3(THREADS), 0, s, tile_ptrs_dev, tile_base_dev, tile_stride,
                           tile_pitch, pairs_dev, out);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(SQ_ERR_HIP, "sq_pair_overlap_moments: launch failed: %s", hipGetErrorString(e));
    return SQ_OK;
}

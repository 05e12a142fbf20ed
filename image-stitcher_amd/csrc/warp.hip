// Radial lens correction of a batch of staged tile planes for gfx950, out of place (--distortion-correction):
//
//     U = w - 1, V = h - 1                          R2 = max(1, U*U + V*V)
//     for the output pixel (y, x), D in parts per million:
//       u = 2*x - U,  v = 2*y - V                   (half-pixels from the tile centre)
//       rho = ((u*u + v*v) << 24) // R2             (0 .. 2^24: squared radius, 1.0 at the corners)
//       s   = D * rho
//       du  = (u*s + H) // (2*H),  dv = (v*s + H) // (2*H),   H = 10^6 * 2^16     (1/256 pixel, rounded half up; floor division)
//       X = clamp(256*x + du, 0, 256*U),  Y = clamp(256*y + dv, 0, 256*V)          (edges replicated)
//       x0 = X >> 8, fx = X & 255, x1 = min(x0 + 1, U);   y0, fy, y1 likewise
//       out(y, x) = ( I[y0,x0]*(256-fx)*(256-fy) + I[y0,x1]*fx*(256-fy)
//                   + I[y1,x0]*(256-fx)*fy       + I[y1,x1]*fx*fy + 32768 ) >> 16
//
// The reference has no counterpart; the definition is the numpy restatement in tests/warp_ref.py.  Integers only (the map in
// 64 bits: (u*u + v*v) << 24 < 2^58 and |u*s| + 2H < 2^57 at 65535 x 65535 and |D| = 50000; the blend in unsigned 32 bits: the
// four weights add up to 2^16), no atomics, no LDS, no scratch: deterministic.  Every output element is written exactly once and
// nothing outside h x w of a destination plane is written; every tap lies inside its source plane (the clamps above).
//
// Mapping: the map (x0, y0, fx, fy) depends on the position and the plane's shape only, not on the plane, and it costs one
// 64-bit division by R2 and two by the constant 2H per position.  So a thread owns OUTS = 2 consecutive dst columns of one row,
// works their map out ONCE into registers (per column the offset of the first tap, the step to the second row, the four
// weights) and then walks over up to WALK = 16 planes of the batch (blockIdx.y = run of planes).  What bounds the launch is the
// number of tap loads, not the divisions and not the walk (with one tap instead of four the same kernel runs at
// 1.25 x a device copy), so the two taps of a row, I[y, x0] and I[y, x0 + 1], come in ONE load of two elements at the
// element's own alignment (4 bytes of uint16 on a 2-byte boundary, 2 bytes of uint8 on any): per plane and output two loads
// instead of four.  The pair always lies inside the row: where x0 = U (only under the clamp, and then fx = 0) the pair is
// (U - 1, U) and the weights of the first tap move to its second element; a plane one column wide has no pair and loads the
// element.  All loads are in bounds, so none of them waits for a comparison.  A run is stored at once (4 bytes of uint16, 2 of
// uint8) where it lies inside the row on a boundary of that size, element by element otherwise.  The 256 threads of a
// workgroup are tx runs wide (a power of two, at most 64: one wave, 128 columns) and 256 / tx rows tall: the two source rows
// a dst row takes are shared by the waves of one workgroup through its L1 in all but the first of its rows.  blockIdx.x =
// row segment * n_strips + strip.  A run's column beyond the row takes the map of the row's last column: loaded, never stored.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "device_util.h"
#include "plane_batch.h"

using namespace sq;

namespace {

constexpr int THREADS = 256;
constexpr int OUTS = 2;                                   // dst columns of a thread's run
constexpr int TX_MAX = 64;                                // runs across a workgroup, at most
constexpr int WALK = SQ_WARP_PLANES_PER_THREAD;           // planes a thread walks over with one map
constexpr int64_t HALF = (int64_t)1000000 << 16;          // H of the definition

struct WarpArgs {
    const void *src;
    int64_t src_plane_stride, src_pitch;   // elements
    void *dst;
    int64_t dst_plane_stride, dst_pitch;
    int64_t r2;
    int32_t h, w;
    int32_t n_planes;           // of this launch
    int32_t ppm;
    int32_t tx, tx_log2;        // runs across a workgroup
    int32_t n_strips;
};

// (c*s + H) // (2*H) with floor division: 2*H = 10^6 * 2^17, and floor(floor(n / 2^17) / 10^6) = floor(n / (10^6 * 2^17))
__device__ __forceinline__ int32_t displacement(int64_t c, int64_t s) {
    const int64_t t = (c * s + HALF) >> 17;      // (an arithmetic shift: the floor, also of a negative numerator)
    int64_t q = t / 1000000;
    if (t - q * 1000000 < 0) q -= 1;
    return (int32_t)q;
}

template <typename T>
__global__ __launch_bounds__(THREADS) void warp_kernel(const WarpArgs a) {
    const int tid = threadIdx.x;
    const int strip = blockIdx.x % a.n_strips, seg = blockIdx.x / a.n_strips;
    const int lx = tid & (a.tx - 1), ly = tid >> a.tx_log2;
    const int ty = THREADS >> a.tx_log2;
    const int64_t xo_l = ((int64_t)strip * a.tx + lx) * OUTS, y_l = (int64_t)seg * ty + ly;
    if (xo_l >= a.w || y_l >= a.h) return;
    const int xo = (int)xo_l, y = (int)y_l;
    const int U = a.w - 1, V = a.h - 1;

    // the map of the run, once for all planes
    int64_t first[OUTS], row_step[OUTS];
    uint32_t w00[OUTS], w01[OUTS], w10[OUTS], w11[OUTS];
    const int64_t v = 2 * (int64_t)y - V;
#pragma unroll
    for (int i = 0; i < OUTS; ++i) {
        const int x = min(xo + i, U);
        const int64_t u = 2 * (int64_t)x - U;
        const int64_t rho = (int64_t)(((uint64_t)(u * u + v * v) << 24) / (uint64_t)a.r2);
        const int64_t s = (int64_t)a.ppm * rho;
        const int32_t X = min(max(256 * x + displacement(u, s), 0), 256 * U);
        const int32_t Y = min(max(256 * y + displacement(v, s), 0), 256 * V);
        const int32_t xa = X >> 8, ya = Y >> 8;
        const uint32_t fx = (uint32_t)(X & 255), fy = (uint32_t)(Y & 255);
        // the pair (xp, xp + 1) holds both taps of a row: (x0, x0 + 1), or (U - 1, U) where x0 = U -- then fx = 0, x1 = U too,
        // and all of the row's weight goes to the pair's second element.  U = 0: the element alone, its second weight 0.
        const bool last = xa == U && U > 0;
        const int32_t xp = last ? U - 1 : xa;
        const uint32_t wl = last ? 0u : 256u - fx, wr = last ? 256u : fx;
        first[i] = (int64_t)ya * a.src_pitch + xp;
        row_step[i] = ya < V ? a.src_pitch : 0;
        w00[i] = wl * (256u - fy);
        w01[i] = wr * (256u - fy);
        w10[i] = wl * fy;
        w11[i] = wr * fy;
    }
    const bool narrow = U == 0;      // (the same in every thread)

    const int p0 = blockIdx.y * WALK, p1 = min(a.n_planes, p0 + WALK);
    const T *sp = static_cast<const T *>(a.src) + (int64_t)p0 * a.src_plane_stride;
    T *wp = static_cast<T *>(a.dst) + (int64_t)p0 * a.dst_plane_stride + (int64_t)y * a.dst_pitch + xo;
    const int valid = min(OUTS, a.w - xo);
    constexpr int STORE = OUTS * (int)sizeof(T);      // bytes of a run: 4 or 2
    constexpr int BITS = 8 * (int)sizeof(T);
    constexpr uint32_t LOW = (1u << BITS) - 1;
    typedef typename std::conditional<sizeof(T) == 2, pair_of_u16, pair_of_u8>::type Pair;
    for (int p = p0; p < p1; ++p, sp += a.src_plane_stride, wp += a.dst_plane_stride) {
        uint32_t o[OUTS];
#pragma unroll
        for (int i = 0; i < OUTS; ++i) {
            const T *t0 = sp + first[i], *t1 = t0 + row_step[i];
            uint32_t r0, r1;      // a row's two taps: the first in the low half
            if (narrow) {
                r0 = *(const SQ_GLOBAL T *)t0;
                r1 = *(const SQ_GLOBAL T *)t1;
            } else {
                r0 = *(const SQ_GLOBAL Pair *)t0;
                r1 = *(const SQ_GLOBAL Pair *)t1;
            }
            o[i] = ((r0 & LOW) * w00[i] + (r0 >> BITS) * w01[i] + (r1 & LOW) * w10[i] + (r1 >> BITS) * w11[i] + 32768u) >> 16;
        }
        if (valid == OUTS && (reinterpret_cast<uintptr_t>(wp) & (STORE - 1)) == 0) {
            if (sizeof(T) == 2)
                *(SQ_GLOBAL uint32_t *)wp = o[0] | (o[1] << 16);
            else
                *(SQ_GLOBAL uint16_t *)wp = (uint16_t)(o[0] | (o[1] << 8));
        } else {
#pragma unroll
            for (int i = 0; i < OUTS; ++i)
                if (i < valid) *(SQ_GLOBAL T *)(wp + i) = (T)o[i];
        }
    }
}

}   // namespace

extern "C" int sq_warp_tiles(const void *src_dev, void *dst_dev, int32_t n_images, int32_t h, int32_t w,
                             int64_t src_plane_stride, int64_t src_pitch, int64_t dst_plane_stride, int64_t dst_pitch,
                             int32_t dtype, int32_t ppm, void *stream_) {
    if (dtype != SQ_U8 && dtype != SQ_U16) return fail(SQ_ERR_INVALID, "sq_warp_tiles: dtype %d", dtype);
    if (ppm < -SQ_WARP_MAX_PPM || ppm > SQ_WARP_MAX_PPM)
        return fail(SQ_ERR_INVALID, "sq_warp_tiles: ppm %d outside -%d..%d", ppm, SQ_WARP_MAX_PPM, SQ_WARP_MAX_PPM);
    if (n_images < 0 || h <= 0 || w <= 0) return fail(SQ_ERR_INVALID, "sq_warp_tiles: bad sizes (images=%d %dx%d)", n_images, h, w);
    if (h > SQ_WARP_MAX_SIDE || w > SQ_WARP_MAX_SIDE)
        return fail(SQ_ERR_UNSUPPORTED, "sq_warp_tiles: a plane of %d x %d has a side above %d (the map is 64-bit up to there)", h, w,
                    SQ_WARP_MAX_SIDE);
    if (src_pitch < w || dst_pitch < w)
        return fail(SQ_ERR_INVALID, "sq_warp_tiles: pitches %lld, %lld below the width %d", (long long)src_pitch,
                    (long long)dst_pitch, w);
    if (n_images == 0) return SQ_OK;
    if (!src_dev || !dst_dev) return fail(SQ_ERR_INVALID, "sq_warp_tiles: NULL buffer");
    const int esize = dtype == SQ_U16 ? 2 : 1;
    const PlaneBatch src{src_dev, n_images, h, w, src_plane_stride, src_pitch, esize};
    const PlaneBatch dst{dst_dev, n_images, h, w, dst_plane_stride, dst_pitch, esize};
    if (const int rc = check_batches("sq_warp_tiles", "plane", {src, dst})) return rc;
    // a tap is read after its neighbour's result is written
    if (overlap(src, dst)) return fail(SQ_ERR_INVALID, "sq_warp_tiles: src and dst overlap (the correction is out of place)");
    hipStream_t stream = static_cast<hipStream_t>(stream_);

    WarpArgs a{};
    a.h = h;
    a.w = w;
    a.ppm = ppm;
    a.r2 = std::max<int64_t>(1, (int64_t)(w - 1) * (w - 1) + (int64_t)(h - 1) * (h - 1));
    StripGrid g;      // (at most 512 strips times at most 16384 segments: far below a launch's workgroups)
    if (const int rc = strip_grid("sq_warp_tiles", ((int64_t)w + OUTS - 1) / OUTS, TX_MAX, THREADS, 1, h, &g)) return rc;
    a.tx = g.tx;
    a.tx_log2 = g.tx_log2;
    a.n_strips = g.n_strips;
    a.src_plane_stride = src_plane_stride;
    a.src_pitch = src_pitch;
    a.dst_plane_stride = dst_plane_stride;
    a.dst_pitch = dst_pitch;
    return for_each_launch("sq_warp_tiles", 0, n_images, WALK, [&](int64_t p0, int32_t m, unsigned grid_y) {
        const dim3 grid(g.x(), grid_y);      // gridDim.y runs of WALK planes
        a.src = src.at(p0);
        a.dst = dst.at(p0);
        a.n_planes = m;
        if (dtype == SQ_U16)
            warp_kernel<uint16_t><<<grid, dim3(THREADS), 0, stream>>>(a);
        else
            warp_kernel<uint8_t><<<grid, dim3(THREADS), 0, stream>>>(a);
    });
}

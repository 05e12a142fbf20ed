// Constant sub-pixel translation of a batch of staged tile planes for gfx950, out of place (--channel-shift):
//
//     S = (Sy, Sx) in 1/256 pixel, U = w - 1, V = h - 1, for the output pixel (y, x):
//       Y = clamp(256*y + Sy, 0, 256*V),  X = clamp(256*x + Sx, 0, 256*U)          (edges replicated)
//       y0 = Y >> 8, fy = Y & 255, y1 = min(y0 + 1, V);   x0, fx, x1 likewise
//       out(y, x) = ( I[y0,x0]*(256-fx)*(256-fy) + I[y0,x1]*fx*(256-fy)
//                   + I[y1,x0]*(256-fx)*fy       + I[y1,x1]*fx*fy + 32768 ) >> 16
//
// The blend is the one of warp.hip; only the map differs.  The reference has no counterpart; the definition is the numpy
// restatement in tests/shift_ref.py.  Integers only, no atomics, no LDS, no scratch: deterministic.
//
// The form the kernel uses (tests/test_channel_shift_cpu.py proves it equal on every case): with iy = Sy >> 8, ix = Sx >> 8 (the
// arithmetic shift: the floor) the weights are the CONSTANTS fy = Sy & 255, fx = Sx & 255 everywhere, the taps are the rows
// clamp(y + iy, 0, V) and clamp(y + iy + 1, 0, V) and the columns clamp(x + ix, 0, U) and clamp(x + ix + 1, 0, U) -- where the
// coordinate clamp of the definition acts, both taps of that axis are the same element and the weights do not matter -- and the
// blend is separable bit for bit: Hrow(r, x) = I[r,x0]*(256-fx) + I[r,x1]*fx < 2^24, out = (Hrow(y0)*(256-fy) + Hrow(y1)*fy +
// 32768) >> 16, whose sum is below 2^32 (at most 65535 * 2^16 + 2^15).  Every factor is below 2^24 (elements < 2^16, weights
// <= 256, Hrow <= 65535 * 256), so all products are 24-bit multiplies (v_mul_u32_u24 / v_mad_u32_u24: full rate, low 32 bits).
//
// Mapping (despeckle.hip's): a thread owns one 16-byte vector of dst columns (8 uint16 / 16 uint8) and walks down RPT rows with
// the horizontal blend of the previous source row in registers, so every source row of its columns is loaded once per run, plus
// one halo row per run, and dst is written once.  The source row index is monotone in y: a row in the clamped region is the row
// already held and is not loaded again.  The 256 threads of a workgroup are tx vectors wide (a power of two) and 256 / tx runs
// tall; blockIdx.x = row segment * n_strips + strip, blockIdx.y = plane.
//
// Vectors: the vectors are laid at the phase of dst's first row, so a dst whose pitch and plane stride are multiples of a vector
// is stored with 16-byte stores throughout.  The source span of a vector is VEC + 1 elements from column xa + ix, in general at
// another phase than dst: a span that lies inside its row (the interior path, chosen once per thread, no clamp or comparison in
// front of its loads) comes in ONE 16-byte load declared at the element's own alignment plus one element; the hardware takes a
// 16-byte global load at any byte address.  The vectors that reach a row end are read element by element with clamped columns
// and written element by element: nothing outside a source plane is read, nothing outside h x w of a dst plane is written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "device_util.h"
#include "plane_batch.h"

using namespace sq;

namespace {

constexpr int THREADS = 256;
constexpr int RPT = SQ_SHIFT_ROWS_PER_THREAD;     // rows a thread walks down (each run reads one halo row: 3 % of the reads)

struct ShiftArgs {
    const void *src;
    int64_t src_plane_stride, src_pitch;   // elements
    void *dst;
    int64_t dst_plane_stride, dst_pitch;
    int32_t h, w;
    int32_t iy, ix;             // whole pixels of the shift (the floor)
    uint32_t fy, fx;            // its fraction in 1/256
    int32_t mis;                // elements of dst's first row in front of a 16-byte boundary: vector k starts at column k * VEC - mis
    int32_t tx, tx_log2;        // vectors across a workgroup
    int32_t n_strips;
};

// Hrow(row, x) of the thread's VEC columns -> H.  INTERIOR: the span xs ... xs + VEC lies inside the row.
template <typename T, int VEC, bool INTERIOR>
__device__ __forceinline__ void blend_row(const T *__restrict__ rp, int xs, int U, uint32_t fx, uint32_t (&H)[VEC]) {
    uint32_t e[VEC + 1];
    if (INTERIOR) {
        typedef typename std::conditional<sizeof(T) == 2, span_of_u16, span_of_u8>::type Span;
        const u32x4 d = *(const SQ_GLOBAL Span *)(rp + xs);
        e[VEC] = (uint32_t)(*(const SQ_GLOBAL T *)(rp + xs + VEC));
        const uint32_t dq[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (sizeof(T) == 2) {
                e[2 * q] = dq[q] & 0xffffu;
                e[2 * q + 1] = dq[q] >> 16;
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) e[4 * q + s] = (dq[q] >> (8 * s)) & 0xffu;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < VEC + 1; ++k) e[k] = (uint32_t)(*(const SQ_GLOBAL T *)(rp + min(max(xs + k, 0), U)));
    }
    const uint32_t gx = 256u - fx;
#pragma unroll
    for (int j = 0; j < VEC; ++j) H[j] = __umul24(e[j], gx) + __umul24(e[j + 1], fx);      // (24-bit multiplies: full rate)
}

template <typename T, int VEC, bool INTERIOR>
__device__ __forceinline__ void walk(const ShiftArgs &a, const T *__restrict__ src, T *__restrict__ dst, int xa, int y_lo) {
    const int U = a.w - 1, V = a.h - 1;
    const int y_hi = min(a.h, y_lo + RPT);
    const int lo_x = max(xa, 0), hi_x = min(xa + VEC, a.w);
    const int xs = xa + a.ix;
    const uint32_t fx = a.fx, fy = a.fy, gy = 256u - a.fy;
    uint32_t A[VEC], B[VEC];      // Hrow of the source rows ia and ib
    int ia = min(max(y_lo + a.iy, 0), V);
    blend_row<T, VEC, INTERIOR>(src + (int64_t)ia * a.src_pitch, xs, U, fx, A);
    int ib = ia;
#pragma unroll
    for (int j = 0; j < VEC; ++j) B[j] = A[j];
    for (int y = y_lo; y < y_hi; ++y) {
        const int ra = min(max(y + a.iy, 0), V), rb = min(max(y + a.iy + 1, 0), V);
        if (ra != ia) {       // (ra is the rb of the row above, which is held as ib)
#pragma unroll
            for (int j = 0; j < VEC; ++j) A[j] = B[j];
            ia = ib;
        }
        if (rb != ib) {
            blend_row<T, VEC, INTERIOR>(src + (int64_t)rb * a.src_pitch, xs, U, fx, B);
            ib = rb;
        }
        uint32_t o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = (__umul24(A[j], gy) + __umul24(B[j], fy) + 32768u) >> 16;      // (Hrow < 2^24)
        T *wp = dst + (int64_t)y * a.dst_pitch;
        if (hi_x - lo_x == VEC && (reinterpret_cast<uintptr_t>(wp + xa) & 15) == 0) {
            u32x4 d;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (sizeof(T) == 2) {
                    d[q] = o[2 * q] | (o[2 * q + 1] << 16);
                } else {
                    d[q] = o[4 * q] | (o[4 * q + 1] << 8) | (o[4 * q + 2] << 16) | (o[4 * q + 3] << 24);
                }
            }
            *(SQ_GLOBAL u32x4 *)(wp + xa) = d;
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                if (xa + j >= lo_x && xa + j < hi_x) *(SQ_GLOBAL T *)(wp + xa + j) = (T)o[j];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(THREADS) void shift_kernel(const ShiftArgs a) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int tid = threadIdx.x;
    const int strip = blockIdx.x % a.n_strips, seg = blockIdx.x / a.n_strips;
    const int lx = tid & (a.tx - 1), ly = tid >> a.tx_log2;
    const int ty = THREADS >> a.tx_log2;
    const int xa = (strip * a.tx + lx) * VEC - a.mis;       // the vector's first column (negative: it starts in front of the row)
    const int64_t y_lo = ((int64_t)seg * ty + ly) * RPT;
    if (xa >= a.w || xa + VEC <= 0 || y_lo >= a.h) return;
    const T *__restrict__ src = static_cast<const T *>(a.src) + (int64_t)blockIdx.y * a.src_plane_stride;
    T *__restrict__ dst = static_cast<T *>(a.dst) + (int64_t)blockIdx.y * a.dst_plane_stride;
    const int xs = xa + a.ix;
    if (xs >= 0 && xs + VEC <= a.w - 1)
        walk<T, VEC, true>(a, src, dst, xa, (int)y_lo);
    else
        walk<T, VEC, false>(a, src, dst, xa, (int)y_lo);
}

}   // namespace

extern "C" int sq_shift_tiles(const void *src_dev, void *dst_dev, int32_t n_images, int32_t h, int32_t w,
                              int64_t src_plane_stride, int64_t src_pitch, int64_t dst_plane_stride, int64_t dst_pitch,
                              int32_t dtype, const int32_t *shifts_host, int32_t images_per_shift, void *stream_) {
    if (dtype != SQ_U8 && dtype != SQ_U16) return fail(SQ_ERR_INVALID, "sq_shift_tiles: dtype %d", dtype);
    if (n_images < 0 || h <= 0 || w <= 0) return fail(SQ_ERR_INVALID, "sq_shift_tiles: bad sizes (images=%d %dx%d)", n_images, h, w);
    if (h > SQ_SHIFT_MAX_SIDE || w > SQ_SHIFT_MAX_SIDE)
        return fail(SQ_ERR_UNSUPPORTED, "sq_shift_tiles: a plane of %d x %d has a side above %d", h, w, SQ_SHIFT_MAX_SIDE);
    if (src_pitch < w || dst_pitch < w)
        return fail(SQ_ERR_INVALID, "sq_shift_tiles: pitches %lld, %lld below the width %d", (long long)src_pitch,
                    (long long)dst_pitch, w);
    if (images_per_shift < 1 || n_images % images_per_shift != 0)
        return fail(SQ_ERR_INVALID, "sq_shift_tiles: %d images are no multiple of images_per_shift %d", n_images, images_per_shift);
    if (n_images == 0) return SQ_OK;
    if (!src_dev || !dst_dev) return fail(SQ_ERR_INVALID, "sq_shift_tiles: NULL buffer");
    if (!shifts_host) return fail(SQ_ERR_INVALID, "sq_shift_tiles: NULL shift table");
    const int32_t n_shifts = n_images / images_per_shift;
    for (int32_t i = 0; i < 2 * n_shifts; ++i)
        if (shifts_host[i] < -SQ_SHIFT_MAX || shifts_host[i] > SQ_SHIFT_MAX)
            return fail(SQ_ERR_INVALID, "sq_shift_tiles: shift %d of pair %d outside -%d..%d (1/256 pixel)", shifts_host[i], i / 2,
                        SQ_SHIFT_MAX, SQ_SHIFT_MAX);
    const int esize = dtype == SQ_U16 ? 2 : 1;
    const PlaneBatch src{src_dev, n_images, h, w, src_plane_stride, src_pitch, esize};
    const PlaneBatch dst{dst_dev, n_images, h, w, dst_plane_stride, dst_pitch, esize};
    if (const int rc = check_batches("sq_shift_tiles", "plane", {src, dst})) return rc;
    // a thread reads what a neighbour writes
    if (overlap(src, dst)) return fail(SQ_ERR_INVALID, "sq_shift_tiles: src and dst overlap (the shift is out of place)");
    hipStream_t stream = static_cast<hipStream_t>(stream_);

    const int vec = 16 / esize;
    ShiftArgs a{};
    a.h = h;
    a.w = w;
    a.mis = dst.phase(vec);
    StripGrid g;      // (sides up to 65535: at most 512 strips and 2048 segments)
    if (const int rc = strip_grid("sq_shift_tiles", ((int64_t)w + a.mis + vec - 1) / vec, THREADS, THREADS, RPT, h, &g)) return rc;
    a.tx = g.tx;
    a.tx_log2 = g.tx_log2;
    a.n_strips = g.n_strips;
    a.src_plane_stride = src_plane_stride;
    a.src_pitch = src_pitch;
    a.dst_plane_stride = dst_plane_stride;
    a.dst_pitch = dst_pitch;
    // one grid per maximal run of consecutive equal pairs, (0, 0) included: the arguments stay scalar, no table goes to the device
    return for_each_run(shifts_host, n_shifts, 2, [&](const int32_t *t, int32_t s0, int32_t s1) {
        a.iy = t[0] >> 8;
        a.ix = t[1] >> 8;
        a.fy = (uint32_t)(t[0] & 255);
        a.fx = (uint32_t)(t[1] & 255);
        return for_each_launch("sq_shift_tiles", (int64_t)s0 * images_per_shift, (int64_t)s1 * images_per_shift, 1,
                               [&](int64_t p0, int32_t, unsigned grid_y) {
            const dim3 grid(g.x(), grid_y);
            a.src = src.at(p0);
            a.dst = dst.at(p0);
            if (dtype == SQ_U16)
                shift_kernel<uint16_t><<<grid, dim3(THREADS), 0, stream>>>(a);
            else
                shift_kernel<uint8_t><<<grid, dim3(THREADS), 0, stream>>>(a);
        });
    });
}

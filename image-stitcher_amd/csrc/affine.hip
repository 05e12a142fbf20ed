// Per-channel affine map (rotation, scale, shear about the tile centre, composed with a constant shift) of a batch of staged tile
// planes for gfx950, out of place (--channel-affine):
//
//     S = (Sy, Sx) in 1/256 pixel, A = (Ayy, Ayx, Axy, Axx) in parts per million, U = w - 1, V = h - 1, for the output pixel (y, x):
//       u = 2*x - U,  v = 2*y - V                                   (half-pixels from the tile centre)
//       dv = Sy + (16*(Ayy*v + Ayx*u) + 62500) // 125000            (1/256 pixel, rounded half up; floor division)
//       du = Sx + (16*(Axy*v + Axx*u) + 62500) // 125000
//       Y = clamp(256*y + dv, 0, 256*V),  X = clamp(256*x + du, 0, 256*U)        (edges replicated)
//       y0 = Y >> 8, fy = Y & 255, y1 = min(y0 + 1, V);   x0, fx, x1 likewise
//       out(y, x) = ( I[y0,x0]*(256-fx)*(256-fy) + I[y0,x1]*fx*(256-fy)
//                   + I[y1,x0]*(256-fx)*fy       + I[y1,x1]*fx*fy + 32768 ) >> 16
//
// The blend is the one of warp.hip and shift.hip; only the map differs.  The reference has no counterpart; the definition is the
// numpy restatement in tests/affine_ref.py.  Integers only, no atomics, no LDS, no scratch: deterministic.
//
// The map without a division per pixel: along an output row both numerators are linear in x with the steps 32*Ayx and 32*Axx.  A
// thread divides the numerators of its first column once (64 bits: up to 1.05e11) into a quotient and a remainder in [0, 125000)
// and steps both from there in 32 bits -- q += floor(step / 125000), r += step mod 125000, carry where r >= 125000 -- which keeps
// numerator = q * 125000 + r with 0 <= r < 125000, i.e. q is the floor quotient at every column.  The steps' own quotient and
// remainder come from the host.
//
// Mapping: a thread owns one 16-byte vector of dst columns of one row (VEC = 8 uint16 / 16 uint8, laid at the phase of dst's first
// row as in shift.hip), works the map (X, Y) of its VEC positions out once and walks over up to WALK planes of the batch with it
// (blockIdx.y = run of planes), as warp.hip does: the planes of one launch share the map.  The blend is separable bit for bit
// (shift.hip): Hrow(r, j) = I[r,x0]*(256-fx) + I[r,x1]*fx < 2^24, out = (Hrow(y0)*(256-fy) + Hrow(y1)*fy + 32768) >> 16 < 2^32,
// all factors below 2^24 (24-bit multiplies).
//
// Loads: over the VEC <= 16 columns of a vector du and dv change by less than one pixel (32 * 50000 * 15 / 125000 = 192 < 256), so
// x0 - j takes at most two neighbouring values and y0 at most two neighbouring rows.  The FAST path (decided once per thread from
// the final, clamped X and Y, so it does not rest on that bound: a thread whose positions do not fit takes the other path) reads
// the span of VEC + 2 columns from xs = min(x0[j] - j) of the rows ys = min(y0[j]), ys + 1 and, only where two values of y0 occur
// in the wave, ys + 2 (both clamped to the last row once per thread): per row ONE 16-byte load at the element's own alignment plus
// one pair of elements (moved to the row's last two columns where the span ends beyond them), all inside the plane, no clamp or
// comparison in front of a load; the rows of the next plane are asked
// for before this plane's are blended.  Output j then picks its taps out of registers with one bit for the column (k = x0 - j - xs) and
// one for the row (m = y0 - ys).  The SLOW vectors (those whose taps touch the clamp of x or a plane's left edge, and planes
// narrower than a vector) read their four taps element by element at clamped indices; a wave works its slow vectors off together,
// one at a time, a vector's VEC columns x WALK planes dealt out over its 64 lanes, so that their loads are in flight together (a
// lane that walked its slow vector alone, plane after plane, held its wave up for sixteen memory latencies in a row).  Nothing outside a source plane is read, nothing
// outside h x w of a dst plane is written: a full vector on a 16-byte boundary is one store, every other one is written element
// by element.  The 256 threads of a workgroup are tx vectors wide (a power of two, at most 16: 128 uint16 columns) and 256 / tx
// rows tall, so the rows a dst row takes are shared by the waves of a workgroup through L1.  blockIdx.x = row segment * n_strips
// + strip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "device_util.h"
#include "plane_batch.h"

using namespace sq;

namespace {

constexpr int THREADS = 256;
constexpr int TX_MAX = 128;                               // vectors across a workgroup, at most
constexpr int WALK = SQ_AFFINE_PLANES_PER_THREAD;         // planes a thread walks over with one map
constexpr int32_t DEN = 125000;                           // 10^6 / 128 * 16: the definition's divisor

struct AffineArgs {
    const void *src;
    int64_t src_plane_stride, src_pitch;   // elements
    void *dst;
    int64_t dst_plane_stride, dst_pitch;
    int32_t h, w;
    int32_t n_planes;           // of this launch
    int32_t sy, sx;             // 1/256 pixel
    int32_t ayy, ayx, axy, axx; // parts per million
    int32_t vq, vr, uq, ur;     // floor quotient and remainder by DEN of the numerators' steps per column, 32*Ayx and 32*Axx
    int32_t mis;                // elements of dst's first row in front of a 16-byte boundary: vector k starts at column k * VEC - mis
    int32_t tx, tx_log2;        // vectors across a workgroup
    int32_t n_strips;
};

// n = q * DEN + r with 0 <= r < DEN: the floor division, also of a negative numerator
__host__ __device__ __forceinline__ void floor_divmod(int64_t n, int32_t &q, int32_t &r) {
    int64_t quo = n / DEN, rem = n - quo * DEN;
    if (rem < 0) {
        quo -= 1;
        rem += DEN;
    }
    q = (int32_t)quo;
    r = (int32_t)rem;
}

// the floor quotients and remainders of both numerators at one column
struct Map {
    int32_t qv, rv, qu, ru;
    __device__ __forceinline__ void step(const AffineArgs &a) {      // to the next column
        qv += a.vq;
        rv += a.vr;
        if (rv >= DEN) {
            rv -= DEN;
            qv += 1;
        }
        qu += a.uq;
        ru += a.ur;
        if (ru >= DEN) {
            ru -= DEN;
            qu += 1;
        }
    }
};

// the VEC + 2 elements from rp[0] on as they come from memory: one 16-byte load and one pair
struct Raw {
    u32x4 d;
    uint32_t t;
};

template <typename T, int VEC>
__device__ __forceinline__ Raw load_span(const T *__restrict__ rp, int pair_at) {
    typedef typename std::conditional<sizeof(T) == 2, span_of_u16, span_of_u8>::type Span;
    typedef typename std::conditional<sizeof(T) == 2, pair_of_u16, pair_of_u8>::type Pair;
    Raw r;
    r.d = *(const SQ_GLOBAL Span *)rp;
    r.t = (uint32_t)(*(const SQ_GLOBAL Pair *)(rp + pair_at));
    return r;
}

template <typename T, int VEC>
__device__ __forceinline__ void unpack(const Raw &r, uint32_t pair_shift, uint32_t (&e)[VEC + 2]) {
    const uint32_t dq[4] = {r.d.x, r.d.y, r.d.z, r.d.w};
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
    constexpr int BITS = 8 * (int)sizeof(T);
    e[VEC] = (r.t >> pair_shift) & ((1u << BITS) - 1);
    e[VEC + 1] = r.t >> BITS;
}

// acc += Hrow of row ys + R of the span, times the row's vertical weight, under the thread's words (fx in bits 0-7, fy in bits
// 8-15, the column bit k in bit 16, the row bit m in bit 17): output j takes the rows ys + m (weight 256 - fy) and ys + m + 1 (fy)
template <int VEC, int R>
__device__ __forceinline__ void blend_span(const uint32_t (&e)[VEC + 2], const uint32_t (&wt)[VEC], uint32_t (&acc)[VEC]) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const bool k = (wt[j] >> 16) & 1u, m = (wt[j] >> 17) & 1u;
        const uint32_t fx = wt[j] & 255u, fy = (wt[j] >> 8) & 255u, gy = 256u - fy;
        const uint32_t a = k ? e[j + 1] : e[j], b = k ? e[j + 2] : e[j + 1];
        const uint32_t wy = R == 0 ? (m ? 0u : gy) : R == 1 ? (m ? gy : fy) : (m ? fy : 0u);
        acc[j] += __umul24(__umul24(a, 256u - fx) + __umul24(b, fx), wy);      // (Hrow < 2^24)
    }
}

// The fast path's walk over ``n`` planes.  Two sets of row registers take turns: the rows of the next plane are asked for
// before this plane's are blended, so a plane's loads wait behind no arithmetic.  Every turn fetches -- behind the last plane
// the last plane again -- so that the number of loads in flight does not depend on a branch.
template <typename T, int VEC, bool THREE>
__device__ __forceinline__ void walk_planes(const AffineArgs &a, const T *__restrict__ rows, T *__restrict__ out, int64_t second,
                                            int64_t third, int pair_at, uint32_t pair_shift, const uint32_t (&wt)[VEC], int n,
                                            bool whole, int lo, int hi) {
    auto fetch = [&](int plane, Raw &r0, Raw &r1, Raw &r2) {
        const T *rp = rows + (int64_t)min(plane, n - 1) * a.src_plane_stride;
        r0 = load_span<T, VEC>(rp, pair_at);
        r1 = load_span<T, VEC>(rp + second, pair_at);
        if (THREE) r2 = load_span<T, VEC>(rp + third, pair_at);
    };
    auto blend_and_store = [&](int plane, const Raw &r0, const Raw &r1, const Raw &r2) {
        uint32_t e[VEC + 2], o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = 32768u;
        unpack<T, VEC>(r0, pair_shift, e);
        blend_span<VEC, 0>(e, wt, o);
        unpack<T, VEC>(r1, pair_shift, e);
        blend_span<VEC, 1>(e, wt, o);
        if (THREE) {
            unpack<T, VEC>(r2, pair_shift, e);
            blend_span<VEC, 2>(e, wt, o);
        }
        T *wp = out + (int64_t)plane * a.dst_plane_stride;
        if (whole) {
            u32x4 d;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (sizeof(T) == 2) {
                    d[q] = (o[2 * q] >> 16) | (o[2 * q + 1] & 0xffff0000u);
                } else {
                    d[q] = (o[4 * q] >> 16) | ((o[4 * q + 1] >> 16) << 8) | (o[4 * q + 2] & 0x00ff0000u) | ((o[4 * q + 3] >> 16) << 24);
                }
            }
            *(SQ_GLOBAL u32x4 *)wp = d;
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                if (j >= lo && j < hi) *(SQ_GLOBAL T *)(wp + j) = (T)(o[j] >> 16);
        }
    };
    Raw a0, a1, a2 = {}, b0, b1, b2 = {};
    fetch(0, a0, a1, a2);
    for (int p = 0; p < n; p += 2) {
        fetch(p + 1, b0, b1, b2);
        blend_and_store(p, a0, a1, a2);
        fetch(p + 2, a0, a1, a2);
        if (p + 1 < n) blend_and_store(p + 1, b0, b1, b2);
    }
}

template <typename T>
__global__ __launch_bounds__(THREADS) void affine_kernel(const AffineArgs a) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int tid = threadIdx.x;
    const int strip = blockIdx.x % a.n_strips, seg = blockIdx.x / a.n_strips;
    const int lx = tid & (a.tx - 1), ly = tid >> a.tx_log2;
    const int ty = THREADS >> a.tx_log2;
    const int xa = (strip * a.tx + lx) * VEC - a.mis;       // the vector's first column (negative: it starts in front of the row)
    const int64_t y_l = (int64_t)seg * ty + ly;
    // (a thread without a vector stays: the wave works the slow vectors off together, below)
    const bool live = xa < a.w && xa + VEC > 0 && y_l < a.h;
    const int U = a.w - 1, V = a.h - 1;
    const int y = (int)min(y_l, (int64_t)V);

    // the map of the vector, once for all planes: column j stands at x = clamp(xa + j, 0, U) (a column outside the row takes the
    // map of the row's nearest column: loaded, never stored), and the numerators step only where x does
    int32_t X[VEC], Y[VEC];
    Map first_column;
    {
        const int64_t v = 2 * (int64_t)y - V, u = 2 * (int64_t)max(xa, 0) - U;
        floor_divmod(16 * ((int64_t)a.ayy * v + (int64_t)a.ayx * u) + 62500, first_column.qv, first_column.rv);
        floor_divmod(16 * ((int64_t)a.axy * v + (int64_t)a.axx * u) + 62500, first_column.qu, first_column.ru);
        Map m = first_column;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            if (j > 0 && xa + j > 0 && xa + j <= U) m.step(a);
            Y[j] = min(max(256 * y + a.sy + m.qv, 0), 256 * V);
            X[j] = min(max(256 * min(max(xa + j, 0), U) + a.sx + m.qu, 0), 256 * U);
        }
    }
    int xs = X[0] >> 8, ys = Y[0] >> 8, y_top = Y[0] >> 8;
#pragma unroll
    for (int j = 1; j < VEC; ++j) {
        xs = min(xs, (X[j] >> 8) - j);
        ys = min(ys, Y[j] >> 8);
        y_top = max(y_top, Y[j] >> 8);
    }
    const bool three = y_top != ys;
    bool fast = live && xs >= 0 && xs + VEC - 1 <= U && y_top <= ys + 1;
#pragma unroll
    for (int j = 0; j < VEC; ++j) fast = fast && (X[j] >> 8) - j - xs <= 1;

    const int p0 = blockIdx.y * WALK, p1 = min(a.n_planes, p0 + WALK);
    const T *sp = static_cast<const T *>(a.src) + (int64_t)p0 * a.src_plane_stride;
    T *wp = static_cast<T *>(a.dst) + (int64_t)p0 * a.dst_plane_stride + (int64_t)y * a.dst_pitch;
    const int lo_x = max(xa, 0), hi_x = min(xa + VEC, a.w);
    const bool whole = hi_x - lo_x == VEC && (reinterpret_cast<uintptr_t>(wp + xa) & 15) == 0 &&
                       ((a.dst_plane_stride * (int64_t)sizeof(T)) & 15) == 0;

    if (fast) {
        uint32_t wt[VEC];      // fx | fy << 8 | k << 16 | m << 17
#pragma unroll
        for (int j = 0; j < VEC; ++j)
            wt[j] = (uint32_t)(X[j] & 255) | ((uint32_t)(Y[j] & 255) << 8) | ((uint32_t)((X[j] >> 8) - j - xs) << 16) |
                    ((uint32_t)((Y[j] >> 8) - ys) << 17);
        const T *rows = sp + (int64_t)ys * a.src_pitch + xs;
        T *out = wp + xa;
        // the rows behind the first, clamped to the plane's last one: where the clamp acts the row's weight is 0 (fy = 0 at Y =
        // 256 V) or the row is the one the definition's y1 = min(y0 + 1, V) names
        // The span's last two columns come as a pair that starts at column U - 1 at the latest.  A column beyond U is only ever
        // the second tap of x0 = U, whose weight is fx = 0 (X = 256 U there), so what stands in its place does not matter; where
        // the pair was moved by one, column U = xs + VEC is its second element.
        const int pair_at = min(xs + VEC, U - 1) - xs;
        const uint32_t pair_shift = pair_at < VEC ? 8u * (uint32_t)sizeof(T) : 0u;
        const int64_t second = (int64_t)(min(ys + 1, V) - ys) * a.src_pitch;
        const int64_t third = (int64_t)(min(ys + (three ? 2 : 1), V) - ys) * a.src_pitch;
        // the third row is read by the whole wave or not at all (a lane that does not need it reads its second row again and
        // gives it no weight: every m is 0 there), and the choice is made outside the loop over the planes
        if (__ballot(three) != 0)
            walk_planes<T, VEC, true>(a, rows, out, second, third, pair_at, pair_shift, wt, p1 - p0, whole, lo_x - xa, hi_x - xa);
        else
            walk_planes<T, VEC, false>(a, rows, out, second, third, pair_at, pair_shift, wt, p1 - p0, whole, lo_x - xa, hi_x - xa);
    }

    // The vectors that are left: the wave takes them one at a time and deals a vector's VEC columns x n planes out over its 64
    // lanes, an element each -- the four taps one by one at clamped indices, the element stored on its own -- so that the planes
    // of a slow vector are in flight together, not one after the other behind the wave's fast lanes.
    const int lane = (int)(threadIdx.x & 63u), n = p1 - p0;
    for (uint64_t todo = __ballot(live && !fast); todo != 0; todo &= todo - 1) {
        const int owner = __ffsll((unsigned long long)todo) - 1;
        const int oxa = __shfl(xa, owner), oy = __shfl(y, owner);
        Map first;
        first.qv = __shfl(first_column.qv, owner);
        first.rv = __shfl(first_column.rv, owner);
        first.qu = __shfl(first_column.qu, owner);
        first.ru = __shfl(first_column.ru, owner);
        for (int item = lane; item < VEC * n; item += 64) {
            const int x = oxa + item % VEC, p = item / VEC;
            if (x < 0 || x > U) continue;
            Map m = first;
            for (int c = max(oxa, 0); c < x; ++c) m.step(a);
            const int32_t Yj = min(max(256 * oy + a.sy + m.qv, 0), 256 * V);
            const int32_t Xj = min(max(256 * x + a.sx + m.qu, 0), 256 * U);
            const int x0 = Xj >> 8, y0 = Yj >> 8;
            const int x1 = min(x0 + 1, U), y1 = min(y0 + 1, V);
            const uint32_t fx = (uint32_t)(Xj & 255), fy = (uint32_t)(Yj & 255);
            const T *plane = sp + (int64_t)p * a.src_plane_stride;
            const T *r0 = plane + (int64_t)y0 * a.src_pitch, *r1 = plane + (int64_t)y1 * a.src_pitch;
            const uint32_t i00 = *(const SQ_GLOBAL T *)(r0 + x0), i01 = *(const SQ_GLOBAL T *)(r0 + x1);
            const uint32_t i10 = *(const SQ_GLOBAL T *)(r1 + x0), i11 = *(const SQ_GLOBAL T *)(r1 + x1);
            const uint32_t top = __umul24(i00, 256u - fx) + __umul24(i01, fx);
            const uint32_t bot = __umul24(i10, 256u - fx) + __umul24(i11, fx);
            T *o = static_cast<T *>(a.dst) + (int64_t)(p0 + p) * a.dst_plane_stride + (int64_t)oy * a.dst_pitch + x;
            *(SQ_GLOBAL T *)o = (T)((__umul24(top, 256u - fy) + __umul24(bot, fy) + 32768u) >> 16);
        }
    }
}

}   // namespace

extern "C" int sq_affine_tiles(const void *src_dev, void *dst_dev, int32_t n_images, int32_t h, int32_t w,
                               int64_t src_plane_stride, int64_t src_pitch, int64_t dst_plane_stride, int64_t dst_pitch,
                               int32_t dtype, const int32_t *params_host, int32_t images_per_param, void *stream_) {
    if (dtype != SQ_U8 && dtype != SQ_U16) return fail(SQ_ERR_INVALID, "sq_affine_tiles: dtype %d", dtype);
    if (n_images < 0 || h <= 0 || w <= 0) return fail(SQ_ERR_INVALID, "sq_affine_tiles: bad sizes (images=%d %dx%d)", n_images, h, w);
    if (h > SQ_AFFINE_MAX_SIDE || w > SQ_AFFINE_MAX_SIDE)
        return fail(SQ_ERR_UNSUPPORTED, "sq_affine_tiles: a plane of %d x %d has a side above %d", h, w, SQ_AFFINE_MAX_SIDE);
    if (src_pitch < w || dst_pitch < w)
        return fail(SQ_ERR_INVALID, "sq_affine_tiles: pitches %lld, %lld below the width %d", (long long)src_pitch,
                    (long long)dst_pitch, w);
    if (images_per_param < 1 || n_images % images_per_param != 0)
        return fail(SQ_ERR_INVALID, "sq_affine_tiles: %d images are no multiple of images_per_param %d", n_images, images_per_param);
    if (n_images == 0) return SQ_OK;
    if (!src_dev || !dst_dev) return fail(SQ_ERR_INVALID, "sq_affine_tiles: NULL buffer");
    if (!params_host) return fail(SQ_ERR_INVALID, "sq_affine_tiles: NULL parameter table");
    const int32_t n_params = n_images / images_per_param;
    for (int32_t i = 0; i < n_params; ++i) {
        const int32_t *t = params_host + 6 * (int64_t)i;
        for (int c = 0; c < 2; ++c)
            if (t[c] < -SQ_SHIFT_MAX || t[c] > SQ_SHIFT_MAX)
                return fail(SQ_ERR_INVALID, "sq_affine_tiles: shift %d of tuple %d outside -%d..%d (1/256 pixel)", t[c], i, SQ_SHIFT_MAX,
                            SQ_SHIFT_MAX);
        for (int c = 2; c < 6; ++c)
            if (t[c] < -SQ_AFFINE_MAX_PPM || t[c] > SQ_AFFINE_MAX_PPM)
                return fail(SQ_ERR_INVALID, "sq_affine_tiles: coefficient %d of tuple %d outside -%d..%d (parts per million)", t[c], i,
                            SQ_AFFINE_MAX_PPM, SQ_AFFINE_MAX_PPM);
    }
    const int esize = dtype == SQ_U16 ? 2 : 1;
    const PlaneBatch src{src_dev, n_images, h, w, src_plane_stride, src_pitch, esize};
    const PlaneBatch dst{dst_dev, n_images, h, w, dst_plane_stride, dst_pitch, esize};
    if (const int rc = check_batches("sq_affine_tiles", "plane", {src, dst})) return rc;
    // a tap is read after its neighbour's result is written
    if (overlap(src, dst)) return fail(SQ_ERR_INVALID, "sq_affine_tiles: src and dst overlap (the map is out of place)");
    hipStream_t stream = static_cast<hipStream_t>(stream_);

    const int vec = 16 / esize;
    AffineArgs a{};
    a.h = h;
    a.w = w;
    a.mis = dst.phase(vec);
    StripGrid g;      // (at most 512 strips times at most 4096 segments: far below a launch's workgroups)
    if (const int rc = strip_grid("sq_affine_tiles", ((int64_t)w + a.mis + vec - 1) / vec, TX_MAX, THREADS, 1, h, &g)) return rc;
    a.tx = g.tx;
    a.tx_log2 = g.tx_log2;
    a.n_strips = g.n_strips;
    a.src_plane_stride = src_plane_stride;
    a.src_pitch = src_pitch;
    a.dst_plane_stride = dst_plane_stride;
    a.dst_pitch = dst_pitch;
    // one grid per maximal run of consecutive equal tuples, the all-zero one included: the arguments stay scalar, no table goes
    // to the device
    return for_each_run(params_host, n_params, 6, [&](const int32_t *t, int32_t s0, int32_t s1) {
        a.sy = t[0];
        a.sx = t[1];
        a.ayy = t[2];
        a.ayx = t[3];
        a.axy = t[4];
        a.axx = t[5];
        floor_divmod(32 * (int64_t)a.ayx, a.vq, a.vr);
        floor_divmod(32 * (int64_t)a.axx, a.uq, a.ur);
        return for_each_launch("sq_affine_tiles", (int64_t)s0 * images_per_param, (int64_t)s1 * images_per_param, WALK,
                               [&](int64_t p0, int32_t m, unsigned grid_y) {
            const dim3 grid(g.x(), grid_y);      // gridDim.y runs of WALK planes
            a.src = src.at(p0);
            a.dst = dst.at(p0);
            a.n_planes = m;
            if (dtype == SQ_U16)
                affine_kernel<uint16_t><<<grid, dim3(THREADS), 0, stream>>>(a);
            else
                affine_kernel<uint8_t><<<grid, dim3(THREADS), 0, stream>>>(a);
        });
    });
}

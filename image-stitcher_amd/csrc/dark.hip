// Dark-frame subtraction of a batch of staged tile planes for gfx950 (--dark-frame): for a plane I of one dtype (maximum M), a
// dark frame D of that dtype (or a constant c) and a pedestal P in 0..M,
//
//     out(y, x) = clamp(I(y, x) - D(y, x) + P, 0, M)
//
// in a wider signed type.  The reference has no counterpart; the definition is the numpy restatement in tests/dark_ref.py.
// Integers only: deterministic, and bit for bit the definition.  Elementwise and IN PLACE: a thread reads the pixels it writes
// and no others, every tile element is read once and written once.
//
// Mapping: as in dpc.hip.  A thread owns one 16-byte vector of columns (8 uint16 / 16 uint8) and walks down RPT rows; the 256
// threads of a workgroup are tx vectors wide (a power of two) and 256 / tx runs of RPT rows tall.  blockIdx.x = row segment *
// n_strips + strip, blockIdx.y = a group of IPT = SQ_DARK_IMAGES_PER_THREAD consecutive images of the run: the thread keeps
// P - D of its (row, columns) in registers and walks the group with it, so the frame is fetched once per IPT tiles; the 16-byte
// loads of the group are issued before the first store.  The constant path is a template parameter that loads no frame.  No LDS,
// no atomics.
//
// Vectors: the vectors of a row are laid at the phase of that row of the tiles, so every full vector is one 16-byte load and one
// 16-byte store whatever the base and the pitch; the frame is loaded with 16-byte loads where it has the same phase, element by
// element where not.  The vectors a row starts and ends in are touched element by element: nothing outside a row is read or
// written, and the columns between w and the pitch stay as they are.  The images of a group share the row's phase only when the
// plane stride is a whole number of vectors (always, for the stitcher's buffers); a batch where it is not goes image by image
// (the IPT = 1 instance).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_util.h"
#include "plane_batch.h"

using namespace sq;

namespace {

constexpr int THREADS = 256;
constexpr int RPT = 8;      // rows a thread walks down
constexpr int IPT = SQ_DARK_IMAGES_PER_THREAD;

struct DarkArgs {
    void *tiles;                // the run's first image
    const void *frame;          // the run's frame (unused on the constant path)
    int64_t plane_stride, pitch;      // elements
    int64_t frame_pitch;
    int32_t n_images;           // of this grid
    int32_t h, w;
    int32_t pedestal;           // P
    int32_t k;                  // the constant path: P - c
    int32_t tx, tx_log2;        // vectors across a workgroup
    int32_t n_strips;
};

// The VEC pixels of row pointer rp that start at column xa -> v[], 16-byte load where the vector is whole and aligned, else
// element by element over the columns [lo_x, hi_x) the vector has inside the row (the others stay 0).
template <typename T, int VEC>
__device__ __forceinline__ void load_vec(const T *rp, int xa, int lo_x, int hi_x, uint32_t (&v)[VEC]) {
    if (hi_x - lo_x == VEC && (reinterpret_cast<uintptr_t>(rp + xa) & 15) == 0) {
        const u32x4 d = *(const SQ_GLOBAL u32x4 *)(rp + xa);
        const uint32_t dq[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (sizeof(T) == 2) {
                v[2 * q] = dq[q] & 0xffffu;
                v[2 * q + 1] = dq[q] >> 16;
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) v[4 * q + s] = (dq[q] >> (8 * s)) & 0xffu;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const bool in = xa + j >= lo_x && xa + j < hi_x;
            v[j] = in ? (uint32_t)(*(const SQ_GLOBAL T *)(rp + xa + j)) : 0u;
        }
    }
}

// One pixel: k = P - D (or P - c), so the result is clamp(I + k, 0, M); |I + k| <= 2 M fits 32 bits with room.
template <int32_t M>
__device__ __forceinline__ uint32_t dark_pixel(uint32_t i, int32_t k) {
    return (uint32_t)min(max((int32_t)i + k, 0), M);
}

// The 16 bytes d of VEC pixels -> the 16 bytes of their results.
template <typename T, int VEC, bool CONSTANT>
__device__ __forceinline__ u32x4 dark_vector(const u32x4 d, const int32_t (&k)[CONSTANT ? 1 : VEC]) {
    constexpr int32_t M = sizeof(T) == 2 ? 65535 : 255;
    u32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (sizeof(T) == 2) {
            const uint32_t lo = dark_pixel<M>(d[q] & 0xffffu, k[CONSTANT ? 0 : 2 * q]);
            const uint32_t hi = dark_pixel<M>(d[q] >> 16, k[CONSTANT ? 0 : 2 * q + 1]);
            o[q] = lo | (hi << 16);
        } else {
            uint32_t word = 0;
#pragma unroll
            for (int s = 0; s < 4; ++s)
                word |= dark_pixel<M>((d[q] >> (8 * s)) & 0xffu, k[CONSTANT ? 0 : 4 * q + s]) << (8 * s);
            o[q] = word;
        }
    }
    return o;
}

template <typename T, bool CONSTANT, int N_IMG>
__global__ __launch_bounds__(THREADS) void dark_kernel(const DarkArgs a) {
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr int32_t M = sizeof(T) == 2 ? 65535 : 255;
    const int tid = threadIdx.x;
    const int strip = blockIdx.x % a.n_strips, seg = blockIdx.x / a.n_strips;
    const int lx = tid & (a.tx - 1), ly = tid >> a.tx_log2;
    const int ty = THREADS >> a.tx_log2;
    const int64_t y_lo = ((int64_t)seg * ty + ly) * RPT;
    if (y_lo >= a.h) return;
    const int64_t img0 = (int64_t)blockIdx.y * N_IMG;
    const int n_img = (int)min((int64_t)N_IMG, (int64_t)a.n_images - img0);      // >= 1: the grid has ceil(n / N_IMG) groups
    T *first = static_cast<T *>(a.tiles) + img0 * a.plane_stride;
    const T *frame = static_cast<const T *>(a.frame);
    const int y0 = (int)y_lo, y1 = min(a.h, y0 + RPT);
    for (int y = y0; y < y1; ++y) {
        T *wp = first + (int64_t)y * a.pitch;
        // elements of this row in front of a 16-byte boundary: vector k starts at column k * VEC - mis (the same in every image
        // of the group: with N_IMG > 1 the plane stride is a whole number of vectors)
        const int mis = (int)((reinterpret_cast<uintptr_t>(wp) / sizeof(T)) & (uintptr_t)(VEC - 1));
        const int64_t xa64 = ((int64_t)strip * a.tx + lx) * VEC - mis;
        if (xa64 >= a.w) continue;
        const int xa = (int)xa64;
        const int lo_x = max(xa, 0), hi_x = min(xa + VEC, a.w);
        int32_t k[CONSTANT ? 1 : VEC];
        if (CONSTANT) {
            k[0] = a.k;
        } else {
            uint32_t d[VEC];
            load_vec<T, VEC>(frame + (int64_t)y * a.frame_pitch, xa, lo_x, hi_x, d);
#pragma unroll
            for (int j = 0; j < (CONSTANT ? 1 : VEC); ++j) k[j] = a.pedestal - (int32_t)d[j];
        }
        if (hi_x - lo_x == VEC) {      // (aligned: the vectors are laid at this row's phase)
            u32x4 v[N_IMG];
#pragma unroll
            for (int i = 0; i < N_IMG; ++i)
                if (i < n_img) v[i] = *(const SQ_GLOBAL u32x4 *)(wp + (int64_t)i * a.plane_stride + xa);
#pragma unroll
            for (int i = 0; i < N_IMG; ++i)
                if (i < n_img) *(SQ_GLOBAL u32x4 *)(wp + (int64_t)i * a.plane_stride + xa) = dark_vector<T, VEC, CONSTANT>(v[i], k);
        } else {
            for (int i = 0; i < n_img; ++i) {
                T *ip = wp + (int64_t)i * a.plane_stride;
#pragma unroll
                for (int j = 0; j < VEC; ++j)
                    if (xa + j >= lo_x && xa + j < hi_x) {
                        const uint32_t in = (uint32_t)(*(const SQ_GLOBAL T *)(ip + xa + j));
                        *(SQ_GLOBAL T *)(ip + xa + j) = (T)dark_pixel<M>(in, k[CONSTANT ? 0 : j]);
                    }
            }
        }
    }
}

template <typename T, int N_IMG>
void launch(const DarkArgs &a, bool constant, dim3 grid, hipStream_t stream) {
    if (constant)
        dark_kernel<T, true, N_IMG><<<grid, dim3(THREADS), 0, stream>>>(a);
    else
        dark_kernel<T, false, N_IMG><<<grid, dim3(THREADS), 0, stream>>>(a);
}

}   // namespace

extern "C" int sq_dark_tiles(void *tiles_dev, int32_t n_images, int32_t h, int32_t w, int64_t plane_stride, int64_t pitch,
                             int32_t dtype, const void *frames_dev, int32_t n_frames, int64_t frame_stride, int64_t frame_pitch,
                             const int32_t *params_host, int32_t images_per_param, int32_t pedestal, void *stream_) {
    if (dtype != SQ_U8 && dtype != SQ_U16) return fail(SQ_ERR_INVALID, "sq_dark_tiles: dtype %d", dtype);
    const int32_t top = dtype == SQ_U16 ? 65535 : 255;
    if (pedestal < 0 || pedestal > top) return fail(SQ_ERR_INVALID, "sq_dark_tiles: pedestal %d outside 0..%d", pedestal, top);
    if (n_images < 0 || n_frames < 0 || h <= 0 || w <= 0 || h > (1 << 30) || w > (1 << 30) || pitch < w)
        return fail(SQ_ERR_INVALID, "sq_dark_tiles: bad sizes (images=%d frames=%d %dx%d pitch %lld)", n_images, n_frames, h, w,
                    (long long)pitch);
    if (images_per_param < 1 || n_images % images_per_param != 0)
        return fail(SQ_ERR_INVALID, "sq_dark_tiles: %d images are no multiple of images_per_param %d", n_images, images_per_param);
    if (n_images == 0) return SQ_OK;
    if (!tiles_dev) return fail(SQ_ERR_INVALID, "sq_dark_tiles: NULL buffer");
    if (!params_host) return fail(SQ_ERR_INVALID, "sq_dark_tiles: NULL param table");
    const int32_t n_params = n_images / images_per_param;
    bool any_frame = false;
    for (int32_t i = 0; i < n_params; ++i) {
        const int32_t k = params_host[2 * i], c = params_host[2 * i + 1];
        if (k < -1 || k >= n_frames)
            return fail(SQ_ERR_INVALID, "sq_dark_tiles: pair %d names frame %d of %d", i, k, n_frames);
        if (k >= 0 ? c != 0 : (c < 0 || c > top))
            return fail(SQ_ERR_INVALID, "sq_dark_tiles: pair %d: constant %d (0 with a frame, else 0..%d)", i, c, top);
        any_frame = any_frame || k >= 0;
    }
    const int esize = dtype == SQ_U16 ? 2 : 1;
    const PlaneBatch tiles{tiles_dev, n_images, h, w, plane_stride, pitch, esize};
    if (const int rc = check_batches("sq_dark_tiles", "plane", {tiles})) return rc;
    if (any_frame) {
        if (!frames_dev) return fail(SQ_ERR_INVALID, "sq_dark_tiles: NULL frames");
        if (frame_pitch < w) return fail(SQ_ERR_INVALID, "sq_dark_tiles: frame pitch %lld below the width %d", (long long)frame_pitch, w);
        const PlaneBatch frames{frames_dev, n_frames, h, w, frame_stride, frame_pitch, esize};
        if (const int rc = check_batches("sq_dark_tiles", "frame", {frames})) return rc;
        // the call works in place on the tiles
        if (overlap(tiles, frames)) return fail(SQ_ERR_INVALID, "sq_dark_tiles: the frames overlap the tiles");
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);

    const int vec = 16 / esize;
    DarkArgs a{};
    a.h = h;
    a.w = w;
    a.pedestal = pedestal;
    a.plane_stride = plane_stride;
    a.pitch = pitch;
    a.frame_pitch = frame_pitch;
    // vectors a row can touch: its phase is the base's in every row when pitch and plane stride are whole vectors, else any
    const bool stride_whole = n_images == 1 || plane_stride % vec == 0;
    const bool one_phase = pitch % vec == 0 && stride_whole;
    const int64_t mis = one_phase ? tiles.phase(vec) : vec - 1;
    StripGrid g;
    if (const int rc = strip_grid("sq_dark_tiles", ((int64_t)w + mis + vec - 1) / vec, THREADS, THREADS, RPT, h, &g)) return rc;
    a.tx = g.tx;
    a.tx_log2 = g.tx_log2;
    a.n_strips = g.n_strips;
    // the images a thread walks with one frame vector: they must share the row's phase
    const int ipt = stride_whole ? IPT : 1;
    // one grid per maximal run of consecutive equal pairs, none for a run that is the identity: the arguments stay scalar, no
    // table goes to the device
    return for_each_run(params_host, n_params, 2, [&](const int32_t *t, int32_t s0, int32_t s1) {
        const int32_t k = t[0], c = t[1];
        if (k < 0 && c == pedestal) return (int)SQ_OK;      // the identity: nothing is issued, the planes stay untouched
        a.k = pedestal - c;
        a.frame = k < 0 ? nullptr : static_cast<const char *>(frames_dev) + (int64_t)k * frame_stride * esize;
        return for_each_launch("sq_dark_tiles", (int64_t)s0 * images_per_param, (int64_t)s1 * images_per_param, ipt,
                               [&](int64_t p0, int32_t m, unsigned grid_y) {
            const dim3 grid(g.x(), grid_y);
            a.tiles = tiles.at(p0);
            a.n_images = m;
            if (dtype == SQ_U16) {
                if (ipt == 1) launch<uint16_t, 1>(a, k < 0, grid, stream);
                else launch<uint16_t, IPT>(a, k < 0, grid, stream);
            } else {
                if (ipt == 1) launch<uint8_t, 1>(a, k < 0, grid, stream);
                else launch<uint8_t, IPT>(a, k < 0, grid, stream);
            }
        });
    });
}

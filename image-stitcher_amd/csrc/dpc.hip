// Differential phase contrast of a batch of staged tile planes for gfx950 (--dpc): from the two half-pupil brightfield
// planes L and R of one dtype (maximum M) and an integer gain g in 1..16,
//
//     S = L + R,   N = S + 2 g (L - R)
//     DPC = 0 if S == 0, else clamp(floor(M N / (2 S)), 0, M)
//
// The reference has no counterpart; the definition is the numpy restatement in tests/dpc_ref.py.  Integers only in the
// result: deterministic, and bit for bit the definition (dpc_pixel below).  Elementwise, so out may be exactly left (in place:
// a thread reads the pixels it writes and no others); left and right are read once, out is written once.
//
// Mapping: as in despeckle.hip.  A thread owns one 16-byte vector of out columns (8 uint16 / 16 uint8) and walks down RPT rows;
// the 256 threads of a workgroup are tx vectors wide (a power of two, 256 for planes of 2048 uint16 columns and more) and
// 256 / tx runs of RPT rows tall, so narrow planes still fill the workgroup.  blockIdx.x = row segment * n_strips + strip,
// blockIdx.y = plane.  No LDS, no atomics, 30-odd registers: the occupancy is the hardware's maximum and the loads of the
// resident waves cover the latency of one another.
//
// Vectors: the vectors of a row are laid at the phase of that row of out, so every full vector of out is one 16-byte store
// whatever the base and the pitch; left and right are loaded with 16-byte loads where they have the same phase (always, for
// the stitcher's buffers), element by element where not.  The vectors a row starts and ends in are touched element by
// element: nothing outside a row is read or written, and the columns between w and out_pitch stay as they are.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_util.h"
#include "plane_batch.h"

using namespace sq;

namespace {

constexpr int THREADS = 256;
constexpr int RPT = 8;      // rows a thread walks down

struct DpcArgs {
    const void *left, *right;
    void *out;
    int64_t left_plane_stride, left_pitch;     // elements
    int64_t right_plane_stride, right_pitch;
    int64_t out_plane_stride, out_pitch;
    int32_t h, w;
    int32_t gain2;              // 2 g
    int32_t tx, tx_log2;        // vectors across a workgroup
    int32_t n_strips;
};

// One pixel.  With Nc = clamp(N, 0, 2S) and D = max(2S, 2) the definition is floor(M Nc / D) in every case: N <= 0 gives 0,
// N >= 2S gives M, and S == 0 has N == 0.  M Nc < 2^34 and D < 2^18, so the quotient q < 2^16 comes from a float estimate and
// one integer correction: Nc and D are exact floats, the two products round once each (2^-24 relative) and the reciprocal is
// good to one unit in the last place (2^-23), so the estimate is within 2^-22 * 2^16 = 2^-6 of the true quotient and its
// truncation within one of q.  The remainder M Nc - q' D of such a q' lies in [-D, 2D): it is exact in 32-bit wrap-around
// arithmetic, and its sign and its size against D say which way to step.
template <uint32_t M>
__device__ __forceinline__ uint32_t dpc_pixel(uint32_t l, uint32_t r, int32_t gain2) {
    const int32_t s2 = 2 * (int32_t)(l + r);
    const int32_t n = (int32_t)(l + r) + gain2 * ((int32_t)l - (int32_t)r);
    const uint32_t nc = (uint32_t)min(max(n, 0), s2);
    const uint32_t d = (uint32_t)max(s2, 2);
    const float est = ((float)nc * (float)M) * __builtin_amdgcn_rcpf((float)d);
    uint32_t q = (uint32_t)est;
    const int32_t rem = (int32_t)(nc * M - q * d);
    q -= rem < 0 ? 1u : 0u;
    q += rem >= (int32_t)d ? 1u : 0u;
    return q;
}

// The VEC pixels of row pointer rp that start at column xa -> v[], 16-byte load where the vector is whole and aligned,
// else element by element over the columns [lo_x, hi_x) the vector has inside the row (the others stay 0).
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

template <typename T>
__global__ __launch_bounds__(THREADS) void dpc_kernel(const DpcArgs a) {
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr uint32_t M = sizeof(T) == 2 ? 65535u : 255u;
    const int tid = threadIdx.x;
    const int strip = blockIdx.x % a.n_strips, seg = blockIdx.x / a.n_strips;
    const int lx = tid & (a.tx - 1), ly = tid >> a.tx_log2;
    const int ty = THREADS >> a.tx_log2;
    const int64_t y_lo = ((int64_t)seg * ty + ly) * RPT;
    if (y_lo >= a.h) return;
    const T *left = static_cast<const T *>(a.left) + (int64_t)blockIdx.y * a.left_plane_stride;
    const T *right = static_cast<const T *>(a.right) + (int64_t)blockIdx.y * a.right_plane_stride;
    T *out = static_cast<T *>(a.out) + (int64_t)blockIdx.y * a.out_plane_stride;
    const int y0 = (int)y_lo, y1 = min(a.h, y0 + RPT);
    for (int y = y0; y < y1; ++y) {
        T *wp = out + (int64_t)y * a.out_pitch;
        // elements of this row of out in front of a 16-byte boundary: vector k starts at column k * VEC - mis
        const int mis = (int)((reinterpret_cast<uintptr_t>(wp) / sizeof(T)) & (uintptr_t)(VEC - 1));
        const int64_t xa64 = ((int64_t)strip * a.tx + lx) * VEC - mis;
        if (xa64 >= a.w) continue;
        const int xa = (int)xa64;
        const int lo_x = max(xa, 0), hi_x = min(xa + VEC, a.w);
        uint32_t l[VEC], r[VEC], o[VEC];
        load_vec<T, VEC>(left + (int64_t)y * a.left_pitch, xa, lo_x, hi_x, l);
        load_vec<T, VEC>(right + (int64_t)y * a.right_pitch, xa, lo_x, hi_x, r);
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = dpc_pixel<M>(l[j], r[j], a.gain2);
        if (hi_x - lo_x == VEC) {      // (aligned: the vectors are laid at this row's phase)
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

}   // namespace

extern "C" int sq_dpc_tiles(const void *left_dev, const void *right_dev, void *out_dev, int32_t n_images, int32_t h, int32_t w,
                            int64_t left_plane_stride, int64_t left_pitch, int64_t right_plane_stride, int64_t right_pitch,
                            int64_t out_plane_stride, int64_t out_pitch, int32_t dtype, int32_t gain, void *stream_) {
    if (dtype != SQ_U8 && dtype != SQ_U16) return fail(SQ_ERR_INVALID, "sq_dpc_tiles: dtype %d", dtype);
    if (gain < 1 || gain > SQ_DPC_MAX_GAIN) return fail(SQ_ERR_INVALID, "sq_dpc_tiles: gain %d outside 1..%d", gain, SQ_DPC_MAX_GAIN);
    if (n_images < 0 || h <= 0 || w <= 0 || h > (1 << 30) || w > (1 << 30) || left_pitch < w || right_pitch < w || out_pitch < w)
        return fail(SQ_ERR_INVALID, "sq_dpc_tiles: bad sizes (images=%d %dx%d pitches %lld, %lld, %lld)", n_images, h, w,
                    (long long)left_pitch, (long long)right_pitch, (long long)out_pitch);
    if (n_images == 0) return SQ_OK;
    if (!left_dev || !right_dev || !out_dev) return fail(SQ_ERR_INVALID, "sq_dpc_tiles: NULL buffer");
    const int esize = dtype == SQ_U16 ? 2 : 1;
    const PlaneBatch left{left_dev, n_images, h, w, left_plane_stride, left_pitch, esize};
    const PlaneBatch right{right_dev, n_images, h, w, right_plane_stride, right_pitch, esize};
    const PlaneBatch out{out_dev, n_images, h, w, out_plane_stride, out_pitch, esize};
    if (const int rc = check_batches("sq_dpc_tiles", "plane", {left, right, out})) return rc;
    // out is exactly left (in place; a single plane's stride is never used), or its extent meets neither input's
    const bool in_place = out_dev == left_dev && out_pitch == left_pitch && (n_images == 1 || out_plane_stride == left_plane_stride);
    if (!in_place && overlap(left, out))
        return fail(SQ_ERR_INVALID, "sq_dpc_tiles: out overlaps left without being exactly left (base, plane stride, pitch)");
    if (overlap(right, out)) return fail(SQ_ERR_INVALID, "sq_dpc_tiles: out overlaps right");
    hipStream_t stream = static_cast<hipStream_t>(stream_);

    const int vec = 16 / esize;
    DpcArgs a{};
    a.h = h;
    a.w = w;
    a.gain2 = 2 * gain;
    // vectors a row can touch: its phase is the base's in every row when pitch and plane stride are whole vectors, else any
    const bool one_phase = out_pitch % vec == 0 && (n_images == 1 || out_plane_stride % vec == 0);
    const int64_t mis = one_phase ? out.phase(vec) : vec - 1;
    StripGrid g;
    if (const int rc = strip_grid("sq_dpc_tiles", ((int64_t)w + mis + vec - 1) / vec, THREADS, THREADS, RPT, h, &g)) return rc;
    a.tx = g.tx;
    a.tx_log2 = g.tx_log2;
    a.n_strips = g.n_strips;
    a.left_plane_stride = left_plane_stride;
    a.left_pitch = left_pitch;
    a.right_plane_stride = right_plane_stride;
    a.right_pitch = right_pitch;
    a.out_plane_stride = out_plane_stride;
    a.out_pitch = out_pitch;
    return for_each_launch("sq_dpc_tiles", 0, n_images, 1, [&](int64_t p0, int32_t, unsigned grid_y) {
        const dim3 grid(g.x(), grid_y);
        a.left = left.at(p0);
        a.right = right.at(p0);
        a.out = out.at(p0);
        if (dtype == SQ_U16)
            dpc_kernel<uint16_t><<<grid, dim3(THREADS), 0, stream>>>(a);
        else
            dpc_kernel<uint8_t><<<grid, dim3(THREADS), 0, stream>>>(a);
    });
}

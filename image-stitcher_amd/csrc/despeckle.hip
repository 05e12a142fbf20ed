// Hot-pixel removal of a batch of staged tile planes for gfx950, out of place (--despeckle):
//
//     m(y, x) = the median of the nine values I(clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1)), dy, dx in {-1, 0, 1}
//     hot :  out = m if I - m > T    else I
//     both:  out = m if |I - m| > T  else I
//
// The reference has no counterpart; the definition is the numpy restatement in tests/despeckle_ref.py.  Integers only; the one
// atomic is an integer add: deterministic.  Every m comes from the unfiltered plane, so the kernel is out of place: a stencil
// written in place races with the neighbouring workgroup's halo reads.  src is read once (plus one halo row above and below
// a thread's rows, and one pixel left and right of its vector), dst is written once.
//
// Mapping: a thread owns one 16-byte vector of dst columns (8 uint16 / 16 uint8) and walks down RPT rows with the rows y - 1, y,
// y + 1 of its columns and of one column left and right in registers: nothing crosses threads and no pixel goes through LDS.
// The 256 threads of a workgroup are tx vectors wide (a power of two, 256 for planes of 2048 uint16 columns and more) and
// 256 / tx runs of RPT rows tall, so narrow planes still fill the workgroup.  blockIdx.x = row segment * n_strips + strip.
//
// Median: the three values of each column are sorted once (lo, mid, hi: they are shared by the three windows the column is
// part of); the median of nine is then med3(max3(lo), med3(mid), min3(hi)) over the window's three columns.
//
// Vectors: the vectors are laid at the phase of dst's first row, so a dst whose pitch and plane stride are multiples of a
// vector is stored with 16-byte stores throughout; src is loaded with 16-byte loads in the rows where it has the same phase,
// element by element in the others.  The vectors a row starts and ends in are touched element by element, and every
// neighbour column is clamped into the row first: nothing outside a row is read or written, and the columns between W and
// the pitch of dst stay as they are.
//
// Counts: a thread counts what it replaced, the workgroup adds that up in one LDS word and does one 64-bit atomic add into
// counts[plane] (none when it replaced nothing, or when counts is NULL).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_util.h"
#include "plane_batch.h"

using namespace sq;

namespace {

constexpr int THREADS = 256;
constexpr int RPT = 32;     // rows a thread walks down (each run re-reads two halo rows: 6 % of the reads)

struct DespeckleArgs {
    const void *src;
    int64_t src_plane_stride, src_pitch;   // elements
    void *dst;
    int64_t dst_plane_stride, dst_pitch;
    unsigned long long *counts;            // [planes of this launch], or NULL
    int32_t h, w, threshold;
    int32_t mis;                // elements of dst's first row in front of a 16-byte boundary: vector k starts at column k * VEC - mis
    int32_t tx, tx_log2;        // vectors across a workgroup
    int32_t n_strips;
};

__device__ __forceinline__ uint32_t med3(uint32_t a, uint32_t b, uint32_t c) {
    return max(min(a, b), min(max(a, b), c));
}

// Columns xa - 1 ... xa + VEC of row y (both clamped into the plane) -> r[0 ... VEC + 1].  The two neighbour columns go one
// way whatever the vector's path is, and every element of r is written once with a constant index: r stays in registers.
template <typename T, int VEC>
__device__ __forceinline__ void load_row(const T *__restrict__ plane, int64_t pitch, int y, int h, int w, int xa, uint32_t (&r)[VEC + 2]) {
    const int yc = min(max(y, 0), h - 1);
    const T *rp = plane + (int64_t)yc * pitch;
    const uint32_t left = (uint32_t)(*(const SQ_GLOBAL T *)(rp + min(max(xa - 1, 0), w - 1)));
    const uint32_t right = (uint32_t)(*(const SQ_GLOBAL T *)(rp + min(max(xa + VEC, 0), w - 1)));
    u32x4 d;
    if (xa >= 0 && xa + VEC <= w && (reinterpret_cast<uintptr_t>(rp + xa) & 15) == 0) {
        d = *(const SQ_GLOBAL u32x4 *)(rp + xa);
    } else {   // the vector a row starts or ends in, or a row of another phase: element by element, packed like the vector
        uint32_t q0 = 0, q1 = 0, q2 = 0, q3 = 0;
        constexpr int PER = VEC / 4, BITS = 8 * (int)sizeof(T);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            q0 |= (uint32_t)(*(const SQ_GLOBAL T *)(rp + min(max(xa + k, 0), w - 1))) << (BITS * k);
            q1 |= (uint32_t)(*(const SQ_GLOBAL T *)(rp + min(max(xa + PER + k, 0), w - 1))) << (BITS * k);
            q2 |= (uint32_t)(*(const SQ_GLOBAL T *)(rp + min(max(xa + 2 * PER + k, 0), w - 1))) << (BITS * k);
            q3 |= (uint32_t)(*(const SQ_GLOBAL T *)(rp + min(max(xa + 3 * PER + k, 0), w - 1))) << (BITS * k);
        }
        d.x = q0;
        d.y = q1;
        d.z = q2;
        d.w = q3;
    }
    const uint32_t dq[4] = {d.x, d.y, d.z, d.w};
    r[0] = left;
    r[VEC + 1] = right;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (sizeof(T) == 2) {
            r[1 + 2 * q] = dq[q] & 0xffffu;
            r[2 + 2 * q] = dq[q] >> 16;
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) r[1 + 4 * q + s] = (dq[q] >> (8 * s)) & 0xffu;
        }
    }
}

template <typename T, bool BOTH>
__global__ __launch_bounds__(THREADS) void despeckle_kernel(const DespeckleArgs a) {
    constexpr int VEC = 16 / (int)sizeof(T);
    __shared__ uint32_t replaced;
    const int tid = threadIdx.x;
    if (tid == 0) replaced = 0;
    lds_written();
    __syncthreads();

    const int strip = blockIdx.x % a.n_strips, seg = blockIdx.x / a.n_strips;
    const int lx = tid & (a.tx - 1), ly = tid >> a.tx_log2;
    const int ty = THREADS >> a.tx_log2;
    const int xa = (strip * a.tx + lx) * VEC - a.mis;       // the vector's first column (negative: it starts in front of the row)
    const int64_t y_lo = ((int64_t)seg * ty + ly) * RPT;
    const T *__restrict__ src = static_cast<const T *>(a.src) + (int64_t)blockIdx.y * a.src_plane_stride;
    T *__restrict__ dst = static_cast<T *>(a.dst) + (int64_t)blockIdx.y * a.dst_plane_stride;
    const int T_ = a.threshold;

    uint32_t n = 0;
    if (xa < a.w && xa + VEC > 0 && y_lo < a.h) {
        const int y0 = (int)y_lo, y1 = min(a.h, y0 + RPT);
        const int lo_x = max(xa, 0), hi_x = min(xa + VEC, a.w);
        uint32_t A[VEC + 2], B[VEC + 2], C[VEC + 2];
        load_row<T, VEC>(src, a.src_pitch, y0 - 1, a.h, a.w, xa, A);
        load_row<T, VEC>(src, a.src_pitch, y0, a.h, a.w, xa, B);
        for (int y = y0; y < y1; ++y) {
            load_row<T, VEC>(src, a.src_pitch, y + 1, a.h, a.w, xa, C);
            uint32_t lo[VEC + 2], mid[VEC + 2], hi[VEC + 2];
#pragma unroll
            for (int k = 0; k < VEC + 2; ++k) {
                const uint32_t mn = min(A[k], B[k]), mx = max(A[k], B[k]);
                lo[k] = min(mn, C[k]);
                hi[k] = max(mx, C[k]);
                mid[k] = max(mn, min(mx, C[k]));
            }
            uint32_t o[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const uint32_t m = med3(max(max(lo[j], lo[j + 1]), lo[j + 2]), med3(mid[j], mid[j + 1], mid[j + 2]),
                                        min(min(hi[j], hi[j + 1]), hi[j + 2]));
                const int c = (int)B[j + 1];
                const int d = c - (int)m;
                const bool fire = (BOTH ? abs(d) : d) > T_;
                o[j] = fire ? m : (uint32_t)c;
                // (a vector that starts or ends outside the row computes clamped columns it does not own: not counted)
                n += (fire && xa + j >= lo_x && xa + j < hi_x) ? 1u : 0u;
            }
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
#pragma unroll
            for (int k = 0; k < VEC + 2; ++k) {
                A[k] = B[k];
                B[k] = C[k];
            }
        }
    }
    if (n) atomicAdd(&replaced, n);
    lds_written();
    __syncthreads();
    if (tid == 0 && a.counts != nullptr && replaced != 0) atomicAdd(a.counts + blockIdx.y, (unsigned long long)replaced);
}

}   // namespace

extern "C" int sq_despeckle_tiles(const void *src_dev, void *dst_dev, int32_t n_images, int32_t h, int32_t w,
                                  int64_t src_plane_stride, int64_t src_pitch, int64_t dst_plane_stride, int64_t dst_pitch,
                                  int32_t dtype, int32_t mode, int32_t threshold, uint64_t *counts_dev, void *stream_) {
    if (dtype != SQ_U8 && dtype != SQ_U16) return fail(SQ_ERR_INVALID, "sq_despeckle_tiles: dtype %d", dtype);
    if (mode != SQ_DESPECKLE_HOT && mode != SQ_DESPECKLE_BOTH) return fail(SQ_ERR_INVALID, "sq_despeckle_tiles: mode %d", mode);
    if (threshold < 0 || threshold > 65535) return fail(SQ_ERR_INVALID, "sq_despeckle_tiles: threshold %d outside 0..65535", threshold);
    if (n_images < 0 || h <= 0 || w <= 0 || h > (1 << 30) || w > (1 << 30) || src_pitch < w || dst_pitch < w)
        return fail(SQ_ERR_INVALID, "sq_despeckle_tiles: bad sizes (images=%d %dx%d pitches %lld, %lld)", n_images, h, w,
                    (long long)src_pitch, (long long)dst_pitch);
    if (n_images == 0) return SQ_OK;
    if (!src_dev || !dst_dev) return fail(SQ_ERR_INVALID, "sq_despeckle_tiles: NULL buffer");
    if (reinterpret_cast<uintptr_t>(counts_dev) % 8) return fail(SQ_ERR_INVALID, "sq_despeckle_tiles: the counts must be aligned to 8 bytes");
    const int esize = dtype == SQ_U16 ? 2 : 1;
    const PlaneBatch src{src_dev, n_images, h, w, src_plane_stride, src_pitch, esize};
    const PlaneBatch dst{dst_dev, n_images, h, w, dst_plane_stride, dst_pitch, esize};
    if (const int rc = check_batches("sq_despeckle_tiles", "plane", {src, dst})) return rc;
    // the stencil reads what a neighbour writes
    if (overlap(src, dst)) return fail(SQ_ERR_INVALID, "sq_despeckle_tiles: src and dst overlap (the filter is out of place)");
    hipStream_t stream = static_cast<hipStream_t>(stream_);

    const int vec = 16 / esize;
    DespeckleArgs a{};
    a.h = h;
    a.w = w;
    a.threshold = threshold;
    a.mis = dst.phase(vec);
    StripGrid g;
    if (const int rc = strip_grid("sq_despeckle_tiles", ((int64_t)w + a.mis + vec - 1) / vec, THREADS, THREADS, RPT, h, &g)) return rc;
    a.tx = g.tx;
    a.tx_log2 = g.tx_log2;
    a.n_strips = g.n_strips;
    a.src_plane_stride = src_plane_stride;
    a.src_pitch = src_pitch;
    a.dst_plane_stride = dst_plane_stride;
    a.dst_pitch = dst_pitch;
    return for_each_launch("sq_despeckle_tiles", 0, n_images, 1, [&](int64_t p0, int32_t, unsigned grid_y) {
        const dim3 grid(g.x(), grid_y);
        a.src = src.at(p0);
        a.dst = dst.at(p0);
        a.counts = counts_dev ? reinterpret_cast<unsigned long long *>(counts_dev) + p0 : nullptr;
        if (dtype == SQ_U16) {
            if (mode == SQ_DESPECKLE_BOTH)
                despeckle_kernel<uint16_t, true><<<grid, dim3(THREADS), 0, stream>>>(a);
            else
                despeckle_kernel<uint16_t, false><<<grid, dim3(THREADS), 0, stream>>>(a);
        } else {
            if (mode == SQ_DESPECKLE_BOTH)
                despeckle_kernel<uint8_t, true><<<grid, dim3(THREADS), 0, stream>>>(a);
            else
                despeckle_kernel<uint8_t, false><<<grid, dim3(THREADS), 0, stream>>>(a);
        }
    });
}

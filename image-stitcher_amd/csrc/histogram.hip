// Exact value histograms of a batch of 2-D planes for gfx950, added into caller-owned 64-bit rows:
//
//     hist[row_of_plane[p]][v] += #{ (y, x) : planes[p][y][x] == v }
//
// The reference has no counterpart: its OME-Zarr channel windows are np.iinfo(self.dtype).max (stitcher.py:846-850).  The
// histograms are what --contrast-limits percentile turns into per-channel windows (omezarr.contrast_window).
//
// Roofline: HBM, a pure read of level 0.  What keeps a histogram from that roof is atomics, so every count goes through LDS
// first and reaches global memory once per non-empty bin and workgroup (integer adds: the result does not depend on order).
//
// Mapping: one workgroup of 16 waves per CU, each with a contiguous share of the batch's rows.  A row is cut into the
// 16-byte-aligned vectors it touches ("slots", the same number for every row; the first and last slot of a row are partial and
// are read element by element), the slots of the share are dealt to the threads in flat order, four 16-byte loads per thread in
// flight per step.
//   uint16: the workgroup's LDS holds ALL 65536 bins as 16-bit counters, two per dword (128 KiB).  A step adds at most
//           1024 threads x 4 loads x 8 elements = 32768 counts, and a barrier ends it.  The add that takes a counter from below
//           0x8000 to 0x8000 or above (ds_add_rtn returns the old value, so exactly one add sees that) subtracts 0x8000 again
//           and adds 32768 to the global bin; every counter is therefore below 0x8000 at each barrier, stays below 0x10000
//           within a step, and never carries into its neighbour.
//   uint8 : 256 bins as 32-bit counters, 64 copies (wave x lane & 3, interleaved so that the copies of one value lie in
//           different banks), flushed before 2^31 elements.
// Long runs (the zero canvas outside the tiles, saturated areas): a wave whose 64 vectors all hold one value makes ONE add of
// 512 (1024).  The clustered bulk: a lane counts equal values among its 8 elements first and adds each distinct value once.
// Any value anywhere costs one LDS add, never a global one.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "device_util.h"

using namespace sq;

namespace {

constexpr int THREADS = 1024;
constexpr int WAVES = THREADS / 64;
constexpr int LOADS = 4;           // 16-byte loads per thread and step
constexpr int MAX_PLANES = 64;     // planes per launch (their rows travel in the kernel arguments)
static_assert(THREADS * LOADS * 8 <= 32768, "uint16: a step must add fewer than 2^15 + 1 counts");

template <typename T>
struct Lds;
template <>
struct Lds<uint16_t> {
    static constexpr int BINS = 65536, WORDS = 32768;
};
template <>
struct Lds<uint8_t> {
    static constexpr int BINS = 256, WORDS = WAVES * 4 * 256;
};

struct HistArgs {
    const void *src;
    int64_t plane_stride, pitch;   // elements
    int32_t h, w;
    int64_t total_rows;            // n_planes * h
    unsigned long long *hist;
    int32_t row_of_plane[MAX_PLANES];
};

// n counts of value v
template <typename T>
__device__ __forceinline__ void add(uint32_t *lds, unsigned long long *grow, uint32_t v, uint32_t n);
template <>
__device__ __forceinline__ void add<uint16_t>(uint32_t *lds, unsigned long long *grow, uint32_t v, uint32_t n) {
    const uint32_t sh = (v & 1u) * 16u;
    const uint32_t old = atomicAdd(&lds[v >> 1], n << sh);
    const uint32_t oh = (old >> sh) & 0xffffu;
    if (oh < 0x8000u && oh + n >= 0x8000u) {
        atomicSub(&lds[v >> 1], 0x8000u << sh);
        atomicAdd(&grow[v], 32768ull);
    }
}
template <>
__device__ __forceinline__ void add<uint8_t>(uint32_t *lds, unsigned long long *, uint32_t v, uint32_t n) {
    atomicAdd(&lds[(threadIdx.x >> 6) * 1024 + v * 4 + (threadIdx.x & 3)], n);
}

// LDS counters -> the global row, LDS zeroed.  All threads.
template <typename T>
__device__ __forceinline__ void flush(uint32_t *lds, unsigned long long *grow) {
    lds_written();
    __syncthreads();
    if (sizeof(T) == 2) {
        for (int i = threadIdx.x; i < Lds<T>::WORDS; i += THREADS) {
            const uint32_t c = lds[i];
            if (c) {
                if (c & 0xffffu) atomicAdd(&grow[2 * i], (unsigned long long)(c & 0xffffu));
                if (c >> 16) atomicAdd(&grow[2 * i + 1], (unsigned long long)(c >> 16));
                lds[i] = 0u;
            }
        }
    } else {
        if (threadIdx.x < 256) {
            unsigned long long s = 0;
            for (int wv = 0; wv < WAVES; ++wv)
                for (int k = 0; k < 4; ++k) s += lds[wv * 1024 + threadIdx.x * 4 + k];
            if (s) atomicAdd(&grow[threadIdx.x], s);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < Lds<T>::WORDS; i += THREADS) lds[i] = 0u;
    }
    __syncthreads();
}

// The VEC elements of one full vector.
template <typename T>
__device__ __forceinline__ void add_vector(uint32_t *lds, unsigned long long *grow, const u32x4 d);
template <>
__device__ __forceinline__ void add_vector<uint16_t>(uint32_t *lds, unsigned long long *grow, const u32x4 d) {
    uint32_t e[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        e[2 * i] = d[i] & 0xffffu;
        e[2 * i + 1] = d[i] >> 16;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        bool seen = false;
        uint32_t n = 1;
#pragma unroll
        for (int j = 0; j < i; ++j) seen |= e[j] == e[i];
#pragma unroll
        for (int j = i + 1; j < 8; ++j) n += (e[j] == e[i]) ? 1u : 0u;
        if (!seen) add<uint16_t>(lds, grow, e[i], n);
    }
}
template <>
__device__ __forceinline__ void add_vector<uint8_t>(uint32_t *lds, unsigned long long *grow, const u32x4 d) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t b0 = d[i] & 0xffu, b1 = (d[i] >> 8) & 0xffu, b2 = (d[i] >> 16) & 0xffu, b3 = d[i] >> 24;
        // the four bytes of a dword: equal neighbours are counted together
        if (b0 == b1 && b2 == b3) {
            if (b0 == b2) {
                add<uint8_t>(lds, grow, b0, 4);
            } else {
                add<uint8_t>(lds, grow, b0, 2);
                add<uint8_t>(lds, grow, b2, 2);
            }
        } else {
            add<uint8_t>(lds, grow, b0, 1);
            add<uint8_t>(lds, grow, b1, 1);
            add<uint8_t>(lds, grow, b2, 1);
            add<uint8_t>(lds, grow, b3, 1);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(THREADS) void histogram_kernel(const HistArgs a) {
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr int BINS = Lds<T>::BINS;
    __shared__ uint32_t lds[Lds<T>::WORDS];
    const int tid = threadIdx.x;
    for (int i = tid; i < Lds<T>::WORDS; i += THREADS) lds[i] = 0u;
    __syncthreads();

    const T *src = static_cast<const T *>(a.src);
    // slots of a row: the aligned 16-byte vectors it can touch at any phase
    const int32_t S = (a.w + 2 * VEC - 2) / VEC;
    const int32_t step_rows = THREADS / S, step_slots = THREADS % S;
    const int64_t r_begin = a.total_rows * (int64_t)blockIdx.x / gridDim.x;
    const int64_t r_end = a.total_rows * ((int64_t)blockIdx.x + 1) / gridDim.x;
    int cur = -1;
    unsigned long long *grow = a.hist;
    int64_t since_flush = 0;   // uint8: elements counted since the last flush

    for (int64_t r = r_begin; r < r_end;) {
        const int64_t plane = r / a.h;
        const int32_t y0 = (int32_t)(r - plane * a.h);
        const int32_t nrows = (int32_t)std::min<int64_t>(a.h - y0, r_end - r);
        r += nrows;
        const int hr = a.row_of_plane[plane];
        if (hr != cur) {
            if (cur >= 0) flush<T>(lds, grow);
            cur = hr;
            grow = a.hist + (int64_t)hr * BINS;
            since_flush = 0;
        }
        const T *base = src + plane * a.plane_stride + (int64_t)y0 * a.pitch;
        const int64_t n_slots = (int64_t)nrows * S;
        int32_t row = tid / S, slot = tid % S;   // this thread's next slot
        for (int64_t done = 0; done < n_slots; done += (int64_t)THREADS * LOADS) {
            if (sizeof(T) == 1) {
                since_flush += (int64_t)THREADS * LOADS * VEC;
                if (since_flush > (1ll << 31)) {
                    flush<T>(lds, grow);
                    since_flush = (int64_t)THREADS * LOADS * VEC;
                }
            }
            u32x4 d[LOADS];
            uint32_t full = 0;
#pragma unroll
            for (int k = 0; k < LOADS; ++k) {
                d[k] = u32x4{0u, 0u, 0u, 0u};
                if (row < nrows) {
                    const T *rp = base + (int64_t)row * a.pitch;
                    const int mis = (int)((reinterpret_cast<uintptr_t>(rp) / sizeof(T)) & (VEC - 1));
                    const int e0 = slot * VEC - mis;   // the slot's first element, in the row's coordinates
                    if (e0 >= 0 && e0 + VEC <= a.w) {
                        d[k] = *(const SQ_GLOBAL u32x4 *)(rp + e0);
                        full |= 1u << k;
                    } else {   // the slot a row starts or ends in: element by element
                        const int lo = max(e0, 0), hi = min(e0 + VEC, a.w);
                        for (int e = lo; e < hi; ++e) add<T>(lds, grow, (uint32_t)(*(const SQ_GLOBAL T *)(rp + e)), 1u);
                    }
                }
                row += step_rows;
                slot += step_slots;
                if (slot >= S) {
                    slot -= S;
                    ++row;
                }
            }
#pragma unroll
            for (int k = 0; k < LOADS; ++k) {
                const bool f = (full >> k) & 1u;
                const uint32_t d0 = __builtin_amdgcn_readfirstlane(d[k][0]);
                const bool splat = sizeof(T) == 2 ? (d0 & 0xffffu) == (d0 >> 16) : d0 == (d0 & 0xffu) * 0x01010101u;
                const bool same = f && splat && d[k][0] == d0 && d[k][1] == d0 && d[k][2] == d0 && d[k][3] == d0;
                if (__all(same)) {   // the whole wave holds one value
                    if ((tid & 63) == 0) add<T>(lds, grow, d0 & (BINS - 1), 64u * VEC);
                } else if (f) {
                    add_vector<T>(lds, grow, d[k]);
                }
            }
            if (sizeof(T) == 2) lds_written();
            if (sizeof(T) == 2) __syncthreads();   // bounds what a 16-bit counter takes between two checks
        }
    }
    if (cur >= 0) flush<T>(lds, grow);
}

int compute_units() {
    static int cus = 0;
    if (!cus) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
            cus = n;
        else
            return 256;
    }
    return cus;
}

}   // namespace

extern "C" int sq_histogram_planes(const void *planes_dev, int64_t plane_stride, int32_t h, int32_t w, int64_t pitch,
                                   int32_t n_planes, int32_t dtype, const int32_t *row_of_plane, int32_t n_rows,
                                   uint64_t *hist_dev, void *stream_) {
    if (dtype != SQ_U8 && dtype != SQ_U16) return fail(SQ_ERR_UNSUPPORTED, "sq_histogram_planes: dtype %d", dtype);
    if (n_planes < 0 || h <= 0 || w <= 0 || h > (1 << 30) || w > (1 << 30) || pitch < w || n_rows <= 0)
        return fail(SQ_ERR_INVALID, "sq_histogram_planes: bad sizes (planes=%d %dx%d pitch %lld rows=%d)", n_planes, h, w,
                    (long long)pitch, n_rows);
    if (n_planes == 0) return SQ_OK;
    if (!planes_dev || !row_of_plane || !hist_dev) return fail(SQ_ERR_INVALID, "sq_histogram_planes: NULL buffer");
    if (n_planes > 1 && plane_stride < (int64_t)h * pitch)
        return fail(SQ_ERR_INVALID, "sq_histogram_planes: plane stride smaller than a plane");
    const int esize = dtype == SQ_U16 ? 2 : 1;
    if (reinterpret_cast<uintptr_t>(planes_dev) % esize || reinterpret_cast<uintptr_t>(hist_dev) % 8)
        return fail(SQ_ERR_INVALID, "sq_histogram_planes: planes must be aligned to their element, the histogram to 8 bytes");
    for (int32_t p = 0; p < n_planes; ++p)
        if (row_of_plane[p] < 0 || row_of_plane[p] >= n_rows)
            return fail(SQ_ERR_INVALID, "sq_histogram_planes: row_of_plane[%d] = %d is outside [0, %d)", p, row_of_plane[p], n_rows);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int vec = 16 / esize;
    const int64_t slots_per_row = (w + 2 * vec - 2) / vec;
    for (int32_t p0 = 0; p0 < n_planes; p0 += MAX_PLANES) {
        const int32_t m = std::min<int32_t>(MAX_PLANES, n_planes - p0);
        HistArgs a{};
        a.src = static_cast<const char *>(planes_dev) + (int64_t)p0 * plane_stride * esize;
        a.plane_stride = plane_stride;
        a.pitch = pitch;
        a.h = h;
        a.w = w;
        a.total_rows = (int64_t)m * h;
        a.hist = reinterpret_cast<unsigned long long *>(hist_dev);
        for (int32_t p = 0; p < m; ++p) a.row_of_plane[p] = row_of_plane[p0 + p];
        // one workgroup per CU (its LDS holds every bin); fewer when there is less than a step's work for each
        const int64_t steps = (a.total_rows * slots_per_row + THREADS * LOADS - 1) / (THREADS * LOADS);
        const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>({(int64_t)compute_units(), steps, a.total_rows}));
        if (dtype == SQ_U16)
            histogram_kernel<uint16_t><<<dim3((unsigned)blocks), dim3(THREADS), 0, stream>>>(a);
        else
            histogram_kernel<uint8_t><<<dim3((unsigned)blocks), dim3(THREADS), 0, stream>>>(a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(SQ_ERR_HIP, "sq_histogram_planes: launch failed: %s", hipGetErrorString(e));
    }
    return SQ_OK;
}

// Host side of packed_stream.h -- the grid, the argument checks and the empty geometry of the packed-stream encoders -- and
// their one scan kernel.  The refusal texts are part of the interface: tests pin them and which one wins.
#include "packed_stream.h"

namespace sq {

namespace {

// exclusive scan of n sizes in place -> offsets[0..n], one workgroup (n is a few hundred thousand at most)
__global__ __launch_bounds__(1024) void packed_scan_kernel(uint64_t *v, int64_t n, int64_t capacity, uint32_t *status) {
    __shared__ uint64_t part[1024];
    const int tid = threadIdx.x;
    const int64_t per = (n + 1023) / 1024, lo = min(n, tid * per), hi = min(n, lo + per);
    uint64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += v[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        uint64_t run = 0;
        for (int i = 0; i < 1024; ++i) {
            const uint64_t t = part[i];
            part[i] = run;
            run += t;
        }
        v[n] = run;
        if ((int64_t)run > capacity) *status = 1u;
    }
    __syncthreads();
    uint64_t run = part[tid];
    for (int64_t i = lo; i < hi; ++i) {
        const uint64_t t = v[i];
        v[i] = run;
        run += t;
    }
}

}  // namespace

int stream_grid(TileGrid &G, int64_t &n_tiles, const char *codec, const char *what, bool by8, int32_t h, int32_t w, int32_t n_planes,
                int32_t th, int32_t tw) {
    const int step = by8 ? 8 : 1;
    if (h < 1 || w < 1 || n_planes < 0 || th < step || tw < step || th % step || tw % step)
        return fail(SQ_ERR_INVALID, "%s: bad sizes (%dx%d planes %d %s %dx%d%s)", codec, h, w, n_planes, what, th, tw,
                    by8 ? ": tile sides are multiples of 8" : "");
    G.th = th;                   // as given: a tile is always full, zero-padded past the plane's edge (for Blosc the caller clamps
    G.tw = tw;                   // a chunk dimension to the ARRAY's, zarr's rule -- a row band of a plane is shorter than that)
    G.nty = (h + th - 1) / th;
    G.ntx = (w + tw - 1) / tw;
    n_tiles = (int64_t)n_planes * G.nty * G.ntx;
    return SQ_OK;
}

int stream_byte_parts(const TileGrid &G, const char *codec, const char *what, int32_t dtype, int32_t &esz, int32_t &tile_bytes,
                      int32_t &parts) {
    constexpr int PART = 16384;
    if (dtype != SQ_U8 && dtype != SQ_U16) return fail(SQ_ERR_UNSUPPORTED, "%s: dtype %d (uint8 / uint16 planes)", codec, dtype);
    esz = dtype == SQ_U16 ? 2 : 1;
    const int64_t tb = (int64_t)G.th * G.tw * esz;
    if (tb > (int64_t)2048 * PART) return fail(SQ_ERR_UNSUPPORTED, "%s: %s of %lld bytes (at most 32 MiB)", codec, what, (long long)tb);
    tile_bytes = (int32_t)tb;
    parts = (int32_t)((tb + PART - 1) / PART);
    return SQ_OK;
}

int stream_null(const char *fn, const void *planes, const void *scratch, const void *offsets, const void *out, const void *status) {
    if (!planes || !scratch || !offsets || !out || !status) return fail(SQ_ERR_INVALID, "%s: NULL argument", fn);
    return SQ_OK;
}

int stream_args(const char *fn, PackedOut &O, int32_t n_planes, int32_t h, int32_t w, int64_t plane_stride, int64_t pitch,
                const void *scratch, int64_t scratch_bytes, int64_t need, uint64_t *offsets, void *out, int64_t out_capacity,
                uint32_t *status) {
    if (out_capacity < 0) return fail(SQ_ERR_INVALID, "%s: negative out_capacity", fn);
    if (pitch < w || (n_planes > 1 && plane_stride < (int64_t)(h - 1) * pitch + w))
        return fail(SQ_ERR_INVALID, "%s: pitch / plane stride smaller than the plane", fn);
    if (scratch_bytes < need) return fail(SQ_ERR_WORKSPACE, "%s: scratch %lld < %lld bytes", fn, (long long)scratch_bytes, (long long)need);
    if (reinterpret_cast<uintptr_t>(scratch) % 256 || reinterpret_cast<uintptr_t>(offsets) % 8)
        return fail(SQ_ERR_INVALID, "%s: scratch must be 256-byte, offsets 8-byte aligned", fn);
    O.offsets = offsets;
    O.out = static_cast<uint8_t *>(out);
    O.out_capacity = out_capacity;
    O.status = status;
    return SQ_OK;
}

int stream_begin(const char *fn, const PackedOut &O, int64_t n_tiles, hipStream_t s) {
    const hipError_t e = n_tiles == 0 ? hipMemsetAsync(O.offsets, 0, 8, s) : hipMemsetAsync(O.tile_any, 0, (size_t)n_tiles * 4, s);
    if (e != hipSuccess || hipMemsetAsync(O.status, 0, 4, s) != hipSuccess) return fail(SQ_ERR_HIP, "%s: memset", fn);
    return SQ_OK;
}

void stream_scan(const PackedOut &O, int64_t n_tiles, hipStream_t s) {
    hipLaunchKernelGGL(packed_scan_kernel, dim3(1), dim3(1024), 0, s, O.offsets, n_tiles, O.out_capacity, O.status);
}

int stream_end(const char *fn) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SQ_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return SQ_OK;
}

}  // namespace sq

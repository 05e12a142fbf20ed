// White top-hat background removal of a batch of staged tile planes for gfx950, in place (--background-subtract tophat):
//
//     E(y, x) = min I over the (2R+1) x (2R+1) window centred on (y, x), clipped to the plane
//     O(y, x) = max E over the same clipped window
//     out     = I - O
//
// The reference has no counterpart (its BaSiC runs with get_darkfield=False: nothing removes an additive term); the definition
// is the numpy restatement in tests/tophat_ref.py.  Integers only, no atomics: deterministic.
//
// Two launches of ONE kernel: the erosion (row minimum, then column minimum) into the caller's scratch, then the dilation (row
// maximum, then column maximum) of the scratch, which subtracts the result from the plane and stores in place.  A square
// window is separable and a clipped window is a window padded with the operation's identity, so each launch is a 1-D pass along
// the rows followed by one along the columns, both with van Herk / Gil-Werman running extrema: the work per pixel does not
// depend on R.
//
// Mapping: a workgroup of 256 threads owns a strip of `tw` columns (256, or 128 above R = 64) over a segment of the plane's rows
// and walks down it in blocks of `rb` rows:
//   A  the block's rows, `tw` + 2R columns wide, are read with 16-byte loads (the vectors a row starts and ends in element by
//      element, so nothing outside a row is touched) and written twice to LDS as 16-bit values, F and B; columns outside the
//      plane hold the identity;
//   B  every (row, segment of 2R+1 columns) is scanned forwards in F and backwards in B, in place, one thread per scan;
//   C  thread c owns column c: per row the row extremum of its column is min/max(B[c], F[c + 2R]), and it streams down the
//      column through a van Herk buffer V of 2R+1 rows in LDS (a running forward extremum in a register, the previous segment's
//      backward extrema in V, scanned in place by the owning thread when a segment completes), storing one output row per
//      input row.  Nothing in C crosses threads, so a block costs three barriers.
// LDS: V = (2R+1) x tw and F + B = 2 x rb x (tw + 2R) 16-bit values, in one static array of 52, 78 or 156 KiB (three, two or one
// workgroup per CU of 160 KiB); the host takes the smallest that leaves at least 16 rows per block.  F / B rows are an odd
// number of dwords apart, so the scans of different rows fall on different banks.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_util.h"
#include "plane_batch.h"

using namespace sq;

namespace {

constexpr int THREADS = 256;
constexpr int MAX_RADIUS = 127;
constexpr int MAX_RB = 32;
constexpr int LDS_SMALL = 26624, LDS_MEDIUM = 39936, LDS_LARGE = 79872;   // 16-bit values: 52, 78, 156 KiB

struct MorphArgs {
    const void *src;            // what is eroded / dilated
    int64_t src_plane_stride, src_pitch;   // elements
    void *dst;                  // erosion: receives it; dilation: the plane it is subtracted from, in place
    int64_t dst_plane_stride, dst_pitch;
    int32_t h, w, radius;
    int32_t tw;                 // columns of a strip
    int32_t rb;                 // rows of a block
    int32_t pitch;              // 16-bit values between two rows of F (and of B)
    int32_t n_strips, seg_h;    // blockIdx.x = row segment * n_strips + strip
};

template <bool IS_MIN>
__device__ __forceinline__ uint32_t op(uint32_t a, uint32_t b) {
    return IS_MIN ? min(a, b) : max(a, b);
}

// IS_MIN: dst = erosion of src.  Otherwise: dst -= dilation of src.
template <typename T, bool IS_MIN, int LDS_ELEMS>
__global__ __launch_bounds__(THREADS) void morph_kernel(const MorphArgs a) {
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr uint32_t ID = IS_MIN ? 0xffffu : 0u;
    __shared__ __attribute__((aligned(16))) uint16_t lds[LDS_ELEMS];
    const int tid = threadIdx.x;
    const int R = a.radius, wlen = 2 * R + 1;
    const int strip = blockIdx.x % a.n_strips, seg = blockIdx.x / a.n_strips;
    const int x0 = strip * a.tw;
    const int tw_eff = min(a.tw, a.w - x0);
    const int cols = tw_eff + 2 * R;             // F / B column j is plane column x0 - R + j
    const int y_lo = seg * a.seg_h, y_hi = min(a.h, y_lo + a.seg_h);
    const int t0 = y_lo - R, t_end = y_hi + R;   // the rows that are walked; those outside the plane hold the identity
    const int jlo = max(0, R - x0), jhi = min(cols, a.w - x0 + R);   // columns [jlo, jhi) lie inside the plane
    const int glo = x0 - R + jlo;                // plane column of jlo
    const int pad = jlo + (cols - jhi);
    const int S = (jhi - jlo + 2 * VEC - 2) / VEC;   // aligned 16-byte vectors a row's columns can touch at any phase
    const int nseg = (cols + wlen - 1) / wlen;

    uint16_t *V = lds;
    uint16_t *F = V + wlen * a.tw;
    uint16_t *B = F + a.rb * a.pitch;
    const T *src = static_cast<const T *>(a.src) + (int64_t)blockIdx.y * a.src_plane_stride;
    T *dst = static_cast<T *>(a.dst) + (int64_t)blockIdx.y * a.dst_plane_stride;

    uint32_t g = ID;        // column tid: running extremum of the current vertical segment
    int vi = 0;             // position in the vertical segment
    bool first = true;      // still in the first vertical segment: no window is complete before its last row

    for (int tb = t0; tb < t_end; tb += a.rb) {
        const int nrows = min(a.rb, t_end - tb);
        __syncthreads();    // the block before has been read
        // ---- A: rows -> F and B
        for (int idx = tid; idx < nrows * pad; idx += THREADS) {
            const int r = idx / pad, k = idx - r * pad;
            const int j = k < jlo ? k : jhi + (k - jlo);
            F[r * a.pitch + j] = (uint16_t)ID;
            B[r * a.pitch + j] = (uint16_t)ID;
        }
        for (int idx = tid; idx < nrows * S; idx += THREADS) {
            const int r = idx / S, slot = idx - r * S;
            const int t = tb + r;
            if (t < 0 || t >= a.h) continue;
            const T *rp = src + (int64_t)t * a.src_pitch;
            const int mis = (int)((reinterpret_cast<uintptr_t>(rp + glo) / sizeof(T)) & (VEC - 1));
            const int e0 = glo - mis + slot * VEC;          // the slot's first plane column
            const int lo = max(e0, glo), hi = min(e0 + VEC, glo + (jhi - jlo));
            if (lo >= hi) continue;
            const int at = r * a.pitch + (e0 - (x0 - R));    // (negative only for elements below lo)
            if (hi - lo == VEC) {
                const u32x4 d = *(const SQ_GLOBAL u32x4 *)(rp + e0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (sizeof(T) == 2) {
                        F[at + 2 * q] = B[at + 2 * q] = (uint16_t)(d[q] & 0xffffu);
                        F[at + 2 * q + 1] = B[at + 2 * q + 1] = (uint16_t)(d[q] >> 16);
                    } else {
#pragma unroll
                        for (int s = 0; s < 4; ++s) F[at + 4 * q + s] = B[at + 4 * q + s] = (uint16_t)((d[q] >> (8 * s)) & 0xffu);
                    }
                }
            } else {   // the vector a row's columns start or end in
                for (int e = lo; e < hi; ++e) F[at + e - e0] = B[at + e - e0] = (uint16_t)(*(const SQ_GLOBAL T *)(rp + e));
            }
        }
        lds_written();
        __syncthreads();
        // ---- B: forward scans of F, backward scans of B, per (row, segment of wlen columns)
        for (int task = tid; task < nrows * nseg * 2; task += THREADS) {
            const int dir = task & 1, rs = task >> 1;
            const int r = rs / nseg, s = rs - r * nseg;
            const int t = tb + r;
            if (t < 0 || t >= a.h) continue;
            const int c0 = s * wlen, c1 = min(cols, c0 + wlen);
            uint32_t acc = ID;
            if (dir == 0) {
                uint16_t *f = F + r * a.pitch;
#pragma unroll 4
                for (int j = c0; j < c1; ++j) {
                    acc = op<IS_MIN>(acc, f[j]);
                    f[j] = (uint16_t)acc;
                }
            } else {
                uint16_t *b = B + r * a.pitch;
#pragma unroll 4
                for (int j = c1 - 1; j >= c0; --j) {
                    acc = op<IS_MIN>(acc, b[j]);
                    b[j] = (uint16_t)acc;
                }
            }
        }
        lds_written();
        __syncthreads();
        // ---- C: column tid, one row after the other
        if (tid < tw_eff) {
            for (int r = 0; r < nrows; ++r) {
                const int t = tb + r;
                uint32_t v = ID;
                if (t >= 0 && t < a.h) v = op<IS_MIN>(B[r * a.pitch + tid], F[r * a.pitch + tid + 2 * R]);
                g = vi == 0 ? v : op<IS_MIN>(g, v);
                if (!first || vi == wlen - 1) {     // rows t - 2R ... t have all been seen: the window of row t - R
                    uint32_t o = g;
                    if (vi < wlen - 1) o = op<IS_MIN>(o, V[(vi + 1) * a.tw + tid]);
                    const int64_t at = (int64_t)(t - R) * a.dst_pitch + x0 + tid;
                    if (IS_MIN)
                        dst[at] = (T)o;
                    else
                        dst[at] = (T)((uint32_t)dst[at] - o);
                }
                V[vi * a.tw + tid] = (uint16_t)v;
                if (++vi == wlen) {     // the segment is complete: its backward extrema, for the windows that end in the next one
                    vi = 0;
                    first = false;
                    uint32_t acc = v;
                    for (int j = wlen - 2; j >= 1; --j) {
                        acc = op<IS_MIN>(acc, V[j * a.tw + tid]);
                        V[j * a.tw + tid] = (uint16_t)acc;
                    }
                }
            }
        }
        lds_written();
    }
}

struct Geometry {
    int tw, rb, pitch, lds;
};

// Strip width, rows per block and the LDS size for a radius and a plane width.
Geometry geometry(int radius, int w) {
    Geometry g{};
    g.tw = (radius <= 64 && w > 128) ? 256 : 128;
    const int wlen = 2 * radius + 1;
    const int cols = g.tw + 2 * radius;
    g.pitch = (cols + 3) / 4 * 4 + 2;     // an odd number of dwords
    const int v = wlen * g.tw;
    const int sizes[3] = {LDS_SMALL, LDS_MEDIUM, LDS_LARGE};
    for (int i = 0; i < 3; ++i) {
        g.lds = sizes[i];
        g.rb = (sizes[i] - v) / (2 * g.pitch);
        if (g.rb >= 16) break;      // (fewer rows leave most of the workgroup idle in B: rb x segments x 2 scans)
    }
    g.rb = std::min(g.rb, MAX_RB);
    return g;
}
static_assert((2 * MAX_RADIUS + 1) * 128 + 2 * MAX_RB * ((128 + 2 * MAX_RADIUS + 3) / 4 * 4 + 2) <= LDS_LARGE,
              "the largest radius must leave a full block of rows");
static_assert((2 * 64 + 1) * 256 + 2 * MAX_RB * ((256 + 2 * 64 + 3) / 4 * 4 + 2) <= LDS_LARGE,
              "the largest radius of the 256-column strip must leave a full block of rows");

template <typename T, bool IS_MIN>
void launch(const MorphArgs &a, int lds, dim3 grid, hipStream_t stream) {
    if (lds == LDS_SMALL)
        morph_kernel<T, IS_MIN, LDS_SMALL><<<grid, dim3(THREADS), 0, stream>>>(a);
    else if (lds == LDS_MEDIUM)
        morph_kernel<T, IS_MIN, LDS_MEDIUM><<<grid, dim3(THREADS), 0, stream>>>(a);
    else
        morph_kernel<T, IS_MIN, LDS_LARGE><<<grid, dim3(THREADS), 0, stream>>>(a);
}

}   // namespace

extern "C" int64_t sq_tophat_scratch_bytes(int32_t n_images, int32_t h, int32_t w, int32_t dtype) {
    if (dtype != SQ_U8 && dtype != SQ_U16) return fail(SQ_ERR_UNSUPPORTED, "sq_tophat_scratch_bytes: dtype %d", dtype);
    if (n_images < 0 || h <= 0 || w <= 0 || h > (1 << 30) || w > (1 << 30))
        return fail(SQ_ERR_INVALID, "sq_tophat_scratch_bytes: bad sizes (images=%d %dx%d)", n_images, h, w);
    return std::max<int64_t>(16, (int64_t)n_images * h * w * (dtype == SQ_U16 ? 2 : 1));
}

extern "C" int sq_tophat_tiles(void *tiles_dev, int32_t n_images, int32_t h, int32_t w, int64_t plane_stride, int64_t pitch,
                               int32_t dtype, int32_t radius, void *scratch_dev, int64_t scratch_bytes, void *stream_) {
    if (dtype != SQ_U8 && dtype != SQ_U16) return fail(SQ_ERR_UNSUPPORTED, "sq_tophat_tiles: dtype %d", dtype);
    if (n_images < 0 || h <= 0 || w <= 0 || h > (1 << 30) || w > (1 << 30) || pitch < w)
        return fail(SQ_ERR_INVALID, "sq_tophat_tiles: bad sizes (images=%d %dx%d pitch %lld)", n_images, h, w, (long long)pitch);
    if (radius < 1 || radius > MAX_RADIUS) return fail(SQ_ERR_INVALID, "sq_tophat_tiles: radius %d outside 1..%d", radius, MAX_RADIUS);
    if (n_images == 0) return SQ_OK;
    if (!tiles_dev || !scratch_dev) return fail(SQ_ERR_INVALID, "sq_tophat_tiles: NULL buffer");
    const int esize = dtype == SQ_U16 ? 2 : 1;
    const PlaneBatch tiles{tiles_dev, n_images, h, w, plane_stride, pitch, esize};
    if (const int rc = check_batches("sq_tophat_tiles", "plane", {tiles})) return rc;
    if (reinterpret_cast<uintptr_t>(scratch_dev) % 16) return fail(SQ_ERR_INVALID, "sq_tophat_tiles: the scratch must be aligned to 16 bytes");
    const int64_t need = sq_tophat_scratch_bytes(n_images, h, w, dtype);
    if (scratch_bytes < need)
        return fail(SQ_ERR_WORKSPACE, "sq_tophat_tiles: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)need);
    hipStream_t stream = static_cast<hipStream_t>(stream_);

    const Geometry g = geometry(radius, w);
    const int n_strips = (w + g.tw - 1) / g.tw;
    // whole columns per workgroup when the batch fills the card; otherwise row segments (each re-reads 2R rows of halo)
    int n_segs = 1;
    const int64_t base = (int64_t)n_images * n_strips;
    if (base < 1024) {
        const int most = std::max(1, h / std::max(64, 4 * radius));
        n_segs = (int)std::min<int64_t>((1024 + base - 1) / base, most);
    }
    const int seg_h = (h + n_segs - 1) / n_segs;
    n_segs = (h + seg_h - 1) / seg_h;

    MorphArgs a{};
    a.h = h;
    a.w = w;
    a.radius = radius;
    a.tw = g.tw;
    a.rb = g.rb;
    a.pitch = g.pitch;
    a.n_strips = n_strips;
    a.seg_h = seg_h;
    return for_each_launch("sq_tophat_tiles", 0, n_images, 1, [&](int64_t p0, int32_t, unsigned grid_y) {
        const dim3 grid((unsigned)(n_strips * n_segs), grid_y);
        char *scratch = static_cast<char *>(scratch_dev) + p0 * h * w * esize;
        // erosion: tiles -> scratch (dense planes)
        a.src = tiles.at(p0);
        a.src_plane_stride = plane_stride;
        a.src_pitch = pitch;
        a.dst = scratch;
        a.dst_plane_stride = (int64_t)h * w;
        a.dst_pitch = w;
        if (dtype == SQ_U16)
            launch<uint16_t, true>(a, g.lds, grid, stream);
        else
            launch<uint8_t, true>(a, g.lds, grid, stream);
        // dilation of the scratch, subtracted from the tiles in place
        a.src = scratch;
        a.src_plane_stride = (int64_t)h * w;
        a.src_pitch = w;
        a.dst = tiles.at(p0);
        a.dst_plane_stride = plane_stride;
        a.dst_pitch = pitch;
        if (dtype == SQ_U16)
            launch<uint16_t, false>(a, g.lds, grid, stream);
        else
            launch<uint8_t, false>(a, g.lds, grid, stream);
    });
}

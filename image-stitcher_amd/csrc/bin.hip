// K x K binning of a batch of staged tile planes for gfx950, out of place (--tile-binning):
//
//     hb = h / K, wb = w / K (integer division: the last h - K hb rows and w - K wb columns are dropped)
//     S(y, x) = the sum of I over the K x K block at (K y, K x)                      (at most 64 * 65535: 32 bits)
//     mean:  out = floor(S / K^2)          sum:  out = min(S, M), M the dtype's maximum
//
// The reference has no counterpart; the definition is the numpy restatement in tests/bin_ref.py.  Integers only, no atomics, no
// LDS, no scratch: deterministic.  Every source element inside the K hb x K wb area is read exactly once, nothing of the dropped
// rows and columns is read, and nothing outside hb x wb of a destination plane is written.
//
// Mapping: a thread owns a run of OUTS = lcm(K, VEC) / K dst columns (VEC = 8 uint16 / 16 uint8, the elements of 16 bytes)
// and walks down RPT dst rows.  The run's source is K rows of NV = lcm(K, VEC) / VEC consecutive 16-byte vectors -- for K = 2, 4
// and 8 ONE vector, so the lanes of a wave read consecutive vectors; for the other factors 3 to 7 vectors.  For each of the NV
// vectors along the row the loads of all K rows are issued together, and their elements are added into the output they belong
// to (column c of the span belongs to output c / K, a compile-time index: K is a template parameter, everything is unrolled,
// the division by K^2 is by a constant).  The 256 threads of a workgroup are tx runs wide (a power of two, at most 256) and
// 256 / tx runs of RPT rows tall.  blockIdx.x = row segment * n_strips + strip, blockIdx.y = plane.
//
// Phases: run k starts at dst column k * OUTS - shift.  The host picks shift so that the SOURCE span of a run starts on a
// 16-byte boundary in the plane's first row whenever the source's phase allows it (K * shift = src phase mod VEC has a
// solution; of several, the one that also puts dst on a boundary of its store), and so that dst does otherwise.  A span is
// loaded with 16-byte loads in the blocks where it lies inside the row and on a boundary in all K rows, element by element in
// the others (the head and the tail of a row, rows of another phase); an element outside the row's K wb columns is not read.
// A run is stored with one store of its OUTS elements (2 to 16 bytes) where it lies inside the row and on a boundary of that
// size, element by element otherwise.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_util.h"
#include "plane_batch.h"

using namespace sq;

namespace {

constexpr int THREADS = 256;
constexpr int RPT = 4;      // dst rows a thread walks down (K * RPT source rows)

struct BinArgs {
    const void *src;
    int64_t src_plane_stride, src_pitch;   // elements
    void *dst;
    int64_t dst_plane_stride, dst_pitch;
    int32_t hb, wb;             // the binned plane
    int32_t shift;              // run k starts at dst column k * OUTS - shift
    int32_t tx, tx_log2;        // runs across a workgroup
    int32_t n_strips;
};

constexpr int gcd_of(int a, int b) { return b == 0 ? a : gcd_of(b, a % b); }
// dst columns of a thread's run: lcm(K, VEC) / K = VEC / gcd(K, VEC)
constexpr int outs_of(int k, int vec) { return vec / gcd_of(k, vec); }

template <typename T, int K, bool SUM>
__global__ __launch_bounds__(THREADS) void bin_kernel(const BinArgs a) {
    constexpr int VEC = 16 / (int)sizeof(T), PER = VEC / 4, BITS = 8 * (int)sizeof(T);
    constexpr int OUTS = outs_of(K, VEC), NV = OUTS * K / VEC;      // dst columns of a run; 16-byte vectors of its span
    constexpr int STORE = OUTS * (int)sizeof(T);                   // bytes of a run: 2, 4, 8 or 16
    constexpr uint32_t TOP = sizeof(T) == 2 ? 0xffffu : 0xffu;
    const int tid = threadIdx.x;
    const int strip = blockIdx.x % a.n_strips, seg = blockIdx.x / a.n_strips;
    const int lx = tid & (a.tx - 1), ly = tid >> a.tx_log2;
    const int ty = THREADS >> a.tx_log2;
    const int xo = (strip * a.tx + lx) * OUTS - a.shift;      // the run's first dst column (negative: it starts in front of the row)
    const int64_t y_lo = ((int64_t)seg * ty + ly) * RPT;
    if (xo >= a.wb || xo + OUTS <= 0 || y_lo >= a.hb) return;
    const T *__restrict__ src = static_cast<const T *>(a.src) + (int64_t)blockIdx.y * a.src_plane_stride;
    T *__restrict__ dst = static_cast<T *>(a.dst) + (int64_t)blockIdx.y * a.dst_plane_stride;
    const int y0 = (int)y_lo, y1 = min(a.hb, y0 + RPT);
    const int lo_x = max(xo, 0), hi_x = min(xo + OUTS, a.wb);
    const bool whole = hi_x - lo_x == OUTS;      // the run, and so its span of K * OUTS source columns, lies inside the row

    for (int y = y0; y < y1; ++y) {
        const T *r0 = src + (int64_t)y * K * a.src_pitch + (int64_t)xo * K;      // the span in the block's first source row
        T *wp = dst + (int64_t)y * a.dst_pitch + xo;
        bool wide = whole;
#pragma unroll
        for (int r = 0; r < K; ++r) wide = wide && (reinterpret_cast<uintptr_t>(r0 + (int64_t)r * a.src_pitch) & 15) == 0;
        if (wide) {
            uint32_t o[OUTS];
#pragma unroll
            for (int i = 0; i < OUTS; ++i) o[i] = 0;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                u32x4 d[K];      // the j-th vector of the span in all K rows: in flight together
#pragma unroll
                for (int r = 0; r < K; ++r) d[r] = *(const SQ_GLOBAL u32x4 *)(r0 + (int64_t)r * a.src_pitch + j * VEC);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    uint32_t lanes[PER];
#pragma unroll
                    for (int s = 0; s < PER; ++s) lanes[s] = 0;
#pragma unroll
                    for (int r = 0; r < K; ++r) {
                        const uint32_t word = d[r][q];
#pragma unroll
                        for (int s = 0; s < PER; ++s) lanes[s] += (word >> (BITS * s)) & TOP;
                    }
#pragma unroll
                    for (int s = 0; s < PER; ++s) o[(j * VEC + q * PER + s) / K] += lanes[s];      // (a compile-time index)
                }
                // the sums so far, each in its register: without this the compiler re-associates the additions over all j into
                // trees whose leaves stay live to the end (a whole register file for the factors with many vectors)
#pragma unroll
                for (int i = 0; i < OUTS; ++i) asm volatile("" : "+v"(o[i]));
                // K >= 6: every vector of every row in flight would take half the register file: one vector of every row at a
                // time instead
                if (K >= 6 && NV > 1) __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int i = 0; i < OUTS; ++i) o[i] = SUM ? min(o[i], TOP) : o[i] / (uint32_t)(K * K);
            if ((reinterpret_cast<uintptr_t>(wp) & (STORE - 1)) == 0) {
                constexpr int WORDS = STORE >= 4 ? STORE / 4 : 1;
                uint32_t v[WORDS];
#pragma unroll
                for (int q = 0; q < WORDS; ++q) {
                    v[q] = 0;
#pragma unroll
                    for (int s = 0; s < (STORE >= 4 ? PER : OUTS); ++s) v[q] |= o[q * PER + s] << (BITS * s);
                }
                if (STORE == 16) {
                    u32x4 w4;
                    w4.x = v[0];
                    w4.y = v[WORDS > 1 ? 1 : 0];
                    w4.z = v[WORDS > 2 ? 2 : 0];
                    w4.w = v[WORDS > 3 ? 3 : 0];
                    *(SQ_GLOBAL u32x4 *)wp = w4;
                } else if (STORE == 8) {
                    u32x2 w2;
                    w2.x = v[0];
                    w2.y = v[WORDS > 1 ? 1 : 0];
                    *(SQ_GLOBAL u32x2 *)wp = w2;
                } else if (STORE == 4) {
                    *(SQ_GLOBAL uint32_t *)wp = v[0];
                } else {
                    *(SQ_GLOBAL uint16_t *)wp = (uint16_t)v[0];
                }
            } else {
#pragma unroll
                for (int i = 0; i < OUTS; ++i) *(SQ_GLOBAL T *)(wp + i) = (T)o[i];
            }
        } else {
            // the run a row starts or ends in, or a block with a row of another phase: output by output, element by element
#pragma unroll 1
            for (int i = lo_x - xo; i < hi_x - xo; ++i) {
                const T *bp = r0 + i * K;
                uint32_t sum = 0;
#pragma unroll 1
                for (int r = 0; r < K; ++r) {
                    const T *rp = bp + (int64_t)r * a.src_pitch;
#pragma unroll
                    for (int c = 0; c < K; ++c) sum += (uint32_t)(*(const SQ_GLOBAL T *)(rp + c));
                }
                *(SQ_GLOBAL T *)(wp + i) = (T)(SUM ? min(sum, TOP) : sum / (uint32_t)(K * K));
            }
        }
    }
}

template <typename T, int K>
void launch_k(int32_t method, dim3 grid, hipStream_t stream, const BinArgs &a) {
    if (method == SQ_BIN_SUM)
        bin_kernel<T, K, true><<<grid, dim3(THREADS), 0, stream>>>(a);
    else
        bin_kernel<T, K, false><<<grid, dim3(THREADS), 0, stream>>>(a);
}

template <typename T>
void launch(int32_t factor, int32_t method, dim3 grid, hipStream_t stream, const BinArgs &a) {
    switch (factor) {
        case 2: launch_k<T, 2>(method, grid, stream, a); break;
        case 3: launch_k<T, 3>(method, grid, stream, a); break;
        case 4: launch_k<T, 4>(method, grid, stream, a); break;
        case 5: launch_k<T, 5>(method, grid, stream, a); break;
        case 6: launch_k<T, 6>(method, grid, stream, a); break;
        case 7: launch_k<T, 7>(method, grid, stream, a); break;
        default: launch_k<T, 8>(method, grid, stream, a); break;
    }
}

}   // namespace

extern "C" int sq_bin_tiles(const void *src_dev, void *dst_dev, int32_t n_images, int32_t h, int32_t w,
                            int64_t src_plane_stride, int64_t src_pitch, int64_t dst_plane_stride, int64_t dst_pitch,
                            int32_t dtype, int32_t factor, int32_t method, void *stream_) {
    if (dtype != SQ_U8 && dtype != SQ_U16) return fail(SQ_ERR_INVALID, "sq_bin_tiles: dtype %d", dtype);
    if (method != SQ_BIN_MEAN && method != SQ_BIN_SUM) return fail(SQ_ERR_INVALID, "sq_bin_tiles: method %d", method);
    if (factor < 2 || factor > SQ_BIN_MAX_FACTOR)
        return fail(SQ_ERR_INVALID, "sq_bin_tiles: factor %d outside 2..%d", factor, SQ_BIN_MAX_FACTOR);
    if (n_images < 0 || h <= 0 || w <= 0 || h > (1 << 30) || w > (1 << 30))
        return fail(SQ_ERR_INVALID, "sq_bin_tiles: bad sizes (images=%d %dx%d)", n_images, h, w);
    const int32_t hb = h / factor, wb = w / factor;
    if (hb < 1 || wb < 1) return fail(SQ_ERR_INVALID, "sq_bin_tiles: a plane of %d x %d has no %d x %d block", h, w, factor, factor);
    if (src_pitch < w || dst_pitch < wb)
        return fail(SQ_ERR_INVALID, "sq_bin_tiles: pitches %lld, %lld below the widths %d, %d", (long long)src_pitch,
                    (long long)dst_pitch, w, wb);
    if (n_images == 0) return SQ_OK;
    if (!src_dev || !dst_dev) return fail(SQ_ERR_INVALID, "sq_bin_tiles: NULL buffer");
    const int esize = dtype == SQ_U16 ? 2 : 1;
    const PlaneBatch src{src_dev, n_images, h, w, src_plane_stride, src_pitch, esize};
    const PlaneBatch dst{dst_dev, n_images, hb, wb, dst_plane_stride, dst_pitch, esize};
    if (const int rc = check_batches("sq_bin_tiles", "plane", {src, dst})) return rc;
    // a block is read after its neighbour's result is written
    if (overlap(src, dst)) return fail(SQ_ERR_INVALID, "sq_bin_tiles: src and dst overlap (the binning is out of place)");
    hipStream_t stream = static_cast<hipStream_t>(stream_);

    const int vec = 16 / esize, outs = outs_of(factor, vec);      // a thread's run of dst columns (the kernel's OUTS)
    const int src_phase = src.phase(vec), dst_phase = dst.phase(outs);
    BinArgs a{};
    a.hb = hb;
    a.wb = wb;
    a.shift = -1;
    // a span starts at source element (src_phase + factor * (k * outs - shift)), and factor * outs is a multiple of vec: it is
    // on a boundary when factor * shift = src_phase (mod vec).  Of the shifts that do that, the one that puts dst on a
    // boundary of its store too; without any, dst's.
    for (int s = 0; s < outs; ++s)
        if ((factor * s - src_phase) % vec == 0 && (a.shift < 0 || s == dst_phase)) a.shift = s;
    if (a.shift < 0) a.shift = dst_phase;
    StripGrid g;
    if (const int rc = strip_grid("sq_bin_tiles", ((int64_t)wb + a.shift + outs - 1) / outs, THREADS, THREADS, RPT, hb, &g)) return rc;
    a.tx = g.tx;
    a.tx_log2 = g.tx_log2;
    a.n_strips = g.n_strips;
    a.src_plane_stride = src_plane_stride;
    a.src_pitch = src_pitch;
    a.dst_plane_stride = dst_plane_stride;
    a.dst_pitch = dst_pitch;
    return for_each_launch("sq_bin_tiles", 0, n_images, 1, [&](int64_t p0, int32_t, unsigned grid_y) {
        const dim3 grid(g.x(), grid_y);
        a.src = src.at(p0);
        a.dst = dst.at(p0);
        if (dtype == SQ_U16)
            launch<uint16_t>(factor, method, grid, stream, a);
        else
            launch<uint8_t>(factor, method, grid, stream, a);
    });
}

// Per-tile quality words of a batch of staged tile planes for gfx950 (--tile-qc): eight uint64 per plane I [h, w]
//
//     0  min I                      4  number of pixels equal to the dtype's maximum (255 / 65535)
//     1  max I                      5  number of pixels equal to 0
//     2  S  = sum I                 6  Bx = sum over y, x < w - 2 of (I(y, x + 2) - I(y, x))^2      (0 when w <= 2)
//     3  Q  = sum I^2               7  By = sum over y < h - 2, x of (I(y + 2, x) - I(y, x))^2      (0 when h <= 2)
//
// Bx and By are the Brenner focus measure with step 2, one per direction.  The reference has no counterpart; the definition is
// the numpy restatement in tests/tile_qc_ref.py.  Integers only: every pixel product fits 32 bits and is accumulated in 64, and
// the atomics are integer min / max / add, which do not depend on their order -- the words are bit for bit numpy's int64 sums
// whatever the schedule.  The planes are read once (plus two halo rows below a thread's run of rows and two columns right of
// its vector); nothing but the 64 bytes per plane is stored.
//
// Mapping: a thread owns one 16-byte vector of columns (8 uint16 / 16 uint8) and walks down RPT rows two at a time with the rows
// y, y + 1, y + 2, y + 3 of its columns in registers: I(y + 2) - I(y) needs no second fetch, and the two rows of a step are
// independent chains.  I(x + 2) of the vector's last two columns comes from one extra small load of the two columns right of
// the vector.  No pixel goes through LDS.  The 256 threads of a workgroup are tx = 64, 128 or 256 vectors wide (256 for planes
// of 2048 uint16 columns and more) and 256 / tx runs of RPT rows tall: a wave never spans two runs, so the plane, the run's
// first row and its bounds are wave-uniform (SGPRs).  blockIdx.x = row segment * n_strips + strip, blockIdx.y = plane.
//
// Vectors: the vectors are laid at the phase of the first row of the first plane, so planes whose pitch and stride are multiples
// of a vector are read with 16-byte loads throughout; rows of another phase, and the vectors a row starts or ends in, are read
// element by element, and a column outside the row is never read: nothing between w and the pitch, or between h and the plane
// stride, reaches a sum.
//
// Reduction: per thread in registers (32-bit where a run's sum fits, 64-bit otherwise), across the wave with shuffles, across
// the four waves through 256 bytes of LDS, then one 64-bit integer atomic per word per workgroup (min, max, six adds).  The
// entry point sets the words to their identities (all-ones for the min, 0 for the others) on the same stream first, so they
// are overwritten, not added to.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "device_util.h"
#include "plane_batch.h"

using namespace sq;

namespace {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int RPT = SQ_TILE_STATS_ROWS_PER_THREAD;     // rows a thread walks down (each run reads two halo rows: 3 % of the reads)
constexpr int WORDS = SQ_TILE_STATS_WORDS;
static_assert(RPT % 2 == 0, "the row loop takes two rows a step");

struct TileStatsArgs {
    const void *src;
    int64_t plane_stride, pitch;   // elements
    unsigned long long *out;       // [planes of this launch][WORDS]
    int32_t h, w;
    int32_t mis;                   // elements of the first row in front of a 16-byte boundary: vector k starts at column k * VEC - mis
    int32_t tx_log2;               // vectors across a workgroup: 64, 128 or 256
    int32_t n_strips;
};

// What a thread has seen of its plane.  A run is RPT rows of VEC columns: sums of values and counts fit 32 bits
// (64 * 8 * 65535 < 2^25), sums of squares fit them for uint8 only (64 * 16 * 255^2 < 2^26).
template <typename T>
struct Stats {
    typedef typename std::conditional<sizeof(T) == 1, uint32_t, uint64_t>::type Sq;
    uint32_t mn = 0xffffffffu, mx = 0, s = 0, top = 0, zero = 0;
    Sq q = 0, bx = 0, by = 0;
};

// A row of a thread, packed as it was loaded: the vector's VEC columns in d, the two columns right of it in e.
struct Row {
    u32x4 d;
    uint32_t e;
};

// Column j (0 ... VEC + 1, a constant) of a packed row.
template <typename T, int VEC>
__device__ __forceinline__ uint32_t col(const Row &r, int j) {
    constexpr int BITS = 8 * (int)sizeof(T), PER = VEC / 4;
    constexpr uint32_t TOP = (1u << BITS) - 1u;
    if (j >= VEC) return (r.e >> (BITS * (j - VEC))) & TOP;
    return (r.d[j / PER] >> (BITS * (j % PER))) & TOP;
}

// Columns xa ... xa + VEC + 1 of the row at rp (wave-uniform); a column outside [0, w) is not read.  MASKED: the vector has
// columns outside the row; they come back as 0.  The two columns right of the vector come back as the values two columns to
// their left when they are outside the row, so that a vector inside the row needs no mask for its x differences.  A vector
// inside the row is at a 16-byte boundary when the row has the phase of the first (rp - mis is one: wave-uniform too).
template <typename T, int VEC, bool MASKED>
__device__ __forceinline__ Row load_row(const T *__restrict__ rp, int w, int xa, int mis) {
    typedef typename std::conditional<sizeof(T) == 2, uint32_t, uint16_t>::type Pair;
    constexpr int BITS = 8 * (int)sizeof(T), PER = VEC / 4;
    const int xe = xa + VEC;      // >= 1: a thread with no column inside the row loads nothing
    Row r;
    if (!MASKED && ((reinterpret_cast<uintptr_t>(rp) - (uintptr_t)mis * sizeof(T)) & 15) == 0) {
        r.d = *(const SQ_GLOBAL u32x4 *)(rp + (uint32_t)xa);
        if (xe + 1 < w) {
            r.e = (uint32_t)(*(const SQ_GLOBAL Pair *)(rp + (uint32_t)xe));
            return r;
        }
    } else {   // the vector a row starts or ends in, or a row of another phase: element by element, packed like the vector
        uint32_t q[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const int x = xa + k;
            uint32_t v = 0;
            if (!MASKED || (x >= 0 && x < w)) v = (uint32_t)(*(const SQ_GLOBAL T *)(rp + (uint32_t)x));
            q[k / PER] |= v << (BITS * (k % PER));
        }
        r.d.x = q[0];
        r.d.y = q[1];
        r.d.z = q[2];
        r.d.w = q[3];
    }
    uint32_t e0 = col<T, VEC>(r, VEC - 2), e1 = col<T, VEC>(r, VEC - 1);
    if (xe < w) e0 = (uint32_t)(*(const SQ_GLOBAL T *)(rp + (uint32_t)xe));
    if (xe + 1 < w) e1 = (uint32_t)(*(const SQ_GLOBAL T *)(rp + (uint32_t)xe + 1));
    r.e = e0 | (e1 << BITS);
    return r;
}

// Row A (columns xa ... xa + VEC + 1) into the thread's sums; C is the row two below it, or A itself where the plane ends.
// MASKED: the vector has columns outside the row (they hold 0 in A and C).  Values and absolute differences are at most
// 65535: the unsigned 24-bit multiply gives their square exactly (it is below 2^32; the signed one is an int multiply whose
// overflow past 2^31 is undefined, and the compiler then adds two squares in 32 bits).
template <typename T, int VEC, bool MASKED>
__device__ __forceinline__ void add_row(const Row &A, const Row &C, int w, int xa, Stats<T> &st) {
    typedef typename Stats<T>::Sq Sq;
    constexpr uint32_t TOP = (1u << (8 * (int)sizeof(T))) - 1u;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const uint32_t v = col<T, VEC>(A, j);
        const bool in = !MASKED || (xa + j >= 0 && xa + j < w);
        const bool in_x = !MASKED || (in && xa + j + 2 < w);
        st.mn = min(st.mn, in ? v : 0xffffffffu);
        st.mx = max(st.mx, v);
        st.s += v;
        st.q += (Sq)(uint32_t)__umul24(v, v);      // (declared int: the cast keeps it from being sign-extended)
        st.top += (v == TOP) ? 1u : 0u;
        st.zero += (in && v == 0) ? 1u : 0u;
        const uint32_t dx = in_x ? __usad(col<T, VEC>(A, j + 2), v, 0u) : 0u;      // |I(x + 2) - I(x)|
        st.bx += (Sq)(uint32_t)__umul24(dx, dx);
        const uint32_t dy = __usad(col<T, VEC>(C, j), v, 0u);
        st.by += (Sq)(uint32_t)__umul24(dy, dy);
    }
}

template <typename T, int VEC, bool MASKED>
__device__ __forceinline__ void walk(const T *__restrict__ plane, int64_t pitch, int h, int w, int xa, int mis, int y0, int y1,
                                     Stats<T> &st) {
    // y0, y1, h are wave-uniform: the branches on rows are scalar.  A row below the plane stands in as a copy of the row two
    // above it: its y difference is 0 and it is never a row of its own (y1 <= h).
    Row A = load_row<T, VEC, MASKED>(plane + (int64_t)y0 * pitch, w, xa, mis), B = A;
    if (y0 + 1 < h) B = load_row<T, VEC, MASKED>(plane + (int64_t)(y0 + 1) * pitch, w, xa, mis);
    for (int y = y0; y < y1; y += 2) {      // rows y and y + 1 (y1 - y0 is odd only where the plane ends)
        Row C = A, D = B;
        if (y + 2 < h) C = load_row<T, VEC, MASKED>(plane + (int64_t)(y + 2) * pitch, w, xa, mis);
        if (y + 3 < h) D = load_row<T, VEC, MASKED>(plane + (int64_t)(y + 3) * pitch, w, xa, mis);
        add_row<T, VEC, MASKED>(A, C, w, xa, st);
        if (y + 1 < y1) add_row<T, VEC, MASKED>(B, D, w, xa, st);
        A = C;
        B = D;
    }
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m, WAVE), hi = __shfl_xor((uint32_t)(v >> 32), m, WAVE);
    return ((uint64_t)hi << 32) | lo;
}

template <typename T>
__global__ __launch_bounds__(THREADS) void tile_stats_kernel(const TileStatsArgs a) {
    constexpr int VEC = 16 / (int)sizeof(T);
    __shared__ unsigned long long part[THREADS / WAVE][WORDS];
    const int tid = threadIdx.x;
    const int strip = blockIdx.x % a.n_strips, seg = blockIdx.x / a.n_strips;
    const int tx = 1 << a.tx_log2, ty = THREADS >> a.tx_log2;
    const int lx = tid & (tx - 1);
    const int ly = __builtin_amdgcn_readfirstlane(tid >> a.tx_log2);      // tx >= 64: one run of rows per wave
    const int xa = (strip * tx + lx) * VEC - a.mis;       // the vector's first column (negative: it starts in front of the row)
    const int64_t y_lo = ((int64_t)seg * ty + ly) * RPT;
    const T *__restrict__ plane = static_cast<const T *>(a.src) + (int64_t)blockIdx.y * a.plane_stride;

    Stats<T> st;
    if (y_lo < a.h && xa < a.w && xa + VEC > 0) {
        const int y0 = (int)y_lo, y1 = min(a.h, y0 + RPT);
        if (xa >= 0 && xa + VEC <= a.w)
            walk<T, VEC, false>(plane, a.pitch, a.h, a.w, xa, a.mis, y0, y1, st);
        else
            walk<T, VEC, true>(plane, a.pitch, a.h, a.w, xa, a.mis, y0, y1, st);
    }
    uint64_t v[WORDS] = {st.mn, st.mx, st.s, (uint64_t)st.q, st.top, st.zero, (uint64_t)st.bx, (uint64_t)st.by};
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) {
        v[0] = min((uint32_t)v[0], (uint32_t)__shfl_xor((uint32_t)v[0], m, WAVE));
        v[1] = max((uint32_t)v[1], (uint32_t)__shfl_xor((uint32_t)v[1], m, WAVE));
        v[2] += (uint64_t)__shfl_xor((uint32_t)v[2], m, WAVE);      // a wave's sum of values: 64 * 2^25 < 2^32
        v[4] += (uint64_t)__shfl_xor((uint32_t)v[4], m, WAVE);
        v[5] += (uint64_t)__shfl_xor((uint32_t)v[5], m, WAVE);
        v[3] += shfl_xor64(v[3], m);
        v[6] += shfl_xor64(v[6], m);
        v[7] += shfl_xor64(v[7], m);
    }
    if ((tid & (WAVE - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < WORDS; ++k) part[tid / WAVE][k] = v[k];
    }
    lds_written();
    __syncthreads();
    if (tid < WORDS) {
        unsigned long long r = part[0][tid];
        for (int k = 1; k < THREADS / WAVE; ++k) {
            const unsigned long long p = part[k][tid];
            r = tid == 0 ? (p < r ? p : r) : (tid == 1 ? (p > r ? p : r) : r + p);
        }
        unsigned long long *o = a.out + (int64_t)blockIdx.y * WORDS + tid;
        if (tid == 0)
            atomicMin(o, r);
        else if (tid == 1)
            atomicMax(o, r);
        else if (r != 0)
            atomicAdd(o, r);
    }
}

// The identities of the eight words: all-ones for the min, 0 for the others.
__global__ __launch_bounds__(THREADS) void tile_stats_init_kernel(unsigned long long *out, int64_t n_words) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i < n_words) out[i] = (i % WORDS) == 0 ? ~0ull : 0ull;
}

}   // namespace

extern "C" int sq_tile_stats(const void *src_dev, int32_t n_images, int32_t h, int32_t w, int64_t plane_stride, int64_t pitch,
                             int32_t dtype, uint64_t *out_dev, void *stream_) {
    if (dtype != SQ_U8 && dtype != SQ_U16) return fail(SQ_ERR_INVALID, "sq_tile_stats: dtype %d", dtype);
    if (n_images < 0 || h <= 0 || w <= 0 || pitch < w)
        return fail(SQ_ERR_INVALID, "sq_tile_stats: bad sizes (images=%d %dx%d pitch %lld)", n_images, h, w, (long long)pitch);
    if ((int64_t)h * w > (1ll << 31) || h > (1 << 30) || w > (1 << 30))
        return fail(SQ_ERR_UNSUPPORTED, "sq_tile_stats: a plane of %d x %d is beyond 2^31 pixels (or 2^30 a side): a word could wrap", h, w);
    if (n_images == 0) return SQ_OK;
    if (!src_dev || !out_dev) return fail(SQ_ERR_INVALID, "sq_tile_stats: NULL buffer");
    if (reinterpret_cast<uintptr_t>(out_dev) % 8) return fail(SQ_ERR_INVALID, "sq_tile_stats: the words must be aligned to 8 bytes");
    const int esize = dtype == SQ_U16 ? 2 : 1;
    const PlaneBatch src{src_dev, n_images, h, w, plane_stride, pitch, esize};
    if (const int rc = check_batches("sq_tile_stats", "plane", {src})) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);

    const int vec = 16 / esize;
    TileStatsArgs a{};
    a.h = h;
    a.w = w;
    a.pitch = pitch;
    a.plane_stride = plane_stride;
    a.mis = src.phase(vec);
    const int64_t nvec = ((int64_t)w + a.mis + vec - 1) / vec;
    a.tx_log2 = nvec <= 64 ? 6 : (nvec <= 128 ? 7 : 8);
    const int tx = 1 << a.tx_log2, ty = THREADS / tx;
    const int64_t n_strips = (nvec + tx - 1) / tx;
    const int64_t n_segs = ((int64_t)h + (int64_t)ty * RPT - 1) / ((int64_t)ty * RPT);
    if (n_strips * n_segs > INT32_MAX)
        return fail(SQ_ERR_UNSUPPORTED, "sq_tile_stats: a plane of %d x %d needs more workgroups than a launch has", h, w);
    a.n_strips = (int32_t)n_strips;

    const int64_t n_words = (int64_t)n_images * WORDS;
    tile_stats_init_kernel<<<dim3((unsigned)((n_words + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream>>>(
        reinterpret_cast<unsigned long long *>(out_dev), n_words);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SQ_ERR_HIP, "sq_tile_stats: launch failed: %s", hipGetErrorString(e));
    return for_each_launch("sq_tile_stats", 0, n_images, 1, [&](int64_t p0, int32_t, unsigned grid_y) {
        const dim3 grid((unsigned)(n_strips * n_segs), grid_y);
        a.src = src.at(p0);
        a.out = reinterpret_cast<unsigned long long *>(out_dev) + p0 * WORDS;
        if (dtype == SQ_U16)
            tile_stats_kernel<uint16_t><<<grid, dim3(THREADS), 0, stream>>>(a);
        else
            tile_stats_kernel<uint8_t><<<grid, dim3(THREADS), 0, stream>>>(a);
    });
}

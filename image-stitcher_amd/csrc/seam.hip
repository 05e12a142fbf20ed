// Per-seam alignment words of a batch of staged tile planes for gfx950 (--seam-qc): for every plane and every pair of
// overlapping tiles, the exact integer sums a zero-normalised cross-correlation is formed from -- at the placement the tiles
// have and at every integer residual displacement e = (ey, ex) in [-R, R]^2 around it.
//
// Definition (the numpy restatement is tests/seam_qc_ref.py; image-stitcher_amd/seamqc.py derives the table):
//
//   Geometry.  A tile of H x W pixels with rectangle (src_y0, src_x0, h, w, dst_y, dst_x) has the full-tile canvas origin
//   o = (dst_y - src_y0, dst_x - src_x0).  Of two tiles of one region, ref is the one with the smaller fov index and mov the
//   other; d = o_mov - o_ref, and the overlap of the two full tiles at d is (ry0, rx0, my0, mx0, ho, wo).
//   Core.  The overlap inset by R on all four sides: hc = ho - 2R, wc = wo - 2R, n = hc * wc pixels; the ref window starts at
//   (ry0 + R, rx0 + R), the mov window at (my0 + R, mx0 + R).  These core windows at e = 0 are what a pair record holds.
//   Words per (plane, pair).  With a(y, x) = ref[ry + y, rx + x] and b_e(y, x) = mov[my + y - ey, mx + x - ex] over the core:
//       0  Sa = sum a      1  Saa = sum a^2      2  Sad = sum |a - b_0|
//   then, row-major over (ey, ex) from (-R, -R):  Sb_e = sum b_e,  Sbb_e = sum b_e^2,  Sab_e = sum a b_e
//   -- 3 + 3 (2R + 1)^2 non-negative 64-bit words.  When the tiles agree at e, their true displacement is d + e.
//
// Integers only: a product of two 16-bit pixels needs all 32 bits, so no sum of such products is ever held in 32 (the inner
// loop sums products of a pixel and a BYTE of the other pixel, which fit); a thread's sums of values over the 32 rows of one
// or two columns fit 32 bits and are widened before they leave the thread.
// Integer addition is associative: the words are numpy's int64 sums bit for bit whatever the schedule.
//
// Mapping: blockIdx.z = plane, blockIdx.y = pair, blockIdx.x = a TILE_ROWS x TILE_COLS piece of the pair's core.  A thread
// owns one column of the piece.  The loads of a piece are paid once and are all in flight together: the piece of the mov
// window with its R-pixel halo goes to LDS (plain element loads, coalesced across the wave: windows start at any column;
// 38 x 262 against 32 x 256 elements at R = 3), the thread's ref column stays in registers (nobody else reads it).  The
// (2R + 1)^2 offsets are then evaluated from there:
//   Sab_e   one pass per ey with the 2R + 1 sums of that row of offsets in registers (14 registers at R = 3 -- all 147 sums
//           of a lane would not fit): per row and offset two 24-bit multiply-adds into 32-bit sums on a mov element read from LDS.
//   Sb_e, Sbb_e  depend on the mov window alone and are box sums of it: a thread sums its columns of the mov piece over the
//           rows of ey = -R and slides that row window down one ey at a time (one row in, one row out), and the window over the
//           columns is all columns minus the first 2R - j and the last j of them -- th + 4R multiplies per column instead
//           of (2R + 1)^2 th.
// Every sum ends in a wave reduction by shuffles (a butterfly that takes up to eight sums at once) into the wave's row of an
// LDS table; after the last pass the four rows are added and go out as one 64-bit atomic add per word per workgroup, into
// words the entry point zeroes on the same stream first.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "device_util.h"

using namespace sq;

namespace {

#define SQ_LDS __attribute__((address_space(3)))

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int WAVES = THREADS / WAVE;
constexpr int TILE_COLS = THREADS;      // one column of the piece per thread
constexpr int TILE_ROWS = 32;           // 32 rows x 65535 < 2^32: a thread's sums of values fit 32 bits
constexpr int ROW_BLOCK = 8;            // rows a thread takes under one branch on the piece's height
static_assert(TILE_ROWS % ROW_BLOCK == 0, "whole blocks of rows");
constexpr int MAX_R = SQ_SEAM_MAX_RADIUS;
constexpr int MAX_WORDS = 3 + 3 * (2 * MAX_R + 1) * (2 * MAX_R + 1);

struct SeamArgs {
    const void *tiles;
    int64_t plane_stride, tile_stride, pitch;      // elements
    const sq_overlap *pairs;                       // the pairs of this launch
    unsigned long long *out;                       // [planes of this launch][n_pairs][words], the first pair of this launch
    int64_t out_plane_stride;                      // n_pairs * words
};

__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m, WAVE), hi = __shfl_xor((uint32_t)(v >> 32), m, WAVE);
    return ((unsigned long long)hi << 32) | lo;
}

// The sums over the wave of P values per lane (P a power of two up to 8), for the price of P - 1 + (6 - log2 P) exchanges
// instead of 6 P: a butterfly in which a lane hands over half of its values at every step and keeps summing the other half
// (the chain of shuffles of one sum after another was measured at nine tenths of the kernel's time at R = 3).  Afterwards the
// lanes with (lane & (64 / P - 1)) == 0 hold one sum each, in v[0]: lane l holds the sum of value l / (64 / P).
template <int P>
__device__ __forceinline__ void wave_sums(unsigned long long (&v)[P], int lane) {
    static_assert(P == 1 || P == 2 || P == 4 || P == 8, "a power of two up to 8");
    int m = WAVE / 2;
#pragma unroll
    for (int half = P / 2; half >= 1; half /= 2, m /= 2) {      // the lanes with bit m set go on with the upper half
        const bool upper = (lane & m) != 0;
#pragma unroll
        for (int i = 0; i < half; ++i) {
            const unsigned long long keep = upper ? v[i + half] : v[i], send = upper ? v[i] : v[i + half];
            v[i] = keep + shfl_xor64(send, m);
        }
    }
    for (; m >= 1; m /= 2) v[0] += shfl_xor64(v[0], m);
}

// The product of two pixels, or of a pixel and a byte of one (at most 65535 each: the unsigned 24-bit multiply gives all 32
// bits of it exactly, at the full rate).  (__umul24 is declared int: the cast keeps the product from being sign-extended.)
__device__ __forceinline__ uint32_t product(uint32_t a, uint32_t b) { return (uint32_t)__umul24(a, b); }

__host__ __device__ inline int64_t pieces_of(int32_t h, int32_t w) {
    return (((int64_t)h + TILE_ROWS - 1) / TILE_ROWS) * (((int64_t)w + TILE_COLS - 1) / TILE_COLS);
}

template <typename T, int R>
__global__ __launch_bounds__(THREADS) void seam_stats_kernel(const SeamArgs a) {
    constexpr int SIDE = 2 * R + 1;
    constexpr int WORDS = 3 + 3 * SIDE * SIDE;
    constexpr int MOV_ROWS = TILE_ROWS + 2 * R, MOV_COLS = TILE_COLS + 2 * R;
    constexpr int ROWS_PER_WAVE = (MOV_ROWS + WAVES - 1) / WAVES, CHUNKS = (MOV_COLS + WAVE - 1) / WAVE;
    constexpr int EDGE = R > 0 ? 2 * R : 1;
    constexpr int P = SIDE <= 1 ? 2 : (SIDE <= 4 ? 4 : 8);      // sums that go through one butterfly: SIDE rounded up to a power of two
    __shared__ T mov_s[MOV_ROWS][MOV_COLS];
    __shared__ unsigned long long ref_part[WAVES][3];                 // Sa, Saa, Sad of a wave's columns
    __shared__ unsigned long long sab_part[WAVES][SIDE * SIDE];       // Sab_e of a wave's columns
    __shared__ unsigned long long mov_total[WAVES][SIDE][2];          // per ey: sum b and sum b^2 over ALL columns of the mov piece
    __shared__ unsigned long long mov_edge[SIDE][2][EDGE][2];         // per ey: the same of its first and of its last 2R columns

    const sq_overlap p = a.pairs[blockIdx.y];
    if (p.h <= 0 || p.w <= 0 || (int64_t)blockIdx.x >= pieces_of(p.h, p.w)) return;      // uniform over the block
    const int n_ct = (p.w + TILE_COLS - 1) / TILE_COLS;
    const int x0 = ((int)blockIdx.x % n_ct) * TILE_COLS, y0 = ((int)blockIdx.x / n_ct) * TILE_ROWS;
    const int tw = min(TILE_COLS, p.w - x0), th = __builtin_amdgcn_readfirstlane(min(TILE_ROWS, p.h - y0));
    const int mov_rows = th + 2 * R, mov_cols = tw + 2 * R;
    const int tid = threadIdx.x, lane = tid % WAVE;
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);

    const T *plane = static_cast<const T *>(a.tiles) + (int64_t)blockIdx.z * a.plane_stride;
    const T *ref = plane + (int64_t)p.ref_tile * a.tile_stride + (int64_t)(p.ref_y0 + y0) * a.pitch + (p.ref_x0 + x0);
    // the mov piece with its halo: it starts R rows above and R columns left of the piece (inside the tile: the entry point
    // has checked that the mov window lies at least R inside it on every side)
    const T *mov = plane + (int64_t)p.mov_tile * a.tile_stride + (int64_t)(p.mov_y0 + y0 - R) * a.pitch + (p.mov_x0 + x0 - R);

    // every load of the thread is issued before the first is used: the mov piece (rows dealt over the waves, columns over the
    // lanes) on its way to LDS, and the thread's own ref column, which stays in registers (no other thread reads it)
    T staged[ROWS_PER_WAVE][CHUNKS];
#pragma unroll
    for (int i = 0; i < ROWS_PER_WAVE; ++i) {
        const int r = wave + WAVES * i;
#pragma unroll
        for (int j = 0; j < CHUNKS; ++j) {
            const int c = lane + WAVE * j;
            staged[i][j] = 0;
            if (r < mov_rows && c < mov_cols) staged[i][j] = mov[(int64_t)r * a.pitch + c];
        }
    }
    const bool active = tid < tw;      // the thread's column lies inside the piece
    uint32_t col[TILE_ROWS];           // a(y, tid), 0 below the piece and outside it: such a pixel adds nothing to a product
#pragma unroll
    for (int y = 0; y < TILE_ROWS; ++y) {
        col[y] = 0;
        if (y < th && active) col[y] = ref[(int64_t)y * a.pitch + tid];
    }
#pragma unroll
    for (int i = 0; i < ROWS_PER_WAVE; ++i) {
        const int r = wave + WAVES * i;
#pragma unroll
        for (int j = 0; j < CHUNKS; ++j) {
            const int c = lane + WAVE * j;
            if (r < mov_rows && c < mov_cols) mov_s[r][c] = staged[i][j];
        }
    }
    lds_written();
    __syncthreads();

    // The mov side.  Sb_e and Sbb_e are sums over a window of the mov piece: rows [2R - k, 2R - k + th) for ey = k - R and
    // columns [2R - j, 2R - j + tw) for ex = j - R.  A thread sums ITS columns of the piece (column tid, and tid + 256 where
    // the halo reaches that far) over the rows of k = 0 and slides the row window down one k at a time (one row in, one row
    // out); the window over the columns is taken at the end: all columns minus the first 2R - j and the last j of them.
    {
        uint32_t tot_s[SIDE];
        unsigned long long tot_c[SIDE];
#pragma unroll
        for (int k = 0; k < SIDE; ++k) {
            tot_s[k] = 0;
            tot_c[k] = 0;
        }
        for (int xc = tid; xc < mov_cols; xc += THREADS) {
            uint32_t s = 0;
            unsigned long long c2 = 0;
            for (int y = 2 * R; y < 2 * R + th; ++y) {
                const uint32_t v = mov_s[y][xc];
                s += v;
                c2 += product(v, v);
            }
#pragma unroll
            for (int k = 0; k < SIDE; ++k) {
                tot_s[k] += s;
                tot_c[k] += c2;
                if (R > 0 && xc < 2 * R) {
                    mov_edge[k][0][xc][0] = s;
                    mov_edge[k][0][xc][1] = c2;
                }
                if (R > 0 && xc >= mov_cols - 2 * R) {
                    mov_edge[k][1][mov_cols - 1 - xc][0] = s;
                    mov_edge[k][1][mov_cols - 1 - xc][1] = c2;
                }
                if (k + 1 < SIDE) {      // ey + 1: row 2R - k - 1 comes in, row 2R - k + th - 1 goes out
                    const uint32_t vi = mov_s[2 * R - k - 1][xc], vo = mov_s[2 * R - k + th - 1][xc];
                    s = s + vi - vo;
                    c2 = c2 + product(vi, vi) - product(vo, vo);
                }
            }
        }
#pragma unroll
        for (int k0 = 0; k0 < SIDE; k0 += P / 2) {      // P / 2 values of ey at a time: their sums of b and of b^2
            unsigned long long v[P];
#pragma unroll
            for (int i = 0; i < P; ++i) v[i] = 0;
#pragma unroll
            for (int i = 0; i < P / 2; ++i) {
                if (k0 + i < SIDE) {
                    v[2 * i] = tot_s[k0 + i];
                    v[2 * i + 1] = tot_c[k0 + i];
                }
            }
            wave_sums<P>(v, lane);
            const int i = lane / (WAVE / P);
            if (lane % (WAVE / P) == 0 && k0 + i / 2 < SIDE) mov_total[wave][k0 + i / 2][i % 2] = v[0];
        }
    }
    // The ref side: Sa, Saa and Sad of the thread's column.  Rows go in blocks of ROW_BLOCK under ONE uniform branch per block,
    // so that the LDS reads of a block are in flight together; a row below the piece holds a = 0 and adds nothing.
    {
        uint32_t sa = 0, sad = 0;
        unsigned long long saa = 0;
#pragma unroll
        for (int y0b = 0; y0b < TILE_ROWS; y0b += ROW_BLOCK) {
            if (y0b < th) {      // (uniform)
#pragma unroll
                for (int y = y0b; y < y0b + ROW_BLOCK; ++y) {
                    const uint32_t va = col[y], vb = mov_s[y + R][tid + R];
                    sa += va;
                    saa += product(va, va);
                    sad += (active && y < th) ? (va > vb ? va - vb : vb - va) : 0u;
                }
            }
        }
        unsigned long long v[4] = {sa, saa, sad, 0};
        wave_sums<4>(v, lane);
        if (lane % (WAVE / 4) == 0 && lane / (WAVE / 4) < 3) ref_part[wave][lane / (WAVE / 4)] = v[0];
    }
    // Sab_e: one pass per ey with the sums of that row of offsets in registers.  64-bit adds run at a fraction of the 32-bit
    // rate, so the products are kept in 32 bits: a = 256 ah + al, and al * b and ah * b are below 2^24 (v_mad_u32_u24, full rate),
    // 32 rows of them below 2^29 -- two 32-bit sums per offset for uint16 pixels, one for uint8 (ah = 0), joined once per pass.
#pragma unroll 1
    for (int k = 0; k < SIDE; ++k) {      // ey = k - R: the mov row of core row y is y + R - ey = y + 2R - k of the piece
        uint32_t lo[SIDE], hi[SIDE];
#pragma unroll
        for (int j = 0; j < SIDE; ++j) lo[j] = hi[j] = 0;
#pragma unroll
        for (int y = 0; y < TILE_ROWS; ++y) {      // (a row below the piece holds a = 0: no branch on the piece's height)
            const uint32_t al = col[y] & 0xffu, ah = col[y] >> 8;
            // (volatile: one element per read.  Left to itself the compiler joins a lane's 2R + 1 neighbours into 12-byte reads
            // at 2-byte alignment, which overlap from lane to lane and were measured several times slower)
            const volatile SQ_LDS T *mrow = (const volatile SQ_LDS T *)&mov_s[y + 2 * R - k][tid];
#pragma unroll
            for (int j = 0; j < SIDE; ++j) {      // ex = j - R: the mov column of core column x is x + R - ex = x + 2R - j
                const uint32_t vb = mrow[2 * R - j];
                lo[j] += product(al, vb);
                if (sizeof(T) == 2) hi[j] += product(ah, vb);
            }
        }
        unsigned long long v[P];
#pragma unroll
        for (int j = 0; j < P; ++j) v[j] = j < SIDE ? (unsigned long long)lo[j < SIDE ? j : 0] + ((unsigned long long)hi[j < SIDE ? j : 0] << 8) : 0ull;
        wave_sums<P>(v, lane);
        if (lane % (WAVE / P) == 0 && lane / (WAVE / P) < SIDE) sab_part[wave][k * SIDE + lane / (WAVE / P)] = v[0];
    }
    lds_written();
    __syncthreads();
    if (tid < WORDS) {
        unsigned long long s = 0;
        if (tid < 3) {
#pragma unroll
            for (int w = 0; w < WAVES; ++w) s += ref_part[w][tid];
        } else {
            const int q = (tid - 3) / 3, t = (tid - 3) % 3, k = q / SIDE, j = q % SIDE;
            if (t == 2) {
#pragma unroll
                for (int w = 0; w < WAVES; ++w) s += sab_part[w][q];
            } else {
#pragma unroll
                for (int w = 0; w < WAVES; ++w) s += mov_total[w][k][t];
                for (int m = 0; m < 2 * R - j; ++m) s -= mov_edge[k][0][m][t];      // the columns left of the window
                for (int m = 0; m < j; ++m) s -= mov_edge[k][1][m][t];              // and right of it
            }
        }
        if (s) atomicAdd(a.out + (int64_t)blockIdx.z * a.out_plane_stride + (int64_t)blockIdx.y * WORDS + tid, s);
    }
}

template <typename T, int R>
hipError_t launch(const SeamArgs &a, dim3 grid, hipStream_t stream) {
    seam_stats_kernel<T, R><<<grid, dim3(THREADS), 0, stream>>>(a);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_radius(int radius, const SeamArgs &a, dim3 grid, hipStream_t stream) {
    switch (radius) {
        case 0: return launch<T, 0>(a, grid, stream);
        case 1: return launch<T, 1>(a, grid, stream);
        case 2: return launch<T, 2>(a, grid, stream);
        default: return launch<T, 3>(a, grid, stream);
    }
}

}   // namespace

extern "C" int sq_seam_stats(const void *tiles_dev, int32_t n_planes, int32_t n_tiles, int32_t h, int32_t w, int64_t plane_stride,
                             int64_t tile_stride, int64_t pitch, int32_t dtype, const sq_overlap *pairs_host,
                             const sq_overlap *pairs_dev, int32_t n_pairs, int32_t radius, uint64_t *out_dev, void *stream_) {
    static_assert(MAX_WORDS == 150, "SQ_SEAM_MAX_RADIUS and the word layout");
    if (dtype != SQ_U8 && dtype != SQ_U16) return fail(SQ_ERR_INVALID, "sq_seam_stats: dtype %d", dtype);
    if (radius < 0 || radius > MAX_R) return fail(SQ_ERR_INVALID, "sq_seam_stats: radius %d outside 0..%d", radius, MAX_R);
    if (n_planes < 0 || n_tiles < 0 || n_pairs < 0 || h <= 0 || w <= 0 || pitch < w)
        return fail(SQ_ERR_INVALID, "sq_seam_stats: bad sizes (planes=%d tiles=%d pairs=%d %dx%d pitch %lld)", n_planes, n_tiles,
                    n_pairs, h, w, (long long)pitch);
    if (n_pairs == 0 || n_planes == 0) return SQ_OK;
    if (!tiles_dev || !pairs_host || !pairs_dev || !out_dev) return fail(SQ_ERR_INVALID, "sq_seam_stats: NULL buffer");
    const int esize = dtype == SQ_U16 ? 2 : 1;
    if (reinterpret_cast<uintptr_t>(tiles_dev) % esize || reinterpret_cast<uintptr_t>(out_dev) % 8 ||
        reinterpret_cast<uintptr_t>(pairs_dev) % 4)
        return fail(SQ_ERR_INVALID, "sq_seam_stats: tiles must be aligned to their element, the pairs to 4 and the words to 8 bytes");
    const int64_t tile = (int64_t)(h - 1) * pitch + w;
    if (n_tiles > 1 && tile_stride < tile) return fail(SQ_ERR_INVALID, "sq_seam_stats: tile stride smaller than a tile");
    if (n_tiles == 0) return fail(SQ_ERR_INVALID, "sq_seam_stats: %d pairs of no tiles", n_pairs);
    const int64_t limit = INT64_MAX / 4;
    if (tile > limit / n_tiles || tile_stride < 0 || tile_stride > limit / n_tiles)
        return fail(SQ_ERR_INVALID, "sq_seam_stats: extents beyond the address space");
    const int64_t plane = (int64_t)(n_tiles - 1) * tile_stride + tile;
    if (n_planes > 1 && plane_stride < plane) return fail(SQ_ERR_INVALID, "sq_seam_stats: plane stride smaller than a plane's tiles");
    if (plane > limit / n_planes || plane_stride < 0 || plane_stride > limit / n_planes)
        return fail(SQ_ERR_INVALID, "sq_seam_stats: extents beyond the address space");
    int64_t pieces = 1;
    for (int32_t i = 0; i < n_pairs; ++i) {
        const sq_overlap &p = pairs_host[i];
        if (p.ref_tile < 0 || p.ref_tile >= n_tiles || p.mov_tile < 0 || p.mov_tile >= n_tiles)
            return fail(SQ_ERR_INVALID, "sq_seam_stats: pair %d names tiles %d, %d of %d", i, p.ref_tile, p.mov_tile, n_tiles);
        if (p.h < 0 || p.w < 0 || p.ref_y0 < 0 || p.ref_x0 < 0 || (int64_t)p.ref_y0 + p.h > h || (int64_t)p.ref_x0 + p.w > w)
            return fail(SQ_ERR_INVALID, "sq_seam_stats: ref window %d (%d x %d at (%d, %d)) leaves its %d x %d tile", i, p.h, p.w,
                        p.ref_y0, p.ref_x0, h, w);
        if (p.mov_y0 < radius || p.mov_x0 < radius || (int64_t)p.mov_y0 + p.h + radius > h || (int64_t)p.mov_x0 + p.w + radius > w)
            return fail(SQ_ERR_INVALID, "sq_seam_stats: mov window %d (%d x %d at (%d, %d)) is nearer than %d to an edge of its %d x %d tile",
                        i, p.h, p.w, p.mov_y0, p.mov_x0, radius, h, w);
        if ((int64_t)p.h * p.w > (1ll << 31))
            return fail(SQ_ERR_UNSUPPORTED, "sq_seam_stats: core %d of %d x %d is beyond 2^31 pixels: a word could wrap", i, p.h, p.w);
        if (p.h > 0 && p.w > 0) pieces = std::max(pieces, pieces_of(p.h, p.w));
    }
    if (pieces > INT32_MAX) return fail(SQ_ERR_UNSUPPORTED, "sq_seam_stats: a core needs more workgroups than a launch has");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int side = 2 * radius + 1, words = 3 + 3 * side * side;

    hipError_t e = hipMemsetAsync(out_dev, 0, sizeof(uint64_t) * (size_t)n_planes * (size_t)n_pairs * (size_t)words, stream);
    if (e != hipSuccess) return fail(SQ_ERR_HIP, "sq_seam_stats: zeroing the words: %s", hipGetErrorString(e));
    SeamArgs a{};
    a.plane_stride = plane_stride;
    a.tile_stride = tile_stride;
    a.pitch = pitch;
    a.out_plane_stride = (int64_t)n_pairs * words;
    for (int32_t p0 = 0; p0 < n_planes; p0 += 65535) {
        for (int32_t q0 = 0; q0 < n_pairs; q0 += 65535) {
            const dim3 grid((unsigned)pieces, (unsigned)std::min<int32_t>(65535, n_pairs - q0),
                            (unsigned)std::min<int32_t>(65535, n_planes - p0));
            a.tiles = static_cast<const char *>(tiles_dev) + (int64_t)p0 * plane_stride * esize;
            a.pairs = pairs_dev + q0;
            a.out = reinterpret_cast<unsigned long long *>(out_dev) + (int64_t)p0 * a.out_plane_stride + (int64_t)q0 * words;
            e = dtype == SQ_U16 ? launch_radius<uint16_t>(radius, a, grid, stream) : launch_radius<uint8_t>(radius, a, grid, stream);
            if (e != hipSuccess) return fail(SQ_ERR_HIP, "sq_seam_stats: launch failed: %s", hipGetErrorString(e));
        }
    }
    return SQ_OK;
}

// OME-TIFF tiles leave the GPU as baseline JPEG: one self-contained ITU-T T.81 stream per tile (TIFF Compression 7), the lossy
// codec of the pyramid TIFF writer (ometiff.PyramidTiffWriter) next to deflate.hip's lossless one.  uint8 planes only; every
// plane is a grey image, so one quantisation table (Annex K.1 luminance scaled by libjpeg's quality rule) and the fixed Annex
// K.3.3 luminance Huffman tables serve everything.
//
// Stream of a tile of tile_h x tile_w elements (zero past the plane's edge; image-stitcher_amd/jpegtile.py states it in numpy and
// the device is held to that byte for byte):
//   SOI | DQT | SOF0 | DHT (DC 0, AC 0) | DRI (tile_w / 8) | SOS | entropy-coded data | EOI          (312 bytes before the data)
// One restart interval = one row of 8 x 8 blocks: the DC prediction restarts at 0, the interval is padded with 1-bits to a byte,
// RSTm (m mod 8) stands between intervals.  With fixed tables a block's bits depend only on the block and on the DC before it,
// so an interval is coded on its own by one wave and the intervals of a tile are concatenated.  FF 00 for every FF of the data.
// Forward transform in integers (no floating point here): x = pixel - 128, N = C x C^T with C = round(2^10 a(u) cos((2j+1) u
// pi / 16)) as 64 literals (CM below), no intermediate rounding; coefficient = sign(N) ((|N| + D / 2) // D), D = Q 2^20.
// Bounds: a row of |C| sums to at most 8 * 362 = 2896, so |N| <= 128 * 2896^2 < 2^30, D / 2 <= 255 * 2^19 < 2^27: 32 bits hold
// everything, and the inputs of both passes (<= 2 * 2896 * 128 < 2^23) are 24-bit multiplicands.  The division: (|N| + D / 2)
// >> 20 (<= 1151) is divided by Q with the reciprocal floor(2^16 / Q) and one correction step.
// All-zero tiles get size 0 (the writer points them at one shared zero-tile stream).
//
// Kernels:
//   jpeg_intervals_kernel<EMIT>  one WAVE (one 64-thread workgroup) per interval, a lane per block, wider tiles in rounds of 64
//                            blocks: the lane loads its block, transforms and quantises it in registers and leaves the 64
//                            coefficients in zigzag order in LDS; the DC before it comes by a shuffle (lane 0: the carry of the
//                            round before).  The lane counts its block's bits, a wave prefix sum places them, the lane codes the
//                            block again into a 64-bit accumulator whose full words are OR-ed into the round's bit window in LDS.
//                            The window's whole words are then byte-stuffed (a second prefix sum, over bytes + FFs) and leave.
//                            EMIT = false only counts the stuffed bytes (and notes whether the tile holds a non-zero pixel);
//                            EMIT = true repeats the work and writes to the interval's final place -- the exact sizes are known
//                            before any byte is written, so nothing can pass out_capacity and no slot memory is needed.
//   jpeg_tile_kernel         interval sizes -> interval starts inside the tile and the tile's size -> exclusive scan
//                            (packed_stream.h).
// Grid, argument checks, scratch carving, wave helpers and the scan are packed_stream.h's: an interval is a part of its tile.
// Integer / bit work out of LDS; nothing here is GEMM-shaped.  A wave holds 22 KiB of LDS (8 KiB coefficients, 13 KiB bit window
// -- the worst case of 64 blocks, 20 + 63 * 26 bits each --, 1 KiB code tables): 7 waves per CU.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "packed_stream.h"

using namespace sq;

namespace {

constexpr int HEADER = 312;                     // SOI .. SOS
constexpr int MAX_SIDE = 65496;                 // the largest multiple of 8 below libjpeg's JPEG_MAX_DIMENSION (65500)
constexpr int BLOCK_BITS = 20 + 63 * 26;        // longest DC code 9 + 11 bits, 63 times the longest AC code 16 + 10 bits
constexpr int STAGE = (31 + 64 * BLOCK_BITS + 31) / 32 + 3;      // words of the bit window: a carried partial word + 64 blocks

constexpr int CM[8][8] = {{362, 362, 362, 362, 362, 362, 362, 362},     {502, 426, 284, 100, -100, -284, -426, -502},
                          {473, 196, -196, -473, -473, -196, 196, 473}, {426, -100, -502, -284, 284, 502, 100, -426},
                          {362, -362, -362, 362, 362, -362, -362, 362}, {284, -502, 100, 426, -426, -100, 502, -284},
                          {196, -473, 473, -196, -196, 473, -473, 196}, {100, -284, 426, -502, 502, -426, 284, -100}};
constexpr uint8_t BASE[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                              69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                              81, 104, 113, 92, 49, 64, 78,  87,  103, 121, 120, 101, 72, 92, 95,  98,  112, 100, 103, 99};
constexpr uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t DC_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t AC_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D};
constexpr uint8_t AC_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
    0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
    0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5,
    0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};

// the canonical codes of Annex C as code | length << 16, indexed by symbol (0: no code); pos[n]: zigzag position of natural n
struct Tables {
    uint32_t dc[12];
    uint32_t ac[256];
    uint8_t pos[64];
};
constexpr Tables make_tables() {
    Tables t{};
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < DC_BITS[len - 1]; ++i) t.dc[DC_VALS[k++]] = code++ | ((uint32_t)len << 16);
        code <<= 1;
    }
    code = 0;
    k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < AC_BITS[len - 1]; ++i) t.ac[AC_VALS[k++]] = code++ | ((uint32_t)len << 16);
        code <<= 1;
    }
    for (int z = 0; z < 64; ++z) t.pos[ZIGZAG[z]] = (uint8_t)z;
    return t;
}
constexpr Tables TABLES = make_tables();
__constant__ Tables d_tables = make_tables();

struct JpegParams {                   // parts are the tile's restart intervals (rows of blocks)
    const uint8_t *planes;
    int64_t plane_stride, pitch;      // elements
    int32_t n_planes, h, w;
    int32_t th, tw, nty, ntx;         // TileGrid's fields, flat: the struct embedded here changed the counting pass's code
    int32_t parts, nblk;              // intervals per tile, blocks per interval
    int32_t aligned;                  // every block row starts on an 8-byte boundary
    int64_t n_tiles, n_units;
    uint32_t *int_size;               // [n_units]: stuffed bytes of the interval, then its start behind the tile's header
    PackedOut o;
    uint32_t recip[64];               // floor(2^16 / Q), natural order
    uint8_t q[64];                    // the divisors Q, natural order
    uint8_t header[HEADER];
};

struct WaveLds {
    int16_t coef[64][64];             // [zigzag position][lane]: a lane walks its column without bank conflicts
    uint32_t stage[STAGE];            // the round's bits, MSB first in every word
    uint32_t ac[256];
    uint32_t dc[12];
};

// one 8-point pass over a[0], a[S], .., a[7 S]: out[u] = sum_j CM[u][j] a[j], through the symmetry CM[u][7 - j] = (-1)^u CM[u][j]
template <int S>
__device__ __forceinline__ void dct8(int *a) {
    int s[4], d[4], o[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s[j] = a[j * S] + a[(7 - j) * S];
        d[j] = a[j * S] - a[(7 - j) * S];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        int acc = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += __mul24(CM[u][j], (u & 1) ? d[j] : s[j]);
        o[u] = acc;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u * S] = o[u];
}

// A lane's bits: counted (EMIT false) or shifted into a 64-bit accumulator whose upper word leaves for the window when full.
struct Put {
    uint32_t *stage;
    uint64_t acc;
    int fill, w, bits;
};
template <bool EMIT>
__device__ __forceinline__ void put(Put &p, uint32_t val, int nb) {      // 1 <= nb <= 26, fill < 32
    if (!EMIT) {
        p.bits += nb;
        return;
    }
    p.acc |= (uint64_t)val << (64 - p.fill - nb);
    p.fill += nb;
    if (p.fill >= 32) {
        atomicOr(&p.stage[p.w++], (uint32_t)(p.acc >> 32));
        p.acc <<= 32;
        p.fill -= 32;
    }
}

// Code + magnitude bits of v (v != 0 or the DC difference 0) under table entry t of its category
__device__ __forceinline__ int category(int v) { return v ? 32 - __builtin_clz((unsigned)(v < 0 ? -v : v)) : 0; }

template <bool EMIT>
__device__ __forceinline__ void code_block(const WaveLds &L, int lane, int dc_diff, Put &p) {
    {
        const int s = category(dc_diff);
        const uint32_t t = L.dc[s];
        const uint32_t mag = (uint32_t)(dc_diff < 0 ? dc_diff + (1 << s) - 1 : dc_diff);
        put<EMIT>(p, ((t & 0xFFFFu) << s) | mag, (int)(t >> 16) + s);
    }
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int c = L.coef[k][lane];
        if (c == 0) {
            ++run;
            continue;
        }
        while (run >= 16) {
            const uint32_t t = L.ac[0xF0];      // ZRL
            put<EMIT>(p, t & 0xFFFFu, (int)(t >> 16));
            run -= 16;
        }
        const int s = category(c);
        const uint32_t t = L.ac[(run << 4) | s];
        const uint32_t mag = (uint32_t)(c < 0 ? c + (1 << s) - 1 : c);
        put<EMIT>(p, ((t & 0xFFFFu) << s) | mag, (int)(t >> 16) + s);
        run = 0;
    }
    if (run) {                                  // EOB unless coefficient 63 was coded
        const uint32_t t = L.ac[0x00];
        put<EMIT>(p, t & 0xFFFFu, (int)(t >> 16));
    }
}

// The first nbytes bytes of the window leave byte-stuffed (EMIT: to dst + done); -> done + what they take.  Whole wave.
template <bool EMIT>
__device__ __forceinline__ int stuff_out(const uint32_t *stage, int nbytes, uint8_t *dst, int done, int lane) {
    const int nwords = (nbytes + 3) >> 2;
    for (int w0 = 0; w0 < nwords; w0 += 64) {
        const int wi = w0 + lane;
        const int valid = min(4, max(0, nbytes - 4 * wi));
        const uint32_t word = valid ? stage[wi] : 0u;
        int n = valid;
        for (int k = 0; k < valid; ++k) n += ((word >> (24 - 8 * k)) & 0xFFu) == 0xFFu ? 1 : 0;
        const int incl = wave_scan(n, lane);
        if (EMIT) {
            uint8_t *o = dst + done + incl - n;
            for (int k = 0; k < valid; ++k) {
                const uint8_t b = (uint8_t)(word >> (24 - 8 * k));
                *o++ = b;
                if (b == 0xFFu) *o++ = 0;
            }
        }
        done += __shfl(incl, 63);
    }
    return done;
}

template <bool EMIT>
__global__ __launch_bounds__(64) void jpeg_intervals_kernel(const JpegParams P) {
    __shared__ WaveLds L;
    const int lane = threadIdx.x;
    const int64_t gi = blockIdx.x;
    const int64_t tile = gi / P.parts;
    const int b = (int)(gi - tile * P.parts);
    const int per_plane = P.nty * P.ntx;
    const int plane = (int)(tile / per_plane);
    const int ti = (int)(tile - (int64_t)plane * per_plane);
    const int tyi = ti / P.ntx, txi = ti - tyi * P.ntx;
    uint8_t *dst = nullptr;
    if (EMIT) {
        if (*P.o.status) return;
        const uint64_t at = P.o.offsets[tile];
        if (P.o.offsets[tile + 1] == at) return;      // a tile of zeros
        uint8_t *base = P.o.out + at;
        if (b == 0)
            for (int k = lane; k < HEADER; k += 64) base[k] = P.header[k];
        dst = base + HEADER + P.int_size[gi];
    }
    for (int i = lane; i < 256; i += 64) L.ac[i] = d_tables.ac[i];
    if (lane < 12) L.dc[lane] = d_tables.dc[lane];
    for (int i = lane; i < STAGE; i += 64) L.stage[i] = 0;
    wave_sync();

    const int y0 = tyi * P.th + b * 8;
    const uint8_t *rows = P.planes + (int64_t)plane * P.plane_stride + (int64_t)y0 * P.pitch;
    int bitpos = 0, done = 0, dc_carry = 0;
    uint32_t any = 0;
    for (int blk0 = 0; blk0 < P.nblk; blk0 += 64) {
        const int blk = blk0 + lane;
        const bool active = blk < P.nblk;
        int dcq = 0;
        if (active) {
            const int x0 = txi * P.tw + blk * 8;
            int v[64];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                uint64_t px = 0;
                if (y0 + r < P.h && x0 < P.w) {
                    const uint8_t *src = rows + (int64_t)r * P.pitch + x0;
                    if (P.aligned && x0 + 8 <= P.w) {
                        px = *reinterpret_cast<const uint64_t *>(src);
                    } else {
                        const int nx = min(8, P.w - x0);
                        for (int j = 0; j < nx; ++j) px |= (uint64_t)src[j] << (8 * j);
                    }
                }
                any |= (uint32_t)px | (uint32_t)(px >> 32);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[r * 8 + j] = (int)((px >> (8 * j)) & 0xFFu) - 128;
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) dct8<1>(v + r * 8);
#pragma unroll
            for (int c = 0; c < 8; ++c) dct8<8>(v + c);
#pragma unroll
            for (int n = 0; n < 64; ++n) {
                const int N = v[n];
                const uint32_t Q = P.q[n];
                const uint32_t m = ((uint32_t)(N < 0 ? -N : N) + (Q << 19)) >> 20;
                uint32_t qv = (m * P.recip[n]) >> 16;
                if (m - qv * Q >= Q) ++qv;
                const int c = N < 0 ? -(int)qv : (int)qv;
                L.coef[TABLES.pos[n]][lane] = (int16_t)c;
                if (n == 0) dcq = c;
            }
        }
        int prev = __shfl_up(dcq, 1);
        if (lane == 0) prev = dc_carry;
        dc_carry = __shfl(dcq, 63);
        Put count{nullptr, 0, 0, 0, 0};
        if (active) code_block<false>(L, lane, dcq - prev, count);
        const int incl = wave_scan(count.bits, lane);
        if (active) {
            const int start = bitpos + incl - count.bits;
            Put p{L.stage, 0, start & 31, start >> 5, 0};
            code_block<true>(L, lane, dcq - prev, p);
            if (p.fill) atomicOr(&L.stage[p.w], (uint32_t)(p.acc >> 32));
        }
        bitpos += __shfl(incl, 63);
        wave_sync();
        // the whole words leave; the partial one moves to the front of the next round's window
        const int full = bitpos >> 5;
        done = stuff_out<EMIT>(L.stage, 4 * full, dst, done, lane);
        const uint32_t part = L.stage[full];
        wave_sync();
        for (int k = lane; k <= full; k += 64) L.stage[k] = 0;
        wave_sync();
        if (lane == 0) L.stage[0] = part;
        wave_sync();
        bitpos &= 31;
    }
    {   // 1-bits up to the byte boundary, then the last bytes
        const int pad = (8 - (bitpos & 7)) & 7;
        if (lane == 0 && pad) L.stage[0] |= ((1u << pad) - 1u) << (32 - bitpos - pad);
        wave_sync();
        done = stuff_out<EMIT>(L.stage, (bitpos + pad) >> 3, dst, done, lane);
    }
    if (EMIT) {
        if (lane == 0) {                        // RSTm between intervals, EOI behind the last
            dst[done] = 0xFF;
            dst[done + 1] = b == P.parts - 1 ? 0xD9 : (uint8_t)(0xD0 + (b & 7));
        }
    } else {
        if (lane == 0) P.int_size[gi] = (uint32_t)done;
        if (__builtin_amdgcn_ballot_w64(any != 0) && lane == 0) atomicOr(&P.o.tile_any[tile], 1u);
    }
}

// interval sizes of a tile -> their starts behind the header (every interval is followed by a 2-byte marker), and the tile's size
__global__ __launch_bounds__(64) void jpeg_tile_kernel(const JpegParams P, uint64_t *sizes) {
    const int64_t tile = blockIdx.x;
    const int lane = threadIdx.x;
    uint32_t *v = P.int_size + tile * P.parts;
    uint32_t run = 0;
    for (int i0 = 0; i0 < P.parts; i0 += 64) {
        const int i = i0 + lane;
        const int n = i < P.parts ? (int)v[i] + 2 : 0;
        const int incl = wave_scan(n, lane);
        if (i < P.parts) v[i] = run + (uint32_t)(incl - n);
        run += (uint32_t)__shfl(incl, 63);
    }
    if (lane == 0) sizes[tile] = P.o.tile_any[tile] ? (uint64_t)HEADER + run : 0u;
}

constexpr const char *FN = "sq_jpeg_encode_planes";

int geometry(JpegParams &P, int32_t h, int32_t w, int32_t n_planes, int32_t dtype, int32_t th, int32_t tw) {
    TileGrid g{};
    const int rc = stream_grid(g, P.n_tiles, "sq_jpeg", "tiles", true, h, w, n_planes, th, tw);
    if (rc != SQ_OK) return rc;
    P.th = g.th, P.tw = g.tw, P.nty = g.nty, P.ntx = g.ntx;
    if (dtype != SQ_U8) return fail(SQ_ERR_UNSUPPORTED, "sq_jpeg: dtype %d (uint8 planes only: baseline JPEG holds 8 bits)", dtype);
    // T.81 holds sides below 65536, but libjpeg -- the decoder behind nearly every TIFF reader -- refuses more than 65500
    if (th > MAX_SIDE || tw > MAX_SIDE || (int64_t)th * tw > (int64_t)32 << 20)
        return fail(SQ_ERR_UNSUPPORTED, "sq_jpeg: tiles of %d x %d (sides up to %d, at most 32 Mi elements)", th, tw, MAX_SIDE);
    P.n_planes = n_planes, P.h = h, P.w = w;
    P.parts = th / 8;
    P.nblk = tw / 8;
    P.n_units = P.n_tiles * P.parts;
    return SQ_OK;
}

void carve(JpegParams &P, Scratch &sc) {
    P.int_size = sc.take<uint32_t>(P.n_units);
    P.o.tile_any = sc.take<uint32_t>(P.n_tiles);
}

void put16(uint8_t *&o, int v) {
    *o++ = (uint8_t)(v >> 8);
    *o++ = (uint8_t)(v & 0xFF);
}

// libjpeg's jpeg_quality_scaling + jpeg_add_quant_table (baseline), the reciprocals and SOI .. SOS
void tables_and_header(JpegParams &P, int quality) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int n = 0; n < 64; ++n) {
        const int q = std::min(255, std::max(1, (BASE[n] * s + 50) / 100));
        P.q[n] = (uint8_t)q;
        P.recip[n] = 65536u / (uint32_t)q;
    }
    uint8_t *o = P.header;
    put16(o, 0xFFD8);
    put16(o, 0xFFDB);
    put16(o, 67);
    *o++ = 0x00;                                // 8-bit table 0
    for (int z = 0; z < 64; ++z) *o++ = P.q[ZIGZAG[z]];
    put16(o, 0xFFC0);
    put16(o, 11);
    *o++ = 8;
    put16(o, P.th);
    put16(o, P.tw);
    *o++ = 1;                                   // one component: id 1, 1 x 1, table 0
    *o++ = 1;
    *o++ = 0x11;
    *o++ = 0;
    put16(o, 0xFFC4);
    put16(o, 2 + 1 + 16 + 12 + 1 + 16 + 162);
    *o++ = 0x00;                                // DC table 0
    for (int i = 0; i < 16; ++i) *o++ = DC_BITS[i];
    for (int i = 0; i < 12; ++i) *o++ = DC_VALS[i];
    *o++ = 0x10;                                // AC table 0
    for (int i = 0; i < 16; ++i) *o++ = AC_BITS[i];
    for (int i = 0; i < 162; ++i) *o++ = AC_VALS[i];
    put16(o, 0xFFDD);
    put16(o, 4);
    put16(o, P.nblk);
    put16(o, 0xFFDA);
    put16(o, 8);
    *o++ = 1;
    *o++ = 1;                                   // component 1: DC 0, AC 0
    *o++ = 0x00;
    *o++ = 0;                                   // Ss, Se, Ah Al
    *o++ = 63;
    *o++ = 0;
}

}  // namespace

extern "C" int64_t sq_jpeg_chunk_count(int32_t n_planes, int32_t h, int32_t w, int32_t tile_h, int32_t tile_w) {
    JpegParams P{};
    const int rc = geometry(P, h, w, n_planes, SQ_U8, tile_h, tile_w);
    if (rc != SQ_OK) return rc;
    return P.n_tiles;
}

extern "C" int64_t sq_jpeg_out_bound(int32_t n_planes, int32_t h, int32_t w, int32_t dtype, int32_t tile_h, int32_t tile_w) {
    JpegParams P{};
    const int rc = geometry(P, h, w, n_planes, dtype, tile_h, tile_w);
    if (rc != SQ_OK) return rc;
    // every block at its longest codes and every byte of the data an FF; a marker behind every interval
    const int64_t interval = 2 * (((int64_t)P.nblk * BLOCK_BITS + 7) / 8) + 2;
    return P.n_tiles * (HEADER + P.parts * interval);
}

extern "C" int64_t sq_jpeg_scratch_bytes(int32_t n_planes, int32_t h, int32_t w, int32_t dtype, int32_t tile_h, int32_t tile_w) {
    JpegParams P{};
    const int rc = geometry(P, h, w, n_planes, dtype, tile_h, tile_w);
    if (rc != SQ_OK) return rc;
    Scratch sc{0};
    carve(P, sc);
    return sc.bytes();
}

extern "C" int sq_jpeg_encode_planes(const void *planes_dev, int64_t plane_stride, int64_t pitch, int32_t n_planes, int32_t h,
                                     int32_t w, int32_t dtype, int32_t tile_h, int32_t tile_w, int32_t quality, void *scratch_dev,
                                     int64_t scratch_bytes, uint64_t *offsets_dev, void *out_dev, int64_t out_capacity,
                                     uint32_t *status_dev, void *stream_) {
    int rc = stream_null(FN, planes_dev, scratch_dev, offsets_dev, out_dev, status_dev);
    if (rc != SQ_OK) return rc;
    JpegParams P{};
    rc = geometry(P, h, w, n_planes, dtype, tile_h, tile_w);
    if (rc != SQ_OK) return rc;
    if (quality < 1 || quality > 100) return fail(SQ_ERR_INVALID, "%s: quality %d (1..100)", FN, quality);
    Scratch sc{reinterpret_cast<uintptr_t>(scratch_dev)};
    carve(P, sc);
    rc = stream_args(FN, P.o, n_planes, h, w, plane_stride, pitch, scratch_dev, scratch_bytes, sc.bytes(), offsets_dev, out_dev, out_capacity, status_dev);
    if (rc != SQ_OK) return rc;
    if (P.n_units > 2147483647) return fail(SQ_ERR_UNSUPPORTED, "%s: too many tiles", FN);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    rc = stream_begin(FN, P.o, P.n_tiles, s);
    if (rc != SQ_OK || P.n_tiles == 0) return rc;
    P.planes = static_cast<const uint8_t *>(planes_dev), P.plane_stride = plane_stride, P.pitch = pitch;
    P.aligned = ((reinterpret_cast<uintptr_t>(planes_dev) | (uintptr_t)plane_stride | (uintptr_t)pitch) & 7) == 0;
    tables_and_header(P, quality);
    hipLaunchKernelGGL(jpeg_intervals_kernel<false>, dim3((unsigned)P.n_units), dim3(64), 0, s, P);
    hipLaunchKernelGGL(jpeg_tile_kernel, dim3((unsigned)P.n_tiles), dim3(64), 0, s, P, offsets_dev);
    stream_scan(P.o, P.n_tiles, s);
    hipLaunchKernelGGL(jpeg_intervals_kernel<true>, dim3((unsigned)P.n_units), dim3(64), 0, s, P);
    return stream_end(FN);
}

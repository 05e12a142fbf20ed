// OME-TIFF tiles leave the GPU compressed: one RFC 1950 zlib stream per tile (TIFF Compression 8, "Adobe deflate"), with
// TIFF's horizontal differencing (Predictor 2) applied on the way in.  TIFF has no LZ4 and no byte shuffle, so the Blosc
// encoder (blosc.hip) cannot serve the pyramid TIFF writer (ometiff.PyramidTiffWriter).
//
// Stream of a tile of tile_h x tile_w elements (little endian, zero past the plane's edge; tests/deflate_ref.py restates it):
//   78 01 | one deflate block per 16 KiB SEGMENT of the (predicted) tile bytes | Adler-32 of those bytes, big endian
// A segment is coded on its own by one wave, so the segments of a tile can be concatenated:
//   * the only matches are ELEMENT RUNS (distance = itemsize, length 3..258; zlib's Z_RLE carried over to 16-bit elements): an
//     element that equals its left neighbour continues a run; a run is cut into pieces of at most 258 bytes from its start,
//     and a piece shorter than 3 bytes goes out as literals.  No hash table.
//   * one dynamic-Huffman block (BTYPE 10) per segment, code lengths from the segment's own symbol counts (Moffat / Katajainen
//     in-place minimum redundancy over the sorted counts), limited to 15 by moving codes between lengths until the Kraft sum
//     fits; the code-length code is the trivial one (4-bit codes for the lengths 0..15, no repeat codes); the single distance
//     symbol takes one bit (RFC 1951 3.2.7).
//   * a segment that does not shrink is a stored block (BTYPE 00): sq_deflate_out_bound's worst case
//   * a non-final segment ends with an empty stored block (Z_SYNC_FLUSH), which brings it to a byte boundary; the last one
//     carries BFINAL.
// All-zero tiles get size 0 (the writer points them at one shared zero-tile stream).
//
// Kernels:
//   deflate_segments_kernel  one WAVE (one 64-thread workgroup) per segment: gather + predictor into LDS (and the segment's
//                            Adler sums), ballot words of "equals the element before", pass 1 counts the symbols, the code
//                            is built (sort: rank by comparison, all lanes; tree and canonical codes: lane 0), pass 2
//                            derives the same tokens again and emits them: a wave prefix sum over the code lengths gives
//                            every lane its bit position, the bits are OR-ed into a window of LDS words that is flushed to
//                            the segment's slot as whole words.  The exact size is known before pass 2, so a segment that
//                            would not shrink is stored instead and no write can pass the slot.
//   tile_size_kernel / deflate_assemble_kernel
//                            tile sizes -> exclusive scan (packed_stream.h) -> header, segments and the combined Adler-32 packed
//                            densely, so that only the COMPRESSED bytes cross PCIe.
// Grid, argument checks, scratch carving, wave helpers and the scan are packed_stream.h's: a segment is a part of its tile.
// Integer / bit work out of LDS; nothing here is GEMM-shaped.  22 KiB of LDS per wave: 7 waves per CU.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "packed_stream.h"

using namespace sq;

namespace {

constexpr int SEG = 16384;              // bytes of a tile one wave codes
constexpr int SLOT = SEG + 16;          // a coded segment is at most SEG + 5 bytes; whole words are written
constexpr int NSYM = 288;               // literal / length symbols 0..285, padded
constexpr int NLITLEN = 286;
constexpr int STAGE = 160;              // LDS words of the bit window (at most 64 kept + 64 new + the partial one)
constexpr uint32_t ADLER = 65521u;

struct DeflateParams {                // parts are the tile's 16 KiB segments
    const void *planes;
    int64_t plane_stride, pitch;      // elements
    int32_t n_planes, h, w, esz;      // element size 1 or 2
    TileGrid g;
    int32_t tile_bytes, parts;        // uncompressed tile size, segments per tile
    int32_t predictor;                // 1: none, 2: horizontal differencing
    int64_t n_tiles, n_units;
    uint8_t *slots;                   // [n_units][SLOT]
    uint32_t *seg_size;               // [n_units]
    uint32_t *seg_adler;              // [n_units]: sum of bytes | weighted sum << 16, both mod 65521
    PackedOut o;
};

struct WaveLds {
    uint32_t src[SEG / 4 + 4];        // the segment's predicted bytes
    uint64_t eqw[SEG / 64 + 2];       // bit i: element i equals element i - 1
    uint32_t tab[NSYM];               // symbol counts, then bit-reversed code | length << 16
    uint32_t key[NSYM];               // sorted counts, then code lengths in sorted order
    uint16_t sym[NSYM];               // symbols in sorted order
    uint32_t stage[STAGE];
    uint32_t bl[16], next[16];
    uint32_t info[4];                 // data bits, literal / length codes sent
};

// first index j in [cs, lim) whose bit is clear, else lim (lim <= number of elements: no word past the last is read)
__device__ __forceinline__ int run_end(const uint64_t *eqw, int cs, int lim) {
    int j = cs;
    while (j < lim) {
        const uint64_t z = (~eqw[j >> 6]) >> (j & 63);
        if (z) {
            j += __builtin_ctzll(z);
            break;
        }
        j = (j | 63) + 1;
    }
    return min(j, lim);
}

// length 3..258 -> symbol 257..285, number of extra bits, their value
__device__ __forceinline__ void length_code(int len, int &symbol, int &eb, int &ev) {
    const int l = len - 3;
    if (len == 258) {
        symbol = 285, eb = 0, ev = 0;
    } else if (l < 8) {
        symbol = 257 + l, eb = 0, ev = 0;
    } else {
        eb = 29 - __builtin_clz((unsigned)l);         // floor(log2 l) - 2
        symbol = 257 + 4 * (eb + 1) + ((l >> eb) & 3);
        ev = l & ((1 << eb) - 1);
    }
}

// What element i stands for, from the ballot word m of its round and the start `carry` of a run that entered the round:
// 0 nothing (inside a match), 1 literal, 2 a match of `len` bytes that starts here.
template <int ESZ>
__device__ __forceinline__ int token_of(const uint64_t *eqw, uint64_t m, int base, int lane, int carry, int nel, int &len) {
    constexpr int M = 258 / ESZ;                      // elements of the longest match
    if (!((m >> lane) & 1)) return 1;
    const uint64_t zl = ~m & ((lane == 63) ? ~0ull : ((2ull << lane) - 1));
    const int s = zl ? base + 64 - __builtin_clzll(zl) : carry;      // first element of the run of equal neighbours
    const int i = base + lane;
    const int cs = s + ((i - s) / M) * M;             // start of this element's piece of the run
    const int clen = run_end(eqw, cs, min(cs + M, nel)) - cs;
    if (clen * ESZ < 3) return 1;
    if (i != cs) return 0;
    len = clen * ESZ;
    return 2;
}

struct Emitter {
    uint32_t *stage, *outw;
    int wb, bitpos;
};

__device__ __forceinline__ void flush(Emitter &E, int full, int lane) {      // `full` whole words leave the window
    for (int k = lane; k < full; k += 64)
        if (E.wb + k < SLOT / 4) E.outw[E.wb + k] = E.stage[k];      // (the size was worked out beforehand: never past the slot)
    const uint32_t part = E.stage[full];
    wave_sync();
    for (int k = lane; k <= full; k += 64) E.stage[k] = 0;
    wave_sync();
    if (lane == 0) E.stage[0] = part;
    wave_sync();
    E.wb += full;
}

// every lane appends nb (0..32) bits of val, in lane order; called by the whole wave
__device__ __forceinline__ void emit(Emitter &E, uint32_t val, int nb, int lane) {
    const int incl = wave_scan(nb, lane);
    const int total = __shfl(incl, 63);
    if (nb) {
        const int pos = E.bitpos + incl - nb;
        const int w = (pos >> 5) - E.wb;
        const uint64_t v = (uint64_t)val << (pos & 31);
        atomicOr(&E.stage[w], (uint32_t)v);
        if (v >> 32) atomicOr(&E.stage[w + 1], (uint32_t)(v >> 32));
    }
    E.bitpos += total;
    wave_sync();
    const int full = (E.bitpos >> 5) - E.wb;
    if (full >= 64) flush(E, full, lane);
}

__device__ __forceinline__ uint32_t reverse_bits(uint32_t code, int len) { return __builtin_bitreverse32(code) >> (32 - len); }

// Code lengths (limited to 15) and canonical codes of the n used symbols, sorted by count in key / sym: one lane.
__device__ void build_code(WaveLds &L, int n) {
    uint32_t *A = L.key;
    // minimum-redundancy code lengths in place (Moffat & Katajainen 1995): internal node weights and parents, then depths
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        if (leaf >= n || A[root] < A[leaf]) {
            A[next] = A[root];
            A[root++] = (uint32_t)next;
        } else {
            A[next] = A[leaf++];
        }
        if (leaf >= n || (root < next && A[root] < A[leaf])) {
            A[next] += A[root];
            A[root++] = (uint32_t)next;
        } else {
            A[next] += A[leaf++];
        }
    }
    A[n - 2] = 0;
    for (int next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
    for (int l = 0; l < 16; ++l) L.bl[l] = 0;
    {   // depths of the leaves, counted per length; what lies deeper than 15 is counted at 15
        int avbl = 1, used = 0, dpth = 0;
        root = n - 2;
        while (avbl > 0) {
            while (root >= 0 && (int)A[root] == dpth) {
                ++used;
                --root;
            }
            while (avbl > used) {
                L.bl[min(dpth, 15)] += 1;
                --avbl;
            }
            avbl = 2 * used;
            ++dpth;
            used = 0;
        }
    }
    // the limit: while the Kraft sum (in units of 2^-15) exceeds 1, take one code from 15 and split the deepest code above it
    uint32_t total = 0;
    for (int l = 15; l >= 1; --l) total += L.bl[l] << (15 - l);
    while (total > (1u << 15)) {
        L.bl[15] -= 1;
        for (int l = 14; l >= 1; --l)
            if (L.bl[l]) {
                L.bl[l] -= 1;
                L.bl[l + 1] += 2;
                break;
            }
        --total;
    }
    // the least frequent symbols take the longest codes
    uint32_t bits = 0;
    int j = 0;
    for (int l = 15; l >= 1; --l)
        for (uint32_t c = 0; c < L.bl[l]; ++c, ++j) {
            const int s = L.sym[j];
            bits += L.tab[s] * (uint32_t)l;
            L.tab[s] = (uint32_t)l;
        }
    uint32_t code = 0;
    L.next[0] = 0;
    for (int l = 1; l < 16; ++l) {
        code = (code + (l > 1 ? L.bl[l - 1] : 0u)) << 1;
        L.next[l] = code;
    }
    int nlit = 257;
    for (int s = 0; s < NLITLEN; ++s) {
        const int l = (int)L.tab[s];
        if (!l) continue;
        L.tab[s] = reverse_bits(L.next[l]++, l) | ((uint32_t)l << 16);
        if (s >= nlit) nlit = s + 1;
    }
    L.info[0] = bits;
    L.info[1] = (uint32_t)nlit;
}

template <int ESZ>
__global__ __launch_bounds__(64) void deflate_segments_kernel(const DeflateParams P) {
    using T = typename std::conditional<ESZ == 2, uint16_t, uint8_t>::type;
    __shared__ WaveLds L;
    const int lane = threadIdx.x;
    const int64_t gs = blockIdx.x;
    const int64_t tile = gs / P.parts;
    const int b = (int)(gs - tile * P.parts);
    const int per_plane = P.g.nty * P.g.ntx;
    const int plane = (int)(tile / per_plane);
    const int ti = (int)(tile - (int64_t)plane * per_plane);
    const int tyi = ti / P.g.ntx, txi = ti - tyi * P.g.ntx;
    const int n = min(SEG, P.tile_bytes - b * SEG);      // bytes of this segment (a multiple of ESZ)
    const int nel = n / ESZ;
    const int e0 = b * (SEG / ESZ);
    const bool last = b == P.parts - 1;
    T *el = reinterpret_cast<T *>(L.src);
    const T *in = static_cast<const T *>(P.planes);
    // ---- gather + predictor into LDS, Adler sums ------------------------------------------------------------------
    uint32_t any = 0, a1 = 0, a2 = 0;
    for (int e = lane; e < nel; e += 64) {
        const int ce = e0 + e, row = ce / P.g.tw, col = ce - row * P.g.tw;
        const int y = tyi * P.g.th + row, x = txi * P.g.tw + col;
        uint32_t v = 0, left = 0;
        if (y < P.h) {
            const int64_t at = (int64_t)plane * P.plane_stride + (int64_t)y * P.pitch + x;
            if (x < P.w) v = in[at];
            if (P.predictor == 2 && col > 0 && x - 1 < P.w) left = in[at - 1];
        }
        any |= v;
        const uint32_t pv = (v - left) & (ESZ == 2 ? 0xFFFFu : 0xFFu);
        el[e] = (T)pv;
        if (ESZ == 2) {
            const uint32_t lo = pv & 0xFFu, hi = pv >> 8;
            a1 += lo + hi;
            a2 += (uint32_t)(n - 2 * e) * lo + (uint32_t)(n - 2 * e - 1) * hi;
        } else {
            a1 += pv;
            a2 += (uint32_t)(n - e) * pv;
        }
    }
    for (int i = lane; i < NSYM; i += 64) L.tab[i] = 0;
    for (int i = lane; i < STAGE; i += 64) L.stage[i] = 0;
    if (__builtin_amdgcn_ballot_w64(any != 0) && lane == 0) atomicOr(&P.o.tile_any[tile], 1u);
    {
        const uint32_t s1 = (uint32_t)wave_sum((int)(a1 % ADLER)) % ADLER, s2 = (uint32_t)wave_sum((int)(a2 % ADLER)) % ADLER;
        if (lane == 0) P.seg_adler[gs] = s1 | (s2 << 16);
    }
    wave_sync();
    // ---- which elements equal their left neighbour ------------------------------------------------------------------
    const int nr = (nel + 63) / 64;
    for (int r = 0; r < nr; ++r) {
        const int i = r * 64 + lane;
        const bool eq = i > 0 && i < nel && el[i] == el[i - 1];
        const uint64_t m = __builtin_amdgcn_ballot_w64(eq);
        if (lane == 0) L.eqw[r] = m;
    }
    wave_sync();
    // ---- pass 1: symbol counts --------------------------------------------------------------------------------------
    int extra = 0, nmatch = 0, carry = 0;
    for (int r = 0; r < nr; ++r) {
        const int base = r * 64, i = base + lane;
        const uint64_t m = L.eqw[r];
        if (i < nel) {
            int len = 0;
            const int kind = token_of<ESZ>(L.eqw, m, base, lane, carry, nel, len);
            if (kind == 1) {
                const uint32_t v = el[i];
                atomicAdd(&L.tab[v & 0xFFu], 1u);
                if (ESZ == 2) atomicAdd(&L.tab[v >> 8], 1u);
            } else if (kind == 2) {
                int symbol, eb, ev;
                length_code(len, symbol, eb, ev);
                atomicAdd(&L.tab[symbol], 1u);
                extra += eb;
                ++nmatch;
            }
        }
        if (~m) carry = base + 64 - __builtin_clzll(~m);
    }
    if (lane == 0) L.tab[256] = 1;      // end of block
    extra = wave_sum(extra);
    nmatch = wave_sum(nmatch);
    wave_sync();
    // ---- the code: sort the used symbols by (count, symbol), then lengths and codes on one lane ---------------------------
    int used = 0;
    for (int s = lane; s < NLITLEN; s += 64) {
        const uint32_t c = L.tab[s];
        if (!c) continue;
        int rank = 0;
        for (int t = 0; t < NLITLEN; ++t) {
            const uint32_t ct = L.tab[t];
            rank += (ct != 0 && (ct < c || (ct == c && t < s))) ? 1 : 0;
        }
        L.key[rank] = c;
        L.sym[rank] = (uint16_t)s;
        ++used;
    }
    used = wave_sum(used);
    wave_sync();
    if (lane == 0) build_code(L, used);
    wave_sync();
    constexpr int NDIST = ESZ;          // distance codes sent: the symbol of distance ESZ is ESZ - 1
    const int nlit = (int)L.info[1];
    const int total_bits = 17 + 57 + 4 * (nlit + NDIST) + (int)L.info[0] + extra + nmatch;
    const int dyn_bytes = last ? (total_bits + 7) / 8 : (total_bits + 3 + 7) / 8 + 4;
    uint8_t *slot = P.slots + gs * SLOT;
    if (dyn_bytes >= n + 5) {           // no gain: a stored block
        if (lane == 0) {
            slot[0] = last ? 1 : 0;
            slot[1] = (uint8_t)(n & 0xFF);
            slot[2] = (uint8_t)(n >> 8);
            slot[3] = (uint8_t)(~n & 0xFF);
            slot[4] = (uint8_t)((~n >> 8) & 0xFF);
            P.seg_size[gs] = (uint32_t)(n + 5);
        }
        const uint8_t *srcb = reinterpret_cast<const uint8_t *>(L.src);
        for (int k = lane; k < n; k += 64) slot[5 + k] = srcb[k];
        return;
    }
    // ---- pass 2: header, tokens, end of block -------------------------------------------------------------------------
    Emitter E{L.stage, reinterpret_cast<uint32_t *>(slot), 0, 0};
    {   // BFINAL, BTYPE 10, HLIT, HDIST, HCLEN = 15 (all 19 code-length-code lengths, in the order 16 17 18 0 8 7 ...: three
        // zeros, then 4 for each of the lengths 0..15 -- the canonical 4-bit code of length l is l itself)
        uint32_t val = 0;
        int nb = 0;
        if (lane == 0) {
            val = (last ? 1u : 0u) | (2u << 1) | ((uint32_t)(nlit - 257) << 3) | ((uint32_t)(NDIST - 1) << 8) | (15u << 13);
            nb = 17;
        } else if (lane < 20) {
            val = lane < 4 ? 0u : 4u;
            nb = 3;
        }
        emit(E, val, nb, lane);
    }
    for (int i0 = 0; i0 < nlit + NDIST; i0 += 64) {
        const int i = i0 + lane;
        uint32_t val = 0;
        int nb = 0;
        if (i < nlit + NDIST) {
            const uint32_t l = i < nlit ? L.tab[i] >> 16 : (i - nlit == NDIST - 1 ? 1u : 0u);
            val = reverse_bits(l, 4);
            nb = 4;
        }
        emit(E, val, nb, lane);
    }
    carry = 0;
    for (int r = 0; r < nr; ++r) {
        const int base = r * 64, i = base + lane;
        const uint64_t m = L.eqw[r];
        uint32_t val = 0;
        int nb = 0;
        if (i < nel) {
            int len = 0;
            const int kind = token_of<ESZ>(L.eqw, m, base, lane, carry, nel, len);
            if (kind == 1) {
                const uint32_t v = el[i];
                const uint32_t t0 = L.tab[v & 0xFFu];
                val = t0 & 0xFFFFu;
                nb = (int)(t0 >> 16);
                if (ESZ == 2) {
                    const uint32_t t1 = L.tab[v >> 8];
                    val |= (t1 & 0xFFFFu) << nb;
                    nb += (int)(t1 >> 16);
                }
            } else if (kind == 2) {
                int symbol, eb, ev;
                length_code(len, symbol, eb, ev);
                const uint32_t t = L.tab[symbol];
                nb = (int)(t >> 16);
                val = (t & 0xFFFFu) | ((uint32_t)ev << nb);
                nb += eb + 1;               // the one distance symbol: a single 0 bit
            }
        }
        emit(E, val, nb, lane);
        if (~m) carry = base + 64 - __builtin_clzll(~m);
    }
    {
        const uint32_t t = L.tab[256];
        emit(E, lane == 0 ? (t & 0xFFFFu) : 0u, lane == 0 ? (int)(t >> 16) + (last ? 0 : 3) : 0, lane);   // (+ BFINAL 0, BTYPE 00)
        E.bitpos = (E.bitpos + 7) & ~7;
        if (!last) emit(E, 0xFFFF0000u, lane == 0 ? 32 : 0, lane);      // LEN 0, NLEN 0xFFFF
    }
    const int words = (E.bitpos + 31) / 32 - E.wb;
    for (int k = lane; k < words; k += 64)
        if (E.wb + k < SLOT / 4) E.outw[E.wb + k] = E.stage[k];
    if (lane == 0) P.seg_size[gs] = (uint32_t)(E.bitpos >> 3);
}

__global__ __launch_bounds__(64) void tile_size_kernel(const DeflateParams P, uint64_t *sizes) {
    const int64_t tile = blockIdx.x;
    uint64_t s = 0;
    for (int b = threadIdx.x; b < P.parts; b += 64) s += P.seg_size[tile * P.parts + b];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (threadIdx.x == 0) sizes[tile] = P.o.tile_any[tile] ? 2u + s + 4u : 0u;
}

__global__ __launch_bounds__(256) void deflate_assemble_kernel(const DeflateParams P) {
    if (*P.o.status) return;
    const int64_t tile = blockIdx.x;
    const uint64_t at = P.o.offsets[tile], size = P.o.offsets[tile + 1] - at;
    if (size == 0) return;
    uint8_t *dst = P.o.out + at;
    __shared__ uint32_t start[2048];      // tile_bytes <= 2048 * SEG = 32 MiB
    const int tid = threadIdx.x;
    if (tid == 0) {
        uint32_t run = 2, a = 1, b = 0;   // Adler-32 of the concatenation, from the segments' sums
        for (int s = 0; s < P.parts; ++s) {
            start[s] = run;
            run += P.seg_size[tile * P.parts + s];
            const uint32_t ad = P.seg_adler[tile * P.parts + s];
            const uint32_t len = (uint32_t)min(SEG, P.tile_bytes - s * SEG);
            b = (uint32_t)((b + (uint64_t)len * a + (ad >> 16)) % ADLER);
            a = (a + (ad & 0xFFFFu)) % ADLER;
        }
        dst[0] = 0x78;                    // deflate, 32 KiB window
        dst[1] = 0x01;                    // no dictionary, fastest level; 0x7801 is a multiple of 31
        const uint32_t adler = (b << 16) | a;
        for (int j = 0; j < 4; ++j) dst[run + j] = (uint8_t)(adler >> (24 - 8 * j));
    }
    __syncthreads();
    for (int s = 0; s < P.parts; ++s) {
        const uint32_t cb = P.seg_size[tile * P.parts + s];
        uint8_t *o = dst + start[s];
        const uint8_t *src = P.slots + (tile * P.parts + s) * SLOT;
        for (uint32_t k = tid; k < cb; k += 256) o[k] = src[k];
    }
}

constexpr const char *FN = "sq_deflate_encode_planes";

int geometry(DeflateParams &P, int32_t h, int32_t w, int32_t n_planes, int32_t dtype, int32_t th, int32_t tw) {
    int rc = stream_grid(P.g, P.n_tiles, "sq_deflate", "tiles", false, h, w, n_planes, th, tw);
    if (rc == SQ_OK) rc = stream_byte_parts(P.g, "sq_deflate", "tiles", dtype, P.esz, P.tile_bytes, P.parts);
    P.n_planes = n_planes, P.h = h, P.w = w;
    P.n_units = P.n_tiles * P.parts;
    return rc;
}

void carve(DeflateParams &P, Scratch &sc) {
    P.slots = sc.take<uint8_t>(P.n_units * SLOT);
    P.seg_size = sc.take<uint32_t>(P.n_units);
    P.seg_adler = sc.take<uint32_t>(P.n_units);
    P.o.tile_any = sc.take<uint32_t>(P.n_tiles);
}

}  // namespace

extern "C" int64_t sq_deflate_chunk_count(int32_t n_planes, int32_t h, int32_t w, int32_t tile_h, int32_t tile_w) {
    DeflateParams P{};   // the count does not depend on the element size: refuse only what no dtype could encode
    const int rc = geometry(P, h, w, n_planes, SQ_U8, tile_h, tile_w);
    if (rc != SQ_OK) return rc;
    return P.n_tiles;
}

extern "C" int64_t sq_deflate_out_bound(int32_t n_planes, int32_t h, int32_t w, int32_t dtype, int32_t tile_h, int32_t tile_w) {
    DeflateParams P{};
    const int rc = geometry(P, h, w, n_planes, dtype, tile_h, tile_w);
    if (rc != SQ_OK) return rc;
    return P.n_tiles * (2 + 4 + 5 * (int64_t)P.parts + P.tile_bytes);      // every segment stored
}

extern "C" int64_t sq_deflate_scratch_bytes(int32_t n_planes, int32_t h, int32_t w, int32_t dtype, int32_t tile_h, int32_t tile_w) {
    DeflateParams P{};
    const int rc = geometry(P, h, w, n_planes, dtype, tile_h, tile_w);
    if (rc != SQ_OK) return rc;
    Scratch sc{0};
    carve(P, sc);
    return sc.bytes();
}

extern "C" int sq_deflate_encode_planes(const void *planes_dev, int64_t plane_stride, int64_t pitch, int32_t n_planes, int32_t h,
                                        int32_t w, int32_t dtype, int32_t tile_h, int32_t tile_w, int32_t predictor,
                                        void *scratch_dev, int64_t scratch_bytes, uint64_t *offsets_dev, void *out_dev,
                                        int64_t out_capacity, uint32_t *status_dev, void *stream_) {
    int rc = stream_null(FN, planes_dev, scratch_dev, offsets_dev, out_dev, status_dev);
    if (rc != SQ_OK) return rc;
    DeflateParams P{};
    rc = geometry(P, h, w, n_planes, dtype, tile_h, tile_w);
    if (rc != SQ_OK) return rc;
    if (predictor != 1 && predictor != 2) return fail(SQ_ERR_INVALID, "%s: predictor %d (1: none, 2: horizontal)", FN, predictor);
    Scratch sc{reinterpret_cast<uintptr_t>(scratch_dev)};
    carve(P, sc);
    rc = stream_args(FN, P.o, n_planes, h, w, plane_stride, pitch, scratch_dev, scratch_bytes, sc.bytes(), offsets_dev, out_dev, out_capacity, status_dev);
    if (rc != SQ_OK) return rc;
    if (reinterpret_cast<uintptr_t>(planes_dev) % P.esz) return fail(SQ_ERR_INVALID, "%s: planes not aligned to their element", FN);
    if (P.n_units > 2147483647) return fail(SQ_ERR_UNSUPPORTED, "%s: too many tiles", FN);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    rc = stream_begin(FN, P.o, P.n_tiles, s);
    if (rc != SQ_OK || P.n_tiles == 0) return rc;
    P.planes = planes_dev, P.plane_stride = plane_stride, P.pitch = pitch;
    P.predictor = predictor;
    if (P.esz == 2)
        hipLaunchKernelGGL(deflate_segments_kernel<2>, dim3((unsigned)P.n_units), dim3(64), 0, s, P);
    else
        hipLaunchKernelGGL(deflate_segments_kernel<1>, dim3((unsigned)P.n_units), dim3(64), 0, s, P);
    hipLaunchKernelGGL(tile_size_kernel, dim3((unsigned)P.n_tiles), dim3(64), 0, s, P, offsets_dev);
    stream_scan(P.o, P.n_tiles, s);
    hipLaunchKernelGGL(deflate_assemble_kernel, dim3((unsigned)P.n_tiles), dim3(256), 0, s, P);
    return stream_end(FN);
}

// The scaffold of the device encoders that leave densely packed streams (blosc.hip, deflate.hip, jpeg.hip; packed_stream.hip
// holds the host side and the scan).  Such an encoder cuts every plane into full, zero-padded TILES (Blosc: chunks) and every
// tile into PARTS that one wave codes on its own (a 16 KiB block or segment, a JPEG restart interval); a part is a UNIT of the
// launch.  Sizes per tile -> one exclusive scan -> offsets[0 .. n_tiles], and tile i is out[offsets[i] .. offsets[i + 1]), size 0
// for a tile of zeros.  A total beyond out_capacity sets *status and nothing is written.
//
// An encoder provides: a Params struct that embeds TileGrid and PackedOut among its own fields (in the order its kernels have
// always read them: the argument layout of a coding kernel is part of its speed), a geometry() made of stream_grid() + its own
// conditions + the parts per tile, a carve() that takes its scratch arrays from a Scratch (tile_any last) and so defines
// *_scratch_bytes, its kernels, and an entry point: stream_null / geometry / stream_args / stream_begin / kernels around
// stream_scan / stream_end, with its own checks between them where its header comment documents them.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace sq {

struct TileGrid {
    int32_t th, tw, nty, ntx;         // tile shape as given, tiles per plane
};

struct PackedOut {
    uint32_t *tile_any;               // [n_tiles]: the tile holds a non-zero element
    uint64_t *offsets;                // [n_tiles + 1]: sizes, then tile i lives at out[offsets[i] .. offsets[i + 1])
    uint8_t *out;
    int64_t out_capacity;
    uint32_t *status;                 // [0] != 0: out too small
};

// ---- host (packed_stream.hip).  `codec` is the prefix of the size queries' messages ("sq_blosc"), `fn` the entry point's name,
// `what` the plural the messages use for tiles ("chunks" / "tiles").
// plane and tile shape -> grid and number of tiles; refuses sizes below 1 and, with `by8`, tile sides no multiple of 8
int stream_grid(TileGrid &G, int64_t &n_tiles, const char *codec, const char *what, bool by8, int32_t h, int32_t w, int32_t n_planes,
                int32_t th, int32_t tw);
// the byte codecs: uint8 / uint16 elements, a tile of at most 32 MiB in parts of 16 KiB -> element size, tile bytes, parts
int stream_byte_parts(const TileGrid &G, const char *codec, const char *what, int32_t dtype, int32_t &esz, int32_t &tile_bytes,
                      int32_t &parts);
int stream_null(const char *fn, const void *planes, const void *scratch, const void *offsets, const void *out, const void *status);
// out_capacity, pitch / plane stride, scratch size (`need`: what carve() took) and alignment, in this order; fills O but tile_any
int stream_args(const char *fn, PackedOut &O, int32_t n_planes, int32_t h, int32_t w, int64_t plane_stride, int64_t pitch,
                const void *scratch, int64_t scratch_bytes, int64_t need, uint64_t *offsets, void *out, int64_t out_capacity,
                uint32_t *status);
// clears *status and tile_any; with no tile at all offsets[0] = 0 instead, and the caller is done
int stream_begin(const char *fn, const PackedOut &O, int64_t n_tiles, hipStream_t s);
// the sizes in offsets[0 .. n_tiles) -> offsets[0 .. n_tiles] in place; *status = 1 when the total exceeds out_capacity
void stream_scan(const PackedOut &O, int64_t n_tiles, hipStream_t s);
int stream_end(const char *fn);      // hipGetLastError() of the launches

inline int64_t up256(int64_t v) { return (v + 255) & ~int64_t(255); }

// The scratch buffer in 256-byte aligned arrays; with base 0 it only adds up what *_scratch_bytes returns.
struct Scratch {
    uintptr_t base;
    int64_t used = 0;
    template <class T>
    T *take(int64_t count) {
        T *p = reinterpret_cast<T *>(base + (uintptr_t)used);
        used += up256(count * (int64_t)sizeof(T));
        return p;
    }
    int64_t bytes() const { return used + 256; }
};

// ---- device: the wave helpers.  (The unit -> tile, part, plane, tile row, tile column arithmetic and the "any non-zero" ballot stay
// written out in the coding kernels: as shared functions they changed those kernels' instruction streams.)
static __device__ __forceinline__ void wave_sync() {   // LDS (and slot) writes of this wave are visible to its other lanes
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

static __device__ __forceinline__ int wave_sum(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

static __device__ __forceinline__ int wave_scan(int v, int lane) {      // inclusive
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    return v;
}

}  // namespace sq

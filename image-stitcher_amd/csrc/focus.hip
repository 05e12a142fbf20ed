// ---------------------------------------------------------------------------------------------
// best-focus (extended depth of field) projection over z (sq_fuse_project_focus; an extension: the reference has none)
// ---------------------------------------------------------------------------------------------
// Definition in include/squidstitch.h (and DESIGN.md 5.2b).  Two stages:
//  (1) focus_tiles_kernel, tile space: one workgroup per (tile, FOC_BW x FOC_BH block).  Per plane z of the call: the block
//      plus a halo of R + 1 pixels (coordinates clamped to the tile) into LDS; ML over the block plus a halo of R, each halo
//      position taking the ML of its clamped position; the separable box sum (columns by a running sum down 8 rows per lane,
//      rows directly); the running best (score, z level, plane index) of the thread's 8 outputs in registers.  After the last
//      plane the winners go to the caller's scratch: uint32 score + uint8 plane index per tile pixel.
//  (2) focus_canvas_kernel, canvas space: the overwrite plan's items like project_max_kernel (static walk or the per-XCD
//      queues, no seam owners); per voxel the owner pixel's winner, its raw value from the winning plane through that plane's
//      gains (flat_generic: what sq_fuse_planes stores, bit for bit) and its key; ACC merges by key maximum.
// Algorithmic traffic: Z x sizeof(T) B read per tile pixel + 5 B written / read per tile pixel of scratch + (sizeof(T) + 8) B
// written per canvas voxel (+ sizeof(T) + gain bytes read per covered voxel).
#include "fuse_device.h"

namespace {
constexpr int FOC_BW = 64, FOC_BH = 32;   // output block of a workgroup: 64 lanes x (4 waves x 8 rows)
static_assert(FOC_BH == 4 * 8 && FOC_BW == 64, "the F stage maps one column per lane and 8 rows per wave");
constexpr int FOC_LROWS = (FOC_BH + 2 * SQ_FOCUS_MAX_RADIUS + 2 + 3) / 4;    // raw-block rows a wave loads at most (16)
constexpr int FOC_LCOLS = (FOC_BW + 2 * SQ_FOCUS_MAX_RADIUS + 2 + 63) / 64;  // 64-lane column runs of a raw-block row (2)
constexpr int FOC_XU = 4;   // canvas stage: pixels a lane has in flight at once

struct FocusParams {
    const uint32_t *zlev;   // z level of each of the call's planes
    uint32_t *score;        // [n_tiles][tile_h][tile_w] best F of every tile pixel
    uint8_t *plane;         // [n_tiles][tile_h][tile_w] its plane index within the call
    uint64_t *key;          // the key plane, key_pitch elements between rows
    int32_t key_pitch;
    int32_t radius;
    int32_t bx, by;         // blocks across / down a tile
};

struct FocusLayout {
    int64_t score, plane, total;
};
FocusLayout focus_layout(int64_t n_tiles, int64_t tile_h, int64_t tile_w) {
    FocusLayout L;
    const int64_t px = n_tiles * tile_h * tile_w;
    L.score = 0;
    L.plane = (px * 4 + 127) & ~int64_t(127);
    L.total = L.plane + ((px + 127) & ~int64_t(127));
    return L;
}
// LDS words of one workgroup for radius R: the raw block (later the column sums, which are smaller) + the ML block
int64_t focus_lds_words(int R) {
    const int lw = FOC_BW + 2 * R + 2, lh = FOC_BH + 2 * R + 2, mw = FOC_BW + 2 * R, mh = FOC_BH + 2 * R;
    return (int64_t)lw * lh + (int64_t)mw * mh;
}

template <typename T>
__global__ __launch_bounds__(256) void focus_tiles_kernel(const FuseParams P, const FocusParams F) {
    extern __shared__ uint32_t s_focus[];
    const int R = F.radius;
    const int LW = FOC_BW + 2 * R + 2, LH = FOC_BH + 2 * R + 2, MW = FOC_BW + 2 * R, MH = FOC_BH + 2 * R;
    uint32_t *sI = s_focus;             // [LH][LW] raw pixels of the block + halo R + 1; then [FOC_BH][MW] column sums
    uint32_t *sM = s_focus + LW * LH;   // [MH][MW] ML of the block + halo R
    const int per_tile = F.bx * F.by;
    const int tile = (int)(blockIdx.x / (unsigned)per_tile);
    const int blk = (int)blockIdx.x - tile * per_tile;
    const int by = blk / F.bx;
    const int x0 = (blk - by * F.bx) * FOC_BW, y0 = by * FOC_BH;
    const int H = P.tile_h, W = P.tile_w;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int oy = wave * 8;   // this thread's outputs: block column `lane`, block rows oy .. oy + 7
    uint32_t best[8] = {}, bestz[8] = {}, bestp[8] = {};
    // the raw block of a plane into registers (clamped reads), issued one plane ahead: the loads of plane z + 1 are in flight
    // while plane z is reduced.  Lanes past the block's width load a valid pixel that is not kept.
    uint32_t px[FOC_LROWS][FOC_LCOLS] = {};
    auto load_raw = [&](int z) {
        const T *src = sgpr(tile_ptr<T>(P, z, tile));
#pragma unroll
        for (int k = 0; k < FOC_LROWS; ++k) {
            const int i = wave + 4 * k;
            if (i < LH) {
                const T *srow = src + (int64_t)min(max(y0 - R - 1 + i, 0), H - 1) * P.tile_pitch;
#pragma unroll
                for (int m = 0; m < FOC_LCOLS; ++m) px[k][m] = ldg_s<T>(srow + min(max(x0 - R - 1 + lane + 64 * m, 0), W - 1));
            }
        }
    };
    load_raw(0);
    // the ML walk: this thread's first position and the step of 256 positions, as (row, column) of the MH x MW region
    const int ml_i0 = (int)threadIdx.x / MW, ml_j0 = (int)threadIdx.x - ml_i0 * MW;
    const int ml_di = 256 / MW, ml_dj = 256 - ml_di * MW;
    const bool inner = y0 - R >= 0 && y0 + FOC_BH + R <= H && x0 - R >= 0 && x0 + FOC_BW + R <= W;
    for (int z = 0; z < P.n_planes; ++z) {
        const uint32_t zl = F.zlev[z];
        // raw pixels at logical (y0 - R - 1 + i, x0 - R - 1 + j), read at the clamped position
#pragma unroll
        for (int k = 0; k < FOC_LROWS; ++k) {
            const int i = wave + 4 * k;
#pragma unroll
            for (int m = 0; m < FOC_LCOLS; ++m)
                if (i < LH && lane + 64 * m < LW) sI[i * LW + lane + 64 * m] = px[k][m];
        }
        __syncthreads();
        if (z + 1 < P.n_planes) load_raw(z + 1);
        // ML at logical (y0 - R + i, x0 - R + j) = ML at the clamped position, which lies inside the raw block with its
        // neighbours (whose values are the clamped reads).  One flat walk over the MH x MW positions (every lane busy: the rows
        // are wider than 64); a block whose ML region lies inside the tile needs no clamp
        for (int e = threadIdx.x, i = ml_i0, j = ml_j0; e < MH * MW; e += 256) {
            const int cy = inner ? i + 1 : min(max(y0 - R + i, 0), H - 1) - (y0 - R - 1);
            const int cx = inner ? j + 1 : min(max(x0 - R + j, 0), W - 1) - (x0 - R - 1);
            const int c = cy * LW + cx;
            const int c2 = 2 * (int)sI[c];
            const int h = c2 - (int)sI[c - 1] - (int)sI[c + 1];
            const int v = c2 - (int)sI[c - LW] - (int)sI[c + LW];
            sM[e] = (uint32_t)(abs(h) + abs(v));
            i += ml_di;
            j += ml_dj;
            if (j >= MW) {
                j -= MW;
                ++i;
            }
        }
        __syncthreads();
        // column sums over 2R + 1 ML rows for the block's rows: a running sum down the wave's 8 rows
        for (int j = lane; j < MW; j += 64) {
            uint32_t s = 0;
            for (int d = 0; d <= 2 * R; ++d) s += sM[(oy + d) * MW + j];
            sI[oy * MW + j] = s;
#pragma unroll
            for (int k = 1; k < 8; ++k) {
                s += sM[(oy + k + 2 * R) * MW + j] - sM[(oy + k - 1) * MW + j];
                sI[(oy + k) * MW + j] = s;
            }
        }
        __syncthreads();
        // row sums over 2R + 1 column sums -> F; keep the larger key (higher score, on a tie the lower z level)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            uint32_t f = 0;
            for (int d = 0; d <= 2 * R; ++d) f += sI[(oy + k) * MW + lane + d];
            if (z == 0 || f > best[k] || (f == best[k] && zl < bestz[k])) {
                best[k] = f;
                bestz[k] = zl;
                bestp[k] = (uint32_t)z;
            }
        }
        __syncthreads();   // the next plane's raw pixels overwrite the column sums
    }
    const int x = x0 + lane;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int y = y0 + oy + k;
        if (x < W && y < H) {
            const int64_t at = ((int64_t)tile * H + y) * W + x;
            stg_s<uint32_t>(F.score + at, best[k]);
            stg_s<uint8_t>(F.plane + at, (uint8_t)bestp[k]);
        }
    }
}

template <typename T, typename G, bool ACC>
__device__ __forceinline__ void focus_item(const FuseParams &P, const FocusParams &F, const Item &it, const int wave, const int lane) {
    constexpr bool GAINS = !std::is_same<G, NoGain>::value;
    typedef typename std::conditional<GAINS, G, float>::type GT;
    const int rows = it.hw >> 16, n = it.hw & 0xFFFF;
    T *canvas = static_cast<T *>(P.canvas);
    if (!it.nref) {   // uncovered canvas: 0 and key 0 (accumulating: left alone)
        if (!ACC)
            for (int r = wave; r < rows; r += 4) {
                T *drow = canvas + (int64_t)(it.dst_y + r) * P.canvas_pitch + it.dst_x;
                uint64_t *krow = F.key + (int64_t)(it.dst_y + r) * F.key_pitch + it.dst_x;
                for (int x = lane; x < n; x += 64) {
                    stg_s<T>(drow + x, (T)0);
                    stg_s<uint64_t>(krow + x, (uint64_t)0);
                }
            }
        return;
    }
    const int64_t tbase = (int64_t)it.a * P.tile_h * P.tile_w;
    for (int r = wave; r < rows; r += 4) {
        T *drow = canvas + (int64_t)(it.dst_y + r) * P.canvas_pitch + it.dst_x;
        uint64_t *krow = F.key + (int64_t)(it.dst_y + r) * F.key_pitch + it.dst_x;
        const int64_t soff = (int64_t)(it.b + r) * P.tile_pitch + it.c;   // elements into the winning plane's tile
        const int64_t foff = (int64_t)(it.b + r) * P.tile_w + it.c;       // elements into a gain image / the winners
        // FOC_XU pixels per lane at a time, loads of all of them first (clamped to the row: every address is valid), then the
        // dependent loads, then the stores: the winners' loads do not wait behind the previous pixel's stores
        for (int x0 = lane; x0 < n; x0 += 64 * FOC_XU) {
            uint32_t sc[FOC_XU], zi[FOC_XU];
#pragma unroll
            for (int u = 0; u < FOC_XU; ++u) {
                const int xc = min(x0 + 64 * u, n - 1);
                sc[u] = ldg_s<uint32_t>(F.score + tbase + foff + xc);
                zi[u] = ldg_s<uint8_t>(F.plane + tbase + foff + xc);
            }
            uint64_t key[FOC_XU];
            T t[FOC_XU];
            GT g[FOC_XU];
            bool has_g[FOC_XU], put[FOC_XU];
#pragma unroll
            for (int u = 0; u < FOC_XU; ++u) {
                const int xc = min(x0 + 64 * u, n - 1);
                key[u] = ((uint64_t)sc[u] << 32) | (uint64_t)(0xFFFFFFFFu - ldg_s<uint32_t>(F.zlev + zi[u]));
                put[u] = x0 + 64 * u < n;
                if (ACC) put[u] = put[u] && key[u] > ldg_s<uint64_t>(krow + xc);
                t[u] = ldg_s<T>(tile_ptr<T>(P, (int)zi[u], it.a) + soff + xc);
                has_g[u] = false;
                g[u] = (GT)1;
                if constexpr (GAINS) {
                    const GT *fz = static_cast<const GT *>(P.flat_ptrs[zi[u]]);
                    has_g[u] = fz != nullptr;
                    if (has_g[u]) g[u] = ldg_s<GT>(fz + foff + xc);
                }
            }
#pragma unroll
            for (int u = 0; u < FOC_XU; ++u) {
                if (!put[u]) continue;
                T v = t[u];
                if constexpr (GAINS) {
                    if (has_g[u]) v = flat_generic<T, GT>(t[u], g[u]);
                }
                stg_s<T>(drow + x0 + 64 * u, v);
                stg_s<uint64_t>(krow + x0 + 64 * u, key[u]);
            }
        }
    }
}

template <typename T, typename G, bool ACC, bool DYN>
__global__ __launch_bounds__(256) void focus_canvas_kernel(const FuseParams P, const int64_t n_items, const int64_t n_work,
                                                           const FocusParams F) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    for_each_item<DYN>(P, n_items, n_work, [&](const Item &it) { focus_item<T, G, ACC>(P, F, it, wave, lane); });
}
}  // namespace

extern "C" int64_t sq_focus_scratch_bytes(int32_t n_tiles, int32_t tile_h, int32_t tile_w) {
    if (n_tiles < 0 || tile_h < 0 || tile_w < 0)
        return fail(SQ_ERR_INVALID, "sq_focus_scratch_bytes: n_tiles %d, tile %d x %d", n_tiles, tile_h, tile_w);
    return focus_layout(n_tiles, tile_h, tile_w).total;
}

extern "C" int sq_fuse_project_focus(const sq_fuse_args *a, const sq_focus_args *f, int32_t flags, void *stream_) {
    static const char *who = "sq_fuse_project_focus";
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    FuseParams P;
    int32_t fl = 0;
    if (const int rc = project_setup(who, a, flags, stream, P, &fl)) return rc;
    if (!f || !f->z_levels_dev || !f->key_dev) return fail(SQ_ERR_INVALID, "%s: NULL focus arguments / z levels / key plane", who);
    if (f->radius < 0 || f->radius > SQ_FOCUS_MAX_RADIUS)
        return fail(SQ_ERR_INVALID, "%s: focus radius %d outside 0..%d", who, f->radius, SQ_FOCUS_MAX_RADIUS);
    if (a->n_planes > SQ_FOCUS_MAX_PLANES)
        return fail(SQ_ERR_INVALID, "%s: %d planes, the scratch's uint8 plane index holds %d", who, a->n_planes, SQ_FOCUS_MAX_PLANES);
    if (f->key_pitch < a->canvas_w || reinterpret_cast<uintptr_t>(f->key_dev) % 8)
        return fail(SQ_ERR_INVALID, "%s: key plane pitch %d < width %d, or not 8-byte aligned", who, f->key_pitch, a->canvas_w);
    const FocusLayout FL = focus_layout(a->n_tiles, a->tile_h, a->tile_w);
    if (FL.total > 0 && (!f->scratch_dev || reinterpret_cast<uintptr_t>(f->scratch_dev) % 128))
        return fail(SQ_ERR_INVALID, "%s: focus scratch missing or not 128-byte aligned", who);
    if (f->scratch_bytes < FL.total)
        return fail(SQ_ERR_WORKSPACE, "%s: focus scratch %lld < %lld bytes", who, (long long)f->scratch_bytes, (long long)FL.total);
    FocusParams F{};
    F.zlev = f->z_levels_dev;
    F.score = reinterpret_cast<uint32_t *>(static_cast<char *>(f->scratch_dev) + FL.score);
    F.plane = reinterpret_cast<uint8_t *>(static_cast<char *>(f->scratch_dev) + FL.plane);
    F.key = static_cast<uint64_t *>(f->key_dev);
    F.key_pitch = f->key_pitch;
    F.radius = f->radius;
    F.bx = (a->tile_w + FOC_BW - 1) / FOC_BW;
    F.by = (a->tile_h + FOC_BH - 1) / FOC_BH;
    const int64_t tile_blocks = (int64_t)a->n_tiles * F.bx * F.by;
    if (tile_blocks >= (int64_t(1) << 31)) return fail(SQ_ERR_UNSUPPORTED, "%s: %lld tile blocks", who, (long long)tile_blocks);
    const bool acc = (fl & SQ_FOCUS_ACCUMULATE) != 0, u16 = a->tile_dtype == SQ_U16;
    const int flat = a->flat_ptrs_dev ? (a->flat_dtype == SQ_F64 ? 2 : 1) : 0;
    if (tile_blocks > 0) {
        const size_t lds = (size_t)focus_lds_words(F.radius) * 4;
        if (u16) hipLaunchKernelGGL(focus_tiles_kernel<uint16_t>, dim3((unsigned)tile_blocks), dim3(256), lds, stream, P, F);
        else hipLaunchKernelGGL(focus_tiles_kernel<uint8_t>, dim3((unsigned)tile_blocks), dim3(256), lds, stream, P, F);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(SQ_ERR_HIP, "%s: tile stage launch failed: %s", who, hipGetErrorString(e));
    }
    const int64_t n_items = a->plan->header().n_items;
    return dispatch_projection(u16, flat, acc, P.queue != nullptr, [&](auto t, auto g, auto acc_c, auto dyn_c) {
        return launch(who, focus_canvas_kernel<decltype(t), decltype(g), acc_c(), dyn_c()>, P, n_items, stream, a->grid_blocks, n_items, n_items, F);
    });
}

// ---------------------------------------------------------------------------------------------
// guide channel of the best-focus projection (sq_focus_depth_plane, sq_fuse_select_depth)
// ---------------------------------------------------------------------------------------------
// Definition in include/squidstitch.h.  depth_plane_kernel: key plane -> unsigned depth plane (z* + 1, 0 = uncovered), streaming.
// select_depth_kernel, canvas space: the overwrite plan's items like focus_canvas_kernel; per voxel the guide's depth, the plane
// of this call at that z level (a table in LDS) and that plane's owner pixel through that plane's gains.
// Algorithmic traffic of the select: 1..2 B (depth) read per voxel + sizeof(T) + gain bytes read per covered voxel whose depth is
// in the call, sizeof(T) B written per voxel.
namespace {
constexpr int DEPTH_PER = 8;      // keys of a lane: four 16-byte loads, one 8- or 16-byte store
constexpr int SEL_XU = 4;         // select: pixels a lane has in flight at once
constexpr int SEL_MAP = 1024;     // z levels (counted from the call's lowest) the direct LDS table holds; beyond: a search

template <typename D>
__device__ __forceinline__ uint32_t depth_of_key(uint32_t lo, uint32_t hi) {
    constexpr uint32_t TOP = sizeof(D) == 1 ? 0xFFu : 0xFFFFu;
    if ((lo | hi) == 0) return 0u;             // no plane covers the voxel
    const uint32_t z = 0xFFFFFFFFu - lo;
    return z >= TOP ? TOP : z + 1u;            // (a z level the dtype cannot hold saturates; the caller sizes the dtype)
}

template <typename D>
__global__ __launch_bounds__(256) void depth_plane_kernel(const uint64_t *key, int64_t key_pitch, int h, int w, D *depth,
                                                          int64_t depth_pitch) {
    const int x0 = (int)(blockIdx.x * 256 + threadIdx.x) * DEPTH_PER;
    if (x0 >= w) return;
    for (int y = blockIdx.y; y < h; y += gridDim.y) {
        const uint64_t *krow = key + (int64_t)y * key_pitch + x0;
        D *drow = depth + (int64_t)y * depth_pitch + x0;
        if (x0 + DEPTH_PER <= w) {
            u32x4 k[DEPTH_PER / 2];
#pragma unroll
            for (int i = 0; i < DEPTH_PER / 2; ++i) k[i] = ldg<U32x4U>(krow + 2 * i);
            uint32_t d[DEPTH_PER];
#pragma unroll
            for (int i = 0; i < DEPTH_PER / 2; ++i) {
                d[2 * i] = depth_of_key<D>(k[i][0], k[i][1]);
                d[2 * i + 1] = depth_of_key<D>(k[i][2], k[i][3]);
            }
            if constexpr (sizeof(D) == 1) {
                ((SQ_GLOBAL U32x2U *)drow)->v =
                    u32x2{d[0] | (d[1] << 8) | (d[2] << 16) | (d[3] << 24), d[4] | (d[5] << 8) | (d[6] << 16) | (d[7] << 24)};
            } else {
                ((SQ_GLOBAL U32x4U *)drow)->v = u32x4{d[0] | (d[1] << 16), d[2] | (d[3] << 16), d[4] | (d[5] << 16), d[6] | (d[7] << 16)};
            }
        } else {
            for (int i = 0; x0 + i < w; ++i) {
                const u32x2 k = ldg<U32x2U>(krow + i);
                stg_s<D>(drow + i, (D)depth_of_key<D>(k[0], k[1]));
            }
        }
    }
}

struct SelectParams {
    const void *depth;      // the guide's depth plane, depth_pitch elements between rows
    const uint32_t *zlev;   // z level of each of the call's planes
    int32_t depth_pitch;
    int32_t depth16;        // elements are uint16 (else uint8)
};

// the call's z levels for one workgroup: s_zlev[plane] and the direct table s_map[z - lowest z] = plane + 1 (0: not in the
// call; of two planes with one z level the first).  -> (lowest z, whether a level lies beyond the table)
__device__ __forceinline__ void select_table(const FuseParams &P, const SelectParams &S, uint32_t *s_zlev, uint16_t *s_map,
                                             uint32_t &zmin, bool &sparse) {
    const int nz = P.n_planes;
    for (int p = threadIdx.x; p < nz; p += 256) s_zlev[p] = ldg_s<uint32_t>(S.zlev + p);
    __syncthreads();
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (int p = 0; p < nz; ++p) {
        lo = min(lo, s_zlev[p]);
        hi = max(hi, s_zlev[p]);
    }
    for (int e = threadIdx.x; e < SEL_MAP; e += 256) {
        uint32_t m = 0;
        for (int p = nz - 1; p >= 0; --p)
            if (s_zlev[p] - lo == (uint32_t)e) m = (uint32_t)p + 1u;
        s_map[e] = (uint16_t)m;
    }
    __syncthreads();
    zmin = (uint32_t)sgpr((int)lo);
    sparse = sgpr((int)(hi - lo >= (uint32_t)SEL_MAP)) != 0;
}

// plane index within the call of depth value d (z + 1; 0 = uncovered), -1 when the call has no plane at that level
__device__ __forceinline__ int select_plane(uint32_t d, uint32_t zmin, bool sparse, int nz, const uint32_t *s_zlev,
                                            const uint16_t *s_map) {
    if (d == 0u) return -1;
    const uint32_t rel = d - 1u - zmin;
    if (rel < (uint32_t)SEL_MAP) return (int)s_map[rel] - 1;
    if (sparse)
        for (int p = 0; p < nz; ++p)
            if (s_zlev[p] == d - 1u) return p;
    return -1;
}

template <typename T, typename G, bool ACC>
__device__ __forceinline__ void select_item(const FuseParams &P, const SelectParams &S, const Item &it, const int wave, const int lane,
                                            const uint32_t zmin, const bool sparse, const uint32_t *s_zlev, const uint16_t *s_map) {
    constexpr bool GAINS = !std::is_same<G, NoGain>::value;
    typedef typename std::conditional<GAINS, G, float>::type GT;
    const int rows = it.hw >> 16, n = it.hw & 0xFFFF;
    const int nz = P.n_planes;
    T *canvas = static_cast<T *>(P.canvas);
    const bool d16 = S.depth16 != 0;
    auto depth_at = [&](const char *row, int x) -> uint32_t {
        return d16 ? (uint32_t)ldg_s<uint16_t>(row + 2 * x) : (uint32_t)ldg_s<uint8_t>(row + x);
    };
    if (!it.nref) {   // uncovered canvas: 0, like that plane of the stack (accumulating: only where the depth is this call's)
        for (int r = wave; r < rows; r += 4) {
            T *drow = canvas + (int64_t)(it.dst_y + r) * P.canvas_pitch + it.dst_x;
            if (!ACC) {
                row_zero<T>(drow, n, lane);
                continue;
            }
            const char *prow = static_cast<const char *>(S.depth) + ((int64_t)(it.dst_y + r) * S.depth_pitch + it.dst_x) * (d16 ? 2 : 1);
            for (int x = lane; x < n; x += 64)
                if (select_plane(depth_at(prow, x), zmin, sparse, nz, s_zlev, s_map) >= 0) stg_s<T>(drow + x, (T)0);
        }
        return;
    }
    for (int r = wave; r < rows; r += 4) {
        T *drow = canvas + (int64_t)(it.dst_y + r) * P.canvas_pitch + it.dst_x;
        const char *prow = static_cast<const char *>(S.depth) + ((int64_t)(it.dst_y + r) * S.depth_pitch + it.dst_x) * (d16 ? 2 : 1);
        const int64_t soff = (int64_t)(it.b + r) * P.tile_pitch + it.c;   // elements into the chosen plane's tile
        const int64_t foff = (int64_t)(it.b + r) * P.tile_w + it.c;       // elements into a gain image
        // SEL_XU pixels per lane at a time: the depths of all of them first (clamped to the row: every address is valid), then
        // the loads that depend on them, then the stores
        for (int x0 = lane; x0 < n; x0 += 64 * SEL_XU) {
            uint32_t d[SEL_XU];
#pragma unroll
            for (int u = 0; u < SEL_XU; ++u) d[u] = depth_at(prow, min(x0 + 64 * u, n - 1));
            int zi[SEL_XU];
            T t[SEL_XU];
            GT g[SEL_XU];
            bool has_g[SEL_XU];
#pragma unroll
            for (int u = 0; u < SEL_XU; ++u) {
                const int xc = min(x0 + 64 * u, n - 1);
                zi[u] = select_plane(d[u], zmin, sparse, nz, s_zlev, s_map);
                const int zp = max(zi[u], 0);      // (a voxel without a plane loads plane 0's pixel and does not use it)
                t[u] = ldg_s<T>(tile_ptr<T>(P, zp, it.a) + soff + xc);
                has_g[u] = false;
                g[u] = (GT)1;
                if constexpr (GAINS) {
                    const GT *fz = static_cast<const GT *>(P.flat_ptrs[zp]);
                    has_g[u] = fz != nullptr;
                    if (has_g[u]) g[u] = ldg_s<GT>(fz + foff + xc);
                }
            }
#pragma unroll
            for (int u = 0; u < SEL_XU; ++u) {
                if (x0 + 64 * u >= n) continue;
                if (zi[u] < 0) {
                    if (!ACC) stg_s<T>(drow + x0 + 64 * u, (T)0);
                    continue;
                }
                T v = t[u];
                if constexpr (GAINS) {
                    if (has_g[u]) v = flat_generic<T, GT>(t[u], g[u]);
                }
                stg_s<T>(drow + x0 + 64 * u, v);
            }
        }
    }
}

template <typename T, typename G, bool ACC, bool DYN>
__global__ __launch_bounds__(256) void select_depth_kernel(const FuseParams P, const int64_t n_items, const int64_t n_work,
                                                           const SelectParams S) {
    __shared__ uint32_t s_zlev[SQ_FOCUS_MAX_PLANES];
    __shared__ uint16_t s_map[SEL_MAP];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    uint32_t zmin;
    bool sparse;
    select_table(P, S, s_zlev, s_map, zmin, sparse);
    for_each_item<DYN>(P, n_items, n_work, [&](const Item &it) {
        select_item<T, G, ACC>(P, S, it, wave, lane, zmin, sparse, s_zlev, s_map);
    });
}
}  // namespace

extern "C" int sq_focus_depth_plane(const void *key_dev, int32_t key_pitch, int32_t h, int32_t w, void *depth_dev,
                                    int32_t depth_pitch, int32_t depth_dtype, void *stream_) {
    static const char *who = "sq_focus_depth_plane";
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (h < 0 || w < 0) return fail(SQ_ERR_INVALID, "%s: plane %d x %d", who, h, w);
    if (depth_dtype != SQ_U8 && depth_dtype != SQ_U16)
        return fail(SQ_ERR_INVALID, "%s: depth dtype %d (uint8/uint16 only)", who, depth_dtype);
    if (h == 0 || w == 0) return SQ_OK;
    if (!key_dev || !depth_dev) return fail(SQ_ERR_INVALID, "%s: NULL key / depth plane", who);
    if (key_pitch < w || depth_pitch < w) return fail(SQ_ERR_INVALID, "%s: pitch smaller than width", who);
    if (reinterpret_cast<uintptr_t>(key_dev) % 8 || reinterpret_cast<uintptr_t>(depth_dev) % (size_t)depth_dtype)
        return fail(SQ_ERR_INVALID, "%s: key plane not 8-byte aligned or depth plane not aligned to its element size", who);
    const dim3 grid((unsigned)((w + 256 * DEPTH_PER - 1) / (256 * DEPTH_PER)), (unsigned)std::min(h, 65535));
    if (depth_dtype == SQ_U8)
        hipLaunchKernelGGL(depth_plane_kernel<uint8_t>, grid, dim3(256), 0, stream, static_cast<const uint64_t *>(key_dev),
                           (int64_t)key_pitch, h, w, static_cast<uint8_t *>(depth_dev), (int64_t)depth_pitch);
    else
        hipLaunchKernelGGL(depth_plane_kernel<uint16_t>, grid, dim3(256), 0, stream, static_cast<const uint64_t *>(key_dev),
                           (int64_t)key_pitch, h, w, static_cast<uint16_t *>(depth_dev), (int64_t)depth_pitch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SQ_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
    return SQ_OK;
}

extern "C" int sq_fuse_select_depth(const sq_fuse_args *a, const void *depth_dev, int32_t depth_pitch, int32_t depth_dtype,
                                    const uint32_t *z_levels_dev, int32_t flags, void *stream_) {
    static const char *who = "sq_fuse_select_depth";
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    FuseParams P;
    int32_t fl = 0;
    if (const int rc = project_setup(who, a, flags, stream, P, &fl)) return rc;
    if (!depth_dev || !z_levels_dev) return fail(SQ_ERR_INVALID, "%s: NULL depth plane / z levels", who);
    if (depth_dtype != SQ_U8 && depth_dtype != SQ_U16)
        return fail(SQ_ERR_INVALID, "%s: depth dtype %d (uint8/uint16 only)", who, depth_dtype);
    if (a->n_planes > SQ_FOCUS_MAX_PLANES)
        return fail(SQ_ERR_INVALID, "%s: %d planes, a call selects among at most %d", who, a->n_planes, SQ_FOCUS_MAX_PLANES);
    if (depth_pitch < a->canvas_w || reinterpret_cast<uintptr_t>(depth_dev) % (size_t)depth_dtype)
        return fail(SQ_ERR_INVALID, "%s: depth plane pitch %d < width %d, or not aligned to its element size", who, depth_pitch,
                    a->canvas_w);
    SelectParams S{};
    S.depth = depth_dev;
    S.zlev = z_levels_dev;
    S.depth_pitch = depth_pitch;
    S.depth16 = depth_dtype == SQ_U16;
    const int64_t n_items = a->plan->header().n_items;
    const bool acc = (fl & SQ_SELECT_ACCUMULATE) != 0, u16 = a->tile_dtype == SQ_U16;
    const int flat = a->flat_ptrs_dev ? (a->flat_dtype == SQ_F64 ? 2 : 1) : 0;
    return dispatch_projection(u16, flat, acc, P.queue != nullptr, [&](auto t, auto g, auto acc_c, auto dyn_c) {
        return launch(who, select_depth_kernel<decltype(t), decltype(g), acc_c(), dyn_c()>, P, n_items, stream, a->grid_blocks, n_items, n_items, S);
    });
}

// ---------------------------------------------------------------------------------------------
// maximum-intensity projection over z (sq_fuse_project_max; an extension: the reference has none)
// ---------------------------------------------------------------------------------------------
// One OUTPUT plane from the Z planes of an overwrite plan: per voxel the value sq_fuse_planes would store in each plane (the same
// divide routines, so every bit is theirs), reduced by an unsigned maximum.  Algorithmic traffic: Z x sizeof(T) B read per covered
// voxel + sizeof(T) B written per canvas voxel (+ the gains, loaded ONCE per slot for all Z planes when they all name one image).
// Structure: the persistent grid of the overwrite kernels (static walk or the per-XCD queues of for_each_queued_item) over the
// plan's items; the z loop runs inside a slot, so one item is one output store stream and nothing is shared between
// workgroups.  Seam owners are not used: each item writes exactly its own pixels (the partition SQ_FUSE_NO_SEAM_OWNERS keeps).
// ACC: max(existing, projection) on the covered voxels, uncovered ones untouched.
#include "fuse_device.h"

namespace {
constexpr int PROJ_ZU = 4;   // planes whose pixel vectors a lane has in flight at once

// per-component unsigned maximum of two 32-bit words of packed pixels (v_pk_max_u16 for uint16)
template <typename T>
__device__ __forceinline__ uint32_t max_packed(uint32_t a, uint32_t b) {
    if constexpr (sizeof(T) == 2) {
        typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
        return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
    } else {
        typedef unsigned char u8x4 __attribute__((ext_vector_type(4)));
        return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u8x4, a), __builtin_bit_cast(u8x4, b)));
    }
}
// the fast divide's operand range (flat_classify_kernel): 2^FAST_MIN_EXP <= |g| < 2^FAST_END_EXP
template <typename GT>
__device__ __forceinline__ bool in_fast_range(GT g) {
    const GT a = g < 0 ? -g : g;
    return a >= (GT)__builtin_ldexp(1.0, FAST_MIN_EXP) && a < (GT)__builtin_ldexp(1.0, FAST_END_EXP);   // NaN fails both
}
// one 32-bit word of pixels through the generic divide, gains g[0 .. 4 / sizeof(T))
template <typename T, typename GT>
__device__ __forceinline__ uint32_t word_generic(uint32_t w, const GT *g) {
    constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    uint32_t out = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) out |= (uint32_t)flat_generic<T, GT>((T)(w >> (BITS * e)), g[e]) << (BITS * e);
    return out;
}
// the same word through the shortened divide of the plane groups (gains in the fast range, r = recip_of<0>(g))
template <typename T, typename GT>
__device__ __forceinline__ uint32_t word_fast(uint32_t w, const GT *g, const GT *r) {
    if constexpr (sizeof(T) == 2) return quot_pair<0, GT>(w, g[0], g[1], r[0], r[1]);
    else return quot_quad<0, GT>(w, g, r);
}

// SHARED: every plane names the gain image flat_ptrs[0] (not NULL).  Otherwise each plane's entry is looked up (NULL = identity)
// and divided by the generic sequence: exact, not fast.
template <typename T, typename G, bool SHARED, bool ACC>
__device__ __forceinline__ void project_item(const FuseParams &P, const Item &it, const int wave, const int lane) {
    constexpr bool GAINS = !std::is_same<G, NoGain>::value;
    typedef typename std::conditional<GAINS, G, float>::type GT;
    constexpr uint32_t GSZ = sizeof(GT), TSZ = sizeof(T);
    constexpr int VEC = 16 / (int)sizeof(T), LINE = 128 / (int)sizeof(T), PER = 4 / (int)sizeof(T);
    constexpr int SLOTS = BLOCK_COLS / VEC / 64 + 1;
    const int rows = it.hw >> 16, n = it.hw & 0xFFFF;
    const int nz = P.n_planes;
    T *canvas = static_cast<T *>(P.canvas);
    if (!it.nref) {   // uncovered canvas: zeros, like every plane of the stack (accumulating: left alone)
        if (!ACC)
            for (int r = wave; r < rows; r += 4) row_zero<T>(canvas + (int64_t)(it.dst_y + r) * P.canvas_pitch + it.dst_x, n, lane);
        return;
    }
    const GT *flat0 = nullptr;
    if constexpr (GAINS && SHARED) flat0 = sgpr(static_cast<const GT *>(P.flat_ptrs[0]));
    for (int r = wave; r < rows; r += 4) {
        char *drow = reinterpret_cast<char *>(canvas + (int64_t)(it.dst_y + r) * P.canvas_pitch + it.dst_x);
        const int64_t soff = (int64_t)(it.b + r) * P.tile_pitch + it.c;   // elements into every plane's tile
        const int64_t foff = (int64_t)(it.b + r) * P.tile_w + it.c;       // elements into a gain image
        // vector v covers row pixels [v * VEC - mis, +VEC): stores start on the canvas' 128-byte lines (row_setup)
        const int mis = (int)((reinterpret_cast<uintptr_t>(drow) / sizeof(T)) & (LINE - 1));
        const int v_first = (mis + VEC - 1) / VEC, v_end = (n + mis) / VEC;
#pragma unroll
        for (int k = 0; k < SLOTS; ++k) {
            if (64 * k >= v_end || v_end <= v_first) break;   // wave-uniform: no whole vector (left) in this row
            const int v = lane + 64 * k;
            const bool act = v >= v_first && v < v_end;
            // lanes without a vector of their own load the row's first / last whole vector; only their store is masked
            const uint32_t o = (uint32_t)min(max(v * VEC - mis, v_first * VEC - mis), (v_end - 1) * VEC - mis);
            u32x4 acc = {0u, 0u, 0u, 0u};
            if (ACC) acc = ldg<U32x4U>(drow + o * TSZ);
            GT g[VEC], rc[VEC];
            bool fast = true;
            if constexpr (GAINS && SHARED) {
                load_gains(reinterpret_cast<const char *>(flat0 + foff) + o * GSZ, g);
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    fast = fast && in_fast_range(g[c]);
                    rc[c] = recip_of<0>(g[c]);
                }
            }
            for (int z0 = 0; z0 < nz; z0 += PROJ_ZU) {
                u32x4 px[PROJ_ZU];
#pragma unroll
                for (int u = 0; u < PROJ_ZU; ++u)
                    if (z0 + u < nz) px[u] = ldg<U32x4U>(reinterpret_cast<const char *>(tile_ptr<T>(P, z0 + u, it.a) + soff) + o * TSZ);
#pragma unroll
                for (int u = 0; u < PROJ_ZU; ++u) {
                    if (z0 + u >= nz) break;
                    if constexpr (!GAINS) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[c] = max_packed<T>(acc[c], px[u][c]);
                    } else if constexpr (SHARED) {
                        if (fast) {
#pragma unroll
                            for (int c = 0; c < 4; ++c) acc[c] = max_packed<T>(acc[c], word_fast<T, GT>(px[u][c], &g[PER * c], &rc[PER * c]));
                        } else {
#pragma unroll
                            for (int c = 0; c < 4; ++c) acc[c] = max_packed<T>(acc[c], word_generic<T, GT>(px[u][c], &g[PER * c]));
                        }
                    } else {
                        const GT *fz = sgpr(static_cast<const GT *>(P.flat_ptrs[z0 + u]));
                        if (fz) {
                            GT gz[VEC];
                            load_gains(reinterpret_cast<const char *>(fz + foff) + o * GSZ, gz);
#pragma unroll
                            for (int c = 0; c < 4; ++c) acc[c] = max_packed<T>(acc[c], word_generic<T, GT>(px[u][c], &gz[PER * c]));
                        } else {
#pragma unroll
                            for (int c = 0; c < 4; ++c) acc[c] = max_packed<T>(acc[c], px[u][c]);
                        }
                    }
                }
            }
            if (act) stg_nt_at(drow, o * TSZ, acc);
        }
        // the row's edges (pixels before the first / after the last whole vector): lanes 0..VEC-1 the head, VEC..2VEC-1 the
        // tail, one pixel each, through the generic divide
        const int head_end = min(n, v_first * VEC - mis);
        const int tail_start = max(head_end, v_end * VEC - mis);
        int ep = -1;
        if (lane < VEC) {
            if (lane < head_end) ep = lane;
        } else if (lane < 2 * VEC) {
            if (tail_start + (lane - VEC) < n) ep = tail_start + (lane - VEC);
        }
        if (ep >= 0) {
            uint32_t m = ACC ? (uint32_t)ldg_s<T>(drow + ep * TSZ) : 0u;
            for (int z = 0; z < nz; ++z) {
                const T t = ldg_s<T>(tile_ptr<T>(P, z, it.a) + soff + ep);
                uint32_t q = t;
                if constexpr (GAINS) {
                    const GT *fz = SHARED ? flat0 : static_cast<const GT *>(P.flat_ptrs[z]);
                    if (fz) q = flat_generic<T, GT>(t, ldg_s<GT>(fz + foff + ep));
                }
                m = max(m, q);
            }
            stg_s<T>(drow + ep * TSZ, (T)m);
        }
    }
}

template <typename T, typename G, bool ACC, bool DYN>
__global__ __launch_bounds__(256) void project_max_kernel(const FuseParams P, const int64_t n_items, const int64_t n_work) {
    constexpr bool GAINS = !std::is_same<G, NoGain>::value;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    bool shared = false;   // every plane names one gain image: load it and take its reciprocals once for all planes
    if constexpr (GAINS) {
        const void *f0 = P.flat_ptrs[0];
        shared = f0 != nullptr;
        for (int z = 1; z < P.n_planes && shared; ++z) shared = P.flat_ptrs[z] == f0;
        shared = sgpr((int)shared) != 0;
    }
    for_each_item<DYN>(P, n_items, n_work, [&](const Item &it) {
        if (!GAINS || shared) project_item<T, G, true, ACC>(P, it, wave, lane);
        else project_item<T, G, false, ACC>(P, it, wave, lane);
    });
}
}  // namespace

extern "C" int sq_fuse_project_max(const sq_fuse_args *a, int32_t flags, void *stream_) {
    static const char *who = "sq_fuse_project_max";
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    FuseParams P;
    int32_t fl = 0;
    if (const int rc = project_setup(who, a, flags, stream, P, &fl)) return rc;
    const int64_t n_items = a->plan->header().n_items;
    const bool acc = (fl & SQ_PROJECT_ACCUMULATE) != 0, u16 = a->tile_dtype == SQ_U16;
    const int flat = a->flat_ptrs_dev ? (a->flat_dtype == SQ_F64 ? 2 : 1) : 0;
    return dispatch_projection(u16, flat, acc, P.queue != nullptr, [&](auto t, auto g, auto acc_c, auto dyn_c) {
        return launch(who, project_max_kernel<decltype(t), decltype(g), acc_c(), dyn_c()>, P, n_items, stream, a->grid_blocks, n_items, n_items);
    });
}

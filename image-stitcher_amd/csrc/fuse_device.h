// What the fusion kernel families share (fuse.hip: overwrite, feather, self-tests; project.hip: maximum projection; focus.hip:
// best-focus projection and depth select): the packed vector types and global-memory accessors, FuseParams, the flatfield divide
// routines, the row geometry, the work-queue walk, and on the host side the argument checks, the scratch layout, the persistent
// launch and the (dtype, gains, mode) -> kernel instantiation dispatch.  Internal to csrc/: everything is forced inline or in an
// anonymous namespace, so each translation unit compiles its own copy and the kernels keep their names.
#ifndef SQ_FUSE_DEVICE_H
#define SQ_FUSE_DEVICE_H
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <map>
#include <type_traits>

#include "common.h"
#include "device_util.h"

using namespace sq;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

struct __attribute__((packed)) U32x4U {  // 16 bytes at any alignment
    u32x4 v;
};
struct __attribute__((packed)) F32x4U {
    f32x4 v;
};
struct __attribute__((packed)) U32x2U {  // 8 bytes at any alignment
    u32x2 v;
};
struct __attribute__((packed)) F64x2U {
    f64x2 v;
};

// Explicit global-address-space accessors: pointers that come out of a table are generic to the
// compiler and would be lowered to flat_* instructions.
template <typename V>
__device__ __forceinline__ auto ldg(const void *p) {
    return ((const SQ_GLOBAL V *)p)->v;
}
template <typename S>
__device__ __forceinline__ S ldg_s(const void *p) {
    return *(const SQ_GLOBAL S *)p;
}
__device__ __forceinline__ void stg_nt(void *p, u32x4 v) {
    __builtin_nontemporal_store(v, (SQ_GLOBAL u32x4 *)p);
}
// 16-byte non-temporal store at scalar base + 32-bit lane offset (bytes): no 64-bit address pair in vector registers
// (nt measured best here too: 0.623 against 0.599 plain, 0.622 "sc1 nt", 0.602 "sc0 sc1"; profiles/r02_exp21_store_policy.log)
__device__ __forceinline__ void stg_nt_at(void *base, uint32_t byte_off, u32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, %2 nt" ::"v"(byte_off), "v"(v), "s"(base) : "memory");
}
template <typename S>
__device__ __forceinline__ void stg_s(void *p, S v) {
    *(SQ_GLOBAL S *)p = v;
}

struct FuseParams {
    const Span *spans;
    const Ref *refs;
    const Item *items;
    const Seam *seams;            // per item, who writes the canvas line a vertical seam falls in (overwrite plans), or NULL
    const void *const *tile_ptrs;
    const void *tile_base;
    int64_t tile_plane_stride, tile_stride;
    const void *const *flat_ptrs;
    void *canvas;
    int64_t canvas_plane_stride;
    int32_t n_tiles, tile_h, tile_w, tile_pitch;
    int32_t canvas_pitch;
    const uint32_t *flat_class;   // per plane: bit 0 clear = every gain is a normal float in the fast divide's range; bit 1 clear =
                                  // every gain is also moderate (2^-20 <= |g| < 2^20: what the grouped feather blend asks for)
    uint32_t *queue;              // 9 chunk counters (8 XCD lanes + the rest), one 128-byte line each; NULL = static stride
    int32_t lane_items;           // list positions [0, 8 * lane_items) of a plane are lane-interleaved
    int32_t n_planes;
    int32_t chunk;                // consecutive lane positions a workgroup takes per atomic, 1..QUEUE_CHUNK
    const struct PlaneGroup *groups;   // plane groups of the float32-gain kernel (build_groups_kernel), else NULL
    const uint32_t *n_groups;          // how many there are (device side: the host never learns it)
};
// Planes that are divided by the SAME gain image (the z planes of a channel) and whose canvas rows sit at the same
// phase inside a 128-byte line are carried through an item together: the gains and their reciprocals are loaded /
// computed once per group instead of once per plane.  32 bytes.
constexpr int ZB = 5;                // most planes in a group
static_assert(ZB >= 1 && ZB <= 7, "a PlaneGroup holds at most 7 planes");
struct PlaneGroup {
    int32_t n;          // 1..ZB
    int32_t plane[7];
};
static_assert(sizeof(PlaneGroup) == 32, "PlaneGroup layout");
constexpr int QUEUE_STRIDE = 32;   // uint32 words between the counters
constexpr int QUEUE_CHUNK = 8;     // most consecutive lane positions a workgroup takes per atomic

template <typename T>
__device__ __forceinline__ const T *tile_ptr(const FuseParams &P, int plane, int tile) {
    if (P.tile_ptrs) return static_cast<const T *>(P.tile_ptrs[(int64_t)plane * P.n_tiles + tile]);
    return static_cast<const T *>(P.tile_base) + plane * P.tile_plane_stride + tile * P.tile_stride;
}

// divide -> clip -> truncating cast of apply_flatfield_correction (stitcher.py:609-610), in the
// flatfield's own precision like numpy's uint16 / floatXX promotion.  NaN (0/0) -> 0, which is
// what the x86 cast of the reference produces; +inf -> dtype max through the clip.
// RND = 0: truncate (the reference's astype).  RND = 1: round half to even first -- feather mode's
// integer output (np.rint) for a voxel a single tile covers.
template <typename T, int RND = 0>
__device__ __forceinline__ T flat_f32(T v, float g) {
    float q = __fdiv_rn((float)v, g);
    if (RND) q = rintf(q);
    const float hi = sizeof(T) == 1 ? 255.0f : 65535.0f;
    q = fminf(fmaxf(q, 0.0f), hi);
    return (T)q;
}
// Fast exact flatfield divide for THIS operand class: numerator an integer in [0, 65535], gain a
// float32 with 2^-100 <= |g| < 2^100 (either sign).  Markstein's scheme -- the hardware reciprocal
// (v_rcp_f32, 1 ulp), one quotient, one exact-residual correction -- gives the correctly rounded
// quotient here: with r = (1/g)(1 + e), q = n r has relative error h <= |e| + 2^-24, the residual
// n - g q is exact in one FMA, and q + rem r = (n/g)(1 - h e), i.e. wrong by < 2^-44 relative
// before its single rounding, while a 16-bit numerator keeps n/g at least 2^-41 (relative) away
// from every rounding boundary.  A Newton step on r (two more FMAs) is therefore not needed; it was
// there in earlier versions.  Below 2^-112 the first quotient
// would overflow and the correction turn into inf - inf; the guard leaves a wide margin.  None of
// this is taken on faith: sq_selftest_flat_divide compares the final clipped integers with the
// IEEE path for ALL 2^23 mantissas x 65536 numerators in every binade of the range, on the GPU the
// tests run on (tests/test_fuse_gpu.py).  Zeros, denormals, tiny gains, infinities and NaNs among
// a plane's gains are found by a pre-pass (flat_classify_kernel) and send that plane through the
// generic IEEE sequence instead.
// 4 VALU slots + the reciprocal instead of the 11 of the IEEE sequence (two v_div_scale, v_div_fmas,
// v_div_fixup, two refinements).  Doing two pixels per instruction on the packed-float32 pipe
// (v_pk_mul_f32 / v_pk_fma_f32) was tried: it needs 86 VGPRs (5 waves) and measured no faster.
__device__ __forceinline__ float div_u16_normal(float n, float g) {
    const float r = __builtin_amdgcn_rcpf(g);
    const float q = n * r;
    const float rem = fmaf(-g, q, n);
    return fmaf(rem, r, q);
}
constexpr int FAST_MIN_EXP = -100;   // fast divide allowed for 2^FAST_MIN_EXP <= |g| < 2^FAST_END_EXP:
constexpr int FAST_END_EXP = 100;    // (every non-zero quotient n/g is then a normal float)
constexpr int BLEND_ACC_MIN_EXP = -44, BLEND_ACC_END_EXP = 53, BLEND_WSUM_MAX = 16384;   // what the grouped blend's last division sees
constexpr int MODERATE_EXP = 20;     // grouped feather blend: 2^-20 <= |g| < 2^20 keeps sums of weighted quotients far from the range ends

// float -> uint32 the way the hardware does it: negative and NaN -> 0, too large -> 0xFFFFFFFF.
// (C++'s (uint32_t)f is undefined outside the range, so say the instruction.)
__device__ __forceinline__ uint32_t cvt_u32_sat(float f) {
    uint32_t r;
    asm("v_cvt_u32_f32 %0, %1" : "=v"(r) : "v"(f));
    return r;
}

// RND = 1 (feather mode rounds the float32 quotient half to even): the reference's result then hangs
// on how n/g rounds to float32 right next to a representable k + 0.5, and n/g can be within 2^-48 of
// that float midpoint -- with the RAW hardware reciprocal the short sequence is not enough there (401 of
// the 2^39 operand pairs of a binade come out one ulp off, e.g. 4075 / 0x1.dbf3fep-3).  With ONE Newton
// step on the reciprocal it is: on gfx950 v_rcp_f32 + one step IS the correctly rounded reciprocal for
// every one of the 2^23 mantissas, and Markstein's theorem then makes quotient + one exact-residual
// correction the correctly rounded quotient (tools/div_probe.hip: 0 of 2^39 pairs differ in every binade
// tried, either sign; the second correction of rounds 1-3 -- the compiler's own IEEE sequence has it --
// changed nothing).  6 slots, not the compiler's 11; sq_selftest_flat_divide compares it with the
// compiler's division for every operand pair, on the GPU the tests run on.
__device__ __forceinline__ float div_u16_normal_ieee(float n, float g) {
    float r = __builtin_amdgcn_rcpf(g);
    r = fmaf(fmaf(-g, r, 1.0f), r, r);
    const float q = n * r;
    return fmaf(fmaf(-g, q, n), r, q);
}
template <int RND>
__device__ __forceinline__ float quotient_u16_normal(float n, float g) {
    if (!RND) return div_u16_normal(n, g);
    return __builtin_rintf(div_u16_normal_ieee(n, g));   // v_rndne_f32
}
template <typename T, int RND = 0>
__device__ __forceinline__ T flat_f32_fast(T v, float g) {
    // clip(q, 0, max) then truncate == saturating conversions: NaN never occurs on this path
    const uint32_t k = cvt_u32_sat(quotient_u16_normal<RND>((float)v, g));
    return (T)min(k, sizeof(T) == 1 ? 255u : 65535u);
}
// two pixels of one 32-bit word at once: v_cvt_pk_u16_u32 saturates to 65535 and packs
template <int RND = 0>
__device__ __forceinline__ uint32_t flat_f32_fast_pair(uint32_t word, float g_lo, float g_hi) {
    const uint32_t a = cvt_u32_sat(quotient_u16_normal<RND>((float)(word & 0xFFFFu), g_lo));
    const uint32_t b = cvt_u32_sat(quotient_u16_normal<RND>((float)(word >> 16), g_hi));
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const u16x2 p = __builtin_amdgcn_cvt_pk_u16(a, b);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 16);
}

// float64 gains: the compiler's IEEE sequence is v_div_scale x2, v_rcp_f64, two Newton steps, quotient,
// residual, v_div_fmas, v_div_fixup.  For a numerator in [0, 65535] and a gain with 2^-100 <= |g| < 2^100
// the scaling is the identity and the fix-up never fires, so the same arithmetic without those three
// instructions yields the same double, bit for bit (sq_selftest_flat_divide_f64 compares the doubles and
// the clipped integers for 2^15 random gains per binade x every numerator; tests/test_fuse_gpu.py).
// v_cvt_u32_f64 saturates like its float32 sibling: clip + truncate in one instruction.
__device__ __forceinline__ double div_u16_normal_f64(double n, double g) {
    double r = __builtin_amdgcn_rcp(g);
    r = fma(r, fma(-g, r, 1.0), r);
    r = fma(r, fma(-g, r, 1.0), r);
    const double q = n * r;
    return fma(fma(-g, q, n), r, q);
}
__device__ __forceinline__ uint32_t cvt_u32_sat(double f) {
    uint32_t r;
    asm("v_cvt_u32_f64 %0, %1" : "=v"(r) : "v"(f));
    return r;
}
template <typename T>
__device__ __forceinline__ T flat_f64_fast(T v, double g) {
    return (T)min(cvt_u32_sat(div_u16_normal_f64((double)v, g)), sizeof(T) == 1 ? 255u : 65535u);
}

template <typename T>
__device__ __forceinline__ T flat_f64(T v, double g) {
    double q = __ddiv_rn((double)v, g);
    const double hi = sizeof(T) == 1 ? 255.0 : 65535.0;
    q = fmin(fmax(q, 0.0), hi);
    return (T)q;
}

template <typename T>
struct Pix;  // 16 bytes of pixels
template <>
struct Pix<uint16_t> {
    static constexpr int N = 8;
    __device__ static uint16_t get(const u32x4 &v, int e) { return (uint16_t)(v[e >> 1] >> ((e & 1) * 16)); }
    __device__ static void set(u32x4 &v, int e, uint16_t x) {
        v[e >> 1] = (e & 1) ? ((v[e >> 1] & 0x0000FFFFu) | ((uint32_t)x << 16)) : ((v[e >> 1] & 0xFFFF0000u) | x);
    }
};
template <>
struct Pix<uint8_t> {
    static constexpr int N = 16;
    __device__ static uint8_t get(const u32x4 &v, int e) { return (uint8_t)(v[e >> 2] >> ((e & 3) * 8)); }
    __device__ static void set(u32x4 &v, int e, uint8_t x) {
        const int sh = (e & 3) * 8;
        v[e >> 2] = (v[e >> 2] & ~(0xFFu << sh)) | ((uint32_t)x << sh);
    }
};

// a row of an item as the overwrite kernels cut it (fuse.hip: the slot pipeline): edges one pixel per lane, whole 16-byte vectors between
constexpr int NO_EDGE = -(1 << 20);
template <typename T>
struct Row {
    T *drow;
    const T *srow;
    const char *frow;
    const T *lsrow;       // seam owner: the left neighbour's pixel that would land on drow[0] ...
    const char *lfrow;    // ... and its gain
    int mis, n;
    int v_first, v_end;   // whole vectors are v in [v_first, v_end)
    int edge_p;           // this lane's head pixel: before the first whole vector, or lane - mis over the seam's line
                          // (< 0: the left neighbour's); NO_EDGE: none
    int tail_p;           // this lane's pixel after the last whole vector (or -1)
    bool lzero;           // the left neighbour is zero fill
};

template <typename T>
__device__ __forceinline__ void row_setup(Row<T> &J, int lane, int seam_flags = 0) {
    constexpr int VEC = Pix<T>::N;
    // Vector v covers row pixels [v*VEC - mis, +VEC).  mis is the row's phase inside a 128-byte
    // line, not just inside 16 bytes: vector 0 then starts ON a line boundary, so every 1 KiB
    // wave-store covers 8 whole lines instead of straddling 9 (measured +10-15 % on canvases
    // whose pitch is not a multiple of 128 bytes, which is the normal case).
    constexpr int LINE = 128 / (int)sizeof(T);
    J.mis = (int)((reinterpret_cast<uintptr_t>(J.drow) / sizeof(T)) & (LINE - 1));
    const bool seams = sizeof(T) == 2 && J.n > 0;
    const bool head_line = seams && (seam_flags & SEAM_HAS_LEFT) && J.mis > 0;
    const int n_own = (seams && (seam_flags & SEAM_LEAVE_TAIL)) ? J.n - ((J.n + J.mis) & (LINE - 1)) : J.n;   // n >= LINE there
    J.v_first = head_line ? LINE / VEC : (J.mis + VEC - 1) / VEC;
    J.v_end = (n_own + J.mis) / VEC;
    const int head_end = head_line ? 0 : min(n_own, J.v_first * VEC - J.mis);   // pixels [0, head_end)
    const int tail_start = max(head_end, J.v_end * VEC - J.mis);               // pixels [tail_start, n_own)
    J.edge_p = head_line ? lane - J.mis : (lane < head_end ? lane : NO_EDGE);
    J.tail_p = (lane < VEC && tail_start + lane < n_own) ? tail_start + lane : -1;
    J.lzero = (seam_flags & SEAM_LEFT_ZERO) != 0;
}

template <typename T>
__device__ __forceinline__ void row_zero(T *drow, int n, int lane, bool leave_tail = false) {
    constexpr int VEC = Pix<T>::N;
    constexpr int SLOTS = BLOCK_COLS / VEC / 64 + 1;
    Row<T> J;
    J.drow = drow;
    J.n = n;
    // leave_tail: the line the row ends in is written by the right neighbour (Seam in common.h; n >= one line)
    row_setup<T>(J, lane, leave_tail ? SEAM_LEAVE_TAIL : 0);
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
        const int v = lane + 64 * k;
        // (plain instead of non-temporal stores for the zeros: 0.634 against 0.642 for the whole launch)
        if (v >= J.v_first && v < J.v_end) stg_nt(drow + (v * VEC - J.mis), u32x4{0, 0, 0, 0});
    }
    if (J.edge_p > NO_EDGE) stg_s<T>(drow + J.edge_p, 0);
    if (J.tail_p >= 0) stg_s<T>(drow + J.tail_p, 0);
}

// Work distribution.
//  * static (no scratch given): a persistent grid-stride walk, block b takes items b, b + G, ...
//  * dynamic: per plane the item list is 8 interleaved lanes (one per XCD: lane x holds the items of the
//    tile-row blocks == x mod 8, see plan.cpp) followed by a short rest.  Nine device counters hand out
//    chunks of QUEUE_CHUNK consecutive positions of a lane; a workgroup reads the XCD it really runs on
//    (HW_REG_XCC_ID), pulls from THAT lane, and moves on to the next lane / the rest once its own is
//    drained.  The items in flight on an XCD are then always one contiguous window of its lane -- same
//    flatfield rows, fetched into that XCD's L2 once, however unevenly workgroups progress (with the
//    static stride they drift apart over a 35 ms launch: PMC, 52 GB of gains re-fetched per launch)
//    -- and the launch ends with every workgroup busy.  One atomic and one barrier per chunk (the
//    first attempt paid both per item and lost 7 %); the atomic for the next chunk is issued before
//    the current chunk is processed and its result only looked at afterwards.
struct Chunk {
    int q;         // 0..7 lane, 8 rest, -1 none
    uint32_t c;    // chunk index inside the queue
};

// wave-uniform values the compiler cannot prove uniform (they come out of LDS): pin them to scalar registers
__device__ __forceinline__ int sgpr(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ Item sgpr(Item it) {
    it.dst_y = sgpr(it.dst_y);
    it.dst_x = sgpr(it.dst_x);
    it.hw = sgpr(it.hw);
    it.nref = sgpr(it.nref);
    it.a = sgpr(it.a);
    it.b = sgpr(it.b);
    it.c = sgpr(it.c);
    it.span = sgpr(it.span);
    return it;
}
template <typename T>
__device__ __forceinline__ const T *sgpr(const T *p) {
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = (uint32_t)sgpr((int)(uint32_t)v), hi = (uint32_t)sgpr((int)(uint32_t)(v >> 32));
    return reinterpret_cast<const T *>(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ Seam sgpr(Seam s) {
    s.a = sgpr(s.a);
    s.b = sgpr(s.b);
    s.c = sgpr(s.c);
    s.flags = sgpr(s.flags);
    return s;
}

// The queue walk shared by the fusion kernels: calls body(plane, item, aux) for every (plane, item) this
// workgroup is handed, all threads of the workgroup together, arguments in scalar registers.
// aux = pre(plane, item, list position) is evaluated by the thread that loads the descriptor (the overwrite kernel
// fetches the tile pointer there, so that eight of them are in flight at once).
template <typename Aux, typename Pre, typename Body>
__device__ __forceinline__ void for_each_queued_item(const FuseParams &P, const int64_t n_items, const uint32_t n_units, Pre pre,
                                                     Body body) {
    __shared__ int s_q[2];
    __shared__ uint32_t s_c[2];
    __shared__ Item s_item[QUEUE_CHUNK];          // the chunk's descriptors, loaded by QUEUE_CHUNK threads at once
    __shared__ int s_plane[QUEUE_CHUNK];
    __shared__ Aux s_aux[QUEUE_CHUNK];
    const int home = (int)(__builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u);   // HW_REG_XCC_ID[3:0]
    // queue q holds n_planes * per_plane(q) positions; 32-bit arithmetic (the host checks the sizes)
    auto per_plane_of = [&](int q) { return (uint32_t)(q < 8 ? (int64_t)P.lane_items : n_items - 8 * (int64_t)P.lane_items); };
    auto total_of = [&](int q) { return n_units * per_plane_of(q); };
    int given_up = 0;   // thread 0: queues found empty so far (own lane first, then the others, then the rest)
    auto queue_of = [&](int k) { return k < 8 ? ((home + k) & 7) : 8; };
    auto settle = [&](uint32_t c) -> Chunk {   // thread 0: make (given_up, c) a real chunk or move on
        while (true) {
            const int q = queue_of(given_up);
            if ((uint64_t)c * (uint32_t)P.chunk < total_of(q)) return {q, c};
            if (++given_up > 8) return {-1, 0u};
            c = atomicAdd(&P.queue[queue_of(given_up) * QUEUE_STRIDE], 1u);
        }
    };
    // lds_written() (device_util.h) after thread 0 has written the NEXT chunk's (queue, index) into LDS: the barrier at the top
    // of the loop is what publishes them, and it is reached round the back edge straight after the ds_write.
    if (threadIdx.x == 0) {
        const Chunk first = settle(atomicAdd(&P.queue[queue_of(0) * QUEUE_STRIDE], 1u));
        s_q[0] = first.q;
        s_c[0] = first.c;
        lds_written();
    }
    for (int iter = 0;; ++iter) {
        __syncthreads();
        const int q = sgpr(s_q[iter & 1]);
        if (q < 0) break;
        const uint32_t c = (uint32_t)sgpr((int)s_c[iter & 1]);
        uint32_t pending = 0;
        const bool pull = threadIdx.x == 0 && given_up <= 8;
        if (pull) pending = atomicAdd(&P.queue[queue_of(given_up) * QUEUE_STRIDE], 1u);   // next chunk; looked at after this one
        const uint32_t u0 = c * (uint32_t)P.chunk;
        const int count = (int)min((uint32_t)P.chunk, total_of(q) - u0);
        if ((int)threadIdx.x < count) {   // one descriptor per thread: queue position -> (plane, list position)
            const uint32_t per_plane = per_plane_of(q);
            const uint32_t u = u0 + threadIdx.x;
            // (unit-major: all items of unit 0, then unit 1 ...  The other way round -- position r of every unit, then r + 1,
            // so that the chip writes into ALL groups' planes at once -- was measured in round 3: 0.680 whatever the grouping,
            // between consecutive groups (0.647) and spread + dealt ones (0.692) on the same buffers;
            // profiles/r03_exp_unit_minor_*.log)
            const int plane = (int)(u / per_plane);
            const uint32_t r = u - (uint32_t)plane * per_plane;
            const int64_t pos = q < 8 ? (int64_t)r * 8 + q : 8 * (int64_t)P.lane_items + r;
            const Item it = P.items[pos];
            s_item[threadIdx.x] = it;
            s_plane[threadIdx.x] = plane;
            s_aux[threadIdx.x] = pre(plane, it, pos);
        }
        __syncthreads();
        for (int j = 0; j < count; ++j) body(sgpr(s_plane[j]), sgpr(s_item[j]), s_aux[j]);
        if (threadIdx.x == 0) {
            const Chunk nxt = pull ? settle(pending) : Chunk{-1, 0u};
            s_q[(iter + 1) & 1] = nxt.q;
            s_c[(iter + 1) & 1] = nxt.c;
            lds_written();
        }
    }
}

// The walk of the canvas-space projection kernels (project.hip, focus.hip): body(item) for every item this workgroup takes, all
// its threads together, the item in scalar registers -- by the persistent grid stride, or (DYN) through the queues above with
// one unit: an item carries all Z planes of the call, and nothing rides along with its descriptor.
template <bool DYN, typename Body>
__device__ __forceinline__ void for_each_item(const FuseParams &P, const int64_t n_items, const int64_t n_work, Body body) {
    if constexpr (!DYN) {
        for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) body(sgpr(P.items[w]));
    } else {
        for_each_queued_item<int>(
            P, n_items, 1u, [](int, const Item &, int64_t) -> int { return 0; }, [&](int, const Item &it, const int &) { body(it); });
    }
}

// RND = 0 (overwrite: truncate): Markstein with r = v_rcp_f32(g), the arithmetic of div_u16_normal.
// RND = 1 (feather, a voxel one tile covers: round half to even): the arithmetic of div_u16_normal_ieee with its Newton
// step on the reciprocal hoisted -- r arrives refined (recip_for), two exact-residual corrections here, v_rndne.
template <int RND>
__device__ __forceinline__ float recip_for(float g) {
    float r = __builtin_amdgcn_rcpf(g);
    if (RND) r = fmaf(fmaf(-g, r, 1.0f), r, r);
    return r;
}
template <int RND>
__device__ __forceinline__ float quot_one(float n, float g, float r) {
    float q = n * r;
    q = fmaf(fmaf(-g, q, n), r, q);      // r refined (RND = 1): the correctly rounded quotient (div_u16_normal_ieee)
    if (RND) q = __builtin_rintf(q);
    return q;
}
// float64 gains (overwrite mode): the arithmetic of div_u16_normal_f64 with its reciprocal -- v_rcp_f64 and two Newton
// steps, 5 of its 8 instructions -- hoisted out of the planes' loop
__device__ __forceinline__ double recip_f64(double g) {
    double r = __builtin_amdgcn_rcp(g);
    r = fma(r, fma(-g, r, 1.0), r);
    return fma(r, fma(-g, r, 1.0), r);
}
template <int RND>
__device__ __forceinline__ float recip_of(float g) { return recip_for<RND>(g); }
template <int RND>
__device__ __forceinline__ double recip_of(double g) { return recip_f64(g); }
template <int RND>
__device__ __forceinline__ float quot_of(float n, float g, float r) { return quot_one<RND>(n, g, r); }
template <int RND>
__device__ __forceinline__ double quot_of(double n, double g, double r) {
    const double q = n * r;
    return fma(fma(-g, q, n), r, q);
}
// Two float32 lanes per instruction (v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32: IEEE per component, so every bit is the scalar
// form's).  The overwrite quotient (RND = 0: 3 of its 5.8 instructions per pixel) measured no faster packed, twice (round 1 on the
// per-plane kernel, round 4 on the grouped structure in a mixed arena: tools/membw_gains "A2", 0.712 against 0.713) -- that path
// waits on memory.  The feather paths do 8.5 (one tile, rounded) to 27 (two-tile strips) instructions per pixel: there it pays.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
// div_u16_normal_ieee / div_by_refined on two lanes: n / d correctly rounded, r = the refined reciprocal of d
__device__ __forceinline__ f32x2 div_by_refined2(f32x2 n, f32x2 d, f32x2 r) {
    const f32x2 q = n * r;
    return pk_fma(pk_fma(-d, q, n), r, q);
}
template <int RND, typename G>
__device__ __forceinline__ uint32_t quot_pair(uint32_t word, G g_lo, G g_hi, G r_lo, G r_hi) {
    if constexpr (RND == 1 && std::is_same<G, float>::value) {
        const f32x2 n = {(float)(word & 0xFFFFu), (float)(word >> 16)};
        const f32x2 q = div_by_refined2(n, f32x2{g_lo, g_hi}, f32x2{r_lo, r_hi});
        typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
        const u16x2 p = __builtin_amdgcn_cvt_pk_u16(cvt_u32_sat(__builtin_rintf(q[0])), cvt_u32_sat(__builtin_rintf(q[1])));
        return (uint32_t)p[0] | ((uint32_t)p[1] << 16);
    }
    const G n0 = (G)(word & 0xFFFFu), n1 = (G)(word >> 16);
    const uint32_t a = cvt_u32_sat(quot_of<RND>(n0, g_lo, r_lo));
    const uint32_t b = cvt_u32_sat(quot_of<RND>(n1, g_hi, r_hi));
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const u16x2 p = __builtin_amdgcn_cvt_pk_u16(a, b);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 16);
}
// four uint8 pixels of one 32-bit word (uint8 planes in groups, round 4): the same quotient -- the exhaustive proof of the
// shortened divide covers every numerator below 65536 -- clipped to 255 and packed
template <int RND, typename G>
__device__ __forceinline__ uint32_t quot_quad(uint32_t word, const G *g, const G *r) {
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const G n = (G)((word >> (8 * k)) & 0xFFu);
        out |= min(cvt_u32_sat(quot_of<RND>(n, g[k], r[k])), 255u) << (8 * k);
    }
    return out;
}
// 8 consecutive gains at any alignment
__device__ __forceinline__ void load_gains(const char *p, float (&g)[8]) {
    const f32x4 a = ldg<F32x4U>(p), b = ldg<F32x4U>(p + 16);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        g[e] = a[e];
        g[4 + e] = b[e];
    }
}
__device__ __forceinline__ void load_gains(const char *p, double (&g)[8]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f64x2 a = ldg<F64x2U>(p + 16 * q);
        g[2 * q] = a[0];
        g[2 * q + 1] = a[1];
    }
}

// 16 consecutive gains (a uint8 plane's 16-byte pixel vector)
template <typename GT>
__device__ __forceinline__ void load_gains(const char *p, GT (&g)[16]) {
    GT lo[8], hi[8];
    load_gains(p, lo);
    load_gains(p + 8 * sizeof(GT), hi);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        g[e] = lo[e];
        g[8 + e] = hi[e];
    }
}

// G = NoGain: planes WITHOUT a flatfield carried through an item together -- nothing is shared between them but the
// geometry, yet five planes per thread write faster than one plane per launch when the planes lie in different stretches
// of device memory (DESIGN.md 5.1 point 9: the bare 5-plane copy 0.72-0.75 of peak against 0.64-0.65 plane by plane)
struct NoGain {};

// the generic (IEEE) flatfield divide of the per-plane kernel in the gain's precision: exact for every gain
template <typename T, typename GT>
__device__ __forceinline__ T flat_generic(T v, GT g) {
    if constexpr (sizeof(GT) == 8) return flat_f64<T>(v, g);
    else return flat_f32<T>(v, g);
}

// scratch: one uint32 gain class per plane | the nine chunk counters of the work queues, a 128-byte line each |
// the number of plane groups (a line) | the plane groups (32 bytes per plane at most)
struct ScratchLayout {
    int64_t queue, n_groups, groups, total;
};
ScratchLayout scratch_layout(int64_t n_planes) {
    ScratchLayout L;
    L.queue = (n_planes * 4 + 127) & ~int64_t(127);
    L.n_groups = L.queue + 9 * QUEUE_STRIDE * 4;
    L.groups = L.n_groups + 128;
    L.total = L.groups + n_planes * (int64_t)sizeof(PlaneGroup);
    return L;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// The checks and the FuseParams fields that sq_fuse_planes and the projections over z share.  fl: in, the flags given beside
// the arguments; out, those | a->flags, each of which has to be in flag_mask.  use_seams: the kernels honour the plan's seam
// owners (unless SQ_FUSE_NO_SEAM_OWNERS).  SQ_OK with P filled -- all but the canvas plane stride, the queue and the groups,
// which are the caller's -- or the failure.  The scratch is checked apart (scratch_check): what a caller asks in between decides
// which error a call with several faults reports.
int fuse_setup(const char *who, const sq_fuse_args *a, int32_t &fl, int32_t flag_mask, int32_t min_planes, bool use_seams,
               FuseParams &P) {
    if (!a || !a->plan || !a->table_dev || !a->canvas_dev) return fail(SQ_ERR_INVALID, "%s: NULL plan/table/canvas", who);
    const TableHeader &h = a->plan->header();
    if (a->plan->spans_only && !a->plan->expanded)
        return fail(SQ_ERR_INVALID, "%s: the plan of sq_fuse_plan_create_spans has not been through sq_fuse_plan_expand", who);
    if (a->table_bytes != a->plan->device_bytes())
        return fail(SQ_ERR_INVALID, "%s: table_bytes %lld != plan %lld", who, (long long)a->table_bytes,
                    (long long)a->plan->device_bytes());
    if (a->mode != h.mode) return fail(SQ_ERR_INVALID, "%s: mode %d but plan was built for %d", who, a->mode, h.mode);
    if (a->n_tiles != h.n_tiles || a->tile_h != h.tile_h || a->tile_w != h.tile_w || a->canvas_h != h.canvas_h ||
        a->canvas_w != h.canvas_w)
        return fail(SQ_ERR_INVALID, "%s: geometry differs from the plan (tiles %d/%d %dx%d/%dx%d canvas %dx%d/%dx%d)", who,
                    a->n_tiles, h.n_tiles, a->tile_h, a->tile_w, h.tile_h, h.tile_w, a->canvas_h, a->canvas_w, h.canvas_h,
                    h.canvas_w);
    if (!a->tile_ptrs_dev && !a->tile_base_dev && h.n_refs > 0)
        return fail(SQ_ERR_INVALID, "%s: no tile table and no tile base", who);
    if (a->tile_pitch < a->tile_w || a->canvas_pitch < a->canvas_w) return fail(SQ_ERR_INVALID, "%s: pitch smaller than width", who);
    if (a->n_planes < min_planes) return fail(SQ_ERR_INVALID, "%s: n_planes %d (at least %d)", who, a->n_planes, min_planes);
    fl |= a->flags;
    if ((fl & ~flag_mask) || a->grid_blocks < 0 || ((fl & SQ_FUSE_FORCE_QUEUES) && (fl & SQ_FUSE_FORCE_STATIC)))
        return fail(SQ_ERR_INVALID, "%s: flags %d / grid_blocks %d", who, fl, a->grid_blocks);
    if (a->tile_dtype != SQ_U8 && a->tile_dtype != SQ_U16)
        return fail(SQ_ERR_UNSUPPORTED, "%s: tile dtype %d (uint8/uint16 only)", who, a->tile_dtype);
    if (a->flat_ptrs_dev && a->flat_dtype != SQ_F32 && a->flat_dtype != SQ_F64)
        return fail(SQ_ERR_UNSUPPORTED, "%s: flatfield dtype %d (float32/float64 only)", who, a->flat_dtype);
    const size_t esz = a->canvas_dtype == SQ_F32 ? 4 : (size_t)a->canvas_dtype;
    if (reinterpret_cast<uintptr_t>(a->canvas_dev) % esz)
        return fail(SQ_ERR_INVALID, "%s: canvas pointer not aligned to its element size", who);

    P = FuseParams{};
    const char *base = static_cast<const char *>(a->table_dev);
    P.spans = reinterpret_cast<const Span *>(base + h.off_spans);
    P.refs = reinterpret_cast<const Ref *>(base + h.off_refs);
    P.items = reinterpret_cast<const Item *>(base + h.off_items);
    P.seams = (use_seams && h.off_seams && !(fl & SQ_FUSE_NO_SEAM_OWNERS)) ? reinterpret_cast<const Seam *>(base + h.off_seams) : nullptr;
    P.tile_ptrs = a->tile_ptrs_dev;
    P.tile_base = a->tile_base_dev;
    P.tile_plane_stride = a->tile_plane_stride;
    P.tile_stride = a->tile_stride;
    P.flat_ptrs = a->flat_ptrs_dev;
    P.canvas = a->canvas_dev;
    P.n_tiles = a->n_tiles;
    P.tile_h = a->tile_h;
    P.tile_w = a->tile_w;
    P.tile_pitch = a->tile_pitch;
    P.canvas_pitch = a->canvas_pitch;
    P.lane_items = (int32_t)h.lane_items;
    P.n_planes = a->n_planes;
    return SQ_OK;
}

// a->scratch_dev, where one is given: room for n_planes (scratch_layout) and on a 128-byte line
int scratch_check(const char *who, const sq_fuse_args *a, const ScratchLayout &SL) {
    if (a->scratch_bytes < SL.total)
        return fail(SQ_ERR_WORKSPACE, "%s: scratch %lld < %lld bytes", who, (long long)a->scratch_bytes, (long long)SL.total);
    if (reinterpret_cast<uintptr_t>(a->scratch_dev) % 128) return fail(SQ_ERR_INVALID, "%s: scratch not 128-byte aligned", who);
    return SQ_OK;
}

// The projections over z (one output plane from the Z planes of one overwrite plan): the shared checks plus what is theirs --
// overwrite plans only, the output keeps the tile dtype, no seam owners, one canvas plane, the queue rule.  SQ_OK with P (and
// P.queue when the work queues are taken) set up and *fl_out the effective flags, or the failure.
int project_setup(const char *who, const sq_fuse_args *a, int32_t flags, hipStream_t stream, FuseParams &P, int32_t *fl_out) {
    if (a && a->mode != SQ_FUSE_OVERWRITE)
        return fail(SQ_ERR_INVALID, "%s: mode %d, only SQ_FUSE_OVERWRITE plans can be projected", who, a->mode);
    // (ahead of the shared checks, and only for a tile dtype they accept: of a call's faults an unsupported tile dtype is reported
    //  first, then this one, then an unsupported flatfield dtype -- the error code depends on the order)
    if (a && (a->tile_dtype == SQ_U8 || a->tile_dtype == SQ_U16) && a->canvas_dtype != a->tile_dtype)
        return fail(SQ_ERR_INVALID, "%s: the output keeps the tile dtype (output %d, tile %d)", who, a->canvas_dtype, a->tile_dtype);
    int32_t fl = flags;
    if (const int rc = fuse_setup(who, a, fl, SQ_FUSE_FORCE_QUEUES | SQ_FUSE_FORCE_STATIC | SQ_FUSE_NO_PLANE_GROUPS | SQ_FUSE_NO_SEAM_OWNERS |
                                      SQ_FUSE_CONSECUTIVE_GROUPS | SQ_PROJECT_ACCUMULATE, 1, false, P))
        return rc;
    if (a->scratch_dev) {
        const ScratchLayout SL = scratch_layout(a->n_planes);
        if (const int rc = scratch_check(who, a, SL)) return rc;
        // the device queues: the size rule of sq_fuse_planes on planes x items, but the 32-bit counters count ITEMS here, not
        // (plane, item) pairs as they do there -- in a projection an item carries all Z planes
        const int64_t n_items = a->plan->header().n_items, n_work = (int64_t)a->n_planes * n_items;
        if ((n_work >= 100000 || (fl & SQ_FUSE_FORCE_QUEUES)) && n_items < (int64_t(1) << 31) && !(fl & SQ_FUSE_FORCE_STATIC)) {
            if (hipMemsetAsync(static_cast<char *>(a->scratch_dev) + SL.queue, 0, 9 * QUEUE_STRIDE * 4, stream) != hipSuccess)
                return fail(SQ_ERR_HIP, "%s: cannot clear the queue counters", who);
            P.queue = reinterpret_cast<uint32_t *>(static_cast<char *>(a->scratch_dev) + SL.queue);
        }
    } else if (fl & SQ_FUSE_FORCE_QUEUES) {
        return fail(SQ_ERR_INVALID, "%s: SQ_FUSE_FORCE_QUEUES needs scratch_dev", who);
    }
    *fl_out = fl;
    return SQ_OK;
}

// Persistent launch of kernel(P, args...): as many workgroups as the chip keeps resident (queried once per kernel), fewer when
// there are fewer than that many units of work, each walking the list with a grid stride or through the queues.  n_work is what
// the walk counts: (plane, item) pairs for the per-plane fusion kernels, items for a projection, and for the plane-group kernels
// -- whose number of (group, item) units is only known on the device -- the fewest units the planes can make.
template <typename K, typename... X>
int launch(const char *who, K kernel, const FuseParams &P, int64_t n_work, hipStream_t stream, int grid_override, X... args) {
    if (n_work == 0) return SQ_OK;
    static thread_local std::map<const void *, int> resident;
    const void *key = reinterpret_cast<const void *>(kernel);
    auto it = resident.find(key);
    if (it == resident.end()) {
        int dev = 0, cus = 256, per_cu = 8;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            cus = prop.multiProcessorCount;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu < 1) per_cu = 4;
        it = resident.emplace(key, cus * std::min(per_cu, 8)).first;
    }
    const int64_t blocks = std::min<int64_t>(n_work, grid_override > 0 ? grid_override : it->second);
    // work-queue chunk: QUEUE_CHUNK items per atomic when every workgroup gets many chunks, fewer for small
    // launches so that the last round does not leave workgroups idle
    FuseParams Q = P;
    Q.chunk = (int32_t)std::max<int64_t>(1, std::min<int64_t>(QUEUE_CHUNK, n_work / (blocks * 16)));
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, stream, Q, args...);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SQ_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
    return SQ_OK;
}

// The instantiation of a canvas-space projection kernel template <T, G, ACC, DYN> for a call: f(t, g, acc, dyn) with a value of
// the tile dtype and one of the gain type (NoGain without a flatfield) as type tags -- decltype(t) -- and accumulate / queue walk
// as std::bool_constants.
template <typename F>
int dispatch_projection(bool u16, int flat, bool acc, bool dyn, F f) {
    auto modes = [&](auto t, auto g) {
        if (acc) return dyn ? f(t, g, std::true_type{}, std::true_type{}) : f(t, g, std::true_type{}, std::false_type{});
        return dyn ? f(t, g, std::false_type{}, std::true_type{}) : f(t, g, std::false_type{}, std::false_type{});
    };
    auto gains = [&](auto t) {
        if (flat == 0) return modes(t, NoGain{});
        return flat == 1 ? modes(t, float{}) : modes(t, double{});
    };
    return u16 ? gains(uint16_t{}) : gains(uint8_t{});
}
}  // namespace
#endif  // SQ_FUSE_DEVICE_H

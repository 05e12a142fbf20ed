// The plane-batch convention of the per-tile filters (include/squidstitch.h, "Plane batches"), once: what a batch is, the checks
// every entry point makes of one, the strip / segment grid of the "a thread owns a vector and walks down rows" kernels, and the
// loops that cut a batch into launches.  Host code only; the kernels and their argument structs know nothing of it.  Only the
// launch loop at the end needs HIP; the rest compiles with any C++17 compiler (and was run under sanitizers that way).
#pragma once
#include <algorithm>
#include <initializer_list>

#include "common.h"

namespace sq {

// n planes of h x w elements of esize bytes: plane p's row y starts at element p * stride + y * pitch of base.
struct PlaneBatch {
    const void *base;
    int64_t n, h, w, stride, pitch;
    int esize;
    int64_t plane() const { return (h - 1) * pitch + w; }                   // elements from a plane's first to past its last
    uintptr_t first() const { return reinterpret_cast<uintptr_t>(base); }   // the extent in bytes: [first, end)
    uintptr_t end() const { return first() + (uintptr_t)(((n - 1) * stride + plane()) * esize); }
    char *at(int64_t p) const { return static_cast<char *>(const_cast<void *>(base)) + p * stride * esize; }
    // elements of the first row in front of a boundary of `vec` elements (a power of two)
    int32_t phase(int vec) const { return (int32_t)((first() / esize) & (uintptr_t)(vec - 1)); }
};

inline bool overlap(const PlaneBatch &a, const PlaneBatch &b) { return a.first() < b.end() && b.first() < a.end(); }

// plane(), or INT64_MAX where (h - 1) * pitch alone is beyond every limit below (the product may then not be formed)
inline int64_t plane_or_max(const PlaneBatch &b) { return b.h > 1 && b.pitch > (INT64_MAX / 4) / (b.h - 1) ? INT64_MAX : b.plane(); }

// Element alignment, then stride against plane, then "n planes fit a quarter of the address space" (so that no extent and no
// kernel offset wraps), each for all batches before the next.  Sizes, pitches and NULL have been checked; n >= 1.
inline int check_batches(const char *fn, const char *noun, std::initializer_list<PlaneBatch> batches) {
    for (const PlaneBatch &b : batches)
        if (b.first() % b.esize) return fail(SQ_ERR_INVALID, "%s: %ss must be aligned to their element", fn, noun);
    for (const PlaneBatch &b : batches)
        if (b.n > 1 && b.stride < plane_or_max(b)) return fail(SQ_ERR_INVALID, "%s: %s stride smaller than a %s", fn, noun, noun);
    for (const PlaneBatch &b : batches) {
        const int64_t limit = (INT64_MAX / 4) / b.n;
        if (b.stride > limit || plane_or_max(b) > limit) return fail(SQ_ERR_INVALID, "%s: extents beyond the address space", fn);
    }
    return SQ_OK;
}

// Workgroups of `threads` threads, tx (a power of two, at most tx_max) units across and threads / tx runs of `rows` rows tall, over
// a plane of `units` vectors (or runs) across and h rows: blockIdx.x = segment * n_strips + strip.
struct StripGrid {
    int32_t tx, tx_log2, n_strips;
    int64_t n_segs;
    unsigned x() const { return (unsigned)(n_strips * n_segs); }
};
inline int strip_grid(const char *fn, int64_t units, int tx_max, int threads, int rows, int64_t h, StripGrid *g) {
    g->tx = 1;
    g->tx_log2 = 0;
    while (g->tx < tx_max && g->tx < units) {
        g->tx *= 2;
        g->tx_log2 += 1;
    }
    const int64_t seg_rows = (int64_t)(threads / g->tx) * rows, n_strips = (units + g->tx - 1) / g->tx;
    g->n_segs = (h + seg_rows - 1) / seg_rows;
    if (n_strips * g->n_segs > INT32_MAX)
        return fail(SQ_ERR_UNSUPPORTED, "%s: a plane of %lld rows and %lld vectors needs more workgroups than a launch has", fn,
                    (long long)h, (long long)units);
    g->n_strips = (int32_t)n_strips;
    return SQ_OK;
}

// body(t, first, last) for every maximal run [first, last) of consecutive equal entries (t: the run's `width` values) of a host
// table; a body that returns non-zero ends the walk with that status.
template <typename F>
int for_each_run(const int32_t *table, int32_t n, int width, F &&body) {
    for (int32_t s0 = 0; s0 < n;) {
        const int32_t *t = table + width * (int64_t)s0;
        int32_t s1 = s0 + 1;
        while (s1 < n && std::equal(t, t + width, table + width * (int64_t)s1)) ++s1;
        if (const int rc = body(t, s0, s1)) return rc;
        s0 = s1;
    }
    return SQ_OK;
}

#ifdef __HIPCC__
// Planes [first, last) in launches of at most 65535 grid rows of `per_row` planes each (the planes a thread of the kernel walks
// over): body(p0, m, grid_y) launches planes [p0, p0 + m) with gridDim.y = grid_y.
template <typename F>
int for_each_launch(const char *fn, int64_t first, int64_t last, int per_row, F &&body) {
    const int64_t per_launch = (int64_t)65535 * per_row;
    for (int64_t p0 = first; p0 < last; p0 += per_launch) {
        const int32_t m = (int32_t)std::min<int64_t>(per_launch, last - p0);
        body(p0, m, (unsigned)((m + per_row - 1) / per_row));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(SQ_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    }
    return SQ_OK;
}
#endif

}   // namespace sq

/*
 * libsquidstitch -- C-ABI of the MI355X (gfx950) registration-and-fusion core.
 *
 * The reference (sohamazing/image-stitcher) has no FFI: its hot path is Python methods of
 * `Stitcher` (stitcher.py:31).  Each entry point below replaces the arithmetic inside one or
 * more of those methods; the integer geometry stays on the host, written exactly as the
 * reference writes it, and only rectangles / crop origins cross this boundary.
 *
 * Conventions
 *  - `extern "C"`, plain C types.  No torch types, no C++ types.
 *  - Every `*_dev` pointer is a DEVICE pointer owned by the caller (e.g. a PyTorch-ROCm
 *    tensor's data_ptr()).  The library never allocates, frees or keeps caller memory
 *    (the one exception is explicit: sq_arena_create hands out device memory the caller asked
 *    for and gives back with sq_arena_destroy).
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).  All device work
 *    is enqueued on it and is asynchronous; no entry point synchronises.
 *  - Return value: 0 = OK, negative = sq_status.  sq_last_error() gives the thread-local
 *    message of the last failure on the calling thread.
 *  - No global mutable state: handles are immutable after creation; safe to use from a
 *    QThread or a multiprocessing child as the reference's front-ends do.
 */
#ifndef SQUIDSTITCH_H
#define SQUIDSTITCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SQ_VERSION 108 /* 0.1.7: sq_write_files (chunk files by native threads); 0.1.6: sq_arena_* (canvas memory mapped over all memory classes of the card); 0.1.5: sq_selftest_normalise_divide; 0.1.4: sq_fuse_plan_create_spans / sq_fuse_plan_expand (work list of an overwrite plan produced on the device) */

typedef enum sq_status {
    SQ_OK = 0,
    SQ_ERR_INVALID = -1,     /* bad argument (NULL, negative size, unknown enum, misaligned) */
    SQ_ERR_HIP = -2,         /* a HIP runtime call or launch failed                          */
    SQ_ERR_UNSUPPORTED = -3, /* valid request this build cannot serve                        */
    SQ_ERR_WORKSPACE = -4,   /* caller workspace too small                                   */
    SQ_ERR_NUMERIC = -5      /* the computation ran but its result is unusable (sq_basic_fit) */
} sq_status;

typedef enum sq_dtype { SQ_U8 = 1, SQ_U16 = 2, SQ_F32 = 4, SQ_F64 = 8 } sq_dtype;

int sq_version(void);
const char *sq_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Fusion: replaces the per-file loop of Stitcher.stitch_region (stitcher.py:652-681) together
 * with place_tile / place_single_channel_tile (:544-605) and apply_flatfield_correction
 * (:607-611), for all (channel, z) planes of one (timepoint, region) in one launch.
 * ---------------------------------------------------------------------------------------- */

/* One tile's rectangle after the reference's crop (stitcher.py:577-587), BEFORE the canvas
 * clip of :590-594 (the library applies that clip).  Array order = the reference's write
 * order (sorted-filename order within a plane, stitcher.py:168,652): a later rect overwrites
 * an earlier one where they overlap. */
typedef struct sq_rect {
    int32_t src_y0, src_x0; /* first tile pixel used (top_crop, left_crop)              */
    int32_t h, w;           /* size of the cropped tile                                 */
    int32_t dst_y, dst_x;   /* canvas position of that first pixel (y_pixel, x_pixel)   */
} sq_rect;

typedef enum sq_fuse_mode {
    SQ_FUSE_OVERWRITE = 0, /* the reference: last writer wins, output dtype = tile dtype   */
    SQ_FUSE_FEATHER = 1    /* extension: distance-to-edge weighted mean of all covering tiles */
} sq_fuse_mode;

/* Opaque host-side plan: the canvas of one plane cut into disjoint spans, each with the
 * tile(s) that own it, plus the launch work-list.  Depends only on integer geometry, so one
 * plan serves every (c, z) plane of a region, every timepoint and every region that share
 * shifts (the reference computes shifts once per run, stitcher.py:1244-1246). */
typedef struct sq_fuse_plan sq_fuse_plan;

/* Build a plan.  Returns NULL on error (see sq_last_error).
 * tile_h/tile_w: full tile size (needed for feather weights and bounds checks). */
sq_fuse_plan *sq_fuse_plan_create(const sq_rect *rects, int32_t n_rects, int32_t tile_h, int32_t tile_w,
                                  int32_t canvas_h, int32_t canvas_w, int32_t mode);
void sq_fuse_plan_destroy(sq_fuse_plan *plan);
/* Size of the device table and a copy of it into caller host memory; the caller uploads it
 * (e.g. torch.from_numpy(...).cuda()) and passes the device copy to sq_fuse_planes. */
int64_t sq_fuse_plan_table_bytes(const sq_fuse_plan *plan);
int sq_fuse_plan_export(const sq_fuse_plan *plan, void *host_buf, int64_t host_bytes);

/* Copy the table to caller-owned device memory (table_bytes >= sq_fuse_plan_table_bytes) on `stream`
 * and wait for the copy: the plan may be destroyed right after.  The plan keeps its table in
 * page-locked host memory when a device is present, so this is one DMA at link speed; prefer it to
 * sq_fuse_plan_export + a copy of your own. */
int sq_fuse_plan_upload(const sq_fuse_plan *plan, void *table_dev, int64_t table_bytes, void *stream);
/* The same plan with its work list produced ON THE DEVICE (overwrite mode; tiles up to 8176 rows): the host stops after
 * the sweep into spans (1.2 of the 5 ms a 32 x 32 grid's plan takes) and uploads those -- ~100 KB instead of the 14.7 MB
 * table; sq_fuse_plan_expand cuts them into items, finds the seam owners and orders the list with five small kernels into the
 * caller's table buffer (>= sq_fuse_plan_table_bytes) using a scratch buffer (>= sq_fuse_plan_expand_scratch_bytes, free
 * again on return), and waits for them.  The table is sq_fuse_plan_create's byte for byte.  Such a plan has no host copy
 * of its items: sq_fuse_plan_export / _upload refuse it, and sq_fuse_planes refuses it until it has been expanded.
 * This is the first thing a job does after registration (reference: stitch_region's tile loop, stitcher.py:652-681,
 * starts from the shifts the same way). */
sq_fuse_plan *sq_fuse_plan_create_spans(const sq_rect *rects, int32_t n_rects, int32_t tile_h, int32_t tile_w,
                                        int32_t canvas_h, int32_t canvas_w, int32_t mode);
int64_t sq_fuse_plan_expand_scratch_bytes(const sq_fuse_plan *plan);
int sq_fuse_plan_expand(sq_fuse_plan *plan, void *table_dev, int64_t table_bytes, void *scratch_dev, int64_t scratch_bytes,
                        void *stream);
/* Introspection (tests, DESIGN.md numbers): n_spans, n_items, covered voxels, max tiles/span. */
int sq_fuse_plan_stats(const sq_fuse_plan *plan, int64_t *n_spans, int64_t *n_items, int64_t *covered_voxels,
                       int32_t *max_refs);

typedef struct sq_fuse_args {
    /* plan */
    const sq_fuse_plan *plan; /* host handle (sizes, launch geometry)                       */
    const void *table_dev;    /* device copy of sq_fuse_plan_export()                       */
    int64_t table_bytes;
    /* tiles: either a device array of n_planes*n_tiles device pointers (plane-major), or    */
    /* tile_base_dev + (plane*plane_stride + tile*tile_stride) elements when tile_ptrs_dev==0 */
    const void *const *tile_ptrs_dev;
    const void *tile_base_dev;
    int64_t tile_plane_stride, tile_stride; /* in elements                                   */
    int32_t n_tiles, tile_h, tile_w;
    int32_t tile_pitch;                     /* elements between tile rows (>= tile_w)        */
    int32_t tile_dtype;                     /* SQ_U8 | SQ_U16                                */
    /* flatfield (apply_flatfield_correction): device array of n_planes device pointers to   */
    /* tile_h x tile_w gains, NULL array or NULL entry = identity for that plane             */
    const void *const *flat_ptrs_dev;
    int32_t flat_dtype; /* SQ_F32 | SQ_F64: decides the division precision like numpy     */
    /* canvas */
    void *canvas_dev;            /* plane p at canvas_dev + p*canvas_plane_stride elements */
    int64_t canvas_plane_stride; /* elements                                               */
    int32_t canvas_h, canvas_w, canvas_pitch;
    int32_t canvas_dtype; /* overwrite: == tile_dtype; feather: tile_dtype or SQ_F32       */
    int32_t n_planes;
    int32_t mode; /* must match the plan                                               */
    /* optional scratch, sq_fuse_scratch_bytes(n_planes) bytes, 128-byte aligned: lets the call classify */
    /* each plane's float32 gains (all normal floats? -> shortened exact divide) and hand out work      */
    /* through per-XCD device queues; NULL = generic divide, static work split                          */
    void *scratch_dev;
    int64_t scratch_bytes;
    /* work distribution: 0 = the library chooses (device queues for big launches, a static walk for     */
    /* small ones); tests force either one.  grid_blocks > 0 caps the persistent grid (0 = resident WGs) */
    int32_t flags; /* sq_fuse_flags */
    int32_t grid_blocks;
} sq_fuse_args;

typedef enum sq_fuse_flags {
    SQ_FUSE_FORCE_QUEUES = 1, /* device work queues whatever the launch size (needs scratch_dev) */
    SQ_FUSE_FORCE_STATIC = 2, /* static grid-stride walk whatever the launch size                */
    SQ_FUSE_NO_PLANE_GROUPS = 4, /* uint16 / float32 gains: one plane at a time even where planes share a gain image */
    SQ_FUSE_NO_SEAM_OWNERS = 8,  /* plane groups: both items at a vertical seam write their part of the shared cache line */
    SQ_FUSE_CONSECUTIVE_GROUPS = 16 /* plane groups: the planes that share a gain image are taken ZB consecutive ones at a time
                                       (round 2's grouping) instead of being dealt round-robin to the key's groups -- for A/B runs:
                                       a group writes fastest when its planes lie far apart in device memory */
} sq_fuse_flags;

int64_t sq_fuse_scratch_bytes(int32_t n_planes);

/* Fuse n_planes planes.  Every canvas voxel is written exactly once (uncovered voxels = 0,
 * the reference starts from da.zeros, stitcher.py:362); no atomics; deterministic. */
int sq_fuse_planes(const sq_fuse_args *args, void *stream);

/* Maximum-intensity projection over z (extension: the reference has no projection).  ONE output plane from the n_planes = Z
 * planes the tile fields address: per voxel the unsigned maximum over the Z planes of exactly the value sq_fuse_planes would
 * store in each of them (same flatfield divide, same clip and truncating cast), so out == max over z of the fused stack, bit
 * for bit.  Uncovered voxels are 0.  The tiles are read once and only the projection is written: Z x elem bytes read per
 * covered voxel, elem bytes written per output voxel.  `args` keeps its meaning with these differences:
 *   - canvas_dev is the single output plane (canvas_h x canvas_w, canvas_pitch elements between rows, canvas_dtype ==
 *     tile_dtype); canvas_plane_stride is ignored;
 *   - flat_ptrs_dev has Z entries.  When all of them name one gain image (the z planes of a channel) its gains and their
 *     reciprocals are taken once per pixel for all Z planes; entries that differ, or NULL entries (identity), are exact too;
 *   - mode must be SQ_FUSE_OVERWRITE (and the plan an overwrite plan): anything else is SQ_ERR_INVALID;
 *   - scratch_dev (sq_fuse_scratch_bytes(n_planes) bytes, 128-byte aligned, optional) holds the work-queue counters.
 * flags (OR-ed with args->flags): the sq_fuse_flags work-distribution bits (FORCE_QUEUES / FORCE_STATIC; the other bits are
 * accepted and change nothing: there are no plane groups and no seam owners here) plus SQ_PROJECT_ACCUMULATE: the output
 * becomes max(output, projection) on the plan's covered voxels and its uncovered voxels are left untouched -- for the z planes
 * of a channel that come in several calls (ingest batches) or under different plans (ragged acquisitions).
 * Every output voxel is written by one workgroup; no atomics; deterministic.  n_planes >= 1. */
#define SQ_PROJECT_ACCUMULATE 32
int sq_fuse_project_max(const sq_fuse_args *args, int32_t flags, void *stream);

/* Best-focus (extended depth of field) projection over z (extension: the reference has none).  Per channel c and per staged
 * tile k of plane (c, z), all integer and exact:
 *   - I = the tile's RAW staged pixels (before flatfield; for an RGB file the monochrome component the stack pass stages).
 *     Reads outside the tile clamp to its edge.  Windows use the FULL staged tile, not the overwrite rect or the row band,
 *     so cropping, row bands and rank splits cannot change the result;
 *   - ML(y,x) = |2I(y,x) - I(y,x-1) - I(y,x+1)| + |2I(y,x) - I(y-1,x) - I(y+1,x)|  (modified Laplacian, Nayar & Nakagawa);
 *   - F(y,x) = sum over |dy| <= R, |dx| <= R of ML(clamp(y+dy), clamp(x+dx)); R = focus radius 0..15 (default 3).  F fits in
 *     uint32 for R <= 15 with 16-bit input (961 x 262140 < 2^28);
 *   - key of a tile pixel in plane z: (uint64(F) << 32) | (0xFFFFFFFF - z), z = the channel's z level (not the index within a
 *     batch).  The key is always > 0;
 *   - each canvas voxel v of each plane z has an owner tile and source pixel under that plane's overwrite plan; key_z(v) is
 *     that pixel's key, or 0 if plane z does not cover v.  The winning plane z*(v) is the z of max_z key_z(v): the highest
 *     score, on a tie the lowest z;
 *   - output v = exactly what sq_fuse_planes stores for plane z* at v (the same divide routines for none / float32 / float64
 *     gains).  Uncovered voxels are 0.  The depth of v is z*, recovered from the key plane (0xFFFFFFFF - low word).
 * `args` addresses the n_planes = Z planes of ONE plan as for sq_fuse_project_max (canvas_dev = the one output plane,
 * canvas_dtype == tile_dtype, overwrite plans only, scratch_dev = optional work-queue counters).  `focus`:
 *   - z_levels_dev: n_planes uint32 z levels of the call's planes, device memory;
 *   - radius: R, 0..15;
 *   - scratch_dev / scratch_bytes: sq_focus_scratch_bytes(n_tiles, tile_h, tile_w) bytes, 128-byte aligned, caller owned: the
 *     per-tile-pixel winner (uint32 score + uint8 plane index, 5 B per tile pixel) between the two stages of the call;
 *   - key_dev / key_pitch: the uint64 key plane [canvas_h, key_pitch elements], caller owned, written beside the output.
 * Two stages on `stream`: (1) per tile and 64 x 32 block, the block plus a halo of R + 1 of each plane into LDS, ML, the
 * separable box sum and the running best (score, plane) over the Z planes; (2) the plan's items (static walk or the per-XCD
 * work queues of the overwrite kernels): the winner's raw value from its staged plane through the gains, the output and key
 * planes written.  flags: the work-distribution bits as for sq_fuse_project_max, plus SQ_FOCUS_ACCUMULATE: a voxel is
 * rewritten (output and key) only where the new key is greater than the key plane holds; uncovered voxels are left untouched --
 * for the z planes of a channel that come in several calls (ingest batches, any z order) or under different plans (ragged
 * input).  Without it every voxel of both planes is written (uncovered: 0 and key 0).  The library allocates nothing on the
 * device.  SQ_ERR_INVALID for a feather plan, R outside 0..15, n_planes outside 1..256 (the uint8 plane index), a missing key
 * plane or scratch; SQ_ERR_WORKSPACE for scratch that is too small.  No atomics beyond the queue walk; deterministic. */
#define SQ_FOCUS_ACCUMULATE 32
#define SQ_FOCUS_MAX_RADIUS 15
#define SQ_FOCUS_MAX_PLANES 256
typedef struct sq_focus_args {
    const uint32_t *z_levels_dev;
    int32_t radius;
    void *scratch_dev;
    int64_t scratch_bytes;
    void *key_dev;
    int32_t key_pitch;
} sq_focus_args;
int64_t sq_focus_scratch_bytes(int32_t n_tiles, int32_t tile_h, int32_t tile_w);
int sq_fuse_project_focus(const sq_fuse_args *args, const sq_focus_args *focus, int32_t flags, void *stream);

/* Guide channel of the best-focus projection: decide the depth on ONE channel g, apply it to the others (all integer, exact).
 * Let depth_g(v) be the depth sq_fuse_project_focus reports for g at canvas voxel v (-1 where no plane of g covers v).  For
 * every channel c != g:
 *     out_c(v) = stack[c, depth_g(v)](v)   if depth_g(v) >= 0,   else 0
 * where stack[c, z] is exactly what sq_fuse_planes stores for plane (c, z): the same owner tile under that plane's own
 * overwrite plan, the same divide routine for none / float32 / float64 gains, 0 where plane (c, z) does not cover v (ragged
 * input) or does not exist.  In numpy: take_along_axis of the fused stack along z by the guide's depth, 0 where it is -1.
 * The guide's own output is sq_fuse_project_focus's, unchanged.
 *
 * The depth plane handed between the two stages (and written to disk by --focus-depth-map) is unsigned: z* + 1, 0 = uncovered;
 * SQ_U8 when every z level is < 255, else SQ_U16 (z < 65535).  A level the dtype cannot hold saturates to its maximum.
 *
 * sq_focus_depth_plane: key plane (uint64 [h, key_pitch elements], 8-byte aligned, as sq_fuse_project_focus writes it) ->
 * depth plane ([h, depth_pitch elements] of depth_dtype): 0xFFFFFFFF - low word + 1, key 0 -> 0.  One streaming kernel, 8 B
 * read and 1-2 B written per voxel.  SQ_ERR_INVALID for a NULL plane, a pitch below w, a dtype other than SQ_U8 / SQ_U16.
 *
 * sq_fuse_select_depth: `args` addresses the n_planes staged planes of ONE overwrite plan exactly as for sq_fuse_project_max
 * (canvas_dev = the one output plane of channel c, canvas_dtype == tile_dtype, scratch_dev = optional work-queue counters);
 * z_levels_dev: n_planes distinct uint32 z levels of these planes, device memory; depth_dev: the guide's depth plane
 * [canvas_h, depth_pitch elements].  The plan's items are walked on the persistent grid of the projections (static walk or the
 * per-XCD work queues, same size rule and flags).  Per voxel: the depth, the call's plane at that z level, and -- where the
 * item covers the voxel -- the owner pixel of that plane through that plane's gains, stored; 0 where the item does not cover
 * it.  flags: the work-distribution bits plus SQ_SELECT_ACCUMULATE: voxels whose depth is not among this call's z levels are
 * left untouched; without it they are written 0 (so every voxel is written).  That lets the z planes of a channel arrive in
 * several calls (ingest batches), in any z order, under different plans, the first call without the flag.  Reads 1-2 B of
 * depth per voxel + pixel and gain per selected voxel, writes the pixel: 1 + 2 + 4 B read, 2 B written with uint16 tiles,
 * float32 gains and a uint8 depth.  SQ_ERR_INVALID for a feather plan, n_planes outside 1..256, a NULL depth plane or z
 * levels, a depth dtype other than SQ_U8 / SQ_U16.  No atomics beyond the queue walk, no device allocation; deterministic. */
#define SQ_SELECT_ACCUMULATE 32
int sq_focus_depth_plane(const void *key_dev, int32_t key_pitch, int32_t h, int32_t w, void *depth_dev, int32_t depth_pitch,
                         int32_t depth_dtype, void *stream);
int sq_fuse_select_depth(const sq_fuse_args *args, const void *depth_dev, int32_t depth_pitch, int32_t depth_dtype,
                         const uint32_t *z_levels_dev, int32_t flags, void *stream);

/* ------------------------------------------------------------------------------------------
 * Canvas memory.  Replaces the allocation behind Stitcher.init_output (stitcher.py:356-362: the reference's canvas is a
 * lazy dask array; here it is device memory the fusion kernel writes once).  WHERE that memory lies decides how fast the
 * kernel can write it: MI355X device memory falls into a few classes of tens of GiB each (thirds of the card where it was scanned), a row-segment write
 * stream confined to one class runs at 0.55 of the HBM peak and at 0.73-0.76 when spread over the classes, and hipMalloc
 * hands out runs of tens of GiB of one class (csrc/arena.hip).  sq_arena_create takes `bytes` of device
 * memory in physical slices (hipMemCreate), measures which class every 512 MiB unit of them lies in (a pair-fill probe,
 * ~0.3 s for 100 GiB, on `stream`), and maps the slices into ONE contiguous virtual range round-robin over the classes:
 * any canvas laid out in [base_dev, base_dev + bytes) then has all classes under every ~200 MB of it, whatever its plane
 * stride and however the planes are grouped.  The caller sub-allocates (the arena is a flat range; canvases want their
 * planes on 128-byte lines, see sq_fuse_args) and destroys it when no kernel uses it any more.  Synchronises `stream`.
 * Tiles, gains and plans may live anywhere: reads do not depend on the class.
 *   candidate_bytes: the most memory the call may take while it looks for a balanced arena (0 = bytes: whatever comes).  Memory
 *       comes in runs of tens of GiB of one class, so candidates are taken chunk by chunk and classified until the three largest
 *       classes hold a third of `bytes` each (or, after 2.5 x bytes, the two largest half each); the rest is given back -- and
 *       is back -- before the call returns.  Pass what is free (less a reserve) and create the arena FIRST, while the card is
 *       still empty: typically 1.5-2.5 x bytes are taken; the driver clears every slice it hands out and takes back (0.5-6 s
 *       for 80 GiB).
 *   slice_bytes: 0 = 64 MiB (a multiple of 2 MiB);  unit_bytes: 0 = 512 MiB (a multiple of the slice, >= 16 MiB)
 *   flags: SQ_ARENA_NATURAL_ORDER = skip the probe and keep the slices in creation order (the control of A/B runs);
 *          SQ_ARENA_TWO_CLASSES = map slices of the two largest classes only (a measurement aid: two halves against three thirds)
 * Returns NULL on failure (sq_last_error; SQ_ERR_UNSUPPORTED in the message when the platform lacks virtual memory
 * management: allocate the canvas any other way then -- every entry point takes plain device pointers).
 * ---------------------------------------------------------------------------------------- */
#define SQ_ARENA_MAX_CLASSES 8
typedef enum sq_arena_flags { SQ_ARENA_NATURAL_ORDER = 1, SQ_ARENA_TWO_CLASSES = 2 } sq_arena_flags;
typedef struct sq_arena sq_arena;
typedef struct sq_arena_info {
    void *base_dev;       /* first byte of the arena (2 MiB aligned at least)                     */
    int64_t bytes;        /* size, rounded up to whole slices                                     */
    int64_t slice_bytes;
    int32_t n_slices;
    int32_t n_candidates; /* slices taken and classified (>= n_slices); the ones not chosen were given back */
    int32_t n_classes;    /* populations the probe told apart (3 on an MI355X when the arena spans them; 1 = nothing to interleave) */
    int32_t class_slices[SQ_ARENA_MAX_CLASSES];     /* slices of the arena per class     */
    int32_t class_candidates[SQ_ARENA_MAX_CLASSES]; /* slices taken per class            */
    int32_t interleaved;  /* 1: slices mapped round-robin over the classes; 0: creation order */
    float probe_ms;       /* device time of the classification                                   */
    float create_ms;      /* host time of the whole call                                         */
    float min_pair_gbs, max_pair_gbs; /* slowest / fastest pair fill seen by the probe, GB/s written */
} sq_arena_info;
sq_arena *sq_arena_create(int64_t bytes, int64_t candidate_bytes, int64_t slice_bytes, int64_t unit_bytes, int32_t flags,
                          void *stream, sq_arena_info *info);
int sq_arena_info_get(const sq_arena *arena, sq_arena_info *info);
int sq_arena_destroy(sq_arena *arena);

/* ------------------------------------------------------------------------------------------
 * Pyramid: one level of the OME-Zarr multiscale image from the level before.  Replaces
 * ome_zarr.scale.Scaler(max_layer=n-1).nearest(stitched_region) at stitcher.py:797-798 (level
 * count: stitcher.py:346-352), i.e. skimage.transform.resize(plane, (Y//2, X//2), order=0,
 * preserve_range=True, anti_aliasing=False) per plane and level:
 *     dst[p][y][x] = src[p][2*y + 1][2*x + 1],   dst is (src_h / 2) x (src_w / 2), floor.
 * Strides and pitches in elements; dtype SQ_U8 or SQ_U16; src and dst must not overlap.
 * ---------------------------------------------------------------------------------------- */
int sq_downsample2(const void *src_dev, int64_t src_plane_stride, int32_t src_h, int32_t src_w, int64_t src_pitch,
                   void *dst_dev, int64_t dst_plane_stride, int64_t dst_pitch, int32_t n_planes, int32_t dtype,
                   void *stream);

/* ------------------------------------------------------------------------------------------
 * Mean pyramid: levels 1 ... n_levels of the multiscale image from ONE read of the source level.
 * Restates generate_pyramid_levels -> downsample_block at zarr_stitcher.py:614-719 (and
 * generate_pyramid, stitcher_process.py:1583-1602), i.e. per plane and level
 * da.coarsen(np.mean, level, {y: 2, x: 2}, trim_excess=True) of the STORED level before, cast to
 * the integer dtype (the cast truncates):
 *     L(l+1)[p][y][x] = (L(l)[p][2y][2x] + L(l)[p][2y][2x+1] + L(l)[p][2y+1][2x] + L(l)[p][2y+1][2x+1]) >> 2,
 *     L(l+1) is (H_l / 2) x (W_l / 2), floor;  L(0) = src.
 * dst_dev[l], dst_plane_stride[l], dst_pitch[l] (HOST arrays of n_levels entries) describe level
 * l + 1, a (src_h >> (l+1)) x (src_w >> (l+1)) image per plane.  Levels that would be empty end
 * the pyramid: they and everything after them are not written and their entries are not read.
 * One launch yields up to SQ_PYRAMID_MEAN_MAX_LEVELS levels; a longer request is finished by
 * further launches from the last level written (the definition composes).  Strides and pitches in
 * elements; dtype SQ_U8 or SQ_U16; no buffer may overlap another.
 * ---------------------------------------------------------------------------------------- */
#define SQ_PYRAMID_MEAN_MAX_LEVELS 5
int sq_pyramid_mean(const void *src_dev, int64_t src_plane_stride, int32_t src_h, int32_t src_w, int64_t src_pitch,
                    void *const *dst_dev, const int64_t *dst_plane_stride, const int64_t *dst_pitch, int32_t n_levels,
                    int32_t n_planes, int32_t dtype, void *stream);

/* ------------------------------------------------------------------------------------------
 * Histogram: exact per-value counts of a batch of 2-D planes, ADDED into caller-owned 64-bit rows
 * (the caller zeroes them once):
 *     hist[row_of_plane[p]][v] += #{ (y, x) : planes[p][y][x] == v }      for p < n_planes.
 * The reference has no counterpart: the channel windows of its OME-Zarr stores are
 * np.iinfo(self.dtype).max (stitcher.py:846-850); these counts are what --contrast-limits
 * percentile derives the windows from.  dtype SQ_U16 (65536 bins per row) or SQ_U8 (256);
 * plane_stride and pitch in elements, any positive h and w, no alignment asked of the base or
 * the pitch beyond the element's own.  row_of_plane is a HOST array of n_planes entries,
 * 0 <= row < n_rows; hist_dev is [n_rows][bins] uint64 on the device.  A row out of range is
 * SQ_ERR_INVALID and nothing is launched.  Integer adds only: the result does not depend on
 * arrival order.  No scratch, no allocation.
 * ---------------------------------------------------------------------------------------- */
int sq_histogram_planes(const void *planes_dev, int64_t plane_stride, int32_t h, int32_t w, int64_t pitch,
                        int32_t n_planes, int32_t dtype, const int32_t *row_of_plane, int32_t n_rows,
                        uint64_t *hist_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * Composite (--composite: one colour quick-look picture per region).  Additions of 0.1.7; integers only, the definition
 * is the numpy restatement in tests/composite_ref.py ("Composite").
 *
 * sq_block_mean replaces the host-side stack copy and slicing of stitcher.py:861-885, _save_debug_slice: n_planes planes
 * [h, w] -> n_planes planes [ceil(h / f), ceil(w / f)] of the same dtype (SQ_U8 / SQ_U16), f = 2^k, k = 0 ... 8:
 *     dst[p][Y][X] = floor(sum of src[p] over rows Y f ... min(h, (Y + 1) f) - 1 and the same columns / number of those pixels)
 * (partial blocks at the bottom and right edge average the pixels that exist; k = 0 is the identity).  Strides and pitches in
 * elements; no alignment asked of a base or a pitch beyond the element's own.  Row band: only source rows
 * [row0, row0 + n_rows) are read and destination rows row0 / f ... written -- row0 a multiple of f, n_rows a multiple of f or
 * running to h (else SQ_ERR_INVALID); dst_dev is always the address of destination row 0.  One read of the source, no atomics,
 * no scratch, no allocation; deterministic.  n_planes <= 65535.
 * ---------------------------------------------------------------------------------------- */
int sq_block_mean(const void *planes_dev, int64_t plane_stride, int32_t h, int32_t w, int64_t pitch, int32_t n_planes,
                  int32_t dtype, int32_t k, int32_t row0, int32_t n_rows, void *dst_dev, int64_t dst_plane_stride,
                  int64_t dst_pitch, void *stream);

/* sq_composite_render replaces the min/max normalisation and RGB stacking of stitcher.py:861-885, _save_debug_slice:
 * n_planes <= 16 planes [h, w] (SQ_U8 / SQ_U16), a window (start, end) and a colour 0xRRGGBB each -> interleaved RGB8
 * rgb_dev[h][rgb_pitch bytes], 3 w bytes of every row written and nothing else:
 *     v_c = 0 where m <= start_c, 255 where m >= end_c, else floor((m - start_c) * 255 / (end_c - start_c))
 *     rgb[j] = min(255, sum over c of floor(v_c * colour_c[j] / 255))
 * windows (2 n_planes int32: start, end, 0 <= start < end <= 65535) and colors (n_planes uint32) are HOST arrays; they travel
 * in the kernel arguments.  h <= 65535. */
int sq_composite_render(const void *means_dev, int64_t plane_stride, int32_t h, int32_t w, int64_t pitch, int32_t n_planes,
                        int32_t dtype, const int32_t *windows, const uint32_t *colors, uint8_t *rgb_dev, int64_t rgb_pitch,
                        void *stream);

/* ------------------------------------------------------------------------------------------
 * Plane batches: the convention of the nine per-tile filters below (sq_tophat_tiles, sq_despeckle_tiles, sq_tile_stats,
 * sq_dpc_tiles, sq_bin_tiles, sq_warp_tiles, sq_shift_tiles, sq_affine_tiles, sq_dark_tiles; csrc/plane_batch.h is its one
 * implementation).  A batch is n planes of h x w elements of one dtype (SQ_U8 / SQ_U16) behind a base pointer: plane p's row y
 * starts at element p * plane_stride + y * pitch, both in elements, pitch >= w.  Every batch argument of a call has its own
 * base, plane stride and pitch; n, h, w and the dtype are the call's.  No alignment is asked of a base, a pitch or a stride
 * beyond the element's own; the columns between w and the pitch and whatever lies between two planes are neither read into a
 * result nor written.  With one plane the stride is never used for an address.  A batch's extent is the byte range from its
 * first element to its last, gaps included; "must not meet" and "overlap" speak of extents, so interleaved views count.
 * n == 0 is SQ_OK and nothing is launched (after the checks of the call's own parameters, sizes and pitches).  Otherwise
 * SQ_ERR_INVALID, and nothing is launched, for n < 0, h or w < 1, a pitch below the width, a NULL or element-misaligned base,
 * n > 1 with a plane stride smaller than a plane ((h - 1) * pitch + w), and a stride or plane above (INT64_MAX / 4) / n
 * elements ("extents beyond the address space": no offset the library forms can wrap).  A batch longer than a launch's 65535
 * grid rows (times the planes a thread of the kernel walks over) is split into several launches.
 * ---------------------------------------------------------------------------------------- */

/* ------------------------------------------------------------------------------------------
 * Background removal (--background-subtract tophat; extension: the reference has none -- its BaSiC runs with
 * get_darkfield=False, so nothing there removes an additive term).  A white top-hat with a square window of radius R per plane
 * I [h, w] (SQ_U8 / SQ_U16), IN PLACE:
 *     E(y, x) = min I over the (2R+1) x (2R+1) window centred on (y, x), clipped to the plane
 *     O(y, x) = max E over the same clipped window
 *     I      := I - O                       (O <= I, so nothing wraps)
 * The definition is the numpy restatement in tests/tophat_ref.py.  n_images planes plane_stride elements apart, rows pitch
 * elements apart (pitch >= w): a plane batch (above).  1 <= radius <= 127, any
 * h, w >= 1 (windows larger than the plane included).  The caller owns the scratch (16-byte aligned, at least
 * sq_tophat_scratch_bytes(n_images, h, w, dtype) bytes: the erosion of the batch); the library allocates nothing.  Two launches
 * (erosion into the scratch; dilation, subtraction and store), the work per pixel independent of R (running extrema, csrc/tophat.hip);
 * integers only, no atomics, deterministic.  SQ_ERR_INVALID for a radius out of range, a pitch below w, a NULL or misaligned
 * buffer, extents beyond the address space; SQ_ERR_WORKSPACE for scratch that is too small.
 * ---------------------------------------------------------------------------------------- */
#define SQ_TOPHAT_MAX_RADIUS 127
int64_t sq_tophat_scratch_bytes(int32_t n_images, int32_t h, int32_t w, int32_t dtype);
int sq_tophat_tiles(void *tiles_dev, int32_t n_images, int32_t h, int32_t w, int64_t plane_stride, int64_t pitch,
                    int32_t dtype, int32_t radius, void *scratch_dev, int64_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Hot-pixel removal (--despeckle; extension: the reference has none).  A thresholded 3 x 3 median per plane I [h, w]
 * (SQ_U8 / SQ_U16), OUT OF PLACE, with T = threshold in counts of the plane's own dtype:
 *     m(y, x) = the median (5th smallest) of the nine values I(clamp(y + dy, 0, h - 1), clamp(x + dx, 0, w - 1)), dy, dx in {-1, 0, 1}
 *     SQ_DESPECKLE_HOT :  out(y, x) = m(y, x) if I(y, x) - m(y, x) >  T   else I(y, x)
 *     SQ_DESPECKLE_BOTH:  out(y, x) = m(y, x) if |I(y, x) - m(y, x)| > T  else I(y, x)
 * The differences are taken in a wider signed type; every m comes from the unfiltered plane (the filter is not recursive); the
 * edges are replicated, so the window has nine values at every pixel, also for h = 1 or w = 1.  SQ_DESPECKLE_BOTH with T = 0 is
 * the plain 3 x 3 median.  The definition is the numpy restatement in tests/despeckle_ref.py.  n_images planes, the planes a
 * plane stride and the rows a pitch apart (elements, pitch >= w), src and dst each with their own; no alignment asked of a base
 * or a pitch beyond the element's own; any h, w >= 1.  src is read once and dst written once (csrc/despeckle.hip); the columns
 * between w and dst_pitch stay as they are.  counts_dev (optional, [n_images] uint64, 8-byte aligned): the number of pixels
 * replaced in plane i is ADDED to counts_dev[i] (strict >, so replaced <=> changed), by at most one integer atomic add per
 * workgroup.  Integers only, no scratch, no allocation; deterministic.  SQ_ERR_INVALID, and nothing is launched, for an unknown
 * mode or dtype, a threshold outside 0..65535, a pitch below w, a NULL or misaligned pointer, and src and dst extents (first to
 * last element of all planes) that overlap.
 * ---------------------------------------------------------------------------------------- */
#define SQ_DESPECKLE_HOT  1
#define SQ_DESPECKLE_BOTH 2
int sq_despeckle_tiles(const void *src_dev, void *dst_dev, int32_t n_images, int32_t h, int32_t w,
                       int64_t src_plane_stride, int64_t src_pitch, int64_t dst_plane_stride, int64_t dst_pitch,
                       int32_t dtype, int32_t mode, int32_t threshold, uint64_t *counts_dev /* [n_images], added to; may be NULL */,
                       void *stream);

/* ------------------------------------------------------------------------------------------
 * Per-tile quality words (--tile-qc; extension: the reference has none).  For each of n_images planes I [h, w] (SQ_U8 / SQ_U16),
 * the planes a plane stride and the rows a pitch apart (elements, pitch >= w): a plane batch (above).  SQ_TILE_STATS_WORDS = 8
 * uint64 are written to out_dev[n_images][8] (8-byte aligned).  The words are OVERWRITTEN, not added to:
 *     0  min I                4  number of pixels equal to the dtype's maximum (255 / 65535)
 *     1  max I                5  number of pixels equal to 0
 *     2  S = sum I            6  Bx = sum over y, x < w - 2 of (I(y, x + 2) - I(y, x))^2      (0 when w <= 2)
 *     3  Q = sum I^2          7  By = sum over y < h - 2, x of (I(y + 2, x) - I(y, x))^2      (0 when h <= 2)
 * Bx and By are the Brenner focus measure with step 2, one per direction.  The definition is the numpy restatement in
 * tests/tile_qc_ref.py.  Integers only: every pixel product fits 32 bits and is accumulated in 64; the result is bit for bit
 * numpy's int64 sums whatever the schedule (per-workgroup partial sums, then one integer atomic min / max / add per word per
 * workgroup, on words the call itself sets to their identities on `stream` first).  The planes are read once, plus two halo
 * rows per run of SQ_TILE_STATS_ROWS_PER_THREAD rows, and nothing else is stored (csrc/tilestats.hip); the columns between w
 * and the pitch and the rows between h and the plane stride are never read into a sum.  No scratch, no allocation.
 * SQ_ERR_UNSUPPORTED for h * w > 2^31 (or a side above 2^30), so that no word can wrap.  SQ_ERR_INVALID, and nothing is
 * launched, for a NULL or misaligned pointer, a pitch below w, a plane stride smaller than a plane, n_images < 0, h or w < 1 and
 * an unknown dtype.  n_images == 0 is SQ_OK.
 * ---------------------------------------------------------------------------------------- */
#define SQ_TILE_STATS_WORDS 8
#define SQ_TILE_STATS_ROWS_PER_THREAD 64
int sq_tile_stats(const void *src_dev, int32_t n_images, int32_t h, int32_t w, int64_t plane_stride, int64_t pitch,
                  int32_t dtype, uint64_t *out_dev /* [n_images][SQ_TILE_STATS_WORDS], overwritten */, void *stream);

/* ------------------------------------------------------------------------------------------
 * Differential phase contrast (--dpc; extension: the reference has none -- Squid's acquisition software computes it for its
 * live display, generate_dpc, in floats).  From the two half-pupil brightfield planes L and R [h, w] of one dtype (SQ_U8 /
 * SQ_U16, maximum M = 255 / 65535) and an integer gain g, exact in integers:
 *     S = L + R
 *     N = S + 2 g (L - R)
 *     out = 0                                 if S == 0
 *         = clamp(floor(M N / (2 S)), 0, M)   otherwise          (floor of the exact rational)
 * For g = 1 that is M (0.5 + (L - R) / (L + R)), truncated and clipped.  The definition is the numpy restatement in
 * tests/dpc_ref.py, and the result is bit for bit that on every input.  n_images planes, the planes a plane stride and the rows
 * a pitch apart (elements, pitch >= w), left, right and out each with their own: plane batches (above);
 * any h, w >= 1.  out may be EXACTLY left (same base, plane
 * stride and pitch: in place); otherwise its extent (first to last element of all planes) must meet neither input's.  left and
 * right are read once and out is written once (csrc/dpc.hip); the columns between w and out_pitch and the rows between h and
 * the plane stride are never written, and nothing past w or h is read into a result.  No scratch, no allocation, no atomics;
 * asynchronous on `stream`; deterministic.  SQ_ERR_INVALID, and nothing is launched, for an unknown dtype, a gain outside
 * 1..SQ_DPC_MAX_GAIN, a pitch below w, a plane stride smaller than a plane, a NULL or element-misaligned pointer, n_images < 0,
 * h or w < 1, extents beyond the address space, and an out that overlaps right, or left without being exactly left.
 * SQ_ERR_UNSUPPORTED for a plane that needs more workgroups than a launch has.  n_images == 0 is SQ_OK.
 * ---------------------------------------------------------------------------------------- */
#define SQ_DPC_MAX_GAIN 16
int sq_dpc_tiles(const void *left_dev, const void *right_dev, void *out_dev, int32_t n_images, int32_t h, int32_t w,
                 int64_t left_plane_stride, int64_t left_pitch, int64_t right_plane_stride, int64_t right_pitch,
                 int64_t out_plane_stride, int64_t out_pitch, int32_t dtype, int32_t gain, void *stream);

/* ------------------------------------------------------------------------------------------
 * K x K binning of tile planes (--tile-binning; extension: the reference has nothing like it).  For each of n_images planes
 * I [h, w] (SQ_U8 / SQ_U16, maximum M = 255 / 65535) and an integer factor K in 2..SQ_BIN_MAX_FACTOR, OUT OF PLACE, with
 * hb = h / K and wb = w / K (integer division: the last h - K hb rows and the last w - K wb columns are dropped):
 *     S(y, x) = the sum of I over the K x K block at (K y, K x)          (it fits 32 bits)
 *     SQ_BIN_MEAN:  out(y, x) = floor(S(y, x) / K^2)     (the truncated mean, the rule of sq_pyramid_mean: for K = 2 on even
 *                                                          sizes a binned plane is that function's level 1 of the plane)
 *     SQ_BIN_SUM :  out(y, x) = min(S(y, x), M)          (what camera binning does: counts add, and the result saturates)
 * The definition is the numpy restatement in tests/bin_ref.py, and the result is bit for bit that on every input.  n_images
 * planes, the planes a plane stride and the rows a pitch apart (elements; src_pitch >= w, dst_pitch >= wb), src and dst each
 * with their own: plane batches (above).
 * dst [n_images][hb][wb] must not meet src.  Every source element inside the K hb x K wb area is read exactly once, nothing of
 * the dropped rows and columns reaches a result, and nothing outside hb x wb of a destination plane is written
 * (csrc/bin.hip).  No scratch, no allocation, no atomics; asynchronous on `stream`; deterministic.  SQ_ERR_INVALID, and
 * nothing is launched, for an unknown dtype or method, a factor outside 2..8, hb or wb < 1, a pitch below the width, a plane
 * stride smaller than a plane, a NULL or element-misaligned pointer, n_images < 0, extents beyond the address space, and src
 * and dst extents (first to last element of all planes) that overlap.  SQ_ERR_UNSUPPORTED for a plane that needs more
 * workgroups than a launch has.  n_images == 0 is SQ_OK.  (Added without a change of SQ_VERSION: every caller built against
 * 108 still links and runs.)
 * ---------------------------------------------------------------------------------------- */
#define SQ_BIN_MEAN 1
#define SQ_BIN_SUM  2
#define SQ_BIN_MAX_FACTOR 8
int sq_bin_tiles(const void *src_dev, void *dst_dev, int32_t n_images, int32_t h, int32_t w,
                 int64_t src_plane_stride, int64_t src_pitch, int64_t dst_plane_stride, int64_t dst_pitch,
                 int32_t dtype, int32_t factor, int32_t method, void *stream);

/* ------------------------------------------------------------------------------------------
 * Radial lens correction of tile planes (--distortion-correction; extension: the reference has nothing like it -- ASHLAR, which
 * its ashlar_stitcher.py wraps, has --barrel-correction).  For each of n_images planes I [h, w] (SQ_U8 / SQ_U16; h, w <=
 * SQ_WARP_MAX_SIDE) and an integer D = ppm in -SQ_WARP_MAX_PPM..SQ_WARP_MAX_PPM (parts per million: the relative displacement
 * at the plane's corner), OUT OF PLACE, with // the floor division (also of negative numerators):
 *     U = w - 1, V = h - 1                         R2 = max(1, U*U + V*V)
 *     for the output pixel (y, x):
 *       u = 2*x - U,  v = 2*y - V                  (half-pixels from the plane's centre)
 *       rho = ((u*u + v*v) << 24) // R2            (0 .. 2^24: squared radius, 1.0 at the corners)
 *       s   = D * rho
 *       du  = (u*s + H) // (2*H),  dv = (v*s + H) // (2*H),   H = 10^6 * 2^16      (1/256 pixel, rounded half up)
 *       X = clamp(256*x + du, 0, 256*U),  Y = clamp(256*y + dv, 0, 256*V)           (edges replicated)
 *       x0 = X >> 8, fx = X & 255, x1 = min(x0 + 1, U);   y0, fy, y1 likewise
 *       out(y, x) = ( I[y0,x0]*(256-fx)*(256-fy) + I[y0,x1]*fx*(256-fy)
 *                   + I[y1,x0]*(256-fx)*fy       + I[y1,x1]*fx*fy + 32768 ) >> 16
 * i.e. the output at radius r takes the input at radius r (1 + D 10^-6 r^2 / R^2), bilinearly with 8 fractional bits: D > 0
 * samples farther out (it undoes pincushion distortion), D < 0 undoes barrel distortion, D = 0 is an exact copy.  The map fits
 * 64 bits and the blend unsigned 32 bits up to the largest side and |D|.  The definition is the numpy restatement in
 * tests/warp_ref.py, and the result is bit for bit that on every input.  n_images planes, the planes a plane stride and the
 * rows a pitch apart (elements; both pitches >= w), src and dst each with their own: plane batches (above).
 * dst [n_images][h][w] must not meet src.  Every output element
 * is written exactly once, nothing outside h x w of a destination plane is written, and every tap lies inside its source plane
 * (csrc/warp.hip: a thread works the map of its positions out once and walks over SQ_WARP_PLANES_PER_THREAD planes with it; a
 * launch takes 65535 such runs of planes, longer batches are split).  No scratch, no allocation, no atomics; asynchronous on
 * `stream`; deterministic.  SQ_ERR_INVALID, and nothing is launched, for an unknown dtype, ppm outside its range, h or w < 1, a
 * pitch below the width, a plane stride smaller than a plane, a NULL or element-misaligned pointer, n_images < 0, extents beyond
 * the address space, and src and dst extents (first to last element of all planes) that overlap.  SQ_ERR_UNSUPPORTED for a side
 * above SQ_WARP_MAX_SIDE.  n_images == 0 is SQ_OK.  (Added without a change of SQ_VERSION: every caller built against 108 still
 * links and runs.)
 * ---------------------------------------------------------------------------------------- */
#define SQ_WARP_MAX_PPM 50000
#define SQ_WARP_MAX_SIDE 65535
#define SQ_WARP_PLANES_PER_THREAD 16
int sq_warp_tiles(const void *src_dev, void *dst_dev, int32_t n_images, int32_t h, int32_t w,
                  int64_t src_plane_stride, int64_t src_pitch, int64_t dst_plane_stride, int64_t dst_pitch,
                  int32_t dtype, int32_t ppm, void *stream);

/* ------------------------------------------------------------------------------------------
 * Constant sub-pixel translation of tile planes (--channel-shift; extension: the reference has nothing like it).  For each of
 * n_images planes I [h, w] (SQ_U8 / SQ_U16; h, w <= SQ_SHIFT_MAX_SIDE) and a pair S = (Sy, Sx) of integers in 1/256 pixel, each
 * in -SQ_SHIFT_MAX..SQ_SHIFT_MAX (+-64 pixels), OUT OF PLACE:
 *     U = w - 1, V = h - 1, for the output pixel (y, x):
 *       Y = clamp(256*y + Sy, 0, 256*V),  X = clamp(256*x + Sx, 0, 256*U)           (edges replicated)
 *       y0 = Y >> 8, fy = Y & 255, y1 = min(y0 + 1, V);   x0, fx, x1 likewise
 *       out(y, x) = ( I[y0,x0]*(256-fx)*(256-fy) + I[y0,x1]*fx*(256-fy)
 *                   + I[y1,x0]*(256-fx)*fy       + I[y1,x1]*fx*fy + 32768 ) >> 16
 * i.e. the output at (y, x) takes the input at (y + Sy/256, x + Sx/256), bilinearly with 8 fractional bits: the blend of
 * sq_warp_tiles under another map.  S = (0, 0) is an exact copy, a shift by whole pixels a copy with replicated edges.  The
 * definition is the numpy restatement in tests/shift_ref.py, and the result is bit for bit that on every input.
 * shifts_host is a HOST table of n_images / images_per_shift pairs (Sy, Sx), read before the call returns: images
 * [k * images_per_shift, (k + 1) * images_per_shift) take pair k, and n_images must be a multiple of images_per_shift >= 1.
 * One grid is issued per maximal run of consecutive equal pairs (a run of (0, 0) goes through the same kernel as a copy), each
 * split at 65535 planes, so no table goes to the device.  The planes a plane stride and the rows a pitch apart (elements; both
 * pitches >= w), src and dst each with their own: plane batches (above).
 * dst [n_images][h][w] must not meet src.  Every output element is written exactly once,
 * nothing outside h x w of a destination plane is written, and every tap lies inside its source plane (csrc/shift.hip: a
 * thread owns 16 bytes of dst columns and walks down SQ_SHIFT_ROWS_PER_THREAD rows, every source row is read once per run).
 * No scratch, no allocation, no atomics; asynchronous on `stream`; deterministic.  SQ_ERR_INVALID, and nothing is launched,
 * for an unknown dtype, a shift outside its range, h or w < 1, a pitch below the width, a plane stride smaller than a plane,
 * a NULL or element-misaligned pointer, a NULL table, n_images < 0 or no multiple of images_per_shift, extents beyond the
 * address space, and src and dst extents (first to last element of all planes) that overlap.  SQ_ERR_UNSUPPORTED for a side
 * above SQ_SHIFT_MAX_SIDE.  n_images == 0 is SQ_OK, also with a NULL table.  (Added without a change of SQ_VERSION: every
 * caller built against 108 still links and runs.)
 * ---------------------------------------------------------------------------------------- */
#define SQ_SHIFT_MAX 16384
#define SQ_SHIFT_MAX_SIDE 65535
#define SQ_SHIFT_ROWS_PER_THREAD 32
int sq_shift_tiles(const void *src_dev, void *dst_dev, int32_t n_images, int32_t h, int32_t w,
                   int64_t src_plane_stride, int64_t src_pitch, int64_t dst_plane_stride, int64_t dst_pitch,
                   int32_t dtype, const int32_t *shifts_host, int32_t images_per_shift, void *stream);

/* ------------------------------------------------------------------------------------------
 * Per-channel affine map of tile planes: rotation, scale and shear about the tile centre, composed with a constant shift
 * (--channel-affine; extension: the reference has nothing like it).  For each of n_images planes I [h, w] (SQ_U8 / SQ_U16; h, w <=
 * SQ_AFFINE_MAX_SIDE), S = (Sy, Sx) in 1/256 pixel, each in -SQ_SHIFT_MAX..SQ_SHIFT_MAX, and A = (Ayy, Ayx, Axy, Axx), integers in
 * parts per million, each in -SQ_AFFINE_MAX_PPM..SQ_AFFINE_MAX_PPM, OUT OF PLACE, with // the floor division:
 *     U = w - 1, V = h - 1, for the output pixel (y, x):
 *       u = 2*x - U,  v = 2*y - V                                   (half-pixels from the tile centre)
 *       dv = Sy + (16*(Ayy*v + Ayx*u) + 62500) // 125000            (1/256 pixel, rounded half up: 128/10^6 = 16/125000)
 *       du = Sx + (16*(Axy*v + Axx*u) + 62500) // 125000
 *       Y = clamp(256*y + dv, 0, 256*V),  X = clamp(256*x + du, 0, 256*U)        (edges replicated)
 *       y0 = Y >> 8, fy = Y & 255, y1 = min(y0 + 1, V);   x0, fx, x1 likewise
 *       out(y, x) = ( I[y0,x0]*(256-fx)*(256-fy) + I[y0,x1]*fx*(256-fy)
 *                   + I[y1,x0]*(256-fx)*fy       + I[y1,x1]*fx*fy + 32768 ) >> 16
 * i.e. the output at centre + p takes the input at centre + (1 + A 10^-6) p + S/256, bilinearly with 8 fractional bits: the blend
 * of sq_shift_tiles under another map, and with A = 0 that function's result.  A rotation by t is Ayy = Axx = (cos t - 1) 10^6,
 * Ayx = -Axy = sin t 10^6; a magnification m is Ayy = Axx = (m - 1) 10^6.  The numerators need 64 bits (up to 1.05e11 at the
 * largest side).  The definition is the numpy restatement in tests/affine_ref.py, and the result is bit for bit that on every input.
 * params_host is a HOST table of n_images / images_per_param six-tuples (Sy, Sx, Ayy, Ayx, Axy, Axx), read before the call
 * returns: images [k * images_per_param, (k + 1) * images_per_param) take tuple k, and n_images must be a multiple of
 * images_per_param >= 1.  One grid is issued per maximal run of consecutive equal tuples (a run of zeros goes through the same
 * kernel as a copy), each split at 65535 * SQ_AFFINE_PLANES_PER_THREAD planes, so no table goes to the device.  Every other
 * convention is that of sq_shift_tiles: src and dst are plane batches (above; both pitches >= w); dst must not meet src; every
 * output element is written exactly once,
 * nothing outside h x w of a destination plane is written, and every tap lies inside its source plane (csrc/affine.hip: a thread
 * owns 16 bytes of dst columns of one row, steps the map along them without a division per pixel and walks over
 * SQ_AFFINE_PLANES_PER_THREAD planes with it; the taps of a vector come as 16-byte loads of two or three source rows).  No
 * scratch, no allocation, no atomics; asynchronous on `stream`; deterministic.  The refusals and return codes of sq_shift_tiles,
 * plus SQ_ERR_INVALID for a coefficient outside its range.  (Added without a change of SQ_VERSION.)
 * ---------------------------------------------------------------------------------------- */
#define SQ_AFFINE_MAX_PPM 50000
#define SQ_AFFINE_MAX_SIDE 65535
#define SQ_AFFINE_PLANES_PER_THREAD 16
int sq_affine_tiles(const void *src_dev, void *dst_dev, int32_t n_images, int32_t h, int32_t w,
                    int64_t src_plane_stride, int64_t src_pitch, int64_t dst_plane_stride, int64_t dst_pitch,
                    int32_t dtype, const int32_t *params_host, int32_t images_per_param, void *stream);

/* ------------------------------------------------------------------------------------------
 * Dark-frame subtraction of tile planes: the camera's additive term, the other half of the flatfield correction (I - D) / F
 * (--dark-frame; extension: the reference runs BaSiC with get_darkfield=False and subtracts nothing).  For each of n_images
 * planes I [h, w] (SQ_U8 / SQ_U16, maximum M = 255 / 65535), a dark frame D [h, w] of the same dtype (or a constant c in 0..M)
 * and a pedestal P in 0..M, IN PLACE, taken in a wider signed type:
 *     out(y, x) = clamp(I(y, x) - D(y, x) + P, 0, M)
 * The definition is the numpy restatement in tests/dark_ref.py, and the result is bit for bit that on every input.  The
 * operation is elementwise: a thread reads only what it writes.  params_host is a HOST table of n_images / images_per_param
 * pairs (k, c), read before the call returns: images [j * images_per_param, (j + 1) * images_per_param) take pair j, and n_images
 * must be a multiple of images_per_param >= 1.  k >= 0 selects frame k of frames_dev [n_frames] (the frames a frame stride and
 * their rows a frame pitch apart, in elements) and goes with c == 0; k == -1 means the constant c.  One grid is issued per maximal
 * run of consecutive equal pairs; a run that is the identity (k == -1 and c == pedestal) issues nothing and leaves its planes
 * untouched; longer runs are split at 65535 * SQ_DARK_IMAGES_PER_THREAD planes.  No table goes to the device.  The tiles and
 * the frames are plane batches (above); any h, w >= 1; the columns between w and the pitch and the rows beyond h are
 * never written, and nothing there is read into a result.  The frames must not meet the tiles.  csrc/dark.hip: a thread owns one
 * 16-byte vector of columns laid at the phase of the tile row, keeps P - D of its (row, columns) in registers and walks
 * SQ_DARK_IMAGES_PER_THREAD images of the run with it, so a frame is fetched once per that many tiles (image by image where the
 * plane stride is no whole number of 16-byte vectors); the constant path loads no frame.  The value is 1: measured on an MI355X
 * the walk over 4 images took 1.12 x the time of the build with 1 (the frame of a run stays in the caches either way), so the
 * simpler form is the library's; the macro may be set when the file is compiled, which is how tools/dark_probe.py compares.  No scratch, no allocation, no atomics,
 * no LDS; asynchronous on `stream`; deterministic.  SQ_ERR_INVALID, and nothing is launched, for an unknown dtype, a pedestal or
 * a constant outside 0..M, a k outside -1..n_frames - 1 (or a k >= 0 with c != 0), a pitch below w, a stride smaller than a
 * plane, a NULL or element-misaligned pointer (NULL frames are fine when no pair names one), a NULL table, n_images < 0 or no
 * multiple of images_per_param, h or w < 1, extents beyond the address space, and frames whose extent (first to last element)
 * overlaps the tiles'.  SQ_ERR_UNSUPPORTED for a plane that needs more workgroups than a launch has.  n_images == 0 is SQ_OK.
 * (Added without a change of SQ_VERSION: every caller built against 108 still links and runs.)
 * ---------------------------------------------------------------------------------------- */
#ifndef SQ_DARK_IMAGES_PER_THREAD
#define SQ_DARK_IMAGES_PER_THREAD 1
#endif
int sq_dark_tiles(void *tiles_dev, int32_t n_images, int32_t h, int32_t w, int64_t plane_stride, int64_t pitch, int32_t dtype,
                  const void *frames_dev, int32_t n_frames, int64_t frame_stride, int64_t frame_pitch,
                  const int32_t *params_host /* [n_images / images_per_param][2] */, int32_t images_per_param,
                  int32_t pedestal, void *stream);

/* ------------------------------------------------------------------------------------------
 * Registration: replaces normalize_image (stitcher.py:613-617), the crops of
 * calculate_horizontal_shift / calculate_vertical_shift (:504-506, :517-519) and
 * skimage.registration.phase_cross_correlation(upsample_factor=10) (:510, :523), batched
 * over tile pairs.  The python round() and the "- crop width" of :511/:524 stay on the host.
 * ---------------------------------------------------------------------------------------- */

/* Per-tile min and max (normalize_image's reductions): out_minmax_dev[2*i] = min,
 * [2*i+1] = max as uint32, for n_tiles tiles given by pointer table or base+stride. */
int sq_tile_minmax(const void *const *tile_ptrs_dev, const void *tile_base_dev, int64_t tile_stride, int32_t n_tiles,
                   int32_t tile_h, int32_t tile_w, int32_t tile_pitch, int32_t tile_dtype,
                   uint32_t *out_minmax_dev, void *stream);

/* normalize_image (stitcher.py:613-617) on whole tiles: out_dev[i] (dense tile_h x tile_w, same dtype) =
 * ((tile - min) / (max - min) * dtype_max) truncated, in float64 like numpy; minmax from sq_tile_minmax.
 * The registration pipeline fuses the same arithmetic into its first kernel; this entry point exists for
 * callers of the method itself. */
int sq_normalize_tiles(const void *const *tile_ptrs_dev, const void *tile_base_dev, int64_t tile_stride, int32_t n_tiles,
                       int32_t tile_h, int32_t tile_w, int32_t tile_pitch, int32_t tile_dtype,
                       const uint32_t *minmax_dev, void *out_dev, void *stream);

typedef enum sq_normalization {
    SQ_NORM_NONE = 0, /* scikit-image <= 0.18                                       */
    SQ_NORM_PHASE = 1 /* scikit-image >= 0.19 default: P /= max(|P|, 100 eps)       */
} sq_normalization;

/* One pair: crop origin inside the reference tile and inside the moving tile; both crops are
 * n0 x n1 (shared by the whole batch). */
typedef struct sq_pair {
    int32_t ref_tile, mov_tile; /* indices into the tile table / minmax table          */
    int32_t ref_y0, ref_x0;     /* crop origin in the reference tile                   */
    int32_t mov_y0, mov_x0;     /* crop origin in the moving tile                      */
} sq_pair;

/* Result per pair.  shift = round(coarse*u)/u + (fine - fix(ceil(1.5u)/2))/u is formed on the
 * host in float64 exactly as skimage does (_phase_cross_correlation.py:232-250). */
typedef struct sq_pair_result {
    int32_t coarse[2]; /* whole-pixel peak after wrap-around (skimage :215-220); INT32_MIN  */
                       /* in both if the pair's tile index or crop lies outside its tile    */
    int32_t fine[2];   /* argmax index in the 15x15 upsampled neighbourhood (:244)     */
    double ccmax_re, ccmax_im; /* cross-correlation value at the refined peak          */
    double src_amp, tgt_amp;   /* sum |F|^2, sum |G|^2 (:252-254)                      */
} sq_pair_result;

typedef struct sq_register_args {
    const void *const *tile_ptrs_dev; /* or NULL + base/stride                          */
    const void *tile_base_dev;
    int64_t tile_stride;
    int32_t n_tiles, tile_h, tile_w, tile_pitch, tile_dtype;
    const uint32_t *minmax_dev; /* from sq_tile_minmax (2 per tile); an entry with min > max
                                   means "do not normalise this tile" (plain skimage call)  */
    const sq_pair *pairs_dev;
    int32_t n_pairs;
    int32_t n0, n1; /* crop size (rows, cols)                                           */
    int32_t upsample_factor; /* 10 in the reference; >= 1                                */
    int32_t normalization;   /* sq_normalization                                         */
    sq_pair_result *results_dev;
    void *workspace_dev;
    int64_t workspace_bytes;
} sq_register_args;

/* Crop lengths: 2 ... 65535 pixels a side (the reference's pocketfft takes any length, stitcher.py:503-510, 516-523).
 *   - a power of two: radix-2 FFT;
 *   - any other length whose prime factors are all <= 13 (1500, 3000, 6000 ...): mixed-radix Cooley-Tukey (radix 4 / 2 / 3 /
 *     5 / 7 / 11 / 13), directly;
 *   - any other length n: Bluestein's chirp-z form through a smooth length M >= 2n - 1 (2084 -> 4320 points);
 * float64 throughout -- the factorisations pocketfft (the reference's FFT, via scipy / numpy) uses for such lengths.
 * A line of up to 9728 points (complex128) is transformed in the 160 KB of LDS: smooth sides up to 9720, any side up to 4860
 * (crops are about half a tile side long, stitcher.py:504-506 / :517-519: every sensor up to 9720 pixels a side -- a 9568 x 6380
 * one gives 4784 and 3190).  A longer line runs the same transform in a scratch line of the workspace (through the L2; slower,
 * and the workspace grows by 512 such lines).  Beyond 65535: SQ_ERR_UNSUPPORTED.
 * sq_register_line_supported: 1 when a crop side of n pixels is accepted, else 0 (no device needed). */
int sq_register_line_supported(int32_t n);
/* Bytes of workspace sq_register_pairs needs for (n_pairs, n0, n1). */
int64_t sq_register_workspace_bytes(int32_t n_pairs, int32_t n0, int32_t n1, int32_t upsample_factor);
int sq_register_pairs(const sq_register_args *args, void *stream);

/* The launches sq_register_pairs issues for a batch of n_pairs crops of n0 x n1: which transform each axis gets and which
 * kernel instantiation, block size and grid each stage runs with.  sq_register_pairs launches from this very struct, so
 * a test can state which path a case takes and assert it.  Grids are (x, y) in blocks. */
typedef struct sq_register_plan {
    int32_t m0, m1;            /* Bluestein length per axis; 0 = the axis length is smooth and transformed directly      */
    int32_t long0, long1;      /* the axis' line (m or n points) does not fit the LDS: scratch line of the workspace     */
    int32_t gen0, gen1;        /* mixed-radix stages (else the power-of-two transform)                                  */
    int32_t nf0, nf1;          /* stages of the transform of length (m ? m : n), innermost first; 0 = a power of two    */
    uint8_t radix0[16], radix1[16];
    int32_t tc;                /* columns per block of the column kernel; 0 = one column per block (columns_single)     */
    int32_t share;             /* column blocks that share 128-byte lines of the spectra; 0 for a long axis 0           */
    int32_t col_threads;       /* threads of the tc-column kernel; 0 when columns_single runs                           */
    int32_t columns_single;    /* 1: one column per block (a Bluestein column, a column past 4608 points, a long one)   */
    int32_t columns_single_threads; /* its threads; 0 when the tc-column kernel runs                                    */
    int32_t rl_fwd, rl_inv;    /* lines per block of the forward / inverse row kernel                                   */
    int32_t threads_fwd, threads_inv;
    int32_t upsample_rows_tb, upsample_rows_kc; /* instantiation <TB, KC> of the first upsampling kernel; 0, 0 at u = 1 */
    int32_t grid_fwd[2], grid_col[2], grid_inv[2], grid_up_rows[2];
    int64_t lds_fwd, lds_col, lds_inv; /* dynamic LDS bytes per block of the three transform stages                     */
} sq_register_plan;
/* Host only: touches no device, launches nothing.  n_pairs 1 ... 65535, tile_dtype SQ_U8 | SQ_U16 (it selects the pixel
 * type of the forward row kernel, no launch shape).  (An entry point added without changing an existing one keeps
 * SQ_VERSION: every caller built against 108 still links and runs.) */
int sq_register_describe(int32_t n_pairs, int32_t n0, int32_t n1, int32_t upsample_factor, int32_t tile_dtype,
                         sq_register_plan *out);

/* Overlap moments for the confidence of a registered pair (global registration, alignment.py): the exact integer sums
 * a zero-normalised cross-correlation is formed from, over the overlap of the two full tiles at the pair's offset.
 * Tile table as for sq_tile_minmax (pointer table or base + stride, SQ_U8 / SQ_U16). */
typedef struct sq_overlap {          /* one window pair: h x w pixels at (ref_y0, ref_x0) in ref_tile and (mov_y0, mov_x0) in mov_tile */
    int32_t ref_tile, mov_tile, ref_y0, ref_x0, mov_y0, mov_x0, h, w;
} sq_overlap;
/* out_dev[5*i .. 5*i+4] = sum a, sum b, sum a^2, sum b^2, sum a*b over window pair i (uint64, exact; a window of 65535s
 * 2048 x 2048 gives sum a*b = 1.8e16).  out_dev is zeroed on `stream` by every call.  h == 0 or w == 0 gives zeros.  A
 * tile index outside the table or a window that leaves its tile: SQ_ERR_INVALID, nothing launched and out_dev untouched.
 * To check the windows the call reads pairs_dev back to the host, i.e. it synchronises `stream`.  n_pairs <= 65535. */
int sq_pair_overlap_moments(const void *const *tile_ptrs_dev, const void *tile_base_dev, int64_t tile_stride, int32_t n_tiles,
                            int32_t tile_h, int32_t tile_w, int32_t tile_pitch, int32_t tile_dtype,
                            const sq_overlap *pairs_dev, int32_t n_pairs, uint64_t *out_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * Per-seam alignment words (--seam-qc; extension: the reference has none): how well two overlapping tiles agree where they are
 * placed, and at every integer residual displacement e = (ey, ex) in [-R, R]^2 around that placement, R = radius in
 * 0..SQ_SEAM_MAX_RADIUS.  tiles_dev holds n_planes planes of n_tiles tiles [h, w] (SQ_U8 / SQ_U16), the planes a plane stride,
 * the tiles a tile stride and the rows a pitch apart (elements, pitch >= w; no alignment asked beyond the element's own).  ONE
 * pair table applies to every plane: record i is the CORE window pair at e = 0 -- for tiles whose full-tile canvas origins
 * differ by d = o_mov - o_ref, with the overlap (ry0, rx0, my0, mx0, ho, wo) of the two full tiles at d, the core is the overlap
 * inset by R on all four sides: h = ho - 2R, w = wo - 2R, ref window at (ry0 + R, rx0 + R), mov window at (my0 + R, mx0 + R).
 * With a(y, x) = ref[ref_y0 + y, ref_x0 + x] and b_e(y, x) = mov[mov_y0 + y - ey, mov_x0 + x - ex] over the core,
 * out_dev[plane][pair][...] receives 3 + 3 (2R + 1)^2 words:
 *     0  Sa = sum a      1  Saa = sum a^2      2  Sad = sum |a - b_0|
 *     then, row-major over (ey, ex) from (-R, -R):  Sb_e = sum b_e,  Sbb_e = sum b_e^2,  Sab_e = sum a b_e
 * When the tiles agree at e, their true displacement is d + e.  The definition is the numpy restatement in
 * tests/seam_qc_ref.py.  Integers only, 64-bit from the first add of a product; the words are bit for bit numpy's int64 sums
 * whatever the schedule (per-workgroup partial sums, then one 64-bit integer atomic add per word per workgroup into words the
 * call zeroes on `stream` first: out_dev needs no preparation and is OVERWRITTEN).  Every piece of a window is read from global
 * memory once -- the mov piece with its R-pixel halo into LDS, a thread's ref column into registers -- and the offsets are
 * evaluated from there (csrc/seam.hip).
 * pairs_host is the table on the host and is what the call validates -- tile indices, the ref window inside its tile, the mov
 * window at least R inside its tile on every side; pairs_dev is the same table on the device and is what the kernel reads (the
 * caller keeps the two equal).  Asynchronous on `stream`: no host read-back, no allocation, no other stream.  SQ_ERR_INVALID,
 * and nothing is launched, for a bad record, an unknown dtype, a radius outside 0..SQ_SEAM_MAX_RADIUS, negative counts, h or
 * w < 1, a pitch below w, strides smaller than what they step over, and a NULL or misaligned pointer.  SQ_ERR_UNSUPPORTED for a
 * core of more than 2^31 pixels (below that no word can reach 2^63).  n_pairs == 0 or n_planes == 0 is SQ_OK.  A record with
 * h == 0 or w == 0 gives zeros.
 * ---------------------------------------------------------------------------------------- */
#define SQ_SEAM_MAX_RADIUS 3
int sq_seam_stats(const void *tiles_dev, int32_t n_planes, int32_t n_tiles, int32_t h, int32_t w, int64_t plane_stride,
                  int64_t tile_stride, int64_t pitch, int32_t dtype, const sq_overlap *pairs_host, const sq_overlap *pairs_dev,
                  int32_t n_pairs, int32_t radius, uint64_t *out_dev /* [n_planes][n_pairs][3 + 3 (2R+1)^2], overwritten */,
                  void *stream);

/* ------------------------------------------------------------------------------------------
 * Chunk encoding on the device: the chunks of n_planes (t, c, z) planes (chunk_h x chunk_w elements,
 * zero-padded past the plane's edge like zarr pads edge chunks) as Blosc-1 frames -- byte shuffle + LZ4, the
 * default codec of the store the reference writes (zarr.storage.default_compressor, stitcher.py:814-818) -- packed
 * densely into out_dev: chunk i = plane-major, then chunk row, then chunk column, lives at
 * out_dev[offsets_dev[i] .. offsets_dev[i + 1]) (n_chunks + 1 offsets; an all-zero chunk has size 0: the store's
 * fill_value stands for it).  *status_dev != 0 afterwards: out_capacity was too small (sq_blosc_out_bound() never is).
 * Every accepted call clears *status_dev first, also one with no chunk at all (n_planes == 0: offsets_dev[0] = 0 and
 * nothing else); a negative out_capacity is SQ_ERR_INVALID, as for the two tile encoders below.
 * Strides in elements; dtype SQ_U8 or SQ_U16.  Asynchronous on `stream` like the other entry points.
 * The three size queries return a negative sq_status for a geometry the encode call refuses (a chunk may hold at most
 * 32 MiB); sq_blosc_chunk_count is not told the dtype and refuses only what no dtype could encode.
 * ---------------------------------------------------------------------------------------- */
int64_t sq_blosc_chunk_count(int32_t n_planes, int32_t h, int32_t w, int32_t chunk_h, int32_t chunk_w);
int64_t sq_blosc_out_bound(int32_t n_planes, int32_t h, int32_t w, int32_t dtype, int32_t chunk_h, int32_t chunk_w);
int64_t sq_blosc_scratch_bytes(int32_t n_planes, int32_t h, int32_t w, int32_t dtype, int32_t chunk_h, int32_t chunk_w);
int sq_blosc_encode_planes(const void *planes_dev, int64_t plane_stride, int64_t pitch, int32_t n_planes, int32_t h, int32_t w,
                           int32_t dtype, int32_t chunk_h, int32_t chunk_w, void *scratch_dev, int64_t scratch_bytes,
                           uint64_t *offsets_dev, void *out_dev, int64_t out_capacity, uint32_t *status_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * TIFF tile encoding on the device: the tiles of n_planes (t, c, z) planes (tile_h x tile_w elements, little endian, ZERO past
 * the plane's edge: a TIFF tile is always full) as RFC 1950 zlib streams -- TIFF Compression 8 ("Adobe deflate") -- packed
 * densely into out_dev exactly like the Blosc frames above: tile i = plane-major, then tile row, then tile column, lives at
 * out_dev[offsets_dev[i] .. offsets_dev[i + 1]) (n_tiles + 1 offsets; an all-zero tile has size 0: the writer points it at one
 * shared stream).  predictor 2 = TIFF's horizontal differencing (inside every tile row each element but the first is replaced
 * by its difference to its left neighbour, modulo 2^bits) before the bytes are coded, 1 = none.
 * Stream: 78 01, then one deflate block per 16 KiB segment of the (predicted) tile bytes, then their Adler-32 (big endian).
 * The only matches are element runs (distance = element size, length 3..258); every segment is one dynamic-Huffman block
 * with its own code (lengths limited to 15; trivial code-length code; one distance symbol sent with one bit) or, when that
 * does not shrink it, a stored block; a non-final segment ends with an empty stored block (sync flush), the last carries
 * BFINAL.  tests/deflate_ref.py restates the stream in numpy; any inflater reads it.
 * *status_dev != 0 afterwards: out_capacity was too small (sq_deflate_out_bound(), every segment stored, never is) and nothing
 * was written to out_dev.  Strides in elements; dtype SQ_U8 or SQ_U16 (SQ_ERR_UNSUPPORTED otherwise); a tile may hold at most
 * 32 MiB.  The size queries return a negative sq_status for a geometry the encode call refuses; sq_deflate_chunk_count is not
 * told the dtype.  Asynchronous on `stream`.
 * ---------------------------------------------------------------------------------------- */
int64_t sq_deflate_chunk_count(int32_t n_planes, int32_t h, int32_t w, int32_t tile_h, int32_t tile_w);
int64_t sq_deflate_out_bound(int32_t n_planes, int32_t h, int32_t w, int32_t dtype, int32_t tile_h, int32_t tile_w);
int64_t sq_deflate_scratch_bytes(int32_t n_planes, int32_t h, int32_t w, int32_t dtype, int32_t tile_h, int32_t tile_w);
int sq_deflate_encode_planes(const void *planes_dev, int64_t plane_stride, int64_t pitch, int32_t n_planes, int32_t h, int32_t w,
                             int32_t dtype, int32_t tile_h, int32_t tile_w, int32_t predictor, void *scratch_dev,
                             int64_t scratch_bytes, uint64_t *offsets_dev, void *out_dev, int64_t out_capacity,
                             uint32_t *status_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * Lossy TIFF tile encoding on the device: the same tiles, packed the same way (offsets, size 0 for an all-zero tile, status),
 * as baseline JPEG streams -- TIFF Compression 7, one self-contained ITU-T T.81 stream per tile, no JPEGTables tag, no APPn:
 *   SOI | DQT (table 0) | SOF0 (P = 8, Y = tile_h, X = tile_w, one component, H = V = 1, Tq = 0) | DHT (DC 0, AC 0) |
 *   DRI (Ri = tile_w / 8) | SOS (Ss = 0, Se = 63, Ah = Al = 0) | entropy-coded data | EOI
 * Quantisation: the Annex K.1 luminance table scaled by libjpeg's rule for `quality` q in 1..100: s = 5000 / q (integer) for
 * q < 50, else 200 - 2 q; Q = clamp((base s + 50) / 100, 1, 255).  Huffman tables: Annex K.3.3 luminance DC and AC, fixed.
 * One restart interval = one row of blocks: padded with 1-bits to a byte, RSTm (m counting mod 8) between intervals, none after
 * the last, DC prediction 0 at the start of each.  FF 00 for every FF of the data.  Zigzag order, ZRL for runs of 16 zeros,
 * EOB unless coefficient 63 is non-zero; categories up to 11 (DC difference) and 10 (AC).
 * Forward transform, exact in integers: x = pixel - 128; C[u][j] = round(2^10 a(u) cos((2 j + 1) u pi / 16)) (a(0) = sqrt(1/8),
 * else 1/2) as 64 literal integers; N = C x C^T without intermediate rounding; coefficient = sign(N) ((|N| + D / 2) / D) with
 * D = Q 2^20 (integer division).  Bound: the absolute values of a row of C sum to at most 2896, so |N| <= 128 * 2896^2 < 2^30
 * and |N| + D / 2 < 2^31.  image-stitcher_amd/jpegtile.py states all of this in numpy; the device's bytes equal its bytes.
 * dtype SQ_U8 only (SQ_ERR_UNSUPPORTED otherwise); tile sides that are no multiples of 8 and a quality outside 1..100 are
 * SQ_ERR_INVALID; a tile holds at most 32 Mi elements and its sides are at most 65496
 * (libjpeg reads no image above 65500; SQ_ERR_UNSUPPORTED beyond).
 * *status_dev != 0 afterwards: out_capacity was too small, and NO byte was written to out_dev (the exact sizes are known before
 * the first byte is written).  sq_jpeg_out_bound() is the true worst case -- every block at the longest codes (20 + 63 * 26
 * bits) and every byte stuffed, about 6.5 times the raw tiles -- and never too small; callers that allocate less (the raw size
 * is plenty for images) must check the status.  Strides in elements.  Asynchronous on `stream`.
 * ---------------------------------------------------------------------------------------- */
int64_t sq_jpeg_chunk_count(int32_t n_planes, int32_t h, int32_t w, int32_t tile_h, int32_t tile_w);
int64_t sq_jpeg_out_bound(int32_t n_planes, int32_t h, int32_t w, int32_t dtype, int32_t tile_h, int32_t tile_w);
int64_t sq_jpeg_scratch_bytes(int32_t n_planes, int32_t h, int32_t w, int32_t dtype, int32_t tile_h, int32_t tile_w);
int sq_jpeg_encode_planes(const void *planes_dev, int64_t plane_stride, int64_t pitch, int32_t n_planes, int32_t h, int32_t w,
                          int32_t dtype, int32_t tile_h, int32_t tile_w, int32_t quality, void *scratch_dev,
                          int64_t scratch_bytes, uint64_t *offsets_dev, void *out_dev, int64_t out_capacity,
                          uint32_t *status_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * Chunk files. The store of save_region_ome_zarr (stitcher.py:771-859; zarr v2, one file per chunk, chunks (1,1,1,512,512)) is
 * hundreds of thousands of half-MB files per region; written one by one from the interpreter they were the wall of a files ->
 * store run once the codec ran on the device.  sq_write_files writes n_files files from ONE host buffer with native threads:
 * file i is the NUL-terminated string at paths + path_offsets[i] and holds data[data_offsets[i] .. data_offsets[i + 1]) (created
 * or truncated, mode 0644; an empty range makes an empty file).  The directories must exist.  n_threads <= 0: 16.  Stops at the
 * first failure (SQ_ERR_INVALID, the path and errno text in sq_last_error); *bytes_written = bytes that reached the files.
 * Host-only: no device, no stream.
 * ---------------------------------------------------------------------------------------- */
int sq_write_files(const char *paths, const int64_t *path_offsets, const void *data, const int64_t *data_offsets, int64_t n_files,
                   int32_t n_threads, int64_t *bytes_written);

/* ------------------------------------------------------------------------------------------
 * Flatfield ESTIMATE: replaces basicpy.BaSiC(get_darkfield=False, smoothness_flatfield=s).fit(images).flatfield
 * in Stitcher.get_flatfields (stitcher.py:365-419; the call is :374-377) for one channel's sample of tiles
 * (<= 80: the reference adds at most 32 per timepoint and stops once it holds MORE than 48, :381-395 -> up to 48 + 32).
 * PARITY UNPINNED: basicpy is an absent, un-pinned third-party package; this is the published BaSiC algorithm
 * (Peng et al. 2017; LADMAP + re-weighted L1, no darkfield, basicpy's documented defaults) as defined by
 * oracle/basic_oracle.py.  Not on the hot path (the divide by the result is: sq_fuse_planes).
 * Unlike the other entry points this one SYNCHRONISES `stream` (its iteration count is decided by the data).
 * flatfield_dev: tile_h x tile_w float32, dense.  workspace: sq_basic_workspace_bytes(), 256-byte aligned.
 * The definition does not converge on every input (dim stacks, a handful of images, a huge smoothness weight: see
 * oracle/basic_oracle.py): a re-weighting round then stops at the cap of 500 iterations with whatever it holds, counted in
 * info->capped_rounds.  When the 128 x 128 flatfield of the last round is not finite and > 0 everywhere the call returns
 * SQ_ERR_NUMERIC (the minimum and the capped rounds in sq_last_error), fills `info` and leaves flatfield_dev unwritten;
 * S > 0 there carries over to every full-size gain (the up-sampling weights are >= 0 and sum to 1 per pixel).
 * ---------------------------------------------------------------------------------------- */
typedef struct sq_basic_info {
    int32_t reweight_iterations; /* outer re-weighted-L1 rounds run (<= 10)          */
    int32_t ladmap_iterations;   /* inner iterations summed over the rounds          */
    int32_t working_size;        /* 128: the images are resampled to this before the fit */
    int32_t capped_rounds;       /* rounds whose inner loop reached the 500-iteration cap (0 for a fit that settled) */
} sq_basic_info;

int64_t sq_basic_workspace_bytes(int32_t n_images, int32_t tile_h, int32_t tile_w);
int sq_basic_fit(const void *const *tile_ptrs_dev, const void *tile_base_dev, int64_t tile_stride, int32_t n_images,
                 int32_t tile_h, int32_t tile_w, int32_t tile_pitch, int32_t tile_dtype, float smoothness_flatfield,
                 float *flatfield_dev, void *workspace_dev, int64_t workspace_bytes, sq_basic_info *info, void *stream);

/* Self-test (tests only): the fusion kernels divide uint16 pixels by float32 gains with a shortened
 * sequence that is exact for gains with 2^-100 <= |g| < 2^100.  This compares its
 * final clipped integers, truncated (overwrite mode) and rounded (feather mode), with the IEEE path for ALL 2^23 gain
 * mantissas x all 65536 numerators in n_binades consecutive binades starting at 2^exponent (allowed:
 * -100..99), either sign, and leaves the number of differing results in *mismatches_dev (must be 0). */
int sq_selftest_flat_divide(int32_t exponent, int32_t n_binades, int32_t negative, uint64_t *mismatches_dev,
                            void *stream);

/* The same for float64 gains (their shortened sequence = the compiler's IEEE division without its range
 * handling): 2^15 pseudo-random gains per binade (from `seed`; all-zero, all-one and single-bit mantissas
 * included) x all 65536 numerators; compares the quotient doubles and the clipped integers. */
int sq_selftest_flat_divide_f64(int32_t exponent, int32_t n_binades, int32_t negative, uint64_t seed,
                                uint64_t *mismatches_dev, void *stream);

/* normalize_image's division (stitcher.py:615-617: (img - min) / (max - min) in float64) is computed in the registration
 * kernels as a multiply by the reciprocal of the range plus Markstein's correction (two fused multiply-adds).  This
 * compares that with the IEEE division, bit for bit, for ALL numerators 0..65535 x ALL ranges 0..65535 and ADDS the
 * number of differing quotients to *mismatches_dev (zero it first; must stay 0). */
int sq_selftest_normalise_divide(uint64_t *mismatches_dev, void *stream);

/* The grouped feather blend divides the weighted sum of two quotients by the sum of their weights with the IEEE
 * sequence minus its range handling (the reciprocal of the weight sum is shared by the planes of a group).  This
 * compares it with the compiler's division, bit for bit, for ALL 2^23 mantissas of the numerator in n_binades
 * consecutive binades starting at 2^exponent (allowed: -44..52, what moderate gains can produce) x every weight sum
 * 2..16384, either sign; *mismatches_dev must come back 0. */
int sq_selftest_blend_divide(int32_t exponent, int32_t n_binades, int32_t negative, uint64_t *mismatches_dev,
                             void *stream);

/* ------------------------------------------------------------------------------------------
 * Synthetic tiles on the device (bench / tests only): the generator of
 * image-stitcher_amd/synth.py, bit for bit.  out_dev[i] is tile i (tile_h x tile_w, dense).
 * ---------------------------------------------------------------------------------------- */
typedef struct sq_synth_tile {
    uint64_t scene_seed, noise_seed;
    int64_t oy, ox; /* scene origin of the tile */
} sq_synth_tile;

int sq_synth_tiles(const sq_synth_tile *tiles_dev, int32_t n_tiles, int32_t tile_h, int32_t tile_w, int32_t noise_amp,
                   int32_t tile_dtype, void *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SQUIDSTITCH_H */

// Device-side declarations every kernel file of csrc/ used to spell out for itself: the global address space, the packed vector
// types, the "several elements in one load" types and lds_written().  Declarations only -- no kernel helper lives here (sharing
// even small device functions has moved kernels' instruction streams before).  Internal to csrc/: an anonymous namespace, so each
// translation unit has its own copy and the kernels keep their names.
#ifndef SQ_DEVICE_UTIL_H
#define SQ_DEVICE_UTIL_H
#include <hip/hip_runtime.h>

#include <cstdint>

// Explicit global address space: a pointer that comes out of a struct is generic to the compiler and would become flat_*.
#define SQ_GLOBAL __attribute__((address_space(1)))

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
// 16 bytes, and two neighbouring elements, in one load at the alignment of one element: the compiler is told so and picks the
// instruction
typedef u32x4 span_of_u16 __attribute__((aligned(2)));
typedef u32x4 span_of_u8 __attribute__((aligned(1)));
typedef uint32_t pair_of_u16 __attribute__((aligned(2)));
typedef uint16_t pair_of_u8 __attribute__((aligned(1)));

// s_waitcnt lgkmcnt(0) by the wave that has just written (or added into) LDS, in front of a barrier.  A barrier only orders what
// has completed, and the compiler (ROCm 7.2) does not always put the wait in front of it: in the work-queue walk of
// fuse_device.h the barrier at the top of the loop is reached round the back edge straight after thread 0's ds_write, so the
// other waves could read the slot before the write landed, i.e. the (queue, index) of two chunks ago: they repeated an old chunk
// (harmless) and skipped their share of the new one.  Found in round 3 as 28 ... 508 unwritten voxels in 1-2 % of the launches of
// the per-plane feather kernel on a small plan (tools/queue_stress.py; the plane-group kernels never showed it in thousands of
// launches, but their code had the same gap); a no-return ds_add in front of a barrier was later seen without the wait too.
// 0xc07f is the s_waitcnt immediate of the gfx9 family (vmcnt [3:0] + [15:14], expcnt [6:4], lgkmcnt [11:8]): lgkmcnt(0) with
// vmcnt / expcnt at their maxima.  gfx10+ lay the fields out differently -- there the same bits would wait on something else and
// the race would be back, silently -- so a device pass for anything but gfx9 stops here (tools/barrier_scan.py, run by
// tests/test_isa_cpu.py, checks the listing of the build that ships).
__device__ __forceinline__ void lds_written() {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__GFX9__)
#error "lds_written(): the s_waitcnt immediate below is the gfx9 encoding; re-derive it for this target"
#endif
    __builtin_amdgcn_s_waitcnt(0xc07f);
}

}   // namespace

#endif

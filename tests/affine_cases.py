"""The planes, shapes and parameter sets the channel-affine tests share (tests/test_channel_affine_cpu.py,
tests/test_channel_affine_gpu.py).  The planes are those of shift_cases."""
import functools

import affine_ref
import shift_cases

DTYPES = shift_cases.DTYPES
PLANE_NAMES = shift_cases.PLANE_NAMES
planes = shift_cases.planes

# The kernel's own sizes (csrc/affine.hip): a thread owns one 16-byte vector of dst columns of one row (VEC = 8 uint16 / 16
# uint8); its fast path reads a span of VEC + 2 source columns, the last two moved into the row where they would lie beyond it (so
# it exists from a width of VEC on, and without a moved pair from VEC + 2 on); a workgroup of 256 threads is tx vectors wide (a
# power of two up to TX_MAX = 128: strips of 1024 uint16 / 2048 uint8 columns) and 256 / tx rows tall (2 at full width); a thread
# walks over WALK = 16 planes with one map.  No LDS.
THREADS, TX_MAX, WALK = 256, 128, 16
VEC = {'uint8': 16, 'uint16': 8}
SPAN = {dt: v + 2 for dt, v in VEC.items()}
STRIP = {dt: TX_MAX * v for dt, v in VEC.items()}
ROWS = THREADS // TX_MAX

MIXED = shift_cases.MIXED
ZERO = (0, 0, 0, 0)
_ALONE = tuple((((0, 0), tuple(sign * 50000 if i == k else 0 for i in range(4)))) for k in range(4) for sign in (1, -1))
# (S; A): S in 1/256 pixel, A = (Ayy, Ayx, Axy, Axx) in parts per million
PARAMS = (
    ((0, 0), ZERO),                                            # the identity
    (MIXED, ZERO),                                             # a shift alone: sq_shift_tiles' result
    ((0, 0), (-152, 17452, -17452, -152)),                     # rotation by 1 degree
    ((77, -200), (2994, -3501, 3501, 2994)),                   # rotation by -0.2 degree with +0.3 %, and a shift
) + _ALONE + (                                                 # each coefficient alone at +50000 and at -50000
    ((0, 0), (50000, 0, 0, -50000)),                           # stretched along y, squeezed along x
    ((16384, 16384), (50000,) * 4),                            # the range's ends, all signs equal
    ((-16384, -16384), (-50000,) * 4),
)


@functools.lru_cache(maxsize=None)
def shapes(dtype):
    vec, span, strip = VEC[dtype], SPAN[dtype], STRIP[dtype]
    return ((1, 1), (1, 300), (300, 1), (2, 2), (37, 53), (71, 143),           # one pixel; one row; one column; odd x odd
            (5, vec - 1), (5, vec), (5, vec + 1),                              # one short of, exactly and one past a vector
            (5, span - 1), (5, span), (5, span + 1),                           # ... a span: the first width whose pair is not moved
            (5, 2 * vec + 1), (7, 3 * vec + 2),                                # two and three vectors, the last one short
            (127, 11), (128, 11), (129, 11), (255, 3), (256, 3), (257, 3),     # ... a workgroup's rows, two vectors and one wide
            (ROWS + 1, strip - 1), (ROWS + 1, strip), (ROWS + 1, strip + 1))   # ... a workgroup's strip; two rows of workgroups


SMALL = ((1, 1), (1, 300), (300, 1), (2, 2), (37, 53), (71, 143))      # the shapes the Python loop runs on
MANY = (131, 21, WALK + 1)      # (h, w, planes) of the table tests: two rows of workgroups, one plane more than a walk


@functools.lru_cache(maxsize=None)
def reference(dtype, h, w, s, a, n=None):
    out = affine_ref.affine_image(planes(dtype, h, w, n), s, a)
    out.setflags(write=False)
    return out

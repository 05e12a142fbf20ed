"""Flatfield estimate on the device (csrc/basic.hip) against its CPU definition (oracle/basic_oracle.py) and a planted
gain.  Parity with the reference's basicpy call is UNPINNED (the package is absent offline); what is tested is that
the device runs the algorithm the oracle defines, and that the algorithm does its job.

Everything goes through sq_basic_fit as it is (no per-kernel entry point): the inputs are chosen so that one stage
decides the result -- one image at smoothness 0 is the three resampling kernels and nothing else; 1, 2, 79, 80 images
are the median's and the re-weighting's edges; padded tiles and pointer tables are the row kernel's addressing."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

from image_stitcher_amd import native, synth
from oracle import basic_oracle as B
from test_basic_oracle_cpu import planted_stack

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.mark.parametrize('n,h,w,dtype', [(40, 256, 320, 'uint16'), (12, 96, 200, 'uint8'), (33, 2048, 2048, 'uint16')])
def test_device_fit_matches_the_definition_and_the_planted_gain(n, h, w, dtype):
    import torch
    # a sparse foreground is BaSiC's premise: a handful of blobs on the small tiles (30 would cover a fifth of them)
    stack, gain = planted_stack(n, h, w, seed=n + h, objects=6 if h < 128 else 30 * max(1, (h * w) // (256 * 320)) if h > 256 else 30)
    if dtype == 'uint8':
        stack = (stack >> 6).astype(np.uint8)
    flat_dev, info = native.basic_fit(torch.from_numpy(stack).to(_dev()))
    flat = flat_dev.cpu().numpy()
    want, winfo = B.basic_fit(stack)
    assert flat.shape == (h, w) and flat.dtype == np.float32 and info['working_size'] == 128
    # same algorithm: float32 with different summation orders, a few hundred iterations -> 2e-3
    assert np.abs(flat / want - 1.0).max() < 2e-3, (np.abs(flat / want - 1.0).max(), info, winfo['ladmap_iterations'])
    assert abs(info['ladmap_iterations'] - sum(winfo['ladmap_iterations'])) <= 2 * len(winfo['ladmap_iterations'])
    err = np.abs(flat / flat.mean() / gain - 1.0)
    if h == 256:      # the planted gain, where the blobs survive the resampling to 128 x 128 as sparse foreground
        assert err.mean() < 2e-3 and np.quantile(err, 0.999) < 1e-2, (err.mean(), err.max())
    else:
        assert err.mean() < 1e-2, err.mean()


def test_resampling_kernels_equal_the_definition():
    """One 'image' of every pixel value pattern: the device resize (down to 128 x 128 and back up) follows
    oracle.resize to float32 rounding -- checked through a fit of a single-image stack whose gain is the image."""
    import torch
    rng = np.random.default_rng(1)
    img = (2000 + 1000 * synth.synthetic_flatfield(300, 517, np.float32)).astype(np.uint16)
    stack = np.stack([img, img, img])
    flat, _ = native.basic_fit(torch.from_numpy(stack).to(_dev()))
    want, _ = B.basic_fit(stack)
    assert np.abs(flat.cpu().numpy() / want - 1.0).max() < 1e-3


# ---- inputs at the edges, through sq_basic_fit as it is ------------------------------------------------------------
# The resampling round trip.  One image with smoothness_flatfield = 0: the median is the image, the DCT shrink has
# threshold 0, the definition settles after 1 iteration in each of 2 rounds, and the result is
#     up(down(img) / mean(down(img)))
# -- the three resampling kernels (and the DCT there and back, twice) and nothing else.  The error is normalised by the
# reference's maximum: the DCT round trip's error is absolute, so on noise the per-pixel relative error reaches 1e-3.
ROUNDTRIP_SHAPES = [(1, 1), (1, 300), (2, 3), (64, 96), (127, 129), (128, 128), (129, 127), (255, 257), (256, 512),
                    (300, 517), (96, 2048), (1000, 130), (2047, 2049)]
ROUNDTRIP_INFO = {'reweight_iterations': 2, 'ladmap_iterations': 2, 'working_size': 128, 'capped_rounds': 0}
# TOL_ROUNDTRIP = 8 x the float32 DEFINITION's worst error against the float64 reference below over exactly these cases
# (13 shapes x uint16 / uint8, roundtrip_image): 1.82e-6, at 2047 x 2049 uint8 -- measured with oracle.basic_fit on
# the CPU, not with the device.  The factor 8 covers the device's other summation order (banded fmaf, four 128-term
# products in each DCT round trip) and nothing more: a tap dropped or shifted by one costs at least 1e-3 here.
# The device's own worst error over the same cases: 1.78e-6 (at 2047 x 2049 uint8; constant images: 2.4e-7).
TOL_ROUNDTRIP = 8 * 1.82e-6


def resize_matrix64(n_out, n_in):
    """oracle.resize_matrix's formula, kept in float64."""
    scale = n_in / n_out
    width = max(scale, 1.0)
    d = np.abs((np.arange(n_out) + 0.5)[:, None] * scale - (np.arange(n_in) + 0.5)[None, :]) / width
    w = np.maximum(0.0, 1.0 - d)
    return w / w.sum(axis=1, keepdims=True)


def roundtrip_reference(img):
    """float64: down to 128 x 128, divide by the mean, back up."""
    h, w = img.shape
    d = resize_matrix64(128, h) @ img.astype(np.float64) @ resize_matrix64(128, w).T
    d = d / d.mean()
    return resize_matrix64(h, 128) @ d @ resize_matrix64(w, 128).T


def roundtrip_image(h, w, dtype):
    """Random noise over 1 .. the dtype's maximum.  No pixel is 0: at 128 x 128 nothing is averaged, a zero pixel is a
    zero gain (-6e-7 after the DCT round trip), and sq_basic_fit refuses gains that are not > 0 (SQ_ERR_NUMERIC)."""
    top = int(np.iinfo(dtype).max)
    return np.random.default_rng(1000 * h + w).integers(1, top + 1, (h, w)).astype(dtype)


def roundtrip_error(flat, img):
    ref = roundtrip_reference(img)
    return float(np.abs(flat.astype(np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize('dtype', ['uint16', 'uint8'])
@pytest.mark.parametrize('h,w', ROUNDTRIP_SHAPES)
def test_resampling_round_trip_of_one_image_equals_its_float64_formula(h, w, dtype):
    """Sizes below 128 on one or both axes, 128 itself, one off it, multiples and non-multiples of 128, 16-fold
    shrinking, both pixel types."""
    import torch
    img = roundtrip_image(h, w, dtype)
    flat, info = native.basic_fit(torch.from_numpy(img[None]).to(_dev()), smoothness_flatfield=0.0)
    flat = flat.cpu().numpy()
    err = roundtrip_error(flat, img)
    print(f'round trip {h}x{w} {dtype}: normalised error {err:.3g} (bound {TOL_ROUNDTRIP:.3g}), {info}')
    assert flat.shape == (h, w) and flat.dtype == np.float32
    assert err <= TOL_ROUNDTRIP, (err, TOL_ROUNDTRIP)
    assert info == ROUNDTRIP_INFO


@pytest.mark.parametrize('h,w', [(37, 41), (300, 517)])
@pytest.mark.parametrize('value,dtype', [(1, 'uint8'), (255, 'uint8'), (1, 'uint16'), (255, 'uint16'), (65535, 'uint16')])
def test_a_constant_image_gives_unit_gains(value, dtype, h, w):
    """Every resampling row sums to 1, at the borders too: a constant stays a constant, whatever its level."""
    import torch
    img = np.full((1, h, w), value, dtype=dtype)
    flat, info = native.basic_fit(torch.from_numpy(img).to(_dev()), smoothness_flatfield=0.0)
    err = float(np.abs(flat.cpu().numpy().astype(np.float64) - 1.0).max())
    print(f'constant {value} {dtype} {h}x{w}: error {err:.3g}, {info}')
    assert err <= TOL_ROUNDTRIP, err
    assert info == ROUNDTRIP_INFO


@functools.lru_cache(maxsize=None)
def planted(n, h, w, seed, objects):
    stack, _ = planted_stack(n, h, w, seed=seed, objects=objects)
    stack.setflags(write=False)
    return stack


@pytest.fixture(scope='module')
def definition():
    """oracle.basic_fit of a planted stack, computed once per module (80 images cost about 2 s of CPU)."""
    @functools.lru_cache(maxsize=None)
    def fit(n, h, w, seed, objects, smoothness=1.0):
        want, winfo = B.basic_fit(planted(n, h, w, seed, objects), smoothness_flatfield=smoothness)
        want.setflags(write=False)
        return want, tuple(winfo['ladmap_iterations'])
    return fit


@pytest.fixture(scope='module')
def device_fit():
    """native.basic_fit of a planted stack on the default stream, once per module: (gains on the host, info)."""
    @functools.lru_cache(maxsize=None)
    def fit(n, h, w, seed, objects, smoothness=1.0):
        import torch
        flat, info = native.basic_fit(torch.from_numpy(np.array(planted(n, h, w, seed, objects))).to(_dev()), smoothness_flatfield=smoothness)
        flat = flat.cpu().numpy()
        flat.setflags(write=False)
        return flat, info
    return fit


def assert_same_fit(flat, info, want, rounds):
    """The module's rule for 'the same algorithm': gains to 2e-3 (float32, other summation orders, a few hundred
    iterations), the same number of re-weighting rounds, iteration counts within 2 per round, no round at the cap."""
    err = float(np.abs(flat / want - 1.0).max())
    print(f'gain error {err:.3g}, device {info}, definition {rounds}')
    assert flat.shape == want.shape and flat.dtype == np.float32
    assert err < 2e-3, (err, info, rounds)
    assert info['reweight_iterations'] == len(rounds), (info, rounds)
    assert abs(info['ladmap_iterations'] - sum(rounds)) <= 2 * len(rounds), (info, rounds)
    assert info['capped_rounds'] == 0 and info['working_size'] == 128


@pytest.mark.parametrize('n,h,w', [(1, 128, 128), (2, 128, 128), (3, 128, 128), (4, 128, 128), (79, 128, 128), (80, 128, 128),
                                   (1, 150, 97), (2, 150, 97), (5, 150, 97)])
def test_image_counts_at_the_edges(n, h, w, definition, device_fit):
    """One image, the even-count median (2, 4, 80), the odd one (3, 79), the full private array of median_kernel and
    the b[tid] update of the re-weighting at 80, a 6400-block Gram launch; planted stacks, which are well conditioned
    (float32 and float64 definitions agree to 4.1e-6 on them; random noise is not: 7.5e-4)."""
    flat, info = device_fit(n, h, w, n, 6)
    want, rounds = definition(n, h, w, n, 6)
    assert_same_fit(flat, info, want, rounds)


def test_two_images_of_unequal_brightness_need_the_even_count_median():
    """The median only starts the solve, and on stacks of even brightness a wrong start heals within the tolerance:
    median_kernel taking v[n / 2] for an even n passes every case above.  Two images whose levels differ 8-fold do
    not forgive it: the definition started from the upper of the two ends 8.2e-3 away from the definition proper,
    whose float32 and float64 evaluations agree to 2.8e-6 on this stack (and on the rounds: 19, 19)."""
    import torch
    stack = np.array(planted(2, 128, 128, 2, 6))
    stack[1] = np.minimum(stack[1].astype(np.int64) * 8, 65535).astype(np.uint16)
    flat, info = native.basic_fit(torch.from_numpy(stack).to(_dev()))
    want, winfo = B.basic_fit(stack)
    assert_same_fit(flat.cpu().numpy(), info, want, tuple(winfo['ladmap_iterations']))


@pytest.mark.parametrize('smoothness', [0.0, 0.1, 10.0])
def test_smoothness_weights_other_than_one(smoothness, definition, device_fit):
    """The DCT shrink threshold smoothness / (eta mu): none, a tenth of and ten times the one the stitcher asks for."""
    flat, info = device_fit(12, 160, 200, 7, 8, smoothness)
    want, rounds = definition(12, 160, 200, 7, 8, smoothness)
    assert_same_fit(flat, info, want, rounds)


def fit_through_the_c_abi(tile_ptrs, tile_base, tile_stride, n, h, w, pitch, sq_dtype, smoothness=1.0, workspace_short=0,
                          workspace_shift=0, stream=None):
    """sq_basic_fit called directly: (status, gains on the host or None, info dict, sq_last_error)."""
    import torch
    L = native.lib()
    need = int(L.sq_basic_workspace_bytes(min(n, 80), h, w))
    assert need > 0, L.sq_last_error()
    ws = torch.empty(need + 256, dtype=torch.uint8, device=_dev())
    out = torch.full((h, w), -7.0, dtype=torch.float32, device=_dev())
    info = native._BasicInfo()
    status = L.sq_basic_fit(tile_ptrs, tile_base, tile_stride, n, h, w, pitch, sq_dtype, float(smoothness), out.data_ptr(),
                            ws.data_ptr() + workspace_shift, need - workspace_short, C.byref(info), native._stream_ptr(stream))
    torch.cuda.synchronize()
    message = L.sq_last_error().decode()
    out = out.cpu().numpy()
    if status != 0:
        assert (out == -7.0).all()          # a refused or failed call leaves the gains unwritten
    return status, out, {k: getattr(info, k) for k, _ in native._BasicInfo._fields_}, message


def small_stack(dtype):
    """5 x 150 x 97 (a width that is no multiple of 64), in the order 4 3 2 1 0 2: one image twice."""
    stack = planted(5, 150, 97, 5, 6)
    if dtype == 'uint8':
        stack = np.minimum(stack // 28, 255).astype(np.uint8)       # background about 110 counts, bright blobs saturate
    order = [4, 3, 2, 1, 0, 2]
    return stack, order


@pytest.mark.parametrize('dtype', ['uint16', 'uint8'])
def test_padded_tiles_and_pointer_tables_through_the_c_abi(dtype):
    """tile_pitch > tile_w with tile_stride in elements, and tile_base_dev = NULL with a device table of pointers to
    separately allocated tiles (reversed, one listed twice) -- the Python binding passes neither.  Both equal the
    dense fit of the same images in the same order; the padding holds the dtype's maximum, so one read of it would
    move the result by far more than the tolerance."""
    import torch
    stack, order = small_stack(dtype)
    n, (h, w), pad = len(order), stack.shape[1:], 5
    sq_dtype, top = native.sq_dtype_of(stack.dtype), np.iinfo(stack.dtype).max
    dense = np.ascontiguousarray(stack[order])
    want, winfo = native.basic_fit(torch.from_numpy(dense).to(_dev()))
    want = want.cpu().numpy()
    assert winfo['capped_rounds'] == 0 and 1 < winfo['reweight_iterations'] < 10

    def same(got, info, what):
        err = float(np.abs(got / want - 1.0).max())
        print(f'{what} {dtype}: {err:.3g} against the dense fit, {info}')
        assert err < 2e-3, (what, err)
        assert info == winfo, (what, info, winfo)

    padded = np.full((n, h, w + pad), top, dtype=stack.dtype)
    padded[:, :, :w] = dense
    d_padded = torch.from_numpy(padded).to(_dev())
    status, got, info, message = fit_through_the_c_abi(None, d_padded.data_ptr(), h * (w + pad), n, h, w, w + pad, sq_dtype)
    assert status == 0, message
    same(got, info, 'padded')

    singles = [torch.from_numpy(np.array(stack[i])).to(_dev()) for i in range(len(stack))]
    table = native.pointer_table([singles[i] for i in order], _dev())
    status, got, info, message = fit_through_the_c_abi(table.data_ptr(), None, 0, n, h, w, w, sq_dtype)
    assert status == 0, message
    same(got, info, 'pointer table')


def test_fit_on_a_stream_of_its_own(device_fit):
    """Uploads, kernels and the polling copies all go to the caller's stream: the fit of a stack uploaded on a
    non-default stream (no synchronisation in between) equals the default-stream fit."""
    import torch
    want, winfo = device_fit(5, 150, 97, 5, 6)
    stream = torch.cuda.Stream()
    pinned = torch.from_numpy(np.array(planted(5, 150, 97, 5, 6))).pin_memory()
    with torch.cuda.stream(stream):
        stack = pinned.to(_dev(), non_blocking=True)
        flat, info = native.basic_fit(stack, stream=stream)
    stream.synchronize()
    err = float(np.abs(flat.cpu().numpy() / want - 1.0).max())
    print(f'own stream: {err:.3g} against the default stream, {info}')
    assert err < 2e-3 and info == winfo and info['capped_rounds'] == 0


# ---- fits that fail -------------------------------------------------------------------------------------------------
def fit_accounts_for_its_iterations(info):
    """A round counted in capped_rounds ran 500 iterations, any other 1..499."""
    rounds, capped, total = info['reweight_iterations'], info['capped_rounds'], info['ladmap_iterations']
    return 0 <= capped <= rounds <= 10 and 500 * capped + (rounds - capped) <= total <= 500 * capped + 499 * (rounds - capped)


def test_a_smoothness_that_removes_the_flatfield_is_an_error_not_nan_gains():
    """smoothness 1e6 shrinks every DCT coefficient of S to exactly zero and 0 / 0 follows: SQ_ERR_NUMERIC with a
    message that says so and the gains left unwritten (before the check: SQ_OK and NaN gains).  The first round
    settles at S = 0 (fmaxf(NaN, 0) is 0 on the device, so b = 0 and R = I; numpy's maximum keeps the NaN and the
    definition runs all 10 rounds to the cap), the 9 NaN rounds after it cannot settle."""
    import torch
    stack = torch.from_numpy(np.array(planted(12, 160, 200, 7, 8))).to(_dev())
    t0 = time.perf_counter()
    with pytest.raises(native.NativeError, match=r'no usable flatfield: 16384 of 16384 gains.*not finite.*[1-9] of 10 re-weighting rounds stopped at the cap') as e:
        native.basic_fit(stack, smoothness_flatfield=1e6)
    print(f'{time.perf_counter() - t0:.2f} s: {e.value}')
    assert e.value.status == native.SQ_ERR_NUMERIC == -5
    status, _, info, message = fit_through_the_c_abi(None, stack.data_ptr(), 160 * 200, 12, 160, 200, 200, native.SQ_U16, smoothness=1e6)
    assert status == -5 and 'no usable flatfield' in message           # (the helper checks that the gains stay unwritten)
    assert info['reweight_iterations'] == 10 and info['capped_rounds'] >= 1 and fit_accounts_for_its_iterations(info), info


def test_a_dim_stack_fails_loudly_or_gives_positive_gains_and_says_how_many_rounds_hit_the_cap():
    """Background of about 10 counts: the DEFINITION does not settle here (every round at the 500-iteration cap, gains
    down to -2.9 in float32) and such runs are chaotic -- float32 and float64 disagree by orders of magnitude -- so no
    value is compared.  Either the call refuses (SQ_ERR_NUMERIC) or the gains are finite and > 0 and ``capped_rounds``
    accounts for the iterations: a capped round ran 500, any other 1..499.  (Measured on the device: gains of 0.40
    and up, all 10 rounds at the cap, 5000 iterations in 1.6 s.)"""
    import torch
    dim = (planted(4, 128, 128, 4, 6) // 300).astype(np.uint16)
    t0 = time.perf_counter()
    try:
        flat, info = native.basic_fit(torch.from_numpy(dim).to(_dev()))
    except native.NativeError as e:
        print(f'{time.perf_counter() - t0:.2f} s: {e}')
        assert e.status == native.SQ_ERR_NUMERIC and 'no usable flatfield' in str(e)
        return
    print(f'{time.perf_counter() - t0:.2f} s: {info}')
    flat = flat.cpu().numpy()
    assert np.isfinite(flat).all() and flat.min() > 0.0, flat.min()
    assert fit_accounts_for_its_iterations(info), info


def test_bad_arguments(device_fit):
    import torch
    with pytest.raises(native.NativeError, match=r'81 images.*1\.\.80'):
        native.basic_fit(torch.zeros((81, 32, 32), dtype=torch.uint16, device=_dev()))
    flat80, info80 = device_fit(80, 128, 128, 80, 6)            # 80 are taken (test_image_counts_at_the_edges checks the values)
    assert flat80.shape == (128, 128) and np.isfinite(flat80).all() and info80['capped_rounds'] == 0
    with pytest.raises(native.NativeError, match='all zero'):
        native.basic_fit(torch.zeros((4, 32, 32), dtype=torch.uint16, device=_dev()))
    with pytest.raises(ValueError):
        native.basic_fit(torch.zeros((4, 32, 32), dtype=torch.uint16))
    # what the binding cannot express, straight through the C ABI; every refusal leaves the gains unwritten
    h, w = 150, 97
    stack = torch.from_numpy(np.array(planted(5, h, w, 5, 6))).to(_dev())
    many = torch.zeros((81, 32, 40), dtype=torch.uint16, device=_dev())
    status, _, _, message = fit_through_the_c_abi(None, many.data_ptr(), 32 * 40, 81, 32, 40, 40, native.SQ_U16)
    assert status == native.SQ_ERR_INVALID and '1..80' in message          # sq_basic_fit's own limit, not the workspace query's
    for bad in (-1.0, -1e-30, float('nan')):
        with pytest.raises(native.NativeError, match='smoothness_flatfield'):
            native.basic_fit(stack, smoothness_flatfield=bad)
    status, _, _, message = fit_through_the_c_abi(None, stack.data_ptr(), h * w, 5, h, w, w - 1, native.SQ_U16)
    assert status == native.SQ_ERR_INVALID and f'pitch {w - 1}' in message
    status, _, _, message = fit_through_the_c_abi(None, stack.data_ptr(), h * w, 5, h, w, w, native.SQ_U16, workspace_short=1)
    assert status == native.SQ_ERR_WORKSPACE == -4 and 'workspace' in message
    status, _, _, message = fit_through_the_c_abi(None, stack.data_ptr(), h * w, 5, h, w, w, native.SQ_U16, workspace_shift=16)
    assert status == native.SQ_ERR_INVALID and 'aligned' in message
    status, got, info, message = fit_through_the_c_abi(None, stack.data_ptr(), h * w, 5, h, w, w, native.SQ_U16)
    want, winfo = device_fit(5, h, w, 5, 6)
    assert status == 0 and np.abs(got / want - 1.0).max() < 2e-3 and info == winfo, message     # the same call, unbroken

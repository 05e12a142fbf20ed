"""Harness and case table of tests/test_streams_gpu.py: every device entry point of image_stitcher_amd.native run off the
default stream, behind a backlog, and held to the references the suite already has.

The product never runs on the default stream of an idle device (the ingest chain of stitcher.py runs inside
``with torch.cuda.stream(...)``, registration on a side stream between two events, the plan and pointer tables over
``native._copy_stream``), so a wrapper that allocates, clears or launches on another stream than the one it was given
corrupts pixels only now and then.  Two experiments make that deterministic:

E1  "waits for its stream".  The inputs hold a poison pattern, the outputs a canary.  On S: ``lag``, then the real inputs
    are copied in.  A probe on O, enqueued right after, must still read the poison in full (the lag was running when the
    call began).  Then the entry point is called -- mode A inside ``with torch.cuda.stream(S)`` without ``stream=``, mode B
    with ``stream=S`` while the default stream is current -- and the outputs, read through S, must be the reference's for
    the real inputs.  Work that went to another stream ran at once, on the poison.
E2  "touches no other stream" (mode B).  S is idle, O is lagged with an event recorded behind the lag and is the current
    stream.  The outputs read through S must be the reference's while O's event is still pending, and again after O has
    drained: a zero-fill that went to O lands late and wipes them.

``lag`` is one ``torch.cuda._sleep`` kernel: a single wave that spins on the clock for a fixed number of ticks and ends by
itself; nothing waits for a flag.  The ticks per millisecond are measured once per module (``Streams.open``), so LAG_MS is
a time, not a tick count.

Measured on the MI355X (host side, ``time.perf_counter`` around the call of E2, where nothing blocks): the longest call of
the table is ``fuse_planes`` with a fresh plan, whose table upload it waits for, at 0.5 ms (0.65 ms the slowest run seen);
most calls take 0.03 ... 0.4 ms.  Ten times that is 6.5 ms, so the floor of 20 ms decides; LAG_MS = 50 leaves the host a
hundred times the longest call, and a lag asked to last 100 ms was measured at 98.7 ms (the sleep kernel's clock makes
2.37 million ticks per millisecond).  The probes are asserted, so a lag that turns out too short on a busy host fails the case
loudly instead of passing it.

Nothing here needs a device at import: the inputs and references are numpy."""
import contextlib
import time

import numpy as np

import blosc_ref
import composite_ref
import despeckle_ref
import dpc_ref
import focus_guide_ref
import focus_ref
import register_cases as R
import tile_qc_ref
import tophat_ref
from image_stitcher_amd import native, registration, synth
from oracle import stitch_oracle as O

LAG_MS = 50.0
MAX_DRAWS = 32
SENTINEL_POISON = 0x5EED


# ---------------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------------

class Streams:
    """The pair (S, O) of independent torch streams, the copy stream and the default stream of the device, and the lag."""

    def __init__(self, dev, ticks_per_ms):
        import torch
        self.dev = dev
        self.ticks_per_ms = ticks_per_ms
        self.default = torch.cuda.default_stream(dev)
        self.copy = native._copy_stream(dev)
        self.S = self.O = None
        self.draws = 0
        self.lag_ms_seen = None
        self._probe = torch.zeros(256, dtype=torch.int32, device=dev)

    def lag(self, stream, ms=LAG_MS):
        """Bounded device work on `stream`: one kernel that spins for `ms` milliseconds of the device clock."""
        import torch
        with torch.cuda.stream(stream):
            torch.cuda._sleep(int(ms * self.ticks_per_ms))

    def progresses_while_lagged(self, lagged, other):
        """`other` finishes a small kernel while `lagged` is still inside its lag."""
        import torch
        self.lag(lagged)
        behind = torch.cuda.Event()
        behind.record(lagged)
        with torch.cuda.stream(other):
            self._probe.add_(1)
        done = torch.cuda.Event()
        done.record(other)
        done.synchronize()
        ok = not behind.query()
        lagged.synchronize()
        return ok

    def independent(self, a, b):
        return self.progresses_while_lagged(a, b) and self.progresses_while_lagged(b, a)

    @classmethod
    def open(cls, dev):
        """Measure the sleep kernel's clock, then draw torch streams until two of them are independent of each other, of
        the copy stream and of the default stream (streams that share a hardware queue serialise, which would hide every
        race).  Returns the Streams; ``S`` is None when no pair was found among MAX_DRAWS draws."""
        import torch
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ticks = 2_000_000
        torch.cuda._sleep(1000)      # loads the kernel
        t0.record()
        torch.cuda._sleep(ticks)
        t1.record()
        t1.synchronize()
        st = cls(dev, ticks / t0.elapsed_time(t1))
        t0.record()
        st.lag(st.default)
        t1.record()
        t1.synchronize()
        st.lag_ms_seen = t0.elapsed_time(t1)
        good = []
        for _ in range(MAX_DRAWS):
            s = torch.cuda.Stream(device=dev)
            st.draws += 1
            if not (st.independent(s, st.copy) and st.independent(s, st.default)):
                continue
            for g in good:
                if st.independent(g, s):
                    st.S, st.O = g, s
                    return st
            good.append(s)
        return st


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------

class Case:
    """One entry point at one shape.

    real, poison: {name: numpy array}, the device inputs (same shapes and dtypes; both are valid inputs).
    canary:       {name: numpy array}, the caller-made outputs and what they hold before the call.
    prepare(dev): -> ctx, whatever the call needs beside them (plans, constant tables); made once, on the default stream.
    call(ctx, inp, out, stream): runs the entry point(s) with ``stream=stream`` on the device tensors `inp` and `out`;
                  returns {name: device tensor, or a function that returns a numpy array}.
    fresh():      optional; -> what the call gets in place of ctx, made anew for every experiment before its lag begins and kept
                  until the experiment has drained (a plan whose first use lies inside the experiment).
    finish(host): optional, {name: numpy} as read back -> {name: numpy} as compared (a decoder).
    reference(inputs, strict): {name: expected}; strict is False for the poison (no conditions on the inputs are checked).
    compare(name, got, want): None or a message; equality unless given.  as_got(name, want): a reference value in the form
                  of a result (for comparing two references)."""

    def __init__(self, name, real, poison, canary, call, reference, prepare=None, finish=None, compare=None, as_got=None,
                 fresh=None):
        self.name, self.real, self.poison, self.canary = name, real, poison, canary
        self.call, self.reference = call, reference
        self.prepare = prepare or (lambda dev: None)
        self.fresh = fresh
        self.finish = finish or (lambda host: host)
        self.compare = compare or equal
        self.as_got = as_got or (lambda name, want: want)
        assert set(real) == set(poison)
        for k in real:
            assert real[k].shape == poison[k].shape and real[k].dtype == poison[k].dtype, k

    def mismatch(self, got, want):
        """None when every output is the reference's, else the first message."""
        for k in want:
            msg = self.compare(k, got[k], want[k])
            if msg:
                return f'{self.name}: {msg}'
        return None


def equal(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f'{name}: {got.dtype}{got.shape}, the reference has {want.dtype}{want.shape}'
    bad = np.flatnonzero(got.ravel() != want.ravel())
    if bad.size:
        i = int(bad[0])
        return f'{name}: {bad.size} of {got.size} values differ, the first at {i}: read {got.ravel()[i]}, the reference has {want.ravel()[i]}'
    return None


def host_conditions(case):
    """The reference's outputs for the real inputs, after the two conditions that need no device: they differ from its outputs
    for the poison and from the canary."""
    want = case.reference(case.real, True)
    want_poison = case.reference(case.poison, False)
    for k in want:
        # (a case without device inputs, the tile generator, has no poison: E1 then rests on the sentinel and the canary)
        assert not case.real or case.compare(k, case.as_got(k, want_poison[k]), want[k]) is not None, \
            f'{case.name}: the reference gives the same {k} for the poison as for the real inputs'
        if k in case.canary:
            assert case.compare(k, case.canary[k], want[k]) is not None, f'{case.name}: {k} of the reference is the canary'
    return want


class Prepared:
    """A case on the device: its ctx, the reference's outputs (computed once, never modified) and the conditions that make
    a pass mean something -- checked on the host; then one call on the default stream, which loads the code objects, caches
    the plan table and has to give the reference's outputs too."""

    def __init__(self, case, st):
        import torch
        self.case = case
        self.want = host_conditions(case)
        self.ctx = case.prepare(st.dev)
        inp, out = to_device(case.real, st.dev), to_device(case.canary, st.dev)
        torch.cuda.synchronize()
        res = case.call(self.ctx if case.fresh is None else case.fresh(), inp, out, None)
        got = case.finish(read(res, st.default))
        torch.cuda.synchronize()
        msg = case.mismatch(got, self.want)
        assert msg is None, f'on the default stream of an idle device already: {msg}'


def to_device(arrays, dev):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v).copy()).to(dev) for k, v in arrays.items()}


def read(res, stream):
    """The outputs to the host through `stream`, then `stream.synchronize()`."""
    import torch
    host = {}
    with torch.cuda.stream(stream):
        for k, v in res.items():
            host[k] = v() if callable(v) else v.cpu().numpy()
    stream.synchronize()
    return host


class E1Result:
    def __init__(self, mismatch, probe_full):
        self.mismatch, self.probe_full = mismatch, probe_full


class E2Result:
    def __init__(self, first, after, event_pending, host_ms):
        self.first, self.after, self.event_pending, self.host_ms = first, after, event_pending, host_ms


def experiment_e1(case, ctx, want, st, mode):
    """E1 of the module docstring; mode 'A' or 'B'."""
    import torch
    assert mode in ('A', 'B')
    inp, real_dev, out = to_device(case.poison, st.dev), to_device(case.real, st.dev), to_device(case.canary, st.dev)
    sentinel = torch.full((1024,), SENTINEL_POISON, dtype=torch.int32, device=st.dev)
    sentinel_real = torch.zeros(1024, dtype=torch.int32, device=st.dev)
    probes = {k: torch.empty_like(v) for k, v in inp.items()}
    sentinel_probe = torch.empty_like(sentinel)
    ctx = ctx if case.fresh is None else case.fresh()
    torch.cuda.synchronize()
    st.lag(st.S)
    with torch.cuda.stream(st.S):
        for k in inp:
            inp[k].copy_(real_dev[k])
        sentinel.copy_(sentinel_real)
    with torch.cuda.stream(st.O):
        for k in inp:
            probes[k].copy_(inp[k])
        sentinel_probe.copy_(sentinel)
    if mode == 'A':
        with torch.cuda.stream(st.S):
            res = case.call(ctx, inp, out, None)
    else:
        res = case.call(ctx, inp, out, st.S)
    got = case.finish(read(res, st.S))
    st.O.synchronize()
    probe_full = bool((sentinel_probe.cpu() == SENTINEL_POISON).all()) and \
        all(equal(k, probes[k].cpu().numpy(), case.poison[k]) is None for k in inp)
    torch.cuda.synchronize()
    return E1Result(case.mismatch(got, want), probe_full)


def experiment_e2(case, ctx, want, st):
    """E2 of the module docstring."""
    import torch
    inp, out = to_device(case.real, st.dev), to_device(case.canary, st.dev)
    ctx = ctx if case.fresh is None else case.fresh()
    torch.cuda.synchronize()
    st.lag(st.O)
    behind = torch.cuda.Event()
    behind.record(st.O)
    with torch.cuda.stream(st.O):
        t0 = time.perf_counter()
        res = case.call(ctx, inp, out, st.S)
        host_ms = (time.perf_counter() - t0) * 1e3
    host = read(res, st.S)
    pending = not behind.query()
    first = case.mismatch(case.finish(host), want)
    st.O.synchronize()
    after = case.mismatch(case.finish(read(res, st.S)), want)
    torch.cuda.synchronize()
    return E2Result(first, after, pending, host_ms)


# ---------------------------------------------------------------------------------------------------------------------
# the harness's own two cases: misplaced work it has to report (no product code)
# ---------------------------------------------------------------------------------------------------------------------

def selftest_copy_on_the_other_stream(st):
    """``out.copy_(inp)`` issued on O whatever stream it was given: E1 has to read the poison's copy."""
    import torch
    rng = np.random.default_rng(1)
    real, poison = rng.integers(1, 1000, 4096).astype(np.int32), np.full(4096, -77, np.int32)

    def call(ctx, inp, out, stream):
        with torch.cuda.stream(st.O):
            out['y'].copy_(inp['x'])
        return {'y': out['y']}
    return Case('selftest-copy-on-O', {'x': real}, {'x': poison}, {'y': np.zeros(4096, np.int32)}, call,
                lambda a, strict: {'y': a['x']})


def selftest_zero_fill_on_the_current_stream(st):
    """``hist.zero_()`` on the current stream (the lagged O of E2), then the counts added on the stream given: E2 has to find
    them wiped once O has drained."""
    import torch
    rng = np.random.default_rng(2)
    real, poison = rng.integers(1, 1000, 4096).astype(np.int64), np.full(4096, -77, np.int64)

    def call(ctx, inp, out, stream):
        out['hist'].zero_()
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            out['hist'].add_(inp['x'])
        return {'hist': out['hist']}
    return Case('selftest-zero-fill-on-current', {'x': real}, {'x': poison}, {'hist': np.zeros(4096, np.int64)}, call,
                lambda a, strict: {'hist': a['x']})


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------

CASES = []


def add(*args, **kw):
    CASES.append(Case(*args, **kw))


def _pixels(seed, shape, dtype, lo=None, hi=None):
    top = int(np.iinfo(dtype).max)
    return np.random.default_rng(seed).integers(0 if lo is None else lo, (top if hi is None else hi) + 1, shape).astype(dtype)


# ---- fusion: 6 tiles of 48 x 64 on a 150 x 190 canvas, 3 planes, float32 gains ----------------------------------------
TH, TW, CH, CW, NT, NP = 48, 64, 150, 190, 6, 3
_rng = np.random.default_rng(21)
RECTS = np.array([(0, 0, TH, TW, int(y), int(x)) for y, x in zip(_rng.integers(0, CH - 30, NT), _rng.integers(0, CW - 30, NT))])
Z_LEVELS = [0, 1, 2]
RADIUS = 3


def _fuse_inputs(seed):
    rng = np.random.default_rng(seed)
    a = {'tiles': rng.integers(0, 65536, (NP, NT, TH, TW)).astype(np.uint16)}
    for p in range(NP):
        a[f'flat{p}'] = (0.6 + 0.8 * rng.random((TH, TW))).astype(np.float32)
    return a


def _flats(a):
    return [a[f'flat{p}'] for p in range(NP)]


def _fuse_reference(mode, dtype):
    def reference(a, strict):
        if mode == native.SQ_FUSE_OVERWRITE:
            planes = [O.fuse_plane_overwrite(list(a['tiles'][p]), RECTS, CH, CW, a[f'flat{p}']) for p in range(NP)]
        else:
            planes = [O.fuse_plane_feather(list(a['tiles'][p]), RECTS, CH, CW, a[f'flat{p}'], out_dtype=np.dtype(dtype).type)
                      for p in range(NP)]
        return {'canvas': np.stack(planes)}
    return reference


def _plan(mode=native.SQ_FUSE_OVERWRITE, expand=False):
    return native.FusePlan(RECTS, TH, TW, CH, CW, mode, expand_on_device=expand)


def _fuse_call(flags=0, ptrs=False):
    def call(plan, inp, out, stream):
        kw = {}
        tiles = inp['tiles']
        if ptrs:
            flat = tiles.reshape(-1, TH, TW)
            kw['tile_ptrs'] = native.pointer_table([flat[i] for i in range(flat.shape[0])], tiles.device)
            tiles = None
        native.fuse_planes(plan, tiles, out['canvas'], _flats(inp), stream=stream, flags=flags, **kw)
        return {'canvas': out['canvas']}
    return call


def _canvas_canary(dtype):
    return {'canvas': np.full((NP, CH, CW), 7, dtype)}


for _name, _kw in (('fuse-overwrite', {}), ('fuse-overwrite-queues', dict(flags=native.SQ_FUSE_FORCE_QUEUES)),
                   ('fuse-overwrite-pointer-table', dict(ptrs=True))):
    add(_name, _fuse_inputs(30), _fuse_inputs(31), _canvas_canary(np.uint16), _fuse_call(**_kw),
        _fuse_reference(native.SQ_FUSE_OVERWRITE, np.uint16), prepare=lambda dev: _plan())
# FusePlan.device_table: a plan made for the experiment, whose table goes to the device (uploaded, or expanded there) at its
# first use inside it.  The plan is made before the lag begins and dropped after the device has drained: making and dropping a
# plan are not the entry point under test, and a plan's page-locked table that goes back to the driver (hipHostFree, once the
# library's pool of four slabs is full) waits for every stream of the device.
add('fuse-fresh-plan-host-table', _fuse_inputs(30), _fuse_inputs(31), _canvas_canary(np.uint16), _fuse_call(),
    _fuse_reference(native.SQ_FUSE_OVERWRITE, np.uint16), fresh=lambda: _plan(expand=False))
add('fuse-fresh-plan-device-expanded', _fuse_inputs(30), _fuse_inputs(31), _canvas_canary(np.uint16),
    _fuse_call(flags=native.SQ_FUSE_FORCE_QUEUES), _fuse_reference(native.SQ_FUSE_OVERWRITE, np.uint16),
    fresh=lambda: _plan(expand=True))
add('fuse-feather', _fuse_inputs(32), _fuse_inputs(33), _canvas_canary(np.float32), _fuse_call(),
    _fuse_reference(native.SQ_FUSE_FEATHER, np.float32), prepare=lambda dev: _plan(native.SQ_FUSE_FEATHER))


# ---- projections over 3 z levels of the same geometry -------------------------------------------------------------------
def _fused_stack(a):
    return np.stack([O.fuse_plane_overwrite(list(a['tiles'][p]), RECTS, CH, CW, a[f'flat{p}']) for p in range(NP)])


def _max_call(split):
    def call(plan, inp, out, stream):
        t, f = inp['tiles'], _flats(inp)
        if split:      # the channel's planes in two calls on the stream, the second one accumulating
            native.fuse_project_max(plan, t[:2], out['out'], f[:2], stream=stream)
            native.fuse_project_max(plan, t[2:], out['out'], f[2:], accumulate=True, stream=stream)
        else:
            native.fuse_project_max(plan, t, out['out'], f, stream=stream)
        return {'out': out['out']}
    return call


def _focus_call(split):
    def call(plan, inp, out, stream):
        t = inp['tiles']
        if split:
            native.fuse_project_focus(plan, t[:2], out['out'], out['key'], Z_LEVELS[:2], RADIUS, stream=stream)
            native.fuse_project_focus(plan, t[2:], out['out'], out['key'], Z_LEVELS[2:], RADIUS, accumulate=True, stream=stream)
        else:
            native.fuse_project_focus(plan, t, out['out'], out['key'], Z_LEVELS, RADIUS, stream=stream)
        return {'out': out['out'], 'key': out['key']}
    return call


def _focus_reference(a, strict):
    out, key = focus_ref.focus_reference([(a['tiles'], RECTS, None, Z_LEVELS)], CH, CW, RADIUS)
    return {'out': out, 'key': key.view(np.int64)}


def _tiles_only(seed):
    return {'tiles': _fuse_inputs(seed)['tiles']}


_PLANE_CANARY = {'out': np.full((CH, CW), 7, np.uint16)}
_FOCUS_CANARY = {'out': np.full((CH, CW), 7, np.uint16), 'key': np.full((CH, CW), 7, np.int64)}
for _split in (False, True):
    _tag = '-accumulate' if _split else ''
    add('project-max' + _tag, _fuse_inputs(34), _fuse_inputs(35), _PLANE_CANARY, _max_call(_split),
        lambda a, strict: {'out': _fused_stack(a).max(0)}, prepare=lambda dev: _plan())
    add('project-focus' + _tag, _tiles_only(36), _tiles_only(37), _FOCUS_CANARY, _focus_call(_split), _focus_reference,
        prepare=lambda dev: _plan())


def _guide_depth(seed):
    """The unsigned depth plane (z* + 1, 0 = uncovered) of a guide channel: what focus_depth_plane hands to the followers."""
    _, key = focus_ref.focus_reference([(_fuse_inputs(seed)['tiles'], RECTS, None, Z_LEVELS)], CH, CW, RADIUS)
    return key.view(np.int64), focus_guide_ref.unsigned_depth(focus_ref.depth_of(key), len(Z_LEVELS))


def _depth_plane_call(ctx, inp, out, stream):
    native.focus_depth_plane(inp['key'], out=out['depth'], stream=stream)
    return {'depth': out['depth']}


add('focus-depth-plane', {'key': _guide_depth(38)[0]}, {'key': _guide_depth(39)[0]}, {'depth': np.full((CH, CW), 200, np.uint8)},
    _depth_plane_call,
    lambda a, strict: {'depth': focus_guide_ref.unsigned_depth(focus_ref.depth_of(a['key'].view(np.uint64)), len(Z_LEVELS))})


def _select_call(split):
    def call(plan, inp, out, stream):
        t, f = inp['tiles'], _flats(inp)
        if split:
            native.fuse_select_depth(plan, t[:2], out['out'], inp['depth'], Z_LEVELS[:2], f[:2], stream=stream)
            native.fuse_select_depth(plan, t[2:], out['out'], inp['depth'], Z_LEVELS[2:], f[2:], accumulate=True, stream=stream)
        else:
            native.fuse_select_depth(plan, t, out['out'], inp['depth'], Z_LEVELS, f, stream=stream)
        return {'out': out['out']}
    return call


def _select_reference(a, strict):
    return {'out': focus_guide_ref.select_by_depth(_fused_stack(a), a['depth'].astype(np.int64) - 1)}


for _split in (False, True):
    add('select-depth' + ('-accumulate' if _split else ''), dict(_fuse_inputs(40), depth=_guide_depth(38)[1]),
        dict(_fuse_inputs(41), depth=_guide_depth(39)[1]), _PLANE_CANARY, _select_call(_split), _select_reference,
        prepare=lambda dev: _plan())


# ---- min-max and normalisation: 5 x 37 x 61 uint16 -----------------------------------------------------------------------
def _minmax_call(ctx, inp, out, stream):
    return {'minmax': native.tile_minmax(inp['tiles'], stream=stream)}


def _normalize_call(ctx, inp, out, stream):
    return {'tiles': native.normalize_tiles(inp['tiles'], stream=stream)}


_MM = ({'tiles': _pixels(50, (5, 37, 61), np.uint16, 900, 41000)}, {'tiles': _pixels(51, (5, 37, 61), np.uint16, 300, 52000)})
add('tile-minmax', _MM[0], _MM[1], {}, _minmax_call,
    lambda a, strict: {'minmax': np.stack([a['tiles'].min((1, 2)), a['tiles'].max((1, 2))], 1).astype(np.int32)})
add('normalize-tiles', _MM[0], _MM[1], {}, _normalize_call,
    lambda a, strict: {'tiles': np.stack([O.normalize_image(t, np.uint16) for t in a['tiles']])})


# ---- registration: 4 pairs of 64 x 64 crops, u = 10, both normalisations ---------------------------------------------
REG_N, REG_U = 64, 10
_REG_REAL = R.batch_inputs(5, 80, 80, REG_N, REG_N, 4, np.uint16, seed=61)
_REG_POISON = R.batch_inputs(5, 80, 80, REG_N, REG_N, 4, np.uint16, seed=62)
REG_PAIRS = _REG_REAL[1]


def _register_call(norm):
    def call(minmax, inp, out, stream):
        pending = native.register_pairs_async(inp['tiles'], minmax, REG_PAIRS, REG_N, REG_N, REG_U,
                                              registration.NORMALIZATIONS[norm], stream=stream)
        return {'results': pending.fetch}
    return call


def _register_reference(norm):
    def reference(a, strict):
        res, scale = np.zeros(len(REG_PAIRS), native.RESULT_DTYPE), np.ones(len(REG_PAIRS))
        for k, p in enumerate(REG_PAIRS):
            ref = a['tiles'][p['ref_tile']][p['ref_y0']:p['ref_y0'] + REG_N, p['ref_x0']:p['ref_x0'] + REG_N]
            mov = a['tiles'][p['mov_tile']][p['mov_y0']:p['mov_y0'] + REG_N, p['mov_x0']:p['mov_x0'] + REG_N]
            if strict:      # with the conditions of register_cases.reference on the crops
                w = R.reference(ref, mov, REG_U, norm)
                d, scale[k] = w['detail'], w['scale']
            else:
                d = O.phase_cross_correlation(ref, mov, REG_U, norm)[3]
            res[k] = (d['coarse'], d['fine'], d['ccmax_re'], d['ccmax_im'], d['src_amp'], d['tgt_amp'])
        return {'results': dict(res=res, scale=scale)}
    return reference


def register_compare(name, got, want):
    """The rule of tests/test_register_numerics_gpu.py: equal integers, ccmax and the amplitudes within register_cases.TOL."""
    res, scale = want['res'], want['scale']
    for k in range(len(res)):
        g, d = got[k], res[k]
        if g['coarse'].tolist() != d['coarse'].tolist() or g['fine'].tolist() != d['fine'].tolist():
            return f'pair {k}: peak {g["coarse"].tolist()} {g["fine"].tolist()}, the reference has {d["coarse"].tolist()} {d["fine"].tolist()}'
        cc = abs(complex(g['ccmax_re'], g['ccmax_im']) - complex(d['ccmax_re'], d['ccmax_im'])) / scale[k]
        amp = max(abs(g['src_amp'] - d['src_amp']) / d['src_amp'], abs(g['tgt_amp'] - d['tgt_amp']) / d['tgt_amp'])
        if not (cc <= R.TOL and amp <= R.TOL):
            return f'pair {k}: ccmax off by {cc:.3e} of its scale, amplitudes by {amp:.3e} (read {g})'
    return None


def _identity_minmax(dev):
    import torch
    return torch.from_numpy(R.identity_minmax(5)).to(dev)


for _norm in (None, 'phase'):
    add(f'register-pairs-{_norm or "none"}', {'tiles': _REG_REAL[0]}, {'tiles': _REG_POISON[0]}, {}, _register_call(_norm),
        _register_reference(_norm), prepare=_identity_minmax, compare=register_compare, as_got=lambda name, want: want['res'])


# ---- overlap moments: 9 windows on 5 tiles of 96 x 130 -------------------------------------------------------------------
MOM_WINDOWS = np.array([(0, 1, 0, 0, 0, 0, 96, 130), (1, 2, 0, 0, 89, 69, 7, 61), (2, 3, 95, 129, 0, 0, 1, 1), (3, 4, 5, 7, 11, 3, 80, 120),
                        (4, 0, 0, 100, 0, 0, 96, 30), (0, 2, 70, 0, 0, 0, 26, 130), (1, 3, 3, 1, 2, 5, 33, 77), (2, 4, 0, 0, 0, 0, 0, 0),
                        (3, 3, 10, 10, 20, 20, 50, 50)], dtype=np.int32)


def _moments_reference(a, strict):
    out = np.zeros((len(MOM_WINDOWS), 5), dtype=np.int64)
    for i, (rt, mt, ry, rx, my, mx, h, w) in enumerate(MOM_WINDOWS):
        p = a['tiles'][rt, ry:ry + h, rx:rx + w].astype(np.int64)
        q = a['tiles'][mt, my:my + h, mx:mx + w].astype(np.int64)
        out[i] = (p.sum(), q.sum(), (p * p).sum(), (q * q).sum(), (p * q).sum())
    return {'moments': out}


def _moments_call(ctx, inp, out, stream):
    native.pair_overlap_moments(inp['tiles'], MOM_WINDOWS, out=out['moments'], stream=stream)
    return {'moments': out['moments']}


add('pair-overlap-moments', {'tiles': _pixels(70, (5, 96, 130), np.uint16)}, {'tiles': _pixels(71, (5, 96, 130), np.uint16)},
    {'moments': np.full((len(MOM_WINDOWS), 5), -3, np.int64)}, _moments_call, _moments_reference)


# ---- planes of 3 x 71 x 130: pyramids, histograms, block means, composite --------------------------------------------
PH, PW = 71, 130
_PLANES = ({'planes': _pixels(80, (3, PH, PW), np.uint16)}, {'planes': _pixels(81, (3, PH, PW), np.uint16)})


def _mean_level(a):
    h, w = a.shape[-2] // 2 * 2, a.shape[-1] // 2 * 2
    s = a[..., 0:h:2, 0:w:2].astype(np.uint32) + a[..., 0:h:2, 1:w:2] + a[..., 1:h:2, 0:w:2] + a[..., 1:h:2, 1:w:2]
    return (s >> 2).astype(a.dtype)


def _pyramid_mean_reference(a, strict):
    lv, out = a['planes'], {}
    for k in range(1, 4):
        lv = _mean_level(lv)
        out[f'level{k}'] = lv
    return out


def _downsample_call(ctx, inp, out, stream):
    native.downsample2(inp['planes'], out=out['level1'], stream=stream)
    return {'level1': out['level1']}


def _pyramid_mean_call(ctx, inp, out, stream):
    native.pyramid_mean(inp['planes'], 3, out=[out[f'level{k}'] for k in (1, 2, 3)], stream=stream)
    return {f'level{k}': out[f'level{k}'] for k in (1, 2, 3)}


add('downsample2', _PLANES[0], _PLANES[1], {'level1': np.full((3, PH // 2, PW // 2), 7, np.uint16)}, _downsample_call,
    lambda a, strict: {'level1': O.pyramid_nearest(a['planes'], 2)[1]})
add('pyramid-mean', _PLANES[0], _PLANES[1], {f'level{k}': np.full((3, PH >> k, PW >> k), 7, np.uint16) for k in (1, 2, 3)},
    _pyramid_mean_call, _pyramid_mean_reference)

HIST_ROWS = [0, 1, 0]
HIST_EARLIER = np.random.default_rng(82).integers(0, 9, (2, 65536)).astype(np.int64)


def _histogram_reference(earlier):
    def reference(a, strict):
        hist = np.zeros((2, 65536), np.int64) if earlier is None else earlier.copy()
        for p, r in zip(a['planes'], HIST_ROWS):
            hist[r] += np.bincount(p.ravel(), minlength=65536)
        return {'hist': hist}
    return reference


def _histogram_call(given):
    def call(ctx, inp, out, stream):
        if given:
            return {'hist': native.histogram_planes(inp['planes'], HIST_ROWS, hist=out['hist'], stream=stream)}
        return {'hist': native.histogram_planes(inp['planes'], HIST_ROWS, n_rows=2, stream=stream)}
    return call


add('histogram-planes-hist-none', _PLANES[0], _PLANES[1], {}, _histogram_call(False), _histogram_reference(None))
add('histogram-planes-earlier-counts', _PLANES[0], _PLANES[1], {'hist': HIST_EARLIER}, _histogram_call(True),
    _histogram_reference(HIST_EARLIER))

BLOCK_K = 2
COMPOSITE_WINDOWS, COMPOSITE_COLORS = [(1000, 60000), (0, 65535), (20000, 30000)], [0xFF0000, 0x00FF80, 0x4040FF]


def _block_mean_call(ctx, inp, out, stream):
    native.block_mean(inp['planes'], BLOCK_K, out=out['means'], stream=stream)
    return {'means': out['means']}


def _composite_call(ctx, inp, out, stream):
    native.composite_render(inp['planes'], COMPOSITE_WINDOWS, COMPOSITE_COLORS, out=out['rgb'], stream=stream)
    return {'rgb': out['rgb']}


add('block-mean', _PLANES[0], _PLANES[1], {'means': np.full((3, -(-PH // 4), -(-PW // 4)), 7, np.uint16)}, _block_mean_call,
    lambda a, strict: {'means': composite_ref.block_mean(a['planes'], BLOCK_K)})
add('composite-render', _PLANES[0], _PLANES[1], {'rgb': np.full((PH, PW, 3), 7, np.uint8)}, _composite_call,
    lambda a, strict: {'rgb': composite_ref.render(a['planes'], COMPOSITE_WINDOWS, COMPOSITE_COLORS)})


# ---- the tile filters: 4 x 96 x 200, uint16 and uint8 ----------------------------------------------------------------
FH, FW = 96, 200
DESPECKLE_T = {np.uint16: 20000, np.uint8: 80}
DESPECKLE_EARLIER = np.array([5, 0, 11, 2], np.int64)


def _tophat_call(ctx, inp, out, stream):      # in place
    return {'tiles': native.tophat_tiles(inp['tiles'], RADIUS, stream=stream)}


def _despeckle_call(t):
    def call(ctx, inp, out, stream):
        native.despeckle_tiles(inp['tiles'], t, 'hot', out=out['out'], counts=out['counts'], stream=stream)
        return {'out': out['out'], 'counts': out['counts']}
    return call


def _despeckle_reference(t):
    def reference(a, strict):
        out, fired = despeckle_ref.despeckle(a['tiles'], t, 'hot')
        return {'out': out, 'counts': DESPECKLE_EARLIER + fired.sum((1, 2))}
    return reference


def _tile_stats_call(ctx, inp, out, stream):
    native.tile_stats(inp['tiles'], out=out['words'], stream=stream)
    return {'words': out['words']}


def _dpc_call(ctx, inp, out, stream):
    native.dpc_tiles(inp['left'], inp['right'], 2, out=out['dpc'], stream=stream)
    return {'dpc': out['dpc']}


for _dt in (np.uint16, np.uint8):
    _n = np.dtype(_dt).name
    _real, _poison = {'tiles': _pixels(90, (4, FH, FW), _dt)}, {'tiles': _pixels(91, (4, FH, FW), _dt)}
    add(f'tophat-tiles-{_n}', _real, _poison, {}, _tophat_call, lambda a, strict: {'tiles': tophat_ref.tophat(a['tiles'], RADIUS)})
    add(f'despeckle-tiles-{_n}', _real, _poison, {'out': np.full((4, FH, FW), 7, _dt), 'counts': DESPECKLE_EARLIER},
        _despeckle_call(DESPECKLE_T[_dt]), _despeckle_reference(DESPECKLE_T[_dt]))
    add(f'tile-stats-{_n}', _real, _poison, {'words': np.full((4, 8), -3, np.int64)}, _tile_stats_call,
        lambda a, strict: {'words': tile_qc_ref.words_of(a['tiles'])})
    add(f'dpc-tiles-{_n}', {'left': _pixels(92, (4, FH, FW), _dt), 'right': _pixels(93, (4, FH, FW), _dt)},
        {'left': _pixels(94, (4, FH, FW), _dt), 'right': _pixels(95, (4, FH, FW), _dt)}, {'dpc': np.full((4, FH, FW), 7, _dt)},
        _dpc_call, lambda a, strict: {'dpc': dpc_ref.dpc_image(a['left'], a['right'], 2)})


# ---- Blosc frames: 2 x 100 x 130 in 64 x 64 chunks --------------------------------------------------------------------
BH, BW, BC = 100, 130, 64


def _blosc_planes(seed):
    return {'planes': np.stack([synth.scene_patch(seed + p, 0, 0, BH, BW) for p in range(2)]).astype(np.uint16)}


def _blosc_call(ctx, inp, out, stream):
    buf = native.blosc_encode_planes(inp['planes'], BC, BC, stream=stream)
    return {'offsets': buf.offsets, 'frames': buf.out, 'status': buf.status}


def _blosc_chunks(planes):
    ny, nx = -(-BH // BC), -(-BW // BC)
    chunks = np.zeros((len(planes), ny, nx, BC, BC), planes.dtype)
    for iy in range(ny):
        for ix in range(nx):
            part = planes[:, iy * BC:(iy + 1) * BC, ix * BC:(ix + 1) * BC]
            chunks[:, iy, ix, :part.shape[1], :part.shape[2]] = part
    return chunks.reshape(-1, BC, BC)


def _blosc_finish(host):
    """The frames decoded with tests/blosc_ref.py (an empty frame stands for a chunk of zeros)."""
    off, frames = host['offsets'], host['frames']
    chunks = np.zeros((len(off) - 1, BC, BC), np.uint16)
    for i in range(len(off) - 1):
        frame = frames[off[i]:off[i + 1]].tobytes()
        if frame:
            chunks[i] = np.frombuffer(blosc_ref.blosc_decompress(frame), np.uint16).reshape(BC, BC)
    assert int(host['status'][0]) == 0, f"the encoder's status word is {host['status']}"
    return {'chunks': chunks}


add('blosc-encode-planes', _blosc_planes(100), _blosc_planes(110), {}, _blosc_call,
    lambda a, strict: {'chunks': _blosc_chunks(a['planes'])}, finish=_blosc_finish)


# ---- the tile generator: 4 tiles of 64 x 64 against synth.py (its descriptors are host memory: nothing to poison) ----
SYNTH_DESC = np.zeros(4, dtype=native.SYNTH_DTYPE)
for _i in range(4):
    SYNTH_DESC[_i] = (1234 + _i, 99 + _i, 17 * _i - 20, 40 - 23 * _i)
SYNTH_NOISE = 200


def _synth_call(ctx, inp, out, stream):
    native.synth_tiles(SYNTH_DESC, 64, 64, SYNTH_NOISE, np.uint16, out['tiles'].device, out=out['tiles'], stream=stream)
    return {'tiles': out['tiles']}


def _synth_reference(a, strict):
    return {'tiles': np.stack([(synth.scene_patch(int(d['scene_seed']), int(d['oy']), int(d['ox']), 64, 64)
                                + synth.noise_patch(int(d['noise_seed']), 64, 64, SYNTH_NOISE)).astype(np.uint16) for d in SYNTH_DESC])}


add('synth-tiles', {}, {}, {'tiles': np.full((4, 64, 64), 7, np.uint16)}, _synth_call, _synth_reference)

CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

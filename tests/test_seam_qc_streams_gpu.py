"""native.seam_stats off the default stream, through the harness of tests/stream_cases.py (imported, not edited): behind a
backlog on the stream it is given (E1, named both ways) and beside a backlog on another stream (E2).  The zero-fill of the words,
the kernel and the wrapper's allocations all have to be on the caller's stream; the pair table travels on the copy stream."""
import numpy as np
import pytest

import seam_qc_ref
import stream_cases as SC
from image_stitcher_amd import native

pytestmark = pytest.mark.gpu

M, N, H, W, RADIUS = 2, 4, 48, 80, 2
# full overlap (two 32-row pieces), a side-by-side seam, one above the other with a negative dx, a corner
PAIRS = np.array([[0, 1, 2, 2, 2, 2, H - 4, W - 4], [1, 2, 2, 66, 2, 2, H - 4, 10], [3, 2, 42, 2, 2, 7, 2, W - 9],
                  [0, 3, 40, 70, 2, 2, 4, 6]], dtype=np.int32)


def _call(ctx, inp, out, stream):
    native.seam_stats(inp['tiles'], PAIRS, RADIUS, out=out['words'], stream=stream)
    return {'words': out['words']}


def _case(dtype):
    top = int(np.iinfo(dtype).max)
    real = {'tiles': np.random.default_rng(190).integers(0, top + 1, (M, N, H, W)).astype(dtype)}
    poison = {'tiles': np.random.default_rng(191).integers(0, top + 1, (M, N, H, W)).astype(dtype)}
    canary = {'words': np.full((M, len(PAIRS), native.seam_words(RADIUS)), -3, np.int64)}
    return SC.Case(f'seam-stats-{np.dtype(dtype).name}', real, poison, canary, _call,
                   lambda a, strict: {'words': seam_qc_ref.words_of(a['tiles'], PAIRS, RADIUS)})


CASES = {c.name: c for c in (_case(np.uint16), _case(np.uint8))}


@pytest.fixture(scope='module')
def streams():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    st = SC.Streams.open(torch.device('cuda:0'))
    if st.S is None:
        pytest.fail(f'no two of {SC.MAX_DRAWS} torch streams make progress while the other, the copy stream or the default '
                    'stream is lagged: they share hardware queues, and every stream race would stay hidden')
    assert st.lag_ms_seen >= 0.9 * SC.LAG_MS, f'the lag lasts {st.lag_ms_seen} ms, not {SC.LAG_MS}'
    return st


@pytest.fixture(scope='module')
def prepared(streams):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = SC.Prepared(CASES[name], streams)
        return cache[name]
    return get


@pytest.mark.parametrize('mode', ['A', 'B'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_waits_for_its_stream(streams, prepared, name, mode):
    p = prepared(name)
    r = SC.experiment_e1(p.case, p.ctx, p.want, streams, mode)
    assert r.probe_full, f'{name}: the probe did not read the poison in full: the lag had ended when the call began'
    assert r.mismatch is None, f'E1-{mode} {r.mismatch}'


@pytest.mark.parametrize('name', sorted(CASES))
def test_touches_no_other_stream(streams, prepared, name):
    p = prepared(name)
    r = SC.experiment_e2(p.case, p.ctx, p.want, streams)
    assert r.event_pending, (f"{name}: the other stream's event was complete when the outputs had been read (the call took "
                             f'{r.host_ms:.2f} ms on the host): the call waited for that stream, or its lag is too short')
    assert r.first is None, f'E2, the other stream still lagged: {r.first}'
    assert r.after is None, f'E2, after the other stream has drained: {r.after}'

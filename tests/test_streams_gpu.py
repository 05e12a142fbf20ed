"""Every device entry point of image_stitcher_amd.native off the default stream: behind a backlog on the stream it is given
(E1, named both ways: as the current stream and as ``stream=``) and beside a backlog on another stream (E2), against the
references the suite already has.  tests/stream_cases.py holds the harness, its conditions and the table; every test prints
which of the conditions it met (pytest -s shows them).  The harness is itself put to the test first: misplaced work that it
has to report."""
import pytest

import stream_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def streams():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    st = SC.Streams.open(torch.device('cuda:0'))
    print(f'streams: the sleep kernel makes {st.ticks_per_ms:.0f} ticks per ms, a lag of {SC.LAG_MS} ms took {st.lag_ms_seen:.1f} ms; '
          f'{st.draws} streams drawn')
    if st.S is None:
        pytest.fail(f'no two of {SC.MAX_DRAWS} torch streams make progress while the other, the copy stream or the default '
                    'stream is lagged: they share hardware queues, and every stream race would stay hidden')
    assert st.lag_ms_seen >= 0.9 * SC.LAG_MS, f'the lag lasts {st.lag_ms_seen} ms, not {SC.LAG_MS}'
    return st


@pytest.fixture(scope='module')
def prepared(streams):
    """name -> stream_cases.Prepared, made at a case's first test and shared by its others."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = SC.Prepared(SC.CASE_BY_NAME[name], streams)
        return cache[name]
    return get


def test_harness_reports_work_on_the_wrong_stream(streams):
    case = SC.selftest_copy_on_the_other_stream(streams)
    want = case.reference(case.real, True)
    for mode in ('A', 'B'):
        r = SC.experiment_e1(case, None, want, streams, mode)
        assert r.probe_full, 'the probe did not read the poison in full: the lag had ended when the call began'
        assert r.mismatch is not None and 'read -77' in r.mismatch, r.mismatch
        print(f'streams selftest E1-{mode}: probe read the poison in full; reported "{r.mismatch}"')


def test_harness_reports_a_zero_fill_on_another_stream(streams):
    case = SC.selftest_zero_fill_on_the_current_stream(streams)
    want = case.reference(case.real, True)
    r = SC.experiment_e2(case, None, want, streams)
    assert r.event_pending, "the other stream's event was complete when the outputs had been read: its lag is too short"
    assert r.first is None, r.first
    assert r.after is not None and 'read 0' in r.after, r.after
    print(f'streams selftest E2: the event was pending at the first read, which matched; after the drain reported "{r.after}"')


NAMES = [c.name for c in SC.CASES]


@pytest.mark.parametrize('mode', ['A', 'B'])
@pytest.mark.parametrize('name', NAMES)
def test_waits_for_its_stream(streams, prepared, name, mode):
    p = prepared(name)
    r = SC.experiment_e1(p.case, p.ctx, p.want, streams, mode)
    assert r.probe_full, f'{name}: the probe did not read the poison in full: the lag had ended when the call began'
    assert r.mismatch is None, f'E1-{mode} {r.mismatch}'
    print(f'streams {name} E1-{mode}: probe read the poison in full; outputs are the reference\'s for the real inputs, '
          'which differ from the canary and from its outputs for the poison')


@pytest.mark.parametrize('name', NAMES)
def test_touches_no_other_stream(streams, prepared, name):
    p = prepared(name)
    r = SC.experiment_e2(p.case, p.ctx, p.want, streams)
    assert r.event_pending, (f"{name}: the other stream's event was complete when the outputs had been read (the call took "
                             f'{r.host_ms:.2f} ms on the host): the call waited for that stream, or its lag is too short')
    assert r.first is None, f'E2, the other stream still lagged: {r.first}'
    assert r.after is None, f'E2, after the other stream has drained: {r.after}'
    print(f'streams {name} E2: call took {r.host_ms:.2f} ms on the host; the event behind the other stream\'s lag was pending '
          'when the outputs had been read; outputs are the reference\'s then and after that stream has drained')

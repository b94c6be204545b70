"""Every launching entry point on a side stream behind the gate of tests/stream_gate.py: outputs are ordered after prior
work on the stream that is current at the call, whichever stream the object was made under, and no call waits on the
host (include/wurm_hip.h: "Nothing is allocated, freed or synchronised here: each call enqueues kernels on `stream`").
The cases are in tests/stream_cases.py; tests/test_stream_inventory.py checks on the CPU that none is missing."""
import pytest
import torch

from tests import stream_cases, stream_gate
from tests.stream_gate import Case, GateFailure

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


# ------------------------------------------------------------------ the helper itself (torch operations only)

def _fake(call):
    return Case('fake', lambda: {'out': torch.zeros(64, device=DEV)}, call,
                lambda: (torch.arange(64., device=DEV),), lambda: (torch.arange(64., device=DEV) * 3 + 1,), ('none',), min_launches=0)


def test_gate_is_calibrated():
    cycles, ms = stream_gate.calibrate()
    print(f'stream gate: {cycles} cycles = {ms:.1f} ms')
    assert ms >= stream_gate.GATE_MS and cycles <= 2 ** 40


def test_a_launch_on_the_default_stream_is_reported():
    """also the premise on this machine: work on the default stream overtakes the gated side stream (then the copy ran on
    A: a mismatch); if the two shared a hardware queue the gate would be found open — reported all the same"""
    def call(x, inputs):
        with torch.cuda.stream(torch.cuda.default_stream()):
            x['out'].copy_(inputs[0])
        return dict(x)
    with pytest.raises(GateFailure) as err:
        stream_gate.run_case(_fake(call))
    print('reported as:', err.value)
    assert err.value.kind in ('mismatch', 'open')


def test_a_host_synchronisation_is_reported():
    def call(x, inputs):
        x['out'].copy_(inputs[0])
        torch.cuda.current_stream().synchronize()
        return dict(x)
    with pytest.raises(GateFailure) as err:
        stream_gate.run_case(_fake(call))
    assert err.value.kind == 'open'


def test_a_call_on_the_current_stream_passes():
    def call(x, inputs):
        x['out'].copy_(inputs[0])
        return dict(x)
    stream_gate.run_case(_fake(call))


def test_a_case_that_cannot_see_anything_is_reported():
    def call(x, inputs):
        return dict(x)
    with pytest.raises(GateFailure) as err:
        stream_gate.run_case(_fake(call))
    assert err.value.kind == 'blind'


# ------------------------------------------------------------------ the cases

@pytest.mark.parametrize('case', stream_cases.CASES, ids=[c.name for c in stream_cases.CASES])
def test_case(case):
    try:
        stream_gate.run_case(case)
    except RuntimeError as e:
        if 'HIP error' in str(e) or 'illegal memory access' in str(e):   # nothing more is started on a device that faulted
            pytest.exit(f'{case.name}: {e}', returncode=3)
        raise


def _named(name):
    return next(c for c in stream_cases.CASES if c.name == name)


@pytest.mark.parametrize('first,second', [
    ('SingleSnake.rollout route=rollout_s9 S=9', 'SingleSnake.rollout route=generic S=9'),   # (the same knobs)
    ('SingleSnake.rollout route=rollout_s9 S=9', 'abi wurm_single_rollout with both tapes (rollout_s9_injected)'),
    ('SingleSnake.step+reset stepper=c_torchinfo lazy=1 reset_obs=0', 'SingleSnake.step route=lane_step S=9'),
    ('MultiSnake.step + postponed reset, one wave per env', 'MultiSnake.step, one env per workgroup'),
    ('FusedA2CLearner.update gae=0', 'FusedA2CLearner.update gae=1'),
    ('FusedA2CPopulation.update gae=0', 'FusedA2CLearner.update gae=0'),
    ('MultiSnake.policy_window', 'MultiSnake.act_window'),
    ('RolloutStats.update, two chained windows (snake)', 'SingleSnake.policy_rollout narrow (E = 75)'),
])
def test_two_streams_at_once(first, second):
    """two objects gated on two streams, all calls enqueued before either gate opens, completion in the reverse order:
    the entry points keep no state between calls (a static scratch buffer would show here)"""
    stream_gate.run_pair(_named(first), _named(second))

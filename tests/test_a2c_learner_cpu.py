"""The fused A2C learner without a GPU: the parameter re-homing of FusedA2CLearner, what the Python layer and the C ABI
refuse, the workspace query, and the float64 reference of tests/a2c_learner_ref.py against plain torch autograd of the
example's own expression — which pins the reference to the formula before anything on the GPU is compared with it."""
import ctypes

import pytest
import torch

from tests import a2c_learner_ref as ref
from wurm_amd import _lib
from wurm_amd.agents import FeedforwardAgent, pack_policy_params
from wurm_amd.rl import FusedA2CLearner

I64 = ctypes.c_int64
F32 = ctypes.c_float


def test_parameters_move_into_one_buffer():
    torch.manual_seed(0)
    agent = FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=75)
    x = torch.rand(7, 75)
    probs, values = agent(x)
    packed = pack_policy_params(agent)
    learner = FusedA2CLearner(agent)
    p2, v2 = agent(x)
    assert torch.equal(p2, probs) and torch.equal(v2, values)
    assert learner.params.is_contiguous() and learner.params.dtype == torch.float32
    assert torch.equal(learner.params, packed) and torch.equal(pack_policy_params(agent), packed)
    assert learner.step == 0 and learner.exp_avg.shape == packed.shape and not learner.exp_avg_sq.any()
    with torch.no_grad():
        learner.params[0] = 5.0
        learner.params[-1] = -3.0
    sd = agent.state_dict()
    assert sd['feedforward.0.0.weight'][0, 0] == 5.0 and sd['value_head.bias'][0] == -3.0
    agent.load_state_dict({k: v.clone() + 1 for k, v in sd.items()})  # a round trip keeps the views attached
    assert learner.params[0] == 6.0 and learner.params[-1] == -2.0
    assert torch.equal(pack_policy_params(agent), learner.params)
    assert agent.feedforward[0][0].weight.data_ptr() == learner.params.data_ptr()


def test_python_layer_refusals():
    with pytest.raises(NotImplementedError):
        FusedA2CLearner(FeedforwardAgent(num_actions=4, num_layers=3, hidden_units=64, num_inputs=75))
    with pytest.raises(NotImplementedError):
        FusedA2CLearner(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=32, num_inputs=75))
    ok = lambda: FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=75)
    with pytest.raises(NotImplementedError):
        FusedA2CLearner(ok(), use_gae=True)
    with pytest.raises(NotImplementedError):
        FusedA2CLearner(ok(), normalise_returns=True)
    with pytest.raises(NotImplementedError):
        FusedA2CLearner(ok(), value_loss='huber_2')
    learner = FusedA2CLearner(ok())  # CPU tensors: construction works, the kernels do not
    with pytest.raises(_lib.WurmHipError):
        learner.grad(torch.zeros(2, 75), {'observations': torch.zeros(1, 2, 75), 'actions': torch.zeros(1, 2).long(),
                                          'rewards': torch.zeros(1, 2), 'dones': torch.zeros(1, 2).bool()})


def test_c_abi_refusals_without_device():
    lib = _lib.lib()
    N, T, E = 8, 2, 27
    nbytes = lib.wurm_a2c_ff_workspace_bytes(N, T, E)
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)  # a non-null pointer: every call below is refused before anything is read or launched

    def grad(params=p, obs0=p, grad_=p, ws=p, ws_bytes=nbytes, n=N, t=T, e=E, kind=0):
        return lib.wurm_a2c_ff_grad(params, obs0, p, p, p, p, F32(0.99), F32(0.0), kind, grad_, p, None, ws,
                                    I64(ws_bytes), I64(n), I64(t), e, None)

    def update(params=p, m=p, ws_bytes=nbytes, e=E, kind=0, step=1):
        return lib.wurm_a2c_ff_update(params, p, p, p, p, p, F32(0.99), F32(0.0), kind, p, p, None, p, I64(ws_bytes),
                                      I64(N), I64(T), e, m, p, None, I64(step), F32(1e-3), F32(0.9), F32(0.999),
                                      F32(1e-8), F32(0.5), None)

    def apply(params=p, g=p, m=p, step=1, n=1481):
        return lib.wurm_a2c_ff_apply(params, g, m, p, None, I64(step), F32(1e-3), F32(0.9), F32(0.999), F32(1e-8),
                                     F32(0.5), I64(n), None)

    INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED
    assert grad(params=None) == INV and grad(obs0=None) == INV and grad(grad_=None) == INV and grad(ws=None) == INV
    assert grad(n=-1) == INV and grad(t=-2) == INV and grad(n=0) == INV
    assert grad(e=5) == UNS and grad(kind=7) == UNS
    assert grad(ws_bytes=nbytes - 1) == INV and grad(ws_bytes=0) == INV
    assert update(params=None) == INV and update(m=None) == INV and update(step=0) == INV
    assert update(e=5) == UNS and update(kind=7) == UNS and update(ws_bytes=nbytes - 1) == INV
    assert apply(params=None) == INV and apply(g=None) == INV and apply(m=None) == INV
    assert apply(step=0) == INV and apply(n=0) == INV and apply(n=-4) == INV


def test_workspace_query():
    lib = _lib.lib()
    for E in (3, 4, 27, 75, 147, 243, 363, 507):
        sizes = [lib.wurm_a2c_ff_workspace_bytes(n, 5, E) for n in (1, 2, 63, 64, 65, 255, 256, 257, 512, 8192)]
        assert sizes[0] > 0 and sizes == sorted(sizes)
        P = ref.num_params(E)
        assert sizes[0] >= 4 * (P + 3)                       # one partial gradient and the loss sums
        # the partial gradients stop growing at 256 workgroups: past it only the parked rows (32 bytes each) are added
        assert sizes[-1] - sizes[-2] == (8192 - 512) * 6 * 32
    assert lib.wurm_a2c_ff_workspace_bytes(257, 20, 507) < 40 * 2 ** 20
    assert lib.wurm_a2c_ff_workspace_bytes(8, 5, 5) == 0 and lib.wurm_a2c_ff_workspace_bytes(0, 5, 75) == 0


CASES = [(3, 1, 5), (4, 5, 9), (27, 2, 33), (75, 20, 6)]


@pytest.mark.parametrize('E,T,N', CASES)
@pytest.mark.parametrize('value_loss,entropy_coef', [('smooth_l1', 0.01), ('mse', 0.0)])
def test_float64_reference_is_the_examples_expression(E, T, N, value_loss, entropy_coef):
    """spec_float64 (explicit clamp, explicit smooth_l1) == torch fp64 autograd of Categorical / A2C.loss /
    smooth_l1_loss on inputs where no probability comes near a clamp."""
    fx = ref.make_fixture(E, T, N, seed=1, reward_scale=3.0)
    a = ref.spec_float64(fx, entropy_coef, value_loss)
    b = ref.example_loss(fx, torch.float64, 'cpu', entropy_coef, value_loss)
    x = torch.cat([fx['obs0'][None], fx['obs']]).double()
    assert float(ref.forward(ref.split(fx['params'].double(), E), x)[2].min()) > 1e-6  # the clamps do not act
    assert max(ref.block_errors(a['grad'], b['grad'], E).values()) < 1e-12
    assert ref.rel_err(a['losses'], b['losses']) < 1e-12 and ref.rel_err(a['values'], b['values']) < 1e-12


@pytest.mark.parametrize('E,T,N,scale', [(3, 1, 1, 1.0), (4, 5, 63, 3.0), (27, 2, 65, 1.0), (75, 20, 65, 3.0),
                                         (507, 2, 601, 3.0)])
def test_fixture_conditions(E, T, N, scale):
    fx = ref.make_fixture(E, T, N, seed=0, reward_scale=scale)
    assert fx['redrawn'] <= 0.10 and 0.05 <= fx['live'] <= 0.95
    if scale > 1:
        assert 0.05 <= fx['linear_branch'] <= 0.95
    if N >= 2:
        assert bool(fx['dones'][:, 0].all()) and not bool(fx['dones'][:, 1].any())
    assert set(fx['obs'].unique().tolist()) <= {0.0, 1.0} or E == 4
    assert set((fx['rewards'] / scale).unique().tolist()) <= {-1.0, 0.0, 1.0}


def test_sharp_policy_fixture_reaches_both_clamps():
    fx = ref.make_fixture(27, 5, 65, seed=3, wp_scale=30.0)
    s = ref.spec_float64(fx, 0.01)
    assert bool((s['p_action'] < ref.EPS32 / 4).any()) and bool((s['p_action'] > 1 - ref.EPS32 / 4).any())
    plain = ref.spec_float64(fx, 0.01, clamp=False)  # without the clamp those samples have a policy gradient
    assert max(ref.block_errors(plain['grad'], s['grad'], 27).values()) > 1e-3


@pytest.mark.parametrize('text', ['0.9', '0.999', '1e-3', '1e-8', '0.99', '0.5', '3e-4', '0.0'])
def test_hyper_parameters_are_read_as_the_decimal_written(text):
    """wurm_a2c_ff_apply computes 1 - beta and the bias corrections in double from the shortest decimal that rounds to
    the float it was given: for every default of torch.optim.Adam that is the double Python holds for the literal."""
    value = ctypes.c_double(-1.0)
    assert _lib.lib().wurm_a2c_ff_hyper_parameter(F32(float(text)), ctypes.addressof(value)) == _lib.OK
    assert value.value == float(text)
    assert _lib.lib().wurm_a2c_ff_hyper_parameter(F32(float(text)), None) == _lib.ERR_INVALID_ARG


def test_hyper_parameter_without_a_short_decimal_is_kept():
    x = torch.tensor(1 / 3, dtype=torch.float32)  # 0.333333343: nine digits, nothing shorter rounds to it
    value = ctypes.c_double(-1.0)
    assert _lib.lib().wurm_a2c_ff_hyper_parameter(F32(float(x)), ctypes.addressof(value)) == _lib.OK
    assert torch.tensor(value.value, dtype=torch.float32) == x and abs(value.value - float(x)) < 1e-8
    for special in (float('inf'), float('nan')):
        assert _lib.lib().wurm_a2c_ff_hyper_parameter(F32(special), ctypes.addressof(value)) == _lib.OK
        assert value.value == special or value.value != value.value

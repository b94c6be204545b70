"""The fused A2C learner's GAE mode without a GPU: the float64 specification of tests/a2c_gae_ref.py against plain torch
autograd of the reference's own loops (which pins it to the formula before anything on the GPU is compared with it),
what separates it from the n-step specification and what does not, the constructor, and what the two new C entry
points refuse."""
import ctypes

import pytest
import torch

from tests import a2c_gae_ref as gae
from tests import a2c_learner_ref as ref
from tests.test_a2c_learner_cpu import CASES
from wurm_amd import _lib
from wurm_amd.agents import FeedforwardAgent
from wurm_amd.rl import FusedA2CLearner

I64 = ctypes.c_int64
F32 = ctypes.c_float
LAMBDAS = [0.0, 0.5, 0.95, 1.0]


@pytest.mark.parametrize('gae_lambda', LAMBDAS)
@pytest.mark.parametrize('E,T,N', CASES)
@pytest.mark.parametrize('value_loss,entropy_coef', [('smooth_l1', 0.01), ('mse', 0.0)])
def test_float64_reference_is_the_reference_loops(E, T, N, value_loss, entropy_coef, gae_lambda):
    """spec_float64_gae == torch fp64 autograd of Categorical / the loops of a2c.py:50-59 / smooth_l1_loss on inputs where
    no probability comes near a clamp."""
    fx = ref.make_fixture(E, T, N, seed=1, reward_scale=3.0)
    a = gae.spec_float64_gae(fx, gae_lambda, entropy_coef, value_loss)
    b = gae.example_loss_gae(fx, torch.float64, 'cpu', gae_lambda, entropy_coef, value_loss)
    x = torch.cat([fx['obs0'][None], fx['obs']]).double()
    assert float(ref.forward(ref.split(fx['params'].double(), E), x)[2].min()) > 1e-6  # the clamps do not act
    assert max(ref.block_errors(a['grad'], b['grad'], E).values()) < 1e-12
    assert ref.rel_err(a['losses'], b['losses']) < 1e-12 and ref.rel_err(a['values'], b['values']) < 1e-12
    assert ref.rel_err(a['returns'], b['returns']) < 1e-12


@pytest.mark.parametrize('E,T,N', CASES)
@pytest.mark.parametrize('value_loss,entropy_coef', [('smooth_l1', 0.01), ('mse', 0.0)])
def test_lambda_one_is_the_n_step_gradient(E, T, N, value_loss, entropy_coef):
    """At lambda = 1 the values telescope out of R (only the bootstrap is left, which has no gradient): the adjoint's
    extra term vanishes and the gradient is the n-step one."""
    fx = ref.make_fixture(E, T, N, seed=1, reward_scale=3.0)
    a = gae.spec_float64_gae(fx, 1.0, entropy_coef, value_loss)
    b = ref.spec_float64(fx, entropy_coef, value_loss)
    assert max(ref.block_errors(a['grad'], b['grad'], E).values()) < 1e-10
    assert ref.rel_err(a['losses'], b['losses']) < 1e-10


def test_lambda_half_is_another_gradient():
    """The fixture of the GPU test at lambda = 0.5: the value head's gradient is far from the n-step one, so a kernel that
    ignored the switch could not pass there."""
    fx = ref.make_fixture(27, 5, 65, seed=0, reward_scale=3.0)
    a = gae.spec_float64_gae(fx, 0.5, 0.01, 'smooth_l1')
    b = ref.spec_float64(fx, 0.01, 'smooth_l1')
    assert ref.block_errors(a['grad'], b['grad'], 27)['Wv'] > 1e-3


def _agent():
    return FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=75)


def test_constructor():
    learner = FusedA2CLearner(_agent(), gamma=0.99, use_gae=True, gae_lambda=0.95)
    assert learner.use_gae and learner.gae_lambda == 0.95
    assert learner.gamma_lambda == float(torch.tensor(0.99 * 0.95, dtype=torch.float64).float())  # rounded once
    with pytest.raises(NotImplementedError, match='gae_lambda'):
        FusedA2CLearner(_agent(), use_gae=True)
    with pytest.raises(NotImplementedError):
        FusedA2CLearner(_agent(), normalise_returns=True)
    with pytest.raises(NotImplementedError):
        FusedA2CLearner(_agent(), use_gae=True, gae_lambda=0.95, normalise_returns=True)
    plain = FusedA2CLearner(_agent(), use_gae=False, gae_lambda=0.95)  # ignored, as wurm.rl.A2C ignores it
    assert not plain.use_gae and plain.gae_lambda is None
    with pytest.raises(_lib.WurmHipError):  # CPU tensors: construction works, the kernels do not
        learner.grad(torch.zeros(2, 75), {'observations': torch.zeros(1, 2, 75), 'actions': torch.zeros(1, 2).long(),
                                          'rewards': torch.zeros(1, 2), 'dones': torch.zeros(1, 2).bool()})


def test_c_abi_refusals_without_device():
    lib = _lib.lib()
    N, T, E = 8, 2, 27
    nbytes = lib.wurm_a2c_ff_workspace_bytes(N, T, E)
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)  # a non-null pointer: every call below is refused before anything is read or launched

    def grad(params=p, obs0=p, obs=p, actions=p, rewards=p, dones=p, grad_=p, losses=p, ws=p, ws_bytes=nbytes, n=N, t=T,
             e=E, kind=0, gl=0.94, returns=None):
        return lib.wurm_a2c_ff_grad_gae(params, obs0, obs, actions, rewards, dones, F32(0.99), F32(0.0), kind, grad_,
                                        losses, None, ws, I64(ws_bytes), I64(n), I64(t), e, None, F32(gl), returns)

    def update(params=p, m=p, u=p, ws_bytes=nbytes, n=N, t=T, e=E, kind=0, step=1, gl=0.94, returns=None):
        return lib.wurm_a2c_ff_update_gae(params, p, p, p, p, p, F32(0.99), F32(0.0), kind, p, p, None, p,
                                          I64(ws_bytes), I64(n), I64(t), e, m, u, None, I64(step), F32(1e-3), F32(0.9),
                                          F32(0.999), F32(1e-8), F32(0.5), None, F32(gl), returns)

    INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED
    for name in ('params', 'obs0', 'obs', 'actions', 'rewards', 'dones', 'grad_', 'losses', 'ws'):
        assert grad(**{name: None}) == INV, name
    assert grad(n=-1) == INV and grad(n=0) == INV and grad(t=-2) == INV and grad(t=0) == INV
    assert grad(e=5) == UNS and grad(kind=7) == UNS
    assert grad(ws_bytes=nbytes - 1) == INV and grad(ws_bytes=0) == INV
    for bad in (-0.5, float('nan'), float('inf'), -float('inf')):
        assert grad(gl=bad) == INV and update(gl=bad) == INV
        assert grad(gl=bad, returns=p) == INV
    assert update(params=None) == INV and update(m=None) == INV and update(u=None) == INV and update(step=0) == INV
    assert update(n=0) == INV and update(t=0) == INV
    assert update(e=5) == UNS and update(kind=7) == UNS and update(ws_bytes=nbytes - 1) == INV
    # the workspace is the n-step one: GAE parks its extra float in a slot the rows already had
    assert lib.wurm_a2c_ff_workspace_bytes(N, T, E) == nbytes

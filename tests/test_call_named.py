"""CPU checks of `_lib.call_named`: the arguments of an entry point are picked by the parameter names of its prototype in
include/wurm_hip.h, in the header's order.  Against real entry points that answer before any HIP call."""
import numpy as np
import pytest

from wurm_amd import _lib


def test_names_are_the_headers():
    lib = _lib.lib()
    assert lib.wurm_a2c_ff_workspace_bytes.argnames == ('num_envs', 'num_steps', 'num_inputs')
    assert lib.wurm_a2c_ff_pop_hyper.argnames == ('lr', 'gamma', 'entropy_coef', 'gamma_lambda', 'num_members', 'table')
    assert lib.wurm_a2c_ff_league_apply.argnames == (
        'params', 'grad', 'exp_avg', 'exp_avg_sq', 'grad_norm', 'hyper', 'offsets', 'learn', 'step', 'beta1', 'beta2',
        'eps', 'max_grad_norm', 'num_params', 'num_rows', 'num_members', 'stream')
    assert lib.wurm_version.argnames == ()
    for name in _lib.SYMBOLS:  # every prototype names all of its parameters
        fn = getattr(lib, name)
        assert len(fn.argnames) == len(fn.argtypes) and all(n.isidentifier() for n in fn.argnames), name


def test_order_follows_the_header_not_the_dict():
    lib = _lib.lib()
    want = lib.wurm_a2c_ff_workspace_bytes(8, 5, 75)
    assert want > 0 and lib.wurm_a2c_ff_workspace_bytes(75, 5, 8) == 0  # (8 inputs: not a shape the learner has)
    for order in (('num_envs', 'num_steps', 'num_inputs'), ('num_inputs', 'num_steps', 'num_envs'),
                  ('num_steps', 'num_inputs', 'num_envs')):
        values = dict(zip(order, (dict(num_envs=8, num_steps=5, num_inputs=75)[n] for n in order)))
        assert list(values) == list(order)
        assert _lib.call_named(None, lib.wurm_a2c_ff_workspace_bytes, values) == want
    # four arrays of one type: only the names tell them apart
    cols = {'table': np.zeros((2, 4)), 'gamma_lambda': np.float32([0.5, 0.25]), 'entropy_coef': np.float32([3, 4]),
            'gamma': np.float32([0.75, 0.875]), 'lr': np.float32([1e-3, 2.0])}
    values = {n: c.ctypes.data for n, c in cols.items()}
    values['num_members'] = 2
    assert _lib.call_named(None, lib.wurm_a2c_ff_pop_hyper, values) == _lib.OK
    assert cols['table'].tolist() == [[1e-3, 0.75, 3.0, 0.5], [2.0, 0.875, 4.0, 0.25]]


def test_extra_names_are_ignored():
    lib = _lib.lib()
    values = {'num_envs': 8, 'num_steps': 5, 'num_inputs': 75, 'num_members': 3, 'lr': 'not a number', 'stream': None}
    assert _lib.call_named(None, lib.wurm_a2c_ff_workspace_bytes, values) == lib.wurm_a2c_ff_workspace_bytes(8, 5, 75)
    assert _lib.call_named(None, lib.wurm_a2c_ff_pop_workspace_bytes, values) == 0  # (3 members do not divide 8 envs)


def test_a_missing_name_is_a_type_error_that_names_the_entry_point():
    lib = _lib.lib()
    with pytest.raises(TypeError, match=r"wurm_a2c_ff_workspace_bytes.*'num_inputs'"):
        _lib.call_named(None, lib.wurm_a2c_ff_workspace_bytes, {'num_envs': 8, 'num_steps': 5})
    table = np.zeros((2, 4))
    values = {'lr': None, 'gamma': None, 'entropy_coef': None, 'gamma_lambda': None, 'table': table.ctypes.data}
    with pytest.raises(TypeError, match=r"wurm_a2c_ff_pop_hyper.*'num_members'"):
        _lib.call_named(None, lib.wurm_a2c_ff_pop_hyper, values)
    values['num_members'] = 2
    assert _lib.call_named(None, lib.wurm_a2c_ff_pop_hyper, values) == _lib.ERR_INVALID_ARG  # null arrays: refused
    assert not table.any()

"""Every arm of the mirror controller (wurm_amd/envs/_mirror.py) on the GPU, for each of the three env classes: one scripted
caller sequence per arm on an env that steps on the resident mirror and on a twin with `resident_mirror=False,
lazy_reset=False` and the same seed.  Everything returned must be bit-equal after every call; in a second pass of the same
script the state tensors are compared after every call as well (a pass of its own, because reading the state for the
comparison applies a postponed reset and writes a lazy mirror out: the first pass leaves the protocol undisturbed).  The
smallest shapes at which a mirror engages: MultiSnake 40 x 3 x 12, the single-env classes 70 envs of 9 x 9."""
import contextlib

import pytest
import torch

from tests.protocol_enum import pack

pytestmark = pytest.mark.gpu

# arm -> (resident_mirror keyword, events, how mirror_state()['why'] begins afterwards; None: any)
LOOP = ('step', 'reset_noobs', 'step', 'reset_obs', 'step', 'reset_obs')
ARMS = {
    'lazy write-out': (True, LOOP + ('observe', 'step', 'reset_noobs', 'check', 'step', 'observe'), 'on'),
    'adaptive -> eager': (None, LOOP + ('observe', 'step', 'observe', 'step', 'reset_noobs', 'step'), 'adaptive: the state was looked'),
    'adaptive -> off': (None, ('step', 'reset_eager') * 9 + ('step', 'reset_noobs', 'step'), 'adaptive: the state was written'),
    'escape on read': (True, LOOP + ('read', 'step', 'reset_noobs', 'step', 'drop', 'step', 'reset_obs', 'step'), 'the caller holds'),
    'escape on assign': (True, LOOP + ('assign', 'step', 'reset_noobs', 'step', 'reset_obs', 'step'), 'the caller holds'),
    'watch hit': (True, LOOP + ('read', 'step', 'edit', 'step', 'edit', 'step', 'check', 'reset_noobs', 'step'), 'the caller holds'),
    # (the whole script under torch.inference_mode(): nothing the caller gets has a version counter, every reset is eager)
    'no version counter': (True, ('step', 'reset_noobs', 'step', 'read', 'step', 'edit', 'step', 'reset_noobs', 'step'), None),
    'rollout': (True, LOOP + ('rollout', 'step', 'reset_noobs', 'rollout_noobs', 'observe', 'step', 'rollout'), None),
}


class _Multi(object):
    N, K, S = 40, 3, 12

    def __init__(self, mirror, twin):
        from wurm_amd.envs import MultiSnake
        kw = dict(resident_mirror=False, lazy_reset=False) if twin else dict(resident_mirror=mirror)
        self.env = MultiSnake(self.N, self.K, self.S, device='cuda:0', seed=11, food_mode='random_rate', respawn_mode='any', **kw)
        g = torch.Generator().manual_seed(5)
        self.acts = torch.randint(8, (40, self.K, self.N), generator=g).cuda()
        self.t, self.d, self.alias, self.mark = 0, None, None, None

    def _a(self, n=1):
        self.t += n
        return self.acts[self.t - n:self.t]

    def step(self):
        out = self.env.step({'agent_%d' % i: a for i, a in enumerate(self._a()[0])})
        self.d = out[2]['__all__']
        return out

    def reset(self, d, **kw):
        return self.env.reset(d, **kw)

    def rollout(self, **kw):
        return self.env.rollout(self._a(3), **kw)

    def observe(self):
        return self.env._observe()

    def read(self):
        self.alias = self.env.foods
        return self.alias

    def edit(self):
        """a food where env 1 has none, out of every head's reach within a step (a boost move covers two cells): the edit
        changes the state for certain and its effect outlives the next step"""
        K, heads = self.K, self.env._heads           # (the caller holds a tensor: the steps write the tensors, they are current)
        busy = (self.alias[1, 0] != 0) | (heads[K:2 * K, 0] != 0).any(0) | (self.env._bodies[K:2 * K, 0] != 0).any(0)
        self.mark = (1, 0) + _far_cell(busy, (heads[K:2 * K, 0] != 0).any(0), 3)
        self.alias[self.mark] = 1.0

    def assign(self):
        self.env.foods = self.env.foods.clone()

    def state(self):
        return self.env._state(write=False)[:6]


class _Single(object):
    N, S = 70, 9

    def __init__(self, mirror, twin, kind):
        from wurm_amd.envs import SimpleGridworld, SingleSnake
        kw = dict(resident_mirror=False, lazy_reset=False) if twin else dict(resident_mirror=mirror)
        if kind == 'single':
            self.env = SingleSnake(self.N, self.S, observation_mode='partial_2', device='cuda:0', seed=11, **kw)
        else:
            self.env = SimpleGridworld(self.N, self.S, start_location=(4, 4), device='cuda:0', seed=11, **kw)
        g = torch.Generator().manual_seed(5)
        self.acts = torch.randint(4, (40, self.N), generator=g).cuda()
        self.t, self.d, self.alias, self.mark = 0, None, None, None

    _a = _Multi._a

    def step(self):
        out = self.env.step(self._a()[0].clone())
        self.d = out[2]
        return out

    def reset(self, d, **kw):
        return self.env.reset(d, **kw)

    def rollout(self, **kw):
        return self.env.rollout(self._a(3).clone(), **kw)

    def observe(self):
        return self.env._observe(self.env.observation_mode)

    def read(self):
        self.alias = self.env.envs
        return self.alias

    def edit(self):
        """env 1's food moved to an empty cell the head / agent cannot reach within a step: the edit changes the state for
        certain and its effect outlives the next step"""
        e = self.alias[1]
        busy = (e != 0).any(0)
        self.mark = (1, 0) + _far_cell(busy, (e[1:] != 0).any(0), 2)
        e[0].zero_()
        self.alias[self.mark] = 1.0

    def assign(self):
        self.env.envs = self.env.envs.clone()

    def state(self):
        return (self.env._state(write=False),)


def _far_cell(busy, heads, reach):
    """(y, x) of the first interior cell that is not `busy` and lies further than `reach` (Manhattan) from every cell of `heads`"""
    S = busy.shape[-1]
    hs = heads.nonzero().tolist()
    for y in range(1, S - 1):
        for x in range(1, S - 1):
            if not bool(busy[y, x]) and all(abs(y - hy) + abs(x - hx) > reach for hy, hx in hs):
                return (y, x)
    raise AssertionError('no free cell out of reach')


def _event(d, ev):
    if ev == 'step':
        return d.step()
    if ev == 'reset_noobs':
        return d.reset(d.d, return_observations=False)
    if ev == 'reset_obs':
        return d.reset(d.d)
    if ev == 'reset_eager':
        return d.reset(d.d.clone(), return_observations=False)
    if ev == 'observe':
        return d.observe()
    if ev == 'check':
        try:        # (an edit may have made an env inconsistent: then both objects must say so)
            return d.env.check_consistency() if hasattr(d.env, 'check_consistency') else None
        except RuntimeError as e:
            return 'RuntimeError: %s' % e
    if ev == 'read':
        return d.read()
    if ev == 'edit':
        return d.edit()
    if ev == 'drop':
        d.alias = None
        return None
    if ev == 'assign':
        return d.assign()
    if ev == 'rollout':
        return d.rollout()
    if ev == 'rollout_noobs':
        return d.rollout(return_observations=False)
    raise ValueError(ev)


def _packed(x):
    return pack(dict(x.items()) if isinstance(x, dict) else x)   # (a _LazyResetObs: read, as a caller would)


def _run(make, arm):
    from wurm_amd._lib import knobs
    mirror, events, why = ARMS[arm]
    # (the knobs: a mirror under the automatic policy, and the per-call lane kernels that keep it current, at these batches)
    mode = torch.inference_mode() if arm == 'no version counter' else contextlib.nullcontext()
    with knobs(WURM_RESIDENT_MIN_ENVS=0, WURM_LANE_STEP_MIN_ENVS=0), mode:
        for with_state in (False, True):
            d, twin = make(mirror, False), make(mirror, True)
            for i, ev in enumerate(events):
                a, b = _event(d, ev), _event(twin, ev)
                assert _packed(a) == _packed(b), (arm, i, ev, 'returned')
                if ev == 'step' and i > 0 and events[i - 1] == 'edit':
                    # the step ran on the EDITED state (a step on a stale mirror would write the unedited image over it)
                    assert d.mark == twin.mark and float(d.alias[d.mark]) != 0 and float(twin.alias[twin.mark]) != 0, (arm, i)
                if with_state:
                    assert pack(d.state()) == pack(twin.state()), (arm, i, ev, 'state')
            assert pack(d.state()) == pack(twin.state()), (arm, 'final state')
            assert int(d.env._call) == int(twin.env._call), (arm, 'RNG counter')
            st = d.env.mirror_state()
            if why is not None and not with_state:
                assert st['why'].startswith(why), (arm, st)
            if arm == 'no version counter':
                assert st['state'] == 'off' and 'no version counter' in st['why'], st
            assert twin.env.mirror_state()['state'] == 'off'


@pytest.mark.parametrize('arm', list(ARMS))
def test_multi_snake_arm_matches_the_path_without_a_mirror(arm):
    _run(_Multi, arm)


@pytest.mark.parametrize('arm', list(ARMS))
@pytest.mark.parametrize('kind', ['single', 'grid'])
def test_single_env_arm_matches_the_path_without_a_mirror(kind, arm):
    _run(lambda mirror, twin: _Single(mirror, twin, kind), arm)

"""Golden vectors for the acting policy on the inputs beyond make_golden_policy.py's 27-147: the REAL reference agent
(`wurm.agents.FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E)`, wurm/agents/feedforward.py:8-28,
weights as torch initialises them, packed as pack_policy_params packs them) applied to REAL observations of the
reference's envs, for the sizes experiments/main.py:129-137 builds beyond those: E = 4 ('positions' of SingleSnake and
of SimpleGridworld) and E = 363 / 507 ('partial_5' / 'partial_6').  Data only; see make_golden.py.
Run: python tests/golden/make_golden_policy_wide.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_shim  # noqa: E402

ref_shim.install()
from wurm.agents import FeedforwardAgent  # noqa: E402  (the reference's class)
from wurm.envs import SimpleGridworld, SingleSnake  # noqa: E402  (the reference's envs: real observations)

ORDER = ['feedforward.0.0.weight', 'feedforward.0.0.bias', 'feedforward.1.0.weight', 'feedforward.1.0.bias',
         'action_head.weight', 'action_head.bias', 'value_head.weight', 'value_head.bias']


def snake_obs(mode, size, M):
    env = SingleSnake(num_envs=M, size=size, observation_mode=mode, device='cpu')
    obs = env.reset()
    for _ in range(6):  # a few steps so that bodies bend and food moves
        obs, _, done, _ = env.step(torch.randint(4, (M,)))
        env.reset(done)
    return obs.reshape(M, -1).float()


def grid_obs(size, M):
    # the reference's 'positions' observation is written for one env per object (simple_gridworld.py:122-131)
    rows = []
    for i in range(M):
        start = (1 + i % (size - 2), 1 + (3 * i) % (size - 2))
        env = SimpleGridworld(num_envs=1, size=size, observation_mode='positions', device='cpu', start_location=start)
        obs = env.reset()
        for _ in range(i % 4):
            obs, _, done, _ = env.step(torch.randint(4, (1,)))
            if bool(done.any()):
                obs = env.reset(done)
        rows.append(obs.reshape(1, 4).float())
    return torch.cat(rows)


def record(name, obs, size, n, seed):
    M, E = obs.shape
    torch.manual_seed(seed)
    model = FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E)
    with torch.no_grad():
        probs, values = model(obs)
    sd = model.state_dict()
    params = np.concatenate([sd[k].numpy().reshape(-1) for k in ORDER]).astype(np.float32)
    np.savez_compressed(os.path.join(HERE, name + '.npz'), params=params, obs=obs.numpy(), probs=probs.numpy(),
                        values=values.numpy(), meta=np.asarray([M, E, n, size]))
    print(name, params.shape, obs.shape, float(probs.min()), float(probs.max()))


if __name__ == '__main__':
    torch.manual_seed(0)
    record('policy_ff_positions_snake_s12', snake_obs('positions', 12, 64), 12, -1, seed=21)   # 4 inputs
    record('policy_ff_positions_grid_s9', grid_obs(9, 64), 9, -1, seed=22)                    # 4 inputs
    record('policy_ff_n5_s25', snake_obs('partial_5', 25, 64), 25, 5, seed=23)                # 363 inputs
    record('policy_ff_n6_s36', snake_obs('partial_6', 36, 64), 36, 6, seed=24)                # 507 inputs

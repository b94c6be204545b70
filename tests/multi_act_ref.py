"""What tests/test_multi_act_*.py share: the species / env_id / column formulas of `MultiSnake.act` restated by brute force,
and the expected rows of wurm_multi_act from the CPU oracle (oracle.policy_forward; oracle_policy_sample through ctypes).
Not a test module."""
import ctypes

import numpy as np

OBS_N = {27: 1, 75: 2, 147: 3, 243: 4, 363: 5, 507: 6}


def species_by_counting(K, P):
    """species of every snake (experiments/multiagent.py:356: k * P // K) without a division: the largest s with
    s * K <= k * P"""
    out = []
    for k in range(K):
        s = 0
        while (s + 1) * K <= k * P:
            s += 1
        out.append(s)
    return out


def expected_rows(params, obs, num_species, seed, call, env_offset=0):
    """params (P, num_params), obs (K, N, E) numpy -> probs (K, N, 4), values (K, N), actions (K, N) of the oracle"""
    from oracle import oracle as O
    K, N, E = obs.shape
    params = np.ascontiguousarray(params, np.float32).reshape(-1, O.policy_param_count(E))
    sample = O.lib().oracle_policy_sample
    sample.restype = ctypes.c_int
    sample.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]
    species = species_by_counting(K, num_species)
    probs, values = np.empty((K, N, 4), np.float32), np.empty((K, N), np.float32)
    actions = np.empty((K, N), np.int64)
    for k in range(K):
        probs[k], values[k] = O.policy_forward(params[species[k]], obs[k])
        for i in range(N):
            row = np.ascontiguousarray(probs[k, i])
            actions[k, i] = sample(row.ctypes.data, seed, call, (env_offset + i) * K + k)
    return probs, values, actions


def sharp_params(num_species, E, scale=4.0, seed=0):
    """(P, num_params) numpy: torch-initialised FeedforwardAgents whose action head is scaled so that the four
    probabilities are far from uniform"""
    import torch
    from wurm_amd.agents import FeedforwardAgent, pack_policy_params
    rows = []
    for s in range(num_species):
        torch.manual_seed(seed + 100 * s + E)
        agent = FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E)
        with torch.no_grad():
            for block in agent.feedforward:
                block[0].weight.mul_(scale)
            agent.action_head.weight.mul_(scale)
        rows.append(pack_policy_params(agent).numpy())
    return np.stack(rows)


def random_rows(K, N, E, seed=0):
    """(K, N, E) fp32 with negative and large (+-50) entries"""
    g = np.random.default_rng(seed)
    x = g.standard_normal((K, N, E)).astype(np.float32)
    big = g.random((K, N, E)) < 0.02
    x[big] = np.where(g.random(int(big.sum())) < 0.5, -50.0, 50.0).astype(np.float32)
    return x

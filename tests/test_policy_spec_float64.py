"""The arithmetic spec of the fused actor (oracle/policy.c: oracle_policy_forward, oracle_policy_sample) against float64,
at every input size policy_wide_kernel serves.  The kernels are bit-identical to the spec (tests/test_policy_rollout*.py,
tests/test_policy_wide_coverage.py), so what pins the spec to real arithmetic pins them.

The bound is not a number chosen here: on the same weights and inputs, float32 torch (the reference agent's own
arithmetic: Linear, ReLU, softmax) has an error against float64 too, and the spec — the same O(E eps) rounding in
another order — must stay within 8 times it, for probabilities and for values separately.  A ratio past 8 means a
wrong term, not a reordered one.

Measured when this file was written (the 21 cases below, 256 inputs each; max abs error against float64):
  probabilities  spec 3.7e-08 .. 3.1e-05, torch 3.2e-08 .. 4.0e-05, growing with the size of the logits; spec / torch
                 0.47 .. 4.84 (the largest at E 4, scale 1.0, a saturated policy on which torch happens to err by
                 2.1e-07 only; the next largest is 1.45);
  values         spec 2.9e-09 .. 8.1e-04, torch 3.2e-09 .. 9.5e-04 (|v| reaches 3.1e+03); spec / torch 0.65 .. 1.26;
                 relative to max |v| at most 3.4e-07 (spec) and 4.8e-07 (torch).
(the print in the test shows each case's figures: pytest -s)"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle as O

SIZES = [3, 4, 27, 147, 243, 363, 507]   # partial_0, positions, partial_1 .. partial_6
SCALES = [0.05, 0.3, 1.0]
M = 256
RATIO = 8.0
SUM_ATOL = 3e-7   # tests/test_policy_rollout.py's bound on |sum(probs) - 1|


def _inputs(E, rng):
    if E == 4:   # 'positions': (head row, head column, food row, food column)
        return rng.randint(0, 64, (M, 4)).astype(np.float32)
    # 'partial_n': 0, 1 and write_obs's 127 / 255 for the snake's body
    return rng.choice(np.asarray([0.0, 1.0, 127.0 / 255.0], np.float32), size=(M, E), p=[0.6, 0.2, 0.2])


def _split(params, E, xp):
    o, out = 0, []
    for shape in ((64, E), (64,), (64, 64), (64,), (4, 64), (4,), (1, 64), (1,)):
        n = int(np.prod(shape))
        out.append(xp(params[o:o + n].reshape(shape)))
        o += n
    assert o == params.size
    return out


def _forward64(params, x, E):
    W1, b1, W2, b2, Wp, bp, Wv, bv = _split(params, E, lambda a: a.astype(np.float64))
    h = np.maximum(x.astype(np.float64) @ W1.T + b1, 0)
    h = np.maximum(h @ W2.T + b2, 0)
    logits = h @ Wp.T + bp
    e = np.exp(logits - logits.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True), (h @ Wv.T + bv)[:, 0]


def _forward_torch32(params, x, E):
    W1, b1, W2, b2, Wp, bp, Wv, bv = _split(params, E, lambda a: torch.from_numpy(np.ascontiguousarray(a)))
    F = torch.nn.functional
    with torch.no_grad():
        h = F.relu(F.linear(torch.from_numpy(x), W1, b1))
        h = F.relu(F.linear(h, W2, b2))
        return F.softmax(F.linear(h, Wp, bp), dim=-1).numpy(), F.linear(h, Wv, bv)[:, 0].numpy()


@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('E', SIZES)
def test_spec_forward_within_8x_of_torch_fp32_error(E, scale):
    rng = np.random.RandomState(1000 * E + int(100 * scale))
    params = (rng.randn(O.policy_param_count(E)) * scale).astype(np.float32)
    x = _inputs(E, rng)
    p64, v64 = _forward64(params, x, E)
    ps, vs = O.policy_forward(params, x)
    pt, vt = _forward_torch32(params, x, E)
    ep_s, ep_t = np.abs(ps - p64).max(), np.abs(pt - p64).max()
    ev_s, ev_t = np.abs(vs - v64).max(), np.abs(vt - v64).max()
    print(f'E {E} scale {scale}: probs spec {ep_s:.2e} torch {ep_t:.2e} ratio {ep_s / ep_t:.2f}; values spec {ev_s:.2e} '
          f'torch {ev_t:.2e} ratio {ev_s / ev_t:.2f} (max |v| {np.abs(v64).max():.2e})')
    assert ep_t > 0 and ev_t > 0   # the yardstick itself is a rounding error, never exactly zero over 256 inputs
    assert ep_s <= RATIO * ep_t, (ep_s, ep_t)
    assert ev_s <= RATIO * ev_t, (ev_s, ev_t)
    assert np.abs(ps.astype(np.float64).sum(1) - 1).max() <= SUM_ATOL
    assert (ps >= 0).all() and np.isfinite(ps).all() and np.isfinite(vs).all()
    top = np.sort(p64, axis=1)
    clear = top[:, -1] - top[:, -2] > ep_s
    assert clear.any()
    assert (ps.argmax(1)[clear] == p64.argmax(1)[clear]).all()


def _sample(probs, seed, call, env):
    p = np.asarray(probs, np.float32)
    return O.lib().oracle_policy_sample(p.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(seed), ctypes.c_uint64(call),
                                        ctypes.c_uint64(env))


def test_sampler_boundaries():
    """oracle_policy_sample: action = (u >= c0) + (u >= c1) + (u >= c2) with c0 = p0, c1 = c0 + p1, c2 = c1 + p2 and
    u in [0, 1).  One-hot probabilities (the saturated softmax gives exact zeros) must give their own action for every
    u, u = 0 included: (0, 0, 0, 1) -> 3 because u >= 0 three times, (1, 0, 0, 0) -> 0 because no u reaches 1."""
    rng = np.random.RandomState(5)
    keys = [(int(rng.randint(1 << 62)), int(rng.randint(1 << 62)), int(rng.randint(1 << 62))) for _ in range(2000)]
    keys += [(0, 0, 0), (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1)]
    for a in range(4):
        onehot = np.eye(4, dtype=np.float32)[a]
        assert {_sample(onehot, *k) for k in keys} == {a}
    # the formula itself at the ends of u's range
    def formula(p, u):
        p = np.asarray(p, np.float32)
        c0 = p[0]
        c1 = np.float32(c0 + p[1])
        c2 = np.float32(c1 + p[2])
        return int(u >= c0) + int(u >= c1) + int(u >= c2)
    one_below = np.nextafter(np.float32(1), np.float32(0))
    assert formula((1, 0, 0, 0), np.float32(0)) == 0 and formula((1, 0, 0, 0), one_below) == 0
    assert formula((0, 0, 0, 1), np.float32(0)) == 3 and formula((0, 0, 0, 1), one_below) == 3
    # and the function follows the formula on ordinary probabilities: the action's cumulative interval holds u for
    # every key, so the four frequencies follow the probabilities
    p = np.asarray([0.1, 0.2, 0.3, 0.4], np.float32)
    counts = np.bincount([_sample(p, *k) for k in keys], minlength=4) / len(keys)
    assert np.abs(counts - p).max() < 0.044   # 4 sigma of a binomial share at p = 0.4 over 2 002 draws

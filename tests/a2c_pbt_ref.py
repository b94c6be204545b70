"""numpy / pure-Python restatement of the exploit step of population-based training (include/wurm_hip.h:
wurm_a2c_ff_pop_exploit; wurm_amd/csrc/a2c_pbt.hpp), written from the specification, for the tests: the rank rule,
Philox4x32-10 in Python ints with the counter layout of `rng_words` (wurm_device.hpp), mulhi, the factor bits, the clamps
and the float rounding of entropy_coef."""
import math

import numpy as np

RNG_PBT = 9
MASK = 0xFFFFFFFF
DEFAULT_PERTURB = (0.8, 1.2, 0.0, math.inf, 0.8, 1.2, 0.0, math.inf)  # lr_down, lr_up, lr_lo, lr_hi, e_down, e_up, e_lo, e_hi


def philox4x32_10(counter, key):
    """Philox4x32-10 (Random123): counter of four and key of two 32-bit words -> four 32-bit words"""
    M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def rng_words(seed, call, env_id, purpose, sub):
    """counter = (env_id, call_lo, call_hi, purpose | sub << 8), key = seed"""
    return philox4x32_10((env_id & MASK, call & MASK, (call >> 32) & MASK, ((purpose & 0xFF) | (sub << 8)) & MASK),
                         (seed & MASK, (seed >> 32) & MASK))


def mulhi(w, n):
    return (w * n) >> 32


def ranks(scores):
    """rank(p) = #{q : key_q > key_p or (key_q == key_p and q < p)}, key = score with NaN as -inf; straight from the
    definition, O(P^2)"""
    key = np.asarray(scores, dtype=np.float64).copy()
    key[np.isnan(key)] = -np.inf
    P = len(key)
    q, p = np.arange(P)[None, :], np.arange(P)[:, None]
    return ((key[None, :] > key[:, None]) | ((key[None, :] == key[:, None]) & (q < p))).sum(axis=1)


def _fmax(a, b):  # C's fmax / fmin: the other operand where one is a NaN
    return b if a != a else a if b != b else max(a, b)


def _fmin(a, b):
    return b if a != a else a if b != b else min(a, b)


def select(scores, k, seed, generation):
    """(order, parent, words): order[rank(p)] = p; parent[p] = p for rank(p) < P - k, else order[mulhi(w0, k)] with w the
    member's Philox block; words[p] = that block or None"""
    rank = ranks(scores)
    P = len(rank)
    order = np.empty(P, dtype=np.int32)
    order[rank] = np.arange(P, dtype=np.int32)
    parent, words = np.arange(P, dtype=np.int32), [None] * P
    for p in range(P):
        if rank[p] >= P - k:
            words[p] = rng_words(seed, generation, p, RNG_PBT, 0)
            parent[p] = order[mulhi(words[p][0], k)]
    return order, parent, words


def exploit(params, exp_avg, exp_avg_sq, hyper, scores, k, perturb=DEFAULT_PERTURB, seed=0, generation=0):
    """What the call leaves: dict of NEW arrays params, exp_avg, exp_avg_sq (P, num_params) float32, hyper (P, 4) float64,
    order, parent (P,) int32 — plus `hit`, the set of clamps that acted on an lr ('lo', 'hi').  The inputs are numpy
    arrays and are not modified."""
    lr_down, lr_up, lr_lo, lr_hi, e_down, e_up, e_lo, e_hi = (float(x) for x in perturb)
    order, parent, words = select(scores, k, seed, generation)
    out = dict(params=params[parent].copy(), exp_avg=exp_avg[parent].copy(), exp_avg_sq=exp_avg_sq[parent].copy(),
               hyper=hyper.copy(), order=order, parent=parent, hit=set())
    for p, w in enumerate(words):
        if w is None:
            continue
        src = hyper[parent[p]]
        lr = float(src[0]) * (lr_up if w[1] >> 31 else lr_down)
        if lr < lr_lo:
            out['hit'].add('lo')
        if lr > lr_hi:
            out['hit'].add('hi')
        e = float(src[2]) * (e_up if w[2] >> 31 else e_down)
        out['hyper'][p] = (_fmin(_fmax(lr, lr_lo), lr_hi), src[1], float(np.float32(_fmin(_fmax(e, e_lo), e_hi))), src[3])
    return out

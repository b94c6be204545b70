#!/usr/bin/env python3
"""Time of one A2C update, fused learner against the torch learner (lines 38-52 of examples/a2c_fused_actor.py), with HIP
events after warm-up, in one process on the same allocations; then the two examples end to end.  One JSON line per
measurement, appended to profiles/r08_a2c_learner.jsonl (or --out).  Needs the GPU.

    tools/bench_a2c_learner.py                 # update times and end-to-end rates
    tools/bench_a2c_learner.py --trace-only    # a few fused updates only: the target of rocprofv3 --kernel-trace --stats
    tools/bench_a2c_learner.py --gae-lambda 0.95   # both learners with GAE returns (rows carry "gae_lambda")
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))
import torch  # noqa: E402
from torch import nn  # noqa: E402
from torch.distributions import Categorical  # noqa: E402

from wurm_amd import _lib  # noqa: E402
from wurm_amd.agents import FeedforwardAgent  # noqa: E402
from wurm_amd.rl import A2C, FusedA2CLearner  # noqa: E402

SHAPES = [(512, 5, 75), (512, 20, 75), (8192, 20, 75), (512, 20, 507), (8192, 5, 4)]


def window(N, T, E, dev):
    g = torch.Generator().manual_seed(N + T + E)
    obs = (torch.rand((T + 1, N, E), generator=g) < 0.3).float().to(dev)
    out = {'observations': obs[1:].contiguous(), 'actions': torch.randint(0, 4, (T, N), generator=g).to(dev),
           'rewards': (torch.randint(-1, 2, (T, N), generator=g).float()).to(dev),
           'dones': (torch.rand((T, N), generator=g) < 0.1).to(dev)}
    return obs[0].contiguous(), out


def torch_update(model, optimizer, a2c, state, out, entropy=0.01):
    inputs = torch.cat([state.unsqueeze(0), out['observations'][:-1]]).flatten(2)
    probs, values = model(inputs)
    dist = Categorical(probs)
    log_probs = dist.log_prob(out['actions']).unsqueeze(-1)
    entropies = dist.entropy().mean(-1)
    with torch.no_grad():
        _, bootstrap_values = model(out['observations'][-1].flatten(1))
    value_loss, policy_loss = a2c.loss(bootstrap_values, out['rewards'].unsqueeze(-1), values, log_probs,
                                       out['dones'].unsqueeze(-1))
    loss = value_loss + policy_loss - entropy * entropies.mean()
    optimizer.zero_grad()
    loss.backward()
    nn.utils.clip_grad_norm_(model.parameters(), 0.5)
    optimizer.step()


def time_ms(fn, reps, inner):
    """median and range over `reps` event-timed windows of `inner` calls each, in ms per call"""
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return statistics.median(times), min(times), max(times)


def flops(N, T, E):
    """fmaf-counted FLOP of one update: forward of (T + 1) N rows, backward (dZ2, dW2, dH1, dW1, heads) of T N rows"""
    fwd = 2 * (64 * E + 64 * 64 + 5 * 64)
    bwd = 2 * (64 * E + 2 * 64 * 64 + 2 * 5 * 64)
    return (T + 1) * N * fwd + T * N * bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r08_a2c_learner.jsonl'))
    ap.add_argument('--trace-only', action='store_true')
    ap.add_argument('--skip-end-to-end', action='store_true')
    ap.add_argument('--gae-lambda', type=float, default=None, help='GAE returns with this lambda in both learners')
    args = ap.parse_args()
    gae = dict(use_gae=args.gae_lambda is not None, gae_lambda=args.gae_lambda)
    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    dev = torch.device('cuda', 0)
    rows = []
    if args.trace_only:
        state, out = window(512, 5, 75, dev)
        learner = FusedA2CLearner(FeedforwardAgent(4, 2, 64, 75).to(dev), entropy_coef=0.01, **gae)
        before = _lib.lib().wurm_launch_count()
        for _ in range(20):
            learner.update(state, out)
        torch.cuda.synchronize()
        print(json.dumps({'what': 'launches_per_update_library_counter',
                          'value': (_lib.lib().wurm_launch_count() - before) / 20}))
        return
    for N, T, E in SHAPES:
        state, out = window(N, T, E, dev)
        torch.manual_seed(0)
        learner = FusedA2CLearner(FeedforwardAgent(4, 2, 64, E).to(dev), entropy_coef=0.01, **gae)
        model = FeedforwardAgent(4, 2, 64, E).to(dev)
        optimizer, a2c = torch.optim.Adam(model.parameters(), lr=1e-3), A2C(gamma=0.99, **gae)
        fused = lambda: learner.update(state, out)
        eager = lambda: torch_update(model, optimizer, a2c, state, out)
        for _ in range(20):
            fused()
            eager()
        torch.cuda.synchronize()
        res = {}
        for _ in range(2):  # alternate the two learners
            for name, fn in (('fused', fused), ('torch', eager)):
                res.setdefault(name, []).append(time_ms(fn, reps=7, inner=50))
        row = {'what': 'update_ms', 'num_envs': N, 'num_steps': T, 'num_inputs': E, 'gflop': flops(N, T, E) / 1e9,
               'gae_lambda': args.gae_lambda}
        for name, r in res.items():
            row[name + '_ms_median'] = statistics.median(x[0] for x in r)
            row[name + '_ms_min'] = min(x[1] for x in r)
            row[name + '_ms_max'] = max(x[2] for x in r)
        row['speedup'] = row['torch_ms_median'] / row['fused_ms_median']
        row['fused_gflops'] = row['gflop'] / row['fused_ms_median'] * 1e3
        rows.append(row)
        print(json.dumps(row), flush=True)
    if not args.skip_end_to_end and args.gae_lambda is None:  # (examples/a2c_fused_actor.py has n-step returns only)
        import a2c_fused_actor
        import a2c_fused_learner
        for T in (5, 20):
            res = {}
            for mod in (a2c_fused_learner, a2c_fused_actor):
                mod.run(steps=200 * T // 5, update_steps=T, log_interval=10 ** 9, verbose=False)  # warm-up
            for _ in range(3):
                for name, mod in (('fused_learner', a2c_fused_learner), ('fused_actor', a2c_fused_actor)):
                    h = mod.run(steps=4000, update_steps=T, log_interval=10 ** 9, verbose=False)
                    res.setdefault(name, []).append(h[-1]['env_steps_per_s'])
            row = {'what': 'end_to_end_env_steps_per_s', 'num_envs': 512, 'size': 9, 'observation': 'partial_2',
                   'update_steps': T}
            for name, r in res.items():
                row[name + '_median'], row[name + '_min'], row[name + '_max'] = statistics.median(r), min(r), max(r)
            rows.append(row)
            print(json.dumps(row), flush=True)
    with open(args.out, 'a') as f:
        for row in rows:
            f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()

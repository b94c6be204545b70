#!/usr/bin/env python3
"""What the exploit / explore step of population-based training costs (`FusedA2CPopulation.exploit`: two launches), in one
process on one device, with HIP events after warm-up.  Needs the GPU.

(a) what='a2c_pbt_exploit': one `exploit` with k = P // 4 at P in {4, 16, 256}, E = 75, beside the same selection written
    with torch ops that stay on the device (`torch_exploit` below: argsort, index_select / index_copy_ on the three
    buffers, device random numbers, the table edited in place) — alternating, the torch version timed before and after.
(b) what='a2c_pbt_window': the T = 5, M = 512 training window of tools/bench_a2c_population.py (rollout + update, four
    launches) with an exploit every 10 windows, beside the same loop without, as ms per window over blocks of windows,
    alternating, the plain loop timed before and after.
One JSON line each, appended to profiles/r16_a2c_pbt.jsonl (or --out).

    tools/bench_a2c_pbt.py
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from wurm_amd import _lib  # noqa: E402
from wurm_amd.agents import FeedforwardAgent  # noqa: E402
from wurm_amd.envs import SingleSnake  # noqa: E402
from wurm_amd.rl import FusedA2CPopulation  # noqa: E402

DEV, E = 'cuda:0', 75


def population(P, seed=0):
    agents = []
    for p in range(P):
        torch.manual_seed(seed + p)
        agents.append(FeedforwardAgent(num_actions=4, num_layers=2, hidden_units=64, num_inputs=E).to(DEV))
    return FusedA2CPopulation(agents, lr=[1e-3 * (1 + p % 4) for p in range(P)], gamma=0.99, entropy_coef=0.01)


def torch_exploit(pop, scores, k, factors=(0.8, 1.2)):
    """the selection of `exploit` in torch ops, nothing read back (its random numbers are torch's, not Philox's: the same
    work, not the same bits)"""
    P = pop.num_members
    key = torch.where(torch.isnan(scores), torch.full_like(scores, -math.inf), scores)
    order = torch.argsort(key, descending=True, stable=True)
    losers = order[P - k:]
    src = order[torch.randint(k, (k,), device=scores.device)]
    for buf in (pop.params, pop.exp_avg, pop.exp_avg_sq):
        buf.index_copy_(0, losers, buf.index_select(0, src))
    rows = pop.hyper.index_select(0, src)
    coin = torch.rand((k, 2), device=scores.device) < 0.5
    factor = coin.double() * (factors[1] - factors[0]) + factors[0]
    rows[:, 0] = (rows[:, 0] * factor[:, 0]).clamp(0.0, math.inf)
    rows[:, 2] = (rows[:, 2] * factor[:, 1]).clamp(0.0, math.inf).float().double()
    pop.hyper.index_copy_(0, losers, rows)
    return order


def time_ms(fn, reps, inner):
    """median and range over `reps` event-timed runs of `inner` calls each, in ms per call"""
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return [round(x, 5) for x in (statistics.median(times), min(times), max(times))]


def launches(fn):
    before = _lib.lib().wurm_launch_count()
    fn()
    return _lib.lib().wurm_launch_count() - before


def bench_exploit(P, a):
    k = max(1, P // 4)
    fused, plain = population(P), population(P)
    scores = torch.randn(P, dtype=torch.float64, device=DEV, generator=torch.Generator(DEV).manual_seed(P))
    one = lambda: fused.exploit(scores, num_replace=k)
    two = lambda: torch_exploit(plain, scores, k)
    for fn in (one, two):
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    n = launches(one)
    t0, f, t1 = time_ms(two, a.reps, a.inner), time_ms(one, a.reps, a.inner), time_ms(two, a.reps, a.inner)
    return dict(what='a2c_pbt_exploit', device=torch.cuda.get_device_name(0), members=P, num_replace=k, num_inputs=E,
                num_params=fused.params.shape[1], launches=n, exploit_ms=f[0], exploit_ms_range=f[1:],
                torch_ops_ms=t0[0], torch_ops_ms_range=t0[1:], torch_ops_again_ms=t1[0], reps=a.reps,
                calls_per_rep=a.inner)


def bench_window(P, a, M=512, T=5, every=10):
    def loop(pbt):
        env = SingleSnake(num_envs=P * M, size=9, observation_mode='partial_2', device=DEV, seed=0)
        pop, box = population(P), {}
        box['state'] = env.reset()
        scores = torch.randn(P, dtype=torch.float64, device=DEV, generator=torch.Generator(DEV).manual_seed(P))

        def block():  # `every` windows, the last of them followed by an exploit
            for _ in range(every):
                out = env.policy_rollout(pop.params, box['state'], T, check=False, population=P)
                pop.update(box['state'], out)
                box['state'] = out['state']
            if pbt:
                pop.exploit(scores, fraction=0.25)
        return block

    with_pbt, without = loop(True), loop(False)
    for fn in (with_pbt, without):
        for _ in range(a.warmup // every + 1):
            fn()
    torch.cuda.synchronize()
    n = launches(with_pbt)
    blocks = max(1, a.inner // every)
    per_window = lambda t: [round(x / every, 5) for x in t]
    w0 = per_window(time_ms(without, a.reps, blocks))
    w = per_window(time_ms(with_pbt, a.reps, blocks))
    w1 = per_window(time_ms(without, a.reps, blocks))
    return dict(what='a2c_pbt_window', device=torch.cuda.get_device_name(0), members=P, envs_per_member=M, steps=T,
                exploit_every_windows=every, launches_per_block=n, window_ms_with_pbt=w[0], window_ms_with_pbt_range=w[1:],
                window_ms_without=w0[0], window_ms_without_range=w0[1:], window_ms_without_again=w1[0], reps=a.reps,
                windows_per_rep=blocks * every)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r16_a2c_pbt.jsonl'))
    ap.add_argument('--members', type=int, nargs='+', default=[4, 16, 256])
    ap.add_argument('--window-members', type=int, nargs='+', default=[4, 16])
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('tools/bench_a2c_pbt.py measures on the GPU: no HIP device visible')
    rows = [bench_exploit(P, a) for P in a.members] + [bench_window(P, a) for P in a.window_members]
    with open(a.out, 'a') as f:
        for row in rows:
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()

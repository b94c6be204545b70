"""Pins the invariant checkers on FAILING states: recorded states are corrupted in the ways the
reference's checks look for, and for every variant the REAL reference is asked whether — and with which message — it
raises (wurm/utils.py:113-178 `snake_consistency` / `env_consistency`; wurm/envs/multi_snake.py:733-769
`MultiSnake.check_consistency`).  The fixture holds DATA only: the corrupted states and the reference's verdicts.

Run only in the build container (where /root/reference exists):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_checker.py

With `--sizes` it writes a second file instead, checker_failing_states_sizes.npz: the same variants — and those that
add a cell once more at the LAST cell of the grid — at one single-snake size per instantiation of the checker kernel
that the first file misses, and for MultiSnake at shapes where a snake is one, two and three of the kernel's items
(tests/test_checker_batches_cpu.py checks the specification of tests/checker_ref.py against it).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402

SingleSnake, SimpleGridworld, MultiSnake, ref_utils = ref_shim.import_reference()


def verdict(fn):
    try:
        fn()
        return ''
    except RuntimeError as e:
        return str(e)


def single_variants(S, seed, base=None, last_cell=False):
    if base is None:
        torch.manual_seed(seed)
        env = SingleSnake(num_envs=1, size=S, device='cpu')
        # grow the snake a little so that removing / duplicating body values has room
        base = env.envs.clone()
    out = []

    def add(name, e):
        out.append((name, e.clone()))

    def body_cell(e, v):
        ys, xs = np.nonzero(e[0, 2].numpy() == v)
        return int(ys[0]), int(xs[0])

    L = int(base[0, 2].max())
    hy, hx = body_cell(base, L)
    ty, tx = body_cell(base, 1)
    fy, fx = [int(v[0]) for v in np.nonzero(base[0, 0].numpy() > 0)]
    free = [(y, x) for y in range(1, S - 1) for x in range(1, S - 1) if float(base[0, :, y, x].sum()) == 0]

    add('valid', base)
    e = base.clone(); e[0, 1, free[0][0], free[0][1]] = 1; add('two_heads', e)
    e = base.clone(); e[0, 1] = 0; add('no_head', e)
    e = base.clone(); e[0, 0, fy, fx] = 2; add('food_value_2', e)
    e = base.clone(); e[0, 0, free[1][0], free[1][1]] = 0.5; add('food_value_half', e)
    e = base.clone(); e[0, 2] = 0; add('no_body', e)
    e = base.clone(); e[0, 1] = 0; e[0, 2] = 0; add('no_snake_at_all', e)
    my, mx = body_cell(base, 2)
    e = base.clone(); e[0, 2, my, mx] = 0; add('body_value_2_missing', e)
    e = base.clone(); e[0, 1] = 0; e[0, 1, ty, tx] = 1; add('head_on_the_tail', e)
    e = base.clone(); e[0, 2, ty, tx] = 0; e[0, 2, my, mx] = 1; e[0, 2, hy, hx] = 2; add('length_2_snake', e)
    e = base.clone(); e[0, 0] = 0; e[0, 0, hy, hx] = 1; add('food_under_the_head', e)
    e = base.clone(); e[0, 0, free[2][0], free[2][1]] = 1; add('two_foods', e)
    e = base.clone(); e[0, 0] = 0; add('no_food', e)
    e = base.clone(); e[0, 2, free[3][0], free[3][1]] = 2; add('body_value_2_twice', e)
    e = base.clone(); e[0, 2, ty, tx] = 0; e[0, 2, my, mx] = 3; add('values_3_3_sum_is_triangular', e)
    e = base.clone(); e[0, 2, hy, hx] = L + 1; add('head_value_too_large', e)
    e = base.clone(); e[0, 0, fy, fx] = 0; e[0, 0, ty, tx] = 1; add('food_under_the_tail', e)
    e = base.clone(); e[0, 2, free[4][0], free[4][1]] = L + 1; add('stray_larger_body_value', e)
    if last_cell:  # the variants that add a cell, at cell C - 1 (the reference's checks do not know the border)
        e = base.clone(); e[0, 1, S - 1, S - 1] = 1; add('two_heads_last_cell', e)
        e = base.clone(); e[0, 0, S - 1, S - 1] = 1; add('two_foods_last_cell', e)
        e = base.clone(); e[0, 0, S - 1, S - 1] = 2; add('food_value_2_last_cell', e)
        e = base.clone(); e[0, 2, S - 1, S - 1] = 2; add('body_value_2_twice_last_cell', e)
        e = base.clone(); e[0, 2, S - 1, S - 1] = L + 1; add('stray_larger_body_value_last_cell', e)
    return out


def multi_variants(K, S, seed):
    torch.manual_seed(seed)
    env = MultiSnake(num_envs=1, num_snakes=K, size=S, device='cpu', manual_setup=False)
    f0, h0, b0, d0 = env.foods.clone(), env.heads.clone(), env.bodies.clone(), env.dones.clone()
    out = []

    def add(name, f, h, b, d):
        out.append((name, f.clone(), h.clone(), b.clone(), d.clone()))

    def cell(t, s, v):
        ys, xs = np.nonzero(t[s, 0].numpy() == v)
        return int(ys[0]), int(xs[0])

    occupied = (f0[0, 0] + h0[:, 0].sum(0) + b0[:, 0].sum(0)).numpy()
    free = [(y, x) for y in range(1, S - 1) for x in range(1, S - 1) if occupied[y, x] == 0]
    add('valid', f0, h0, b0, d0)
    b = b0.clone(); b[0, 0] = torch.max(b[0, 0], b0[1, 0]); add('snake_0_over_snake_1', f0, h0, b, d0)
    b = b0.clone(); h = h0.clone(); b[1] = b0[0]; h[1] = h0[0]; add('snake_1_on_top_of_snake_0', f0, h, b, d0)
    d = d0.clone(); d[1] = 1; add('dead_snake_with_a_body', f0, h0, b0, d)
    d = d0.clone(); d[1] = 1; h = h0.clone(); b = b0.clone(); h[1] = 0; b[1] = 0; add('dead_snake_cleared', f0, h, b, d)
    h = h0.clone(); h[0, 0, free[0][0], free[0][1]] = 1; add('two_heads_for_snake_0', f0, h, b0, d0)
    h = h0.clone(); h[2] = 0; add('no_head_for_snake_2', f0, h, b0, d0)
    y, x = cell(b0, 1, 2)
    b = b0.clone(); b[1, 0, y, x] = 0; add('body_value_2_missing_in_snake_1', f0, h0, b, d0)
    ty, tx = cell(b0, 0, 1)
    h = h0.clone(); h[0] = 0; h[0, 0, ty, tx] = 1; add('head_of_snake_0_on_its_tail', f0, h, b0, d0)
    hy, hx = cell(b0, 0, int(b0[0].max()))
    f = f0.clone(); f[0, 0, hy, hx] = 1; add('food_under_the_head_of_snake_0', f, h0, b0, d0)
    f = f0.clone(); f[0, 0, free[1][0], free[1][1]] = 2; add('food_value_2', f, h0, b0, d0)
    b = b0.clone(); b[2, 0] = 0; h = h0.clone(); h[2, 0] = 0; add('living_snake_2_without_cells', f0, h, b, d0)
    d = torch.ones_like(d0); add('all_dead_nothing_cleared', f0, h0, b0, d)
    d = torch.ones_like(d0); add('all_dead_all_cleared', f0, torch.zeros_like(h0), torch.zeros_like(b0), d)
    b = b0.clone(); b[0, 0, ty, tx] = 0; y2, x2 = cell(b0, 0, 2); b[0, 0, y2, x2] = 1; b[0, 0, hy, hx] = 2
    add('snake_0_of_length_2', f0, h0, b, d0)
    return out


def multi_variants_sizes(K, S, seed):
    """multi_variants for any K: aimed at snake 0 and at snake K - 1, two-snake variants only where there are two; the
    variants that add a cell at cell C - 1; every snake dead and cleared under a food value of 2"""
    torch.manual_seed(seed)
    env = MultiSnake(num_envs=1, num_snakes=K, size=S, device='cpu', manual_setup=False)
    f0, h0, b0, d0 = env.foods.clone(), env.heads.clone(), env.bodies.clone(), env.dones.clone()
    out = []

    def add(name, f, h, b, d):
        out.append((name, f.clone(), h.clone(), b.clone(), d.clone()))

    def cell(t, s, v):
        ys, xs = np.nonzero(t[s, 0].numpy() == v)
        return int(ys[0]), int(xs[0])

    occupied = (f0[0, 0] + h0[:, 0].sum(0) + b0[:, 0].sum(0)).numpy()
    free = [(y, x) for y in range(1, S - 1) for x in range(1, S - 1) if occupied[y, x] == 0]
    z = K - 1
    add('valid', f0, h0, b0, d0)
    if K > 1:
        b = b0.clone(); b[0, 0] = torch.max(b[0, 0], b0[z, 0]); add('snake_0_over_snake_z', f0, h0, b, d0)
        b = b0.clone(); h = h0.clone(); b[z] = b0[0]; h[z] = h0[0]; add('snake_z_on_top_of_snake_0', f0, h, b, d0)
        b = b0.clone(); b[0, 0, S - 1, S - 1] = 1; b[z, 0, S - 1, S - 1] = 2; add('overlap_segment_last_cell', f0, h0, b, d0)
    for s in sorted({0, z}):
        d = d0.clone(); d[s] = 1; add(f'dead_snake_{s}_with_a_body', f0, h0, b0, d)
        d = d0.clone(); d[s] = 1; h = h0.clone(); b = b0.clone(); h[s] = 0; b[s] = 0; add(f'dead_snake_{s}_cleared', f0, h, b, d)
        b[s, 0, S - 1, S - 1] = 1; add(f'dead_snake_{s}_cleared_but_the_last_cell', f0, h, b, d)
        h = h0.clone(); h[s, 0, free[0][0], free[0][1]] = 1; add(f'two_heads_for_snake_{s}', f0, h, b0, d0)
        h = h0.clone(); h[s, 0, S - 1, S - 1] = 1; add(f'two_heads_for_snake_{s}_last_cell', f0, h, b0, d0)
        h = h0.clone(); h[s] = 0; add(f'no_head_for_snake_{s}', f0, h, b0, d0)
        y, x = cell(b0, s, 2)
        b = b0.clone(); b[s, 0, y, x] = 0; add(f'body_value_2_missing_in_snake_{s}', f0, h0, b, d0)
        b = b0.clone(); b[s, 0, S - 1, S - 1] = 2; add(f'stray_body_value_in_snake_{s}_last_cell', f0, h0, b, d0)
        ty, tx = cell(b0, s, 1)
        h = h0.clone(); h[s] = 0; h[s, 0, ty, tx] = 1; add(f'head_of_snake_{s}_on_its_tail', f0, h, b0, d0)
        hy, hx = cell(b0, s, int(b0[s].max()))
        f = f0.clone(); f[0, 0, hy, hx] = 1; add(f'food_under_the_head_of_snake_{s}', f, h0, b0, d0)
        b = b0.clone(); b[s, 0] = 0; h = h0.clone(); h[s, 0] = 0; add(f'living_snake_{s}_without_cells', f0, h, b, d0)
        b = b0.clone(); b[s, 0, ty, tx] = 0; y2, x2 = cell(b0, s, 2); b[s, 0, y2, x2] = 1; b[s, 0, hy, hx] = 2
        add(f'snake_{s}_of_length_2', f0, h0, b, d0)
        for v in (0.5, 0.6, 1.5):  # the reference rounds the living envs' planes (half to even) before it checks them
            f = f0.clone(); f[0, 0, hy, hx] = v; add(f'food_{v}_under_the_head_of_snake_{s}', f, h0, b0, d0)
    f = f0.clone(); f[0, 0, free[1][0], free[1][1]] = 2; add('food_value_2', f, h0, b0, d0)
    f = f0.clone(); f[0, 0, S - 1, S - 1] = 2; add('food_value_2_last_cell', f, h0, b0, d0)
    d = torch.ones_like(d0); add('all_dead_nothing_cleared', f0, h0, b0, d)
    d = torch.ones_like(d0); add('all_dead_all_cleared', f0, torch.zeros_like(h0), torch.zeros_like(b0), d)
    add('all_dead_all_cleared_food_value_2', f, torch.zeros_like(h0), torch.zeros_like(b0), d)
    return out


SINGLE_SIZES = (8, 16, 20, 25, 36, 45, 50, 64)           # check_kernel<2> (again: 64 cells exactly), <4>, <8>, ... <64>
MULTI_SHAPES = ((1, 10), (3, 12), (4, 25), (2, 27), (10, 36), (3, 46))


def main_sizes():
    out = {'single_sizes': np.array(SINGLE_SIZES), 'multi_shapes': np.array(MULTI_SHAPES)}
    for S in SINGLE_SIZES:
        base = None
        if S < 9:  # the reference builds no env this small; its checks are functions of a tensor
            base = torch.zeros((1, 3, S, S))
            for v, x in enumerate((2, 3, 4)):
                base[0, 2, 3, x] = v + 1
            base[0, 1, 3, 4] = 1
            base[0, 0, 5, 5] = 1
        variants = single_variants(S, 10 + S, base=base, last_cell=True)
        out[f'single_S{S}_names'] = np.array([n for n, _ in variants])
        out[f'single_S{S}_envs'] = np.concatenate([e.numpy() for _, e in variants]).astype(np.float32)
        out[f'single_S{S}_snake_msg'] = np.array([verdict(lambda: ref_utils.snake_consistency(e)) for _, e in variants])
        out[f'single_S{S}_env_msg'] = np.array([verdict(lambda: ref_utils.env_consistency(e)) for _, e in variants])
        batch = torch.cat([e for _, e in variants])
        out[f'single_S{S}_batch_msg'] = np.array(verdict(lambda: ref_utils.env_consistency(batch)))
    for K, S in MULTI_SHAPES:
        variants = multi_variants_sizes(K, S, 100 + S)
        msgs = []
        for name, f, h, b, d in variants:
            env = MultiSnake(num_envs=1, num_snakes=K, size=S, device='cpu', manual_setup=True)
            env.foods, env.heads, env.bodies, env.dones = f, h, b, d
            msgs.append(verdict(env.check_consistency))
        key = f'multi_K{K}_S{S}'
        out[key + '_names'], out[key + '_msg'] = np.array([v[0] for v in variants]), np.array(msgs)
        out[key + '_foods'] = np.stack([v[1].numpy() for v in variants]).astype(np.float32)
        out[key + '_heads'] = np.stack([v[2].numpy() for v in variants]).astype(np.float32)
        out[key + '_bodies'] = np.stack([v[3].numpy() for v in variants]).astype(np.float32)
        out[key + '_dones'] = np.stack([v[4].numpy() for v in variants]).astype(np.uint8)
        for n, m in zip(out[key + '_names'], msgs):
            print(f'{key} {n:44s} {m[:60]!r}')
    path = os.path.join(HERE, 'checker_failing_states_sizes.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {os.path.getsize(path) / 1024:.0f} KiB')


def main():
    names, envs, snake_msg, env_msg = [], [], [], []
    for S, seed in ((9, 1), (12, 2)):
        for name, e in single_variants(S, seed):
            names.append(f'S{S}:{name}')
            envs.append((S, e.numpy()))
            snake_msg.append(verdict(lambda: ref_utils.snake_consistency(e)))
            env_msg.append(verdict(lambda: ref_utils.env_consistency(e)))
    out = {'single_names': np.array(names), 'single_snake_msg': np.array(snake_msg), 'single_env_msg': np.array(env_msg)}
    for i, (S, e) in enumerate(envs):
        out[f'single_env_{i}'] = e.astype(np.float32)
    # the reference on the whole batch of one size: the FIRST failing check in its own order decides the message
    for S in (9, 12):
        batch = torch.tensor(np.concatenate([e for s, e in envs if s == S]))
        out[f'single_batch_msg_S{S}'] = np.array(verdict(lambda: ref_utils.env_consistency(batch)))

    K, S = 3, 12
    mnames, mmsg = [], []
    for i, (name, f, h, b, d) in enumerate(multi_variants(K, S, 3)):
        env = MultiSnake(num_envs=1, num_snakes=K, size=S, device='cpu', manual_setup=True)
        env.foods, env.heads, env.bodies, env.dones = f, h, b, d
        mnames.append(name)
        mmsg.append(verdict(env.check_consistency))
        out[f'multi_foods_{i}'], out[f'multi_heads_{i}'] = f.numpy().astype(np.float32), h.numpy().astype(np.float32)
        out[f'multi_bodies_{i}'], out[f'multi_dones_{i}'] = b.numpy().astype(np.float32), d.numpy().astype(np.uint8)
    out['multi_names'], out['multi_msg'], out['multi_shape'] = np.array(mnames), np.array(mmsg), np.array([K, S])
    path = os.path.join(HERE, 'checker_failing_states.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {os.path.getsize(path) / 1024:.0f} KiB')
    for n, a, b in zip(names, snake_msg, env_msg):
        print(f'{n:40s} snake: {a[:60]!r:64s} env: {b[:60]!r}')
    for n, m in zip(mnames, mmsg):
        print(f'multi {n:36s} {m[:70]!r}')


if __name__ == '__main__':
    main_sizes() if '--sizes' in sys.argv[1:] else main()

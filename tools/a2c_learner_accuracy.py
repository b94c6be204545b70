#!/usr/bin/env python3
"""err = max|g - g64| / max|g64| per parameter block (and for the losses and values) of the fused A2C learner and of
torch's fp32 autograd of the same loss, for the shapes of tests/test_a2c_learner_gpu.py, plus the clip + Adam metric
max|dtheta - dtheta64| / lr.  Writes profiles/r08_a2c_learner_accuracy.json (or --out).  Needs the GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tests import a2c_learner_ref as ref  # noqa: E402
from tests import test_a2c_learner_gpu as t  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r08_a2c_learner_accuracy.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool needs the GPU'
    result = {'bound': 'err(fused) <= 4 * err(torch fp32) + 1e-6', 'grad': [], 'apply': []}
    cases = [c + (1.0,) for c in t.GRAD_CASES] + [(27, 5, 65, 'smooth_l1', 0.01, 1.0, 30.0)]
    for E, T, N, value_loss, ent, scale, wp in cases:
        fx = ref.make_fixture(E, T, N, seed=3 if wp > 1 else 0, reward_scale=scale, wp_scale=wp)
        _, _, g, losses, spec, t32 = t.fused_and_references(fx, ent, value_loss)
        l = torch.stack([losses['value_loss'], losses['policy_loss'], losses['entropy']])
        ef, et = ref.block_errors(g, spec['grad'], E), ref.block_errors(t32['grad'], spec['grad'], E)
        ef['losses'], et['losses'] = ref.rel_err(l, spec['losses']), ref.rel_err(t32['losses'], spec['losses'])
        ef['values'], et['values'] = ref.rel_err(losses['values'], spec['values']), ref.rel_err(t32['values'], spec['values'])
        result['grad'].append({'E': E, 'T': T, 'N': N, 'value_loss': value_loss, 'entropy_coef': ent, 'reward_scale': scale,
                               'wp_scale': wp, 'fused': ef, 'torch_fp32': et})
    for P in (1481, 36929):
        for step in (1, 2, 1000):
            for scale, kind in ((1e-3, 'small'), (10.0, 'large')):
                gen = torch.Generator().manual_seed(P + step)
                theta = (torch.rand(P, generator=gen) - 0.5).to(t.DEV)
                g = (torch.randn(P, generator=gen) * scale).to(t.DEV)
                m, u = (torch.randn(P, generator=gen) * 1e-2).to(t.DEV), (torch.rand(P, generator=gen) * 1e-3).to(t.DEV)
                new, norm, _, _ = t.fused_apply(theta, g, m, u, step, 0.5)
                d64, n64, _, _ = t.torch_adam(theta, g, m, u, step, torch.float64, 0.5)
                d32, n32, _, _ = t.torch_adam(theta, g, m, u, step, torch.float32, 0.5)
                result['apply'].append({
                    'P': P, 'step': step, 'gradient': kind,
                    'fused_dtheta_over_lr': float(((new.double() - theta.double()) - d64).abs().max() / 1e-3),
                    'torch_fp32_dtheta_over_lr': float((d32 - d64).abs().max() / 1e-3),
                    'fused_norm': float((norm - n64).abs() / n64), 'torch_fp32_norm': float((n32 - n64).abs() / n64)})
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()

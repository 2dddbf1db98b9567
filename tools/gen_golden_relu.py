#!/usr/bin/env python3
"""Reference recordings of the ReLU hidden layers of the Obs-DP and CENT policies (TEST INFRASTRUCTURE; runs on a host
that has the Python reference, never on the GPU box).  The reference's four row-MLP runners build their policy with
``hidden_nonlinearity = F.relu if args.hidden_nonlinearity == 'relu' else torch.tanh`` (exp_runners/*/runner_*_obsDP.py,
runner_*_cent.py).  This tool records oracle/gen_golden.py's record_variants and record_ppo_step with F.relu injected
into the two reference policy constructors they call, and writes into tests/golden/:

  variants_relu_{pp_map10,co_map20,pp_map30}.npz   N = 4 / 24 / 72: as variants_*.npz (probabilities with and without
                                                   the avail mask, greedy actions, entropy, log-likelihood, the scalar
                                                   and parameter gradients of both policies, the Gaussian baseline)
  ppo_step_{obsdp,cent}_relu.npz                   as ppo_step_{obsdp,cent}.npz: two optimiser steps of the reference's
                                                   CentralizedMAPPO

The injection wraps the classes on the namespace that oracle.ref_loader.load_reference_variants returns (the one both
recorders load); nothing under oracle/ changes.  The Gaussian baseline and the Comm-DP critic keep tanh, as in the
runners.  Deterministic: re-running it reproduces the fixtures exactly.

Usage:  python tools/gen_golden_relu.py [--out tests/golden] [--only NAME]
"""
import argparse
import os
import sys

import numpy as np
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden, ref_loader  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def _install_relu():
    """Replace the two policy classes on the reference namespace by subclasses whose default is F.relu."""
    ns = ref_loader.load_reference_variants(ref_loader.load_reference())
    for name in ('DecCategoricalMLPPolicy', 'CentralizedCategoricalMLPPolicy'):
        base = getattr(ns, name)
        if getattr(base, '_relu_injected', False):
            continue

        def init(self, *a, _base=base, **k):
            k.setdefault('hidden_nonlinearity', F.relu)
            _base.__init__(self, *a, **k)
        setattr(ns, name, type(name, (base,), {'__init__': init, '_relu_injected': True}))
    return ns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=GOLDEN)
    ap.add_argument('--only', default=None)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    _install_relu()

    def env(name):                                           # the committed env recordings
        return np.load(os.path.join(GOLDEN, f'env_{name}.npz'))
    jobs = {'variants_relu_pp_map10': lambda: gen_golden.record_variants(env('pp_map10_cap2'), 4),
            'variants_relu_co_map20': lambda: gen_golden.record_variants(env('co_map20'), 24, take=3),
            'variants_relu_pp_map30': lambda: gen_golden.record_variants(env('pp_map30_cap4'), 72, take=2),
            'ppo_step_obsdp_relu': lambda: gen_golden.record_ppo_step(seed=12, kind='obsdp'),
            'ppo_step_cent_relu': lambda: gen_golden.record_ppo_step(seed=13, kind='cent')}
    for name, fn in jobs.items():
        if args.only and name != args.only:
            continue
        path = os.path.join(args.out, name + '.npz')
        np.savez_compressed(path, **fn())
        print(f'{name:28s} {os.path.getsize(path) / 1024:8.1f} KiB')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Reference recordings of Comm-DP nets whose layer sizes are NOT the default (TEST INFRASTRUCTURE; runs on a host that
has the Python reference, never on the GPU box).  The reference's Comm-DP runners take --encoder_hidden_sizes,
--embedding_dim and --categorical_mlp_hidden_sizes from the command line (exp_runners/env_uitils.py:83-90) and pass them
to CommCategoricalMLPPolicy, and the first two to CommBaseCritic as well (runner_*_commDP.py:49-74).  This tool records
oracle/gen_golden.py's record_net_grads and record_ppo_step with

    encoder_hidden_sizes=(96, 48)   embedding_dim=32   categorical_mlp_hidden_sizes=(48, 24)

injected as the defaults of the two reference constructors they call, and writes into tests/golden/:

  shapes_net_grads_{pp_map10,co_map20}.npz   N = 4 (d = 21) / N = 24 (d = 77): as net_grads_*.npz (probabilities,
                                             attention, values, the PPO-shaped scalar, the Gaussian NLL and the gradient
                                             of each with respect to every parameter)
  shapes_ppo_step.npz                        as ppo_step.npz: two optimiser steps of the reference's CentralizedMAPPO

The injection wraps the classes on the namespace that oracle.ref_loader.load_reference returns (the one both recorders
load); nothing under oracle/ changes.  Deterministic: re-running it reproduces the fixtures exactly.

Usage:  python tools/gen_golden_shapes.py [--out tests/golden] [--only NAME]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden, ref_loader  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
ENCODER, EMBEDDING, HEAD = (96, 48), 32, (48, 24)


def _install_shapes():
    """Replace the two Comm-DP classes on the reference namespace by subclasses whose size kwargs default to the test shape."""
    ns = ref_loader.load_reference()
    extra = {'CommCategoricalMLPPolicy': dict(categorical_mlp_hidden_sizes=HEAD), 'CommBaseCritic': {}}
    for name, more in extra.items():
        base = getattr(ns, name)
        if getattr(base, '_shapes_injected', False):
            continue

        def init(self, *a, _base=base, _more=more, **k):
            k.setdefault('encoder_hidden_sizes', ENCODER)
            k.setdefault('embedding_dim', EMBEDDING)
            for key, v in _more.items():
                k.setdefault(key, v)
            _base.__init__(self, *a, **k)
        setattr(ns, name, type(name, (base,), {'__init__': init, '_shapes_injected': True}))
    return ns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=GOLDEN)
    ap.add_argument('--only', default=None)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    _install_shapes()

    def env(name):                                           # the committed env recordings
        return np.load(os.path.join(GOLDEN, f'env_{name}.npz'))
    jobs = {'shapes_net_grads_pp_map10': lambda: gen_golden.record_net_grads(env('pp_map10_cap2'), 4, take=2),
            'shapes_net_grads_co_map20': lambda: gen_golden.record_net_grads(env('co_map20'), 24, take=2),
            'shapes_ppo_step': lambda: gen_golden.record_ppo_step(kind='comm')}
    for name, fn in jobs.items():
        if args.only and name != args.only:
            continue
        path = os.path.join(args.out, name + '.npz')
        np.savez_compressed(path, **fn())
        print(f'{name:28s} {os.path.getsize(path) / 1024:8.1f} KiB')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Reference recordings of the entropy settings of CentralizedMAPPO (TEST INFRASTRUCTURE; runs on a host that has the
Python reference, never on the GPU box).  Writes into tests/golden/:

  ppo_epoch_max_{obsdp,cent,comm}.npz   one reference train_once with entropy_method='max', center_adv=False,
                                        stop_entropy_gradient=True, policy_ent_coeff=0.1, 3 minibatches x 3 mini-epochs
                                        (positive_adv=True for CENT): the process_samples tensors, the permutation drawn,
                                        the weights before / after, LossBefore / LossAfter / Entropy (tabular) and the
                                        full-batch losses before / after the update, and the rewards and
                                        advantages of every compute_advantages call (11: loss before, 9 steps, loss after)
  ppo_step_entropy_switches.npz         two full-batch optimiser steps (as oracle/gen_golden.py record_ppo_step records
                                        them) of the Obs-DP nets in 'regularized' mode with use_softplus_entropy=True:
                                        loss and policy gradients, prefixes sp. (entropy gradient on) and spstop.
                                        (stop_entropy_gradient=True), from the same initial weights pol0. / crit0.

Comm-DP patch: with stop_entropy_gradient=True the reference's _compute_policy_entropy calls
self.policy.entropy(obs, avail_actions) (centralized_ma_ppo.py:509-514), but CommCategoricalMLPPolicy.entropy also needs
dist_adj and channels (comm_categorical_mlp_policy.py:121), so train_once raises TypeError at loss_before.  For the Comm-DP
recording algo._compute_policy_entropy is replaced by the reference's own non-stop-gradient Comm-DP call
(policy.entropy(obs, avail, dist_adj, channels), + the softplus the method applies) inside torch.no_grad(): the evident
intent of the stop-gradient branch, and what com_marl_amd computes.

The reference module's get_gpu_alloc reads GPU memory; it is stubbed (0.0) so that train_once runs on the CPU.
Deterministic: re-running it reproduces the fixtures exactly.

Usage:  python tools/gen_golden_entropy.py [--out tests/golden] [--only NAME]
"""
import argparse
import contextlib
import io
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402
from oracle.gen_golden import pp_params  # noqa: E402

PPO_MODULE = "com_marl.torch.algos.centralized_ma_ppo"


def _setup(seed, kind, **algo_kw):
    """record_ppo_step's set-up (PP map10 N=4, Tmax 12, reference sampler, two paths cut short) with other algo kwargs
    -> (ns, algo, policy, critic, paths)."""
    ns = ref_loader.load_reference_ppo(ref_loader.load_reference())
    if kind != 'comm':
        ref_loader.load_reference_variants(ns)
    sys.modules[PPO_MODULE].get_gpu_alloc = lambda device=0: 0.0
    params = pp_params(10, 1, 0.04, 2, max_env_steps=12)
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    env = ns.PredatorPreyWrapper(centralized=True, params=dict(params))
    spec = ref_loader.make_env_spec(84)

    class Shell:                      # what GarageEnv adds for the sampler: .spec, attribute passthrough
        def __init__(self, e):
            self.__dict__['_e'] = e
            self.__dict__['spec'] = spec

        def __getattr__(self, k):
            return getattr(self.__dict__['_e'], k)
    if kind == 'comm':
        policy = ns.CommCategoricalMLPPolicy(spec, n_agents=4)
    elif kind == 'obsdp':
        policy = ns.DecCategoricalMLPPolicy(spec, 4, hidden_sizes=[128, 64, 32], name='dec_categorical_mlp_policy')
    else:
        policy = ns.CentralizedCategoricalMLPPolicy(spec, n_agents=4, hidden_sizes=[128, 64, 32], name='centralized')
    critic = (ns.GaussianMLPBaseline(env_spec=spec, hidden_sizes=(64, 64, 64)) if kind == 'cent'
              else ns.CommBaseCritic(spec, n_agents=4))
    with torch.no_grad():
        for net in (policy, critic):
            for name, p in net.named_parameters():
                if name.endswith('bias') and 'gcn' not in name:
                    p.uniform_(-0.1, 0.1)
    kw = dict(max_path_length=12, discount=0.99, center_adv=True, positive_adv=False, gae_lambda=0.97, policy_ent_coeff=0.1,
              entropy_method='regularized', stop_entropy_gradient=False, clip_grad_norm=7, optimization_n_minibatches=3,
              optimization_mini_epochs=10, device='cpu')
    kw.update(algo_kw)
    algo = ns.CentralizedMAPPO(env_spec=spec, policy=policy, baseline=critic, **kw)
    sampler = ns.ReferenceSampler(algo, Shell(env), n_envs=1)
    sampler.start_worker()
    paths = sampler.obtain_samples(0, batch_size=9 * 12 * 4)
    for i, n in ((1, 5), (4, 9)):                            # ragged batch, as record_ppo_step
        for k, v in list(paths[i].items()):
            if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == 12 and k != 'success':
                paths[i][k] = v[:n]
    return ns, algo, policy, critic, paths


def _weights(out, prefix, policy, critic):
    for name, p in policy.state_dict().items():
        out[f'pol{prefix}.' + name] = p.detach().clone().numpy()
    for name, p in critic.state_dict().items():
        out[f'crit{prefix}.' + name] = p.detach().clone().numpy()


def record_epoch_max(seed, kind, positive_adv):
    """One reference train_once in entropy_method='max' (see the module docstring)."""
    ns, algo, policy, critic, paths = _setup(seed, kind, entropy_method='max', center_adv=False, positive_adv=positive_adv,
                                             stop_entropy_gradient=True, optimization_n_minibatches=3,
                                             optimization_mini_epochs=3)
    mod = sys.modules[PPO_MODULE]
    if kind == 'comm':                                       # the patch of the module docstring
        def entropy_nograd(obs, avail_actions, dist_adj, channels, actions=None):
            with torch.no_grad():
                h = algo.policy.entropy(obs, avail_actions, dist_adj, channels)
            return torch.nn.functional.softplus(h) if algo._use_softplus_entropy else h
        algo._compute_policy_entropy = entropy_nograd
    out = dict(kind=np.array(kind), positive_adv=np.int32(positive_adv), ent_coeff=np.float32(0.1))
    _weights(out, '0', policy, critic)
    calls_r, calls_a = [], []
    orig_ca, orig_ps, orig_perm, orig_rec = mod.compute_advantages, algo.process_samples, np.random.permutation, mod.tabular.record
    rec, tab = {}, {}

    def compute_advantages(discount, gae_lambda, T, baselines, rewards, device):
        adv = orig_ca(discount, gae_lambda, T, baselines, rewards, device)
        calls_r.append(rewards.detach().clone().numpy())
        calls_a.append(adv.detach().clone().numpy())
        return adv

    def process_samples(itr, paths_):
        res = orig_ps(itr, paths_)
        rec['samples'] = [None if t is None else t.detach().clone() for t in res]
        return res

    losses = []
    orig_loss = algo._compute_loss

    def compute_loss(*a, **k):
        loss = orig_loss(*a, **k)
        losses.append(float(loss))
        return loss
    algo._compute_loss = compute_loss

    def permutation(n):
        perm = orig_perm(n)
        rec['perm'] = np.asarray(perm)
        return perm

    def record(k, v):
        tab[k] = v
        return orig_rec(k, v)

    class Runner:
        step_itr, step_path = 0, paths
    mod.compute_advantages, algo.process_samples, np.random.permutation, mod.tabular.record = (compute_advantages, process_samples,
                                                                                               permutation, record)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            algo.train_once(Runner())
    finally:
        mod.compute_advantages, np.random.permutation, mod.tabular.record = orig_ca, orig_perm, orig_rec
    obs, avail, actions, rewards, valids, baselines, returns, dist_adjs, channels = rec['samples']
    P, T = rewards.shape
    out.update(obs=obs.numpy(), actions=actions.numpy().astype(np.int32), rewards=rewards.numpy(),
               valids=np.asarray(valids, np.int32), baselines=baselines.numpy(), returns=returns.numpy(),
               dist_adjs=dist_adjs.numpy(), channels=channels.numpy(),
               rewards64=np.stack([np.pad(np.asarray(p['rewards'], np.float64), (0, T - len(p['rewards']))) for p in paths]),
               perm=rec['perm'].astype(np.int64), n_calls=np.int32(len(calls_a)))
    for i, (r, a) in enumerate(zip(calls_r, calls_a)):
        out[f'call{i}.rewards'] = r
        out[f'call{i}.adv'] = a
    for k in ('LossBefore', 'LossAfter', 'Entropy'):
        out[k] = np.float64(tab[k])
    # the tabular LossBefore is the last minibatch's loss (:361 records loss.item()); the full-batch loss before the update
    # (:198-201, what com_marl_amd logs as LossBefore) is the first _compute_loss call
    out['loss_before_full'] = np.float64(losses[0])
    out['loss_after_full'] = np.float64(losses[-1])
    _weights(out, '1', policy, critic)
    return out


def record_step_switches(seed=14):
    """Two full-batch optimiser steps of the Obs-DP nets, regularized + softplus entropy, with and without the entropy's
    gradient: the weights before, then loss, critic loss and every policy gradient of each step."""
    out = {}
    for tag, stop in (('sp', False), ('spstop', True)):
        ns, algo, policy, critic, paths = _setup(seed, 'obsdp', use_softplus_entropy=True, stop_entropy_gradient=stop)
        with contextlib.redirect_stdout(io.StringIO()):
            obs, avail, actions, rewards, valids, baselines, returns, dist_adjs, channels = algo.process_samples(0, paths)
        P, T = rewards.shape
        if tag == 'sp':
            out.update(obs=obs.numpy(), actions=actions.numpy().astype(np.int32), rewards=rewards.numpy(),
                       valids=np.asarray(valids, np.int32), baselines=baselines.numpy(), returns=returns.numpy(),
                       dist_adjs=dist_adjs.numpy(), channels=channels.numpy(),
                       rewards64=np.stack([np.pad(np.asarray(p['rewards'], np.float64), (0, T - len(p['rewards'])))
                                           for p in paths]))
        if tag == 'sp':
            _weights(out, '0', policy, critic)
        else:                                                # same seed: the same initial weights
            assert all(np.array_equal(out['pol0.' + k], v.numpy()) for k, v in policy.state_dict().items())
        for step in (1, 2):
            loss = algo._compute_loss(0, obs, avail, actions, rewards, valids, baselines, dist_adjs, channels)
            bl = critic.compute_loss(obs, returns, dist_adjs, channels)
            algo._baseline_optimizer.zero_grad()
            bl.backward()
            algo._optimizer.zero_grad()
            loss.backward()
            out[f'{tag}.loss{step}'] = loss.detach().numpy()
            out[f'{tag}.critic_loss{step}'] = bl.detach().numpy()
            for name, p in policy.named_parameters():
                out[f'{tag}.gpol{step}.' + name] = p.grad.clone().numpy()
            torch.nn.utils.clip_grad_norm_(policy.parameters(), 7)
            algo._optimizer.step()
            algo._baseline_optimizer.step()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    ap.add_argument('--only', default=None)
    args = ap.parse_args()
    jobs = {'ppo_epoch_max_obsdp': lambda: record_epoch_max(21, 'obsdp', False),
            'ppo_epoch_max_cent': lambda: record_epoch_max(22, 'cent', True),
            'ppo_epoch_max_comm': lambda: record_epoch_max(23, 'comm', False),
            'ppo_step_entropy_switches': lambda: record_step_switches()}
    for name, fn in jobs.items():
        if args.only and name != args.only:
            continue
        path = os.path.join(args.out, name + '.npz')
        np.savez_compressed(path, **fn())
        print(f'{name:28s} {os.path.getsize(path) / 1024:8.1f} KiB')


if __name__ == '__main__':
    main()

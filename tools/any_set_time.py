"""Policy sets of non-default Comm-DP nets on one MI355X (DESIGN.md §7 "Sets of any layer sizes"): wall time of
evaluate.eval_models_co over K = 8 checkpoints on 1024 envs of CO map 20 (teams of 24, 128 envs per checkpoint, 128 episodes each,
max_env_steps = 200, greedy, one round) with the set's forward as ONE cm_policy_forward_any_multi launch per step
(nets.PolicySet(..., any_sizes=True)) against one cm_policy_forward_any launch per member per step (the set without the keyword;
a mixed set cannot be built without it, so its member-by-member leg is the same set with the engine's multi_forward pinned to
"member").  Two workloads:
  same    8 checkpoints of the m0 shape: encoder (96, 48), embedding 32, head (48, 24);
  mixed   m0, m1, m2, m0, ...: m1 = (40,) | 16 | (100, 20, 12, 8), 'dot', no residual, no GCN bias; m2 = (8, 128, 24) | 128 | (5,).
Whole calls on the host clock, each ending in a synchronise; both legs are warmed up first and their results compared (==), then they
alternate for three rounds; every call gets a fresh wrapper of the same seed.  Forward launches per step are counted from the
engine's form: 1 for "set", K for "member".
    python tools/any_set_time.py [same|mixed]       one workload, no argument both"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from com_marl_amd import envs as E, evaluate, nets  # noqa: E402
from com_marl_amd.evaluate import eval_models_co  # noqa: E402
from com_marl_amd.rollout import RolloutEngine  # noqa: E402

T, ROUNDS, SEED, K, B = 200, 3, 3, 8, 1024
CO = dict(load=2, max_env_steps=T, capture_reward=2, step_cost=0, rm=0, penalty=1, revisit_penalty=0.5, lazy_penalty=1, grid_size=20,
          Rsen=2, n_agents=24, n_preys=0, n_gcn_layers=2, mode="test", teRcom=19, tepl=0, obstComplex="Easy", add_clock=0)
FAMILIES = {
    "m0": dict(encoder_hidden_sizes=(96, 48), embedding_dim=32, categorical_mlp_hidden_sizes=(48, 24)),
    "m1": dict(encoder_hidden_sizes=(40,), embedding_dim=16, categorical_mlp_hidden_sizes=(100, 20, 12, 8), attention_type="dot",
               residual=False, gcn_bias=False),
    "m2": dict(encoder_hidden_sizes=(8, 128, 24), embedding_dim=128, categorical_mlp_hidden_sizes=(5,)),
}
WORKLOADS = {"same": ["m0"] * K, "mixed": [("m0", "m1", "m2")[k % 3] for k in range(K)]}


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


class _Engine(RolloutEngine):
    """The engine eval_models builds, remembered; pin = "member": the forward launched member by member from the start."""
    used, pin = [], None

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        if _Engine.pin and self.multi_forward is not None:
            self.multi_forward = _Engine.pin
        _Engine.used.append(self)


def run(name):
    fams = WORKLOADS[name]
    wrapper = lambda: E.CoverageWrapper(True, params=CO, n_envs=B, device="cuda:0", seed=SEED)     # noqa: E731
    first = wrapper()
    pols = []
    for k, f in enumerate(fams):
        torch.manual_seed(k)
        p = nets.CommCategoricalMLPPolicy(first.spec, n_agents=CO["n_agents"], device="cuda:0", **FAMILIES[f])
        p.set_rng(SEED)
        pols.append(p)
    one_set = nets.PolicySet(pols, any_sizes=True)
    # the member loop: the parent's route for checkpoints of one shape; a mixed set exists only with the keyword
    loop_set = nets.PolicySet(pols) if name == "same" else one_set
    kw = dict(n_eval_episodes=B // K, max_env_steps=T, eval_greedy=True)
    evaluate.RolloutEngine = _Engine

    def leg(ps, pin):
        _Engine.pin, _Engine.used = pin, []
        env = wrapper()
        dt, out = sync_time(lambda: eval_models_co(env, ps, 0, **kw))
        form = _Engine.used[-1].multi_forward
        return dt, out, form

    legs = {"set": (one_set, None), "member": (loop_set, "member" if name == "mixed" else None)}
    got = {}
    for which, (ps, pin) in legs.items():                  # warm-up of both legs, and the comparison
        _, got[which], form = leg(ps, pin)
        assert form == which, (which, form)
    same = got["set"] == got["member"]
    print(f"{name}: eval_models_co of the set launch equals the member loop's: {same}", flush=True)
    print(f"{name}: forward launches per step: set 1, member {K}; success of the first episodes "
          f"{[round(sum(r[1]) / len(r[1]), 3) for r in got['set']]}", flush=True)
    rounds = {"set": [], "member": []}
    for r in range(ROUNDS):
        for which, (ps, pin) in legs.items():
            dt, _, form = leg(ps, pin)
            assert form == which
            rounds[which].append(dt)
            print(f"[{r}] {name} {which:6s} {B} envs, {K} policies x {B // K} episodes x {T} steps: {dt * 1e3:9.2f} ms", flush=True)
    print(json.dumps({"workload": name, "members": fams, "envs": B, "policies": K, "episodes_per_policy": B // K, "steps": T,
                      "results_equal": bool(same), "forward_launches_per_step": {"set": 1, "member": K},
                      "set_ms": [round(x * 1e3, 3) for x in rounds["set"]],
                      "member_ms": [round(x * 1e3, 3) for x in rounds["member"]],
                      "set_ahead_in_every_round_against_every_round": bool(max(rounds["set"]) < min(rounds["member"]))}), flush=True)
    return same


if __name__ == "__main__":
    names = sys.argv[1:] or list(WORKLOADS)
    ok = [run(name) for name in names]
    sys.exit(0 if all(ok) else 1)

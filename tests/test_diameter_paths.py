"""params['calc_diameter'] through the layers above the kernel: the engine's diameter slots and the sampler's
paths[i]['diameters'] (eager and hipGraph spans, two rollouts in a row), the single-env wrapper's .diameter, the PPO class's
Diameter column on both stat routes, and the unchanged answers with the switch off or with Rcom == 0.  Everything is compared
with tests/graph_ref.py applied to the dist_adjs the same path holds."""
import numpy as np
import pytest

from tests import graph_ref

pytestmark = pytest.mark.gpu

MPL = 6


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    return torch


def _pp_params(rcom, **extra):
    return dict(load=2, max_env_steps=MPL, capture_reward=10, step_cost=0.1, rm=0, penalty=0, grid_size=10, Rsen=1, n_agents=4,
                n_preys=4, n_gcn_layers=2, mode="train", trRcom=rcom, trpl=0, seed=5, **extra)


def _co_params(rcom, **extra):
    return dict(load=2, max_env_steps=10, capture_reward=2, step_cost=0, rm=0, penalty=1, revisit_penalty=0.5, lazy_penalty=1,
                grid_size=20, Rsen=2, n_agents=24, n_preys=0, n_gcn_layers=2, mode="train", trRcom=rcom, trpl=0,
                obstComplex="Easy", add_clock=0, seed=5, **extra)


def _setup(torch, scenario, params, B):
    from com_marl_amd import envs as E, nets
    from com_marl_amd.algos import CentralizedMAPPO
    from com_marl_amd.sampler import CentralizedMAOnPolicyVectorizedSampler
    cls = E.PredatorPreyWrapper if scenario == "pp" else E.CoverageWrapper
    env = cls(centralized=True, params=params, n_envs=B, device="cuda:0")
    torch.manual_seed(5)
    pol = nets.CommCategoricalMLPPolicy(env.spec, n_agents=env.n_agents, device="cuda:0")
    crit = nets.CommBaseCritic(env.spec, n_agents=env.n_agents, device="cuda:0")
    pol.set_rng(5)
    algo = CentralizedMAPPO(env_spec=env.spec, policy=pol, baseline=crit, max_path_length=params["max_env_steps"], discount=0.99,
                            center_adv=True, positive_adv=False, gae_lambda=0.97, policy_ent_coeff=0.1,
                            entropy_method='regularized', stop_entropy_gradient=False, clip_grad_norm=7,
                            optimization_n_minibatches=3, optimization_mini_epochs=10, device="cuda:0")
    smp = CentralizedMAOnPolicyVectorizedSampler(algo, env, n_envs=B)
    smp.start_worker()
    return env, algo, smp


def _check_paths(paths, N):
    """Every path's diameters against graph_ref on the SAME path's dist_adjs, step by step -> all values seen."""
    seen = []
    assert len(paths) > 0
    for i in range(len(paths)):
        p = paths[i]
        d = p["diameters"]
        n = len(p["rewards"])
        assert d.shape == (n,) and d.dtype == np.asarray([0, 1]).dtype          # np.asarray(list of ints), as the reference's
        np.testing.assert_array_equal(d, graph_ref.diameters(p["dist_adjs"], n=N), err_msg=f"path {i}")
        assert p["ave_degs"].shape == (n,)
        seen.append(d)
    return np.concatenate(seen)


@pytest.mark.parametrize("use_graph", [False, True])
def test_path_diameters_follow_the_dist_adjs(torch_cuda, use_graph):
    B, N = 8, 4
    env, algo, smp = _setup(torch_cuda, "pp", _pp_params(2, calc_diameter=True), B)
    bs = B * N * MPL + 3                                             # into the second episode: several spans of 4 slots
    values = []
    for itr in range(2):                                             # the second rollout reuses the engine (and its span graphs)
        paths = smp.obtain_samples(itr, batch_size=bs, chunk=4, use_graph=use_graph)
        eng = smp.engine
        assert eng.diameter is not None and eng.diameter.dtype == torch_cuda.int32
        assert tuple(eng.diameter.shape) == tuple(eng.dist_adj.shape[:2])
        values.append(_check_paths(paths, N))
        # the slots themselves, slot 0 (the reset's) included
        T = smp.last_steps
        np.testing.assert_array_equal(eng.diameter[:T + 1].cpu().numpy(), graph_ref.diameters(eng.dist_adj[:T + 1].cpu().numpy()))
    assert smp.last_steps > 4                                        # more than one span was run
    print("PP map 10 diameters seen:", np.bincount(np.concatenate(values)).tolist())


def test_run_chunk_fills_the_carried_slot(torch_cuda):
    """run_chunk: slots 0 .. n as they stand behind the chunk, slot 0 being the one its tail carried over."""
    from com_marl_amd.rollout import RolloutEngine
    env, algo, smp = _setup(torch_cuda, "pp", _pp_params(2, calc_diameter=True), 8)
    eng = RolloutEngine(env.batch, algo.policy, horizon=5)
    eng.reset()
    for use_graph in (False, True):
        eng.run_chunk(use_graph=use_graph)
        torch_cuda.cuda.synchronize()
        adj = eng.dist_adj.cpu().numpy()
        np.testing.assert_array_equal(adj[0], adj[5])
        np.testing.assert_array_equal(eng.diameter.cpu().numpy(), graph_ref.diameters(adj))


@pytest.mark.parametrize("scenario", ["pp", "co"])
def test_single_env_wrapper_diameter_follows_reset_and_step(torch_cuda, scenario):
    from com_marl_amd import envs as E
    if scenario == "pp":
        env = E.PredatorPreyWrapper(centralized=True, params=_pp_params(2, calc_diameter=True), n_envs=1, device="cuda:0")
    else:
        env = E.CoverageWrapper(centralized=True, params=_co_params(3, calc_diameter=True), n_envs=1, device="cuda:0")
    rng = np.random.default_rng(0)
    env.reset()
    seen = []
    for _ in range(2 * MPL + 1):                                     # PP: across an auto-reset
        d = env.diameter
        assert isinstance(d, int) and d == graph_ref.diameter(env.dist_adj)
        seen.append(d)
        env.step(rng.integers(0, 5, env.n_agents))
    print(scenario, "wrapper diameters:", seen)


def test_coverage_diameter_column_on_both_stat_routes(torch_cuda):
    B, N = 4, 24
    env, algo, smp = _setup(torch_cuda, "co", _co_params(3, calc_diameter=True), B)
    paths = smp.obtain_samples(0, batch_size=B * N * 10 * 2)
    d = _check_paths(paths, N)
    assert (d == 0).any() and (d > 0).any(), np.bincount(d)          # disconnected and connected teams both occur
    want = float(np.mean([np.mean(graph_ref.diameters(paths[i]["dist_adjs"], n=N)) for i in range(len(paths))]))
    a = algo.process_samples(0, paths)
    dev = algo._log_performance(0, paths, a[6], a[4])                # device gather
    dicts = [paths[i] for i in range(len(paths))]
    b = algo.process_samples(0, dicts)
    host = algo._log_performance(0, dicts, b[6], b[4])               # path dicts
    assert want > 0
    np.testing.assert_allclose(dev["Diameter"], want, rtol=1e-12)
    np.testing.assert_allclose(host["Diameter"], want, rtol=1e-12)
    np.testing.assert_allclose(dev["AveDegree"], host["AveDegree"], rtol=1e-6)


@pytest.mark.parametrize("switch", [{}, {"calc_diameter": False}, {"calc_diameter": None}])
def test_switch_off_or_absent_keeps_the_zeros(torch_cuda, switch):
    B, N = 8, 4
    env, algo, smp = _setup(torch_cuda, "pp", _pp_params(2, **switch), B)
    paths = smp.obtain_samples(0, batch_size=B * N * MPL + 3, chunk=4)
    assert smp.engine.dist_adj is not None and smp.engine.diameter is None
    for i in range(len(paths)):
        d = paths[i]["diameters"]
        assert d.shape == (len(paths[i]["rewards"]),) and (d == 0).all()
    assert env.diameter == 0
    a = algo.process_samples(0, paths)
    assert algo._log_performance(0, paths, a[6], a[4])["Diameter"] == 0.0


def test_full_range_keeps_n(torch_cuda):
    """trRcom = 9 on map 10 is Rcom == 0: get_graph returns n_agents whatever the switch says (env_communication.py:219-223)."""
    B, N = 8, 4
    env, algo, smp = _setup(torch_cuda, "pp", _pp_params(9, calc_diameter=True), B)
    paths = smp.obtain_samples(0, batch_size=B * N * MPL + 3, chunk=4)
    assert smp.engine.dist_adj is None and smp.engine.diameter is None
    for i in range(len(paths)):
        assert (paths[i]["diameters"] == N).all()
    assert env.diameter == N
    a = algo.process_samples(0, paths)
    assert algo._log_performance(0, paths, a[6], a[4])["Diameter"] == float(N)

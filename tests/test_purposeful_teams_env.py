"""The HIP env step against the CPU oracle where a purposeful team plays (tests/purposeful_teams.py): one case per kernel
form, both sides in lockstep on the production Philox stream, actions from the script computed on the oracle's state.  Compared
after the steps the case names (every step, or every tenth and the last), all exact: done, reward (f64 and f32), details,
agent_pos, step_count, success, rng_step, the prey state or visited / total_capture, obs, dist_adj, channels, ge_state.  The Coverage cases start from the
near-complete snapshot, loaded into both sides.  At the end the oracle's tallies are held to the floors of
tests/test_purposeful_teams_cpu.py, so that a later change of a case cannot hollow the comparison out."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import purposeful_teams as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need the MI355X")
    from tests import hip_adapters
    return hip_adapters


def make_hip(case, hip):
    c = P.CASES[case]
    cfg = O.make_cfg(**c["cfg"], rng_mode=O.RNG_PHILOX, seed=P.SEED)
    if not c.get("conditions"):
        return hip.HipEnv(cfg)
    from com_marl_amd import envs as E

    class CondHipEnv(hip.HipEnv):
        """HipEnv on a batch built with a per-env condition table."""

        def __init__(self):
            scen, p, ch = hip.params_from_cfg(cfg)
            self.cfg = cfg
            self.batch = E.GridEnvBatch(scen, p, cfg.n_envs, device="cuda:0", seed=cfg.seed, max_steps=cfg.max_steps,
                                        max_path_length=cfg.max_path_length, channel=ch, conditions=c["conditions"],
                                        condition_of=np.asarray(c["condition_of"]))
            b = self.batch
            self.B, self.N, self.M, self.S, self.d = b.B, b.N, b.M, b.S, b.d

    return CondHipEnv()


@pytest.mark.parametrize("case", P.PP_CASES)
def test_pp_env_step_matches_oracle_under_a_chasing_team(case, hip):
    t = P.play(case, other=make_hip(case, hip))
    print(f"\n{case}: {t}")
    P.check_pp_floors(case, t)


@pytest.mark.parametrize("case", P.CO_CASES)
def test_co_env_step_matches_oracle_through_full_coverage(case, hip):
    t = P.play(case, other=make_hip(case, hip))
    print(f"\n{case}: {t}")
    P.check_co_floors(case, t)

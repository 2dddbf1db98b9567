"""COMMARL_POLICY_KERNEL selects the kernel family of the default-shape Comm-DP forward (truth table: csrc/cm_policy_host.h).  The
library reads it once per process, so each setting runs in a fresh child process (tests/hip_child.py::_policy_kernel_case, started by
tests/conftest.py before this process touches the GPU): the acting forward of teams of 4 (d = 21, one hop, 19 envs) and of 8 (d = 29,
two hops, 7 envs) against the torch module and against evaluate_nograd, with the tolerances of tests/test_hip_policy_parity.py."""
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("setting", ["unset", "h", "f32", "valu"])
def test_acting_forward_under_every_setting_of_the_switch(setting):
    from tests.conftest import child_result
    res = child_result("policy_kernel_" + setting)
    assert res["rc"] == 0, f"child case policy_kernel_{setting} failed:\n{res['tail']}"
    rep = res["report"]
    assert rep.get("ok") is True and rep["shapes"] == [[4, 21, 1, 19], [8, 29, 2, 7]], rep
    assert rep["setting"] == ("w" if setting == "unset" else setting[0]), rep

"""The run-time-sized critic forward (cm_critic_forward_any) and the any-width graph ops (cm_*_any, csrc/cm_graph_any.hip), the
part that needs no GPU: the library exports the seven symbols, argument errors come back as codes with a text, the slab of
the deterministic twin has one E-float row per workgroup, and the ISA of the new kernels has no private segment and no
spill.  (tests/test_cabi.py holds the header and the ctypes binding to each other.)"""
import ctypes as C

import pytest

from tests import isa

NEW = ("cm_critic_forward_any", "cm_attention_forward_any", "cm_attention_backward_any", "cm_masked_agg_forward_any",
       "cm_masked_agg_backward_any", "cm_masked_agg_backward_any_det", "cm_masked_agg_backward_any_det_ws_bytes")


def test_library_exports_the_new_symbols():
    from com_marl_amd import _lib as L
    lib = L.lib()
    for n in NEW:
        assert n in L.EXPORTED and hasattr(lib, n), n
    assert L.TWINS["cm_masked_agg_backward_any"] == ("cm_masked_agg_backward_any_det", "cm_masked_agg_backward_any_det_ws_bytes")


def test_null_arguments_return_an_error_code_and_a_text():
    from com_marl_amd import _lib as L
    lib = L.lib()
    p = C.c_void_p(16)                                          # plausible, never dereferenced: the checks precede every launch
    calls = {
        "cm_critic_forward_any": lambda: lib.cm_critic_forward_any(None, 4, None, None, None, None, None),
        "cm_attention_forward_any": lambda: lib.cm_attention_forward_any(3, 4, 32, None, p, p, None),
        "cm_attention_backward_any": lambda: lib.cm_attention_backward_any(3, 4, 32, p, p, p, p, None, None, None, p, None),
        "cm_masked_agg_forward_any": lambda: lib.cm_masked_agg_forward_any(3, 4, 32, p, None, None, 0, None, None, p, None),
        "cm_masked_agg_backward_any": lambda: lib.cm_masked_agg_backward_any(3, 4, 32, p, None, None, 0, p, p, None, None, p, p, None, None),
        "cm_masked_agg_backward_any_det": lambda: lib.cm_masked_agg_backward_any_det(3, 4, 32, p, None, None, 0, p, p, None, p, None, p, p,
                                                                                    p, 1 << 20, None),
    }
    for name, call in calls.items():
        assert call() == -1, name
        assert name.encode() in lib.cm_last_error(), name
    # the twin checks its slab before anything is launched
    assert lib.cm_masked_agg_backward_any_det(3, 4, 32, p, None, None, 0, p, p, None, p, p, p, p, None, 0, None) == -1
    assert lib.cm_masked_agg_backward_any_det(3, 4, 32, p, None, None, 0, p, p, None, p, p, p, p, p, 8, None) == -1
    # the critic's head has ONE output column
    w = L.NetWeights()
    w.d, w.n_agents, w.n_hops, w.n_act, w.emb, w.n_enc, w.n_head = 21, 4, 2, 5, 32, 1, 1
    assert lib.cm_critic_forward_any(C.byref(w), 4, p, None, None, p, None) == -1
    assert b"n_act" in lib.cm_last_error()


def test_shapes_outside_the_kernels_answer_without_a_gpu():
    """1 = "not for this shape" (nothing launched): the planes of one workgroup's envs above 160 KB; E outside 1..128 is an
    argument error."""
    from com_marl_amd import _lib as L
    lib = L.lib()
    p = C.c_void_p(16)
    assert lib.cm_masked_agg_forward_any(3, 128, 128, p, None, None, 0, p, None, p, None) == 1
    assert lib.cm_attention_forward_any(3, 128, 128, p, p, p, None) == 1
    assert lib.cm_attention_backward_any(3, 200, 32, p, p, p, p, None, None, p, p, None) == 1
    assert lib.cm_masked_agg_backward_any(3, 128, 128, p, None, None, 0, p, p, None, p, p, p, None, None) == 1
    for E in (0, 129):
        assert lib.cm_masked_agg_forward_any(3, 4, E, p, None, None, 0, p, None, p, None) < 0
        assert lib.cm_attention_forward_any(3, 4, E, p, p, p, None) < 0
    w = L.NetWeights()
    w.d, w.n_agents, w.n_hops, w.n_act, w.emb, w.n_enc, w.n_head = 21, 80, 2, 1, 128, 2, 1
    w.enc_hidden[0], w.enc_hidden[1], w.head_hidden[0] = 128, 128, 128
    assert lib.cm_critic_forward_any(C.byref(w), 4, p, None, None, p, None) == 1
    w.emb = 200
    assert lib.cm_critic_forward_any(C.byref(w), 4, p, None, None, p, None) == 1


@pytest.mark.parametrize("S,N,E", [(1, 4, 1), (37, 4, 32), (2047, 5, 12), (2048, 24, 48), (2300, 5, 12), (100000, 80, 128)])
def test_det_slab_is_one_row_per_workgroup(S, N, E):
    from com_marl_amd import _lib as L
    assert L.lib().cm_masked_agg_backward_any_det_ws_bytes(S, N, E) == min(S, 2048) * E * 4


def test_graph_op_route_without_a_gpu():
    from com_marl_amd import nets
    assert nets.graph_op_route(4, 32) == "hip" and nets.graph_op_route(200, 32) == "framework"
    assert nets.graph_op_route(4, 129) == "framework"
    nets.set_graph_op_route(4, 32, "framework")
    try:
        assert nets.graph_op_route(4, 32) == "framework"
    finally:
        nets.set_graph_op_route(4, 32, None)
    assert nets.graph_op_route(4, 32) == "hip"
    with pytest.raises(ValueError):
        nets.set_graph_op_route(4, 32, "fast")


@pytest.mark.parametrize("unit,names", [
    ("cm_graph_any", ("agg_fwd_any_kernel", "agg_bwd_any_kernel", "agg_bwd_any_kernel", "attn_fwd_any_kernel", "attn_bwd_any_kernel")),
    ("cm_critic_g", ("fwd_any_kernel",)),
    ("cm_policy_g", ("fwd_any_kernel",)),
])
def test_new_kernels_have_no_private_segment_and_no_spill(unit, names):
    ks = isa.kernels(isa.listing(unit))
    assert sorted(names) == sorted(next(n for n in names if n in k.name) for k in ks), [k.name for k in ks]
    for k in ks:
        assert k.private_segment_fixed_size == 0, k.name
        assert k.vgpr_spill_count == 0, k.name
        assert not k.has_flat_or_scratch, k.name
    if unit == "cm_critic_g":                                   # the critic's dense layers are the policy's: f32 MFMA only
        assert ks[0].count("v_mfma_f32_16x16x4_f32") >= 8 and ks[0].count("v_mfma_") == ks[0].count("v_mfma_f32_16x16x4_f32")

"""ctypes binding of libcommarl_hip.so (the C ABI declared in include/commarl.h).

There is no fallback: if the HIP library is missing or does not load, importing the
binding raises.  Nothing in this package routes through oracle/ or a CPU path.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# COMMARL_LIB selects another build of the same ABI (e.g. the -DCM_BOUNDS checked build)
LIB_PATH = os.environ.get("COMMARL_LIB") or os.path.join(HERE, "libcommarl_hip.so")

CM_PP, CM_CO = 0, 1
PACK_F32, PACK_F16, PACK_WAVE, PACK_CHECK, PACK_ALL = 1, 2, 4, 8, 15      # cm_*_pack_sections (include/commarl.h)
CHANNELS = {"FC": 0, "FL": 1, "IID": 2, "GE": 3}
RNG_PHILOX, RNG_TAPE = 0, 1
ENT_ADD, ENT_SOFTPLUS, ENT_STOP_GRAD = 1, 2, 4                              # cm_ppo_surrogate's add_entropy bits
EPI_COLS, SUM_COLS = 9, 12                                                  # cm_episode_stats / cm_episode_means row widths
COMM_COLS, EPC_COLS = 4, 4                                                  # cm_comm_stats / cm_episode_comm, cm_comm_means row widths
ATTN_COLS, EPA_COLS = 6, 6                                                  # cm_attn_stats / cm_episode_attn, cm_attn_means row widths
LISTEN_COLS, EPL_COLS = 6, 6                                                # cm_listen_stats / cm_episode_listen, cm_listen_means row widths
VALUE_COLS, EPV_COLS = 6, 6                                                 # cm_value_stats / cm_episode_value, cm_value_means row widths
BOOT_OUT, BOOT_MAX_R = 4, 4096                                              # cm_boot_quantiles: lo, hi, se, p_gt per key; resamples per call
BOOT_COLUMNS, BOOT_COMM, BOOT_VALUE = 0, 1, 2                               # cm_boot_quantiles' kinds -> 4 / 6 / 9, 5, 7 keys
# cm_ppo_update_stats' row: CM_UPD_COLS columns, in the order of their CM_UPD_* indices
UPD_COLUMNS = ("n_valid", "approx_kl", "kl", "clip_frac", "ratio_min", "ratio_max", "entropy", "stopped")
UPD_COLS = len(UPD_COLUMNS)
# cm_segment_episodes' table: CM_SEG_COLS columns, in the order of their CM_SEG_* indices (details_0..4: CM_SEG_DETAILS + k)
SEG_COLUMNS = ("count", "ret_sum", "ret_sumsq", "ret_min", "ret_max", "disc_sum", "len_sum", "success") + tuple(
    f"details_{k}" for k in range(5))
SEG_COLS = len(SEG_COLUMNS)


class EnvCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "scenario", "n_envs", "n_agents", "n_preys", "grid", "rsen", "load", "max_steps", "max_path_length",
        "n_hops", "rcom", "channel", "obst_hard", "add_clock", "rng_mode", "env_id_offset")] + [
        ("ploss", C.c_float), ("pgb", C.c_float), ("pbg", C.c_float), ("ge_flags", C.c_int32)] + [
        (n, C.c_double) for n in ("capture_reward", "step_cost", "move_cost", "penalty", "lazy_penalty",
                                  "revisit_penalty", "final_reward")] + [("seed", C.c_uint64)]


class RngTape(C.Structure):
    _fields_ = [("prey", C.c_void_p), ("spawn", C.c_void_p), ("spawn_cap", C.c_int32), ("_pad", C.c_int32),
                ("iid_u", C.c_void_p), ("ge_u", C.c_void_p), ("ge_init_u", C.c_void_p)]


class StepOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("obs", "reward", "reward_f64", "done", "details", "dist_adj", "channels",
                                          "prey_alive", "success", "path_len")]


class EnvState(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("agent_pos", "prey_pos", "prey_alive", "visited", "step_count",
                                          "total_capture", "success", "ge_state", "rng_step")]


class EnvCond(C.Structure):
    """cm_env_cond: one env's comm condition (cm_env_set_conditions); envs.COND_DTYPE is the same record for numpy."""
    _fields_ = [("rcom", C.c_int32), ("ploss", C.c_float), ("pgb", C.c_float), ("pbg", C.c_float), ("rng_id", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class PolicyWeights(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("d", "n_agents", "n_hops", "enc_hidden", "emb", "h1", "h2", "h3", "n_act",
                                         "no_residual")] + [
        (n, C.c_void_p) for n in ("enc_w1t", "enc_b1", "enc_w2t", "enc_b2", "attn_wt", "gcn_w", "gcn_b", "hd_w1t",
                                  "hd_b1", "hd_w2t", "hd_b2", "hd_w3t", "hd_b3", "hd_w4t", "hd_b4", "mfma_pack")]


class CriticWeights(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("d", "n_agents", "n_hops", "enc_hidden", "emb", "dec_hidden",
                                         "no_residual", "_pad")] + [
        (n, C.c_void_p) for n in ("enc_w1t", "enc_b1", "enc_w2t", "enc_b2", "attn_wt", "gcn_w", "gcn_b", "dec_w1t",
                                  "dec_b1", "dec_w2t", "dec_b2", "mfma_pack")]


class NetWeights(C.Structure):
    """cm_net_weights: a Comm-DP policy or critic of any layer sizes (cm_policy_forward_any, cm_critic_forward_any)."""
    _fields_ = [(n, C.c_int32) for n in ("d", "n_agents", "n_hops", "n_act", "no_residual", "emb", "n_enc")] + [
        ("enc_hidden", C.c_int32 * 3), ("n_head", C.c_int32), ("head_hidden", C.c_int32 * 4), ("_pad", C.c_int32),
        ("enc_wt", C.c_void_p * 4), ("enc_b", C.c_void_p * 4), ("attn_wt", C.c_void_p), ("gcn_w", C.c_void_p),
        ("gcn_b", C.c_void_p), ("head_wt", C.c_void_p * 5), ("head_b", C.c_void_p * 5)]


class ChunkStrides(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("obs", "actions", "probs", "attn", "reward", "reward_f64", "done", "details",
                                         "dist_adj", "channels", "prey_alive", "success", "path_len")]


class PolicySetT(C.Structure):
    """cm_policy_set: device tables of a multi-policy chunk (cm_rollout_chunk_multi)."""
    _fields_ = [("n_policies", C.c_int32), ("n_wg", C.c_int32), ("packs", C.c_void_p), ("wg_policy", C.c_void_p)]


class ForwardSetWg(C.Structure):
    """cm_forward_set_wg: one workgroup of a cm_policy_forward_multi launch."""
    _fields_ = [("member", C.c_int32), ("block", C.c_int32)]


class ForwardSetMember(C.Structure):
    """cm_forward_set_member: one member's group and weight pointers in the table cm_policy_forward_multi reads."""
    _fields_ = [("first_env", C.c_int32), ("n_envs", C.c_int32)] + [
        (n, C.c_void_p) for n in ("pack", "enc_b1", "enc_b2", "gcn_b", "hd_b1", "hd_b2", "hd_b3", "hd_b4")]


class AnySetMember(C.Structure):
    """cm_any_set_member: one member's group, layer sizes, plane strides and weight pointers in the table
    cm_policy_forward_any_multi reads."""
    _fields_ = [(n, C.c_int32) for n in ("first_env", "n_envs", "emb", "no_residual", "n_enc")] + [
        ("enc_h", C.c_int32 * 3), ("n_head", C.c_int32), ("head_h", C.c_int32 * 4), ("SE", C.c_int32), ("SW", C.c_int32),
        ("_pad", C.c_int32), ("enc_w", C.c_void_p * 3), ("enc_b", C.c_void_p * 3), ("enc_wo", C.c_void_p), ("enc_bo", C.c_void_p),
        ("attn_wt", C.c_void_p), ("gcn_w", C.c_void_p), ("gcn_b", C.c_void_p), ("head_w", C.c_void_p * 4),
        ("head_b", C.c_void_p * 4), ("head_wo", C.c_void_p), ("head_bo", C.c_void_p)]


MLP_MAX_LAYERS = 6


class FwdSaves(C.Structure):
    """cm_fwd_saves: device pointers of the activations the training forward stores (include/commarl.h)."""
    _fields_ = [("a1", C.c_void_p), ("e", C.c_void_p), ("q", C.c_void_p), ("hw", C.c_void_p * 4), ("h", C.c_void_p * 4),
                ("x1", C.c_void_p), ("x2", C.c_void_p), ("x3", C.c_void_p), ("out", C.c_void_p), ("probs", C.c_void_p)]


class MlpWeights(C.Structure):
    _fields_ = [("in_dim", C.c_int32), ("n_layers", C.c_int32), ("out_dim", C.c_int32 * MLP_MAX_LAYERS),
                ("tanh_mask", C.c_int32), ("relu_mask", C.c_int32), ("wt", C.c_void_p * MLP_MAX_LAYERS),
                ("b", C.c_void_p * MLP_MAX_LAYERS), ("mfma_pack", C.c_void_p)]


class MlpSetMember(C.Structure):
    """cm_mlp_set_member: one member's rows and per-layer pointers in the table cm_mlp_policy_forward_multi reads."""
    _fields_ = [("first_row", C.c_int32), ("n_rows", C.c_int32), ("first_env", C.c_int32), ("_pad", C.c_int32),
                ("b", C.c_void_p * MLP_MAX_LAYERS), ("pack", C.c_void_p * MLP_MAX_LAYERS)]


# every symbol include/commarl.h declares, with its signature
_SIGNATURES = {
    "cm_abi_version": (C.c_int, []),
    "cm_last_error": (C.c_char_p, []),
    "cm_env_create": (C.c_int, [C.POINTER(EnvCfg), C.POINTER(C.c_void_p)]),
    "cm_env_destroy": (C.c_int, [C.c_void_p]),
    "cm_env_obs_dim": (C.c_int, [C.c_void_p]),
    "cm_env_n_empty_cells": (C.c_int, [C.c_void_p]),
    "cm_env_adj_is_const": (C.c_int, [C.c_void_p]),
    "cm_env_channels_are_const": (C.c_int, [C.c_void_p]),
    "cm_env_fill_constants": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_env_reset": (C.c_int, [C.c_void_p, C.POINTER(RngTape), C.POINTER(StepOut), C.c_void_p]),
    "cm_env_step": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RngTape), C.POINTER(StepOut), C.c_void_p]),
    "cm_env_status": (C.c_int, [C.c_void_p]),
    "cm_env_get_state": (C.c_int, [C.c_void_p, C.POINTER(EnvState)]),
    "cm_env_set_state": (C.c_int, [C.c_void_p, C.POINTER(EnvState)]),
    "cm_env_set_conditions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_env_has_conditions": (C.c_int, [C.c_void_p]),
    "cm_env_fuse_conditions": (C.c_int, [C.c_void_p, C.c_int32]),
    "cm_policy_forward": (C.c_int, [C.POINTER(PolicyWeights), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_critic_forward": (C.c_int, [C.POINTER(CriticWeights), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "cm_policy_forward_any": (C.c_int, [C.POINTER(NetWeights), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_critic_forward_any": (C.c_int, [C.POINTER(NetWeights), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "cm_rollout_step": (C.c_int, [C.c_void_p, C.POINTER(PolicyWeights), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_uint64, C.c_int32, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.POINTER(RngTape), C.POINTER(StepOut), C.c_void_p]),
    "cm_rollout_chunk": (C.c_int, [C.c_void_p, C.POINTER(PolicyWeights), C.c_int32, C.POINTER(ChunkStrides), C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32, C.c_void_p, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(StepOut), C.c_void_p]),
    "cm_rollout_chunk_multi": (C.c_int, [C.c_void_p, C.POINTER(PolicyWeights), C.POINTER(PolicySetT), C.c_int32,
                                         C.POINTER(ChunkStrides), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32,
                                         C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(StepOut), C.c_void_p]),
    "cm_policy_forward_multi_plan": (C.c_int64, [C.POINTER(PolicyWeights), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_void_p,
                                                 C.c_size_t, C.POINTER(C.c_int32)]),
    "cm_policy_forward_multi": (C.c_int, [C.POINTER(PolicyWeights), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32, C.c_void_p, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_policy_forward_any_multi_plan": (C.c_int64, [C.POINTER(NetWeights), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_void_p,
                                                     C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]),
    "cm_policy_forward_any_multi": (C.c_int, [C.POINTER(NetWeights), C.c_void_p, C.c_int32, C.c_int32, C.c_size_t, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32, C.c_void_p,
                                              C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_rollout_chunk_tail": (C.c_int, [C.c_void_p, C.POINTER(PolicyWeights), C.c_int32, C.POINTER(ChunkStrides), C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32, C.c_void_p, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(StepOut), C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "cm_policy_pack_bytes": (C.c_size_t, [C.POINTER(PolicyWeights)]),
    "cm_policy_pack": (C.c_int, [C.POINTER(PolicyWeights), C.c_void_p, C.c_void_p]),
    "cm_policy_pack_sections": (C.c_int, [C.POINTER(PolicyWeights), C.c_void_p, C.c_int32, C.c_void_p]),
    "cm_critic_pack_sections": (C.c_int, [C.POINTER(CriticWeights), C.c_void_p, C.c_int32, C.c_void_p]),
    "cm_critic_pack_bytes": (C.c_size_t, [C.POINTER(CriticWeights)]),
    "cm_critic_pack": (C.c_int, [C.POINTER(CriticWeights), C.c_void_p, C.c_void_p]),
    "cm_mlp_policy_forward": (C.c_int, [C.POINTER(MlpWeights), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32, C.c_void_p, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_mlp_forward_multi_plan": (C.c_int64, [C.POINTER(MlpWeights), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]),
    "cm_mlp_policy_forward_multi": (C.c_int, [C.POINTER(MlpWeights), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32, C.c_void_p,
                                              C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_mlp_pack_bytes": (C.c_size_t, [C.POINTER(MlpWeights)]),
    "cm_mlp_pack": (C.c_int, [C.POINTER(MlpWeights), C.c_void_p, C.c_void_p]),
    "cm_mlp_value_forward": (C.c_int, [C.POINTER(MlpWeights), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_masked_agg_forward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_masked_agg_backward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "cm_masked_agg_backward_r": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int32, C.c_void_p]),
    "cm_attention_forward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_attention_backward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # the same four for any embedding width 1..128 (csrc/cm_graph_any.hip)
    "cm_masked_agg_forward_any": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_masked_agg_backward_any": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    "cm_attention_forward_any": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_attention_backward_any": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_linear_wgrad": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "cm_policy_forward_saved_wave": (C.c_int, [C.POINTER(PolicyWeights), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.POINTER(FwdSaves), C.c_void_p]),
    "cm_critic_forward_saved_wave": (C.c_int, [C.POINTER(CriticWeights), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.POINTER(FwdSaves), C.c_void_p]),
    "cm_policy_forward_saved": (C.c_int, [C.POINTER(PolicyWeights), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(FwdSaves), C.c_void_p]),
    "cm_critic_forward_saved": (C.c_int, [C.POINTER(CriticWeights), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.POINTER(FwdSaves), C.c_void_p]),
    "cm_env_agent_condition": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_env_agent_fault": (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_uint32, C.c_void_p]),
    "cm_comm_delays": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                 C.c_void_p, C.c_void_p]),
    "cm_graph_diameter": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_episode_stats": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "cm_episode_means": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_comm_stats": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                C.c_void_p]),
    "cm_episode_comm": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "cm_comm_means": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    # per-step evaluation curves (csrc/cm_episode_curves.hip)
    "cm_episode_curves": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "cm_curve_means": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_comm_curves": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                 C.c_int32, C.c_void_p, C.c_void_p]),
    "cm_comm_curve_means": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    # attention statistics (csrc/cm_attn_stats.hip): cm_attn_stats, then the twins of the four comm reductions above
    "cm_attn_stats": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                C.c_void_p, C.c_void_p]),
    "cm_episode_attn": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "cm_attn_means": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_attn_curves": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                 C.c_int32, C.c_void_p, C.c_void_p]),
    "cm_attn_curve_means": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    # listening statistics (csrc/cm_listen_stats.hip): cm_listen_stats, then the attention reductions with every column per agent
    "cm_listen_stats": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                  C.c_void_p, C.c_void_p]),
    "cm_episode_listen": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_void_p, C.c_void_p]),
    "cm_listen_means": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_listen_curves": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_void_p, C.c_void_p]),
    "cm_listen_curve_means": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    # critic statistics (csrc/cm_value_stats.hip): cm_value_stats, then the attention reductions with every column per step
    "cm_value_stats": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                 C.c_void_p]),
    "cm_episode_value": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                   C.c_void_p]),
    "cm_value_means": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_value_curves": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "cm_value_curve_means": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    # bootstrap intervals and paired contrasts of the episode tables (csrc/cm_boot.hip)
    "cm_boot_means": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "cm_boot_quantiles": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                    C.c_void_p]),
    "cm_chunk_tail": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cm_linear_act_forward": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                        C.c_int32, C.c_void_p, C.c_void_p]),
    "cm_linear_act_backward": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_linear_act_backward_ex": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_encoder_backward": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_multi_copy_t": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_multi_adam_step": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_void_p]),
    "cm_gauss_nll_forward": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "cm_gauss_nll_backward": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_adam_bias_corrections": (None, [C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_void_p]),
    "cm_multi_adam_step_dev": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.c_void_p]),
    "cm_ppo_surrogate": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_float, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_entropy_gae": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                 C.c_float, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_discount_returns": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                      C.c_void_p]),
    "cm_gae": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int32,
                         C.c_float, C.c_void_p, C.c_void_p]),
    # deterministic update mode: slab-workspace twins (include/commarl.h)
    "cm_linear_act_backward_det_ws_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "cm_linear_act_backward_det": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                             C.c_void_p]),
    "cm_linear_act_backward_ex_det": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_size_t, C.c_void_p]),
    "cm_encoder_backward_det_ws_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "cm_encoder_backward_det": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cm_masked_agg_backward_det_ws_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "cm_masked_agg_backward_det": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cm_masked_agg_backward_any_det_ws_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "cm_masked_agg_backward_any_det": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cm_linear_wgrad_det_ws_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "cm_linear_wgrad_det": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_size_t, C.c_void_p]),
    "cm_ppo_surrogate_det_ws_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "cm_ppo_surrogate_det": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_float, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    "cm_gauss_nll_forward_det_ws_bytes": (C.c_size_t, [C.c_int64]),
    "cm_gauss_nll_forward_det": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.c_void_p]),
    # per-step PPO update statistics and the device-side KL early stop (csrc/cm_ppo_stats.hip; the gated Adam is in cm_optim.hip)
    "cm_ppo_update_stats_ws_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "cm_ppo_update_stats": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_float, C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                      C.c_void_p]),
    "cm_multi_adam_step_gated": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_void_p]),
    # fixed-length rollout segments (csrc/cm_segments.hip): bootstrapped targets, batch-wide normalisation, episode bookkeeping
    "cm_segment_targets": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cm_adv_normalize_ws_bytes": (C.c_size_t, []),
    "cm_adv_normalize": (C.c_int, [C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cm_segment_episodes_ws_bytes": (C.c_size_t, [C.c_int32]),
    "cm_segment_episodes": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
}
EXPORTED = tuple(_SIGNATURES)

_lib = None


class CommarlError(RuntimeError):
    pass


def lib():
    """The loaded library.  Fails loudly when the HIP extension is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CommarlError(
                f"{LIB_PATH} not found: build it with `make -C com-marl_amd/csrc` (or __graft_entry__.build()). "
                "There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)      # AttributeError if the .so does not export a declared symbol
            fn.restype, fn.argtypes = res, args
        if L.cm_abi_version() != 3:
            raise CommarlError("libcommarl_hip.so ABI version mismatch")
        _lib = L
    return _lib


def slab(nbytes, device):
    """A slab workspace for a cm_*_det twin: torch memory (from the graph pool under capture), contents ignored."""
    import torch
    return torch.empty(max(1, (int(nbytes) + 3) // 4), dtype=torch.float32, device=device)


# deterministic update mode: default entry point -> (its slab twin, the twin's slab size).  A twin takes the default's
# arguments up to its last output pointer (so bias_replicas of _r and the GaussWs of cm_gauss_nll_forward are dropped),
# then (slab, slab bytes, stream).
TWINS = {
    "cm_linear_act_backward": ("cm_linear_act_backward_det", "cm_linear_act_backward_det_ws_bytes"),
    "cm_linear_act_backward_ex": ("cm_linear_act_backward_ex_det", "cm_linear_act_backward_det_ws_bytes"),
    "cm_encoder_backward": ("cm_encoder_backward_det", "cm_encoder_backward_det_ws_bytes"),
    "cm_masked_agg_backward": ("cm_masked_agg_backward_det", "cm_masked_agg_backward_det_ws_bytes"),
    "cm_masked_agg_backward_r": ("cm_masked_agg_backward_det", "cm_masked_agg_backward_det_ws_bytes"),
    "cm_masked_agg_backward_any": ("cm_masked_agg_backward_any_det", "cm_masked_agg_backward_any_det_ws_bytes"),
    "cm_linear_wgrad": ("cm_linear_wgrad_det", "cm_linear_wgrad_det_ws_bytes"),
    "cm_ppo_surrogate": ("cm_ppo_surrogate_det", "cm_ppo_surrogate_det_ws_bytes"),
    "cm_gauss_nll_forward": ("cm_gauss_nll_forward_det", "cm_gauss_nll_forward_det_ws_bytes"),
}


def run(name, *args, device=None, maybe=False):
    """Entry point `name` with `args` on the current stream (of `device`, made current for the call, when given), its return
    code checked -> True.  maybe: a return of 1 ("not for this shape, nothing done") -> False instead of raising."""
    if device is None:
        rc = getattr(lib(), name)(*args, current_stream())
    else:
        import torch
        with torch.cuda.device(device):
            rc = getattr(lib(), name)(*args, current_stream())
    if rc == 0:
        return True
    if maybe and rc == 1:
        return False
    check(rc, name)


def launch(name, args, ws_args, device=None, maybe=False):
    """run(name, *args) - or, in deterministic mode, of its twin instead (TWINS), with a slab of twin_ws_bytes(*ws_args) bytes on
    the current device."""
    from . import deterministic
    if not deterministic():
        return run(name, *args, device=device, maybe=maybe)
    import torch
    twin, ws_bytes = TWINS[name]
    with torch.cuda.device(device):
        nb = getattr(lib(), ws_bytes)(*ws_args)
        n = len(_SIGNATURES[twin][1]) - 3
        return run(twin, *args[:n], ptr(slab(nb, "cuda")), nb, maybe=maybe)


def check(rc, what=""):
    if rc != 0:
        msg = lib().cm_last_error()
        raise CommarlError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def ptr(t):
    """Raw device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    assert t.is_contiguous(), "C ABI takes contiguous buffers"
    return t.data_ptr()


def cptr(t):
    """ptr() of `t` made contiguous (None for None)."""
    return None if t is None else t.contiguous().data_ptr()


def current_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---- hipGraph captures must not contain a hipFree: env handles released while a capture is open (a garbage-collected
# GridEnvBatch -> cm_env_destroy -> hipFree invalidated a capture in round 2) are parked here and destroyed afterwards ----
_capture_depth = 0
_deferred_env_handles = []


def destroy_env(handle):
    """cm_env_destroy now, or after the innermost open capture_guard() has closed."""
    if _capture_depth > 0:
        _deferred_env_handles.append(handle)
        return
    lib().cm_env_destroy(handle)


class capture_guard:
    """``with capture_guard(): <stream capture>``: keeps the cyclic collector off while the capture is open and defers every
    env-handle destruction requested meanwhile (a refcount reaching zero) to the exit.  (No gc.collect() here: a full
    collection costs ~50 ms in a process that has torch loaded, and a sampler captures dozens of span graphs.)"""

    def __enter__(self):
        global _capture_depth
        import gc
        self._gc_was_on = gc.isenabled()
        gc.disable()
        _capture_depth += 1
        return self

    def __exit__(self, *exc):
        global _capture_depth
        import gc
        _capture_depth -= 1
        if self._gc_was_on:
            gc.enable()
        if _capture_depth == 0:
            while _deferred_env_handles:
                lib().cm_env_destroy(_deferred_env_handles.pop())
        return False

"""Batched Predator-Prey / Coverage envs on one MI355X, behind the reference's env interface.

``GridEnvBatch`` owns B independent envs whose SoA state lives in HBM and is advanced by the
HIP step kernel (csrc/cm_env.hip) through the C ABI.  ``PredatorPreyWrapper`` /
``CoverageWrapper`` keep the constructor and attribute surface of the reference wrappers
(envs/predatorprey_wrapper.py:23-73, envs/coverage_wrapper.py:16-57) so that
``runner_pp_commDP.py`` / ``runner_co_commDP.py`` construct them unchanged; the only new
knobs are the keyword-only ``n_envs``, ``device``, ``seed`` (default: params['seed']).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L


def _round_int(v):
    return int(v) if float(v) == int(v) else v


class _Discrete:
    def __init__(self, n):
        self.n = n
        self.flat_dim = n


class _Box:
    def __init__(self, low, high):
        self.low, self.high = np.asarray(low, np.float32), np.asarray(high, np.float32)
        self.shape = self.low.shape
        self.flat_dim = int(np.prod(self.shape))


class EnvSpec:
    """What the nets read from garage's EnvSpec (comm_base_net.py:36-41)."""

    def __init__(self, observation_space, action_space):
        self.observation_space, self.action_space = observation_space, action_space


def make_cfg(scenario, params, n_envs, *, seed=1, env_id_offset=0, rng_mode=L.RNG_PHILOX, max_steps=None,
             max_path_length=None, channel=None):
    """params dict -> (cm_env_cfg, channel type, loss probability, calc_diameter), following predator_prey.py:52-82,
    coverage.py:40-96 and env_communication.py:10-75 (signs: costs are stored as -abs(x)).  calc_diameter
    (env_communication.py:20) is no field of cm_env_cfg: the env step does not know the switch, the diameters are derived
    from the dist_adj it records (graph_diameter below)."""
    p = params
    c = L.EnvCfg()
    pp = scenario == "pp"
    c.scenario = L.CM_PP if pp else L.CM_CO
    c.n_envs, c.n_agents = int(n_envs), int(p["n_agents"])
    c.n_preys = int(p.get("n_preys", 0)) if pp else 0
    c.grid, c.rsen, c.load = int(p["grid_size"]), int(p["Rsen"]), int(p.get("load", 2))
    if pp:
        c.max_steps = int(max_steps if max_steps is not None else p["max_env_steps"])          # :59
    else:
        c.max_steps = int(max_steps if max_steps is not None else 400)                         # coverage.py:39,47
    c.max_path_length = int(max_path_length if max_path_length is not None else p.get("max_env_steps", c.max_steps))
    c.n_hops = int(p["n_gcn_layers"])
    pref = "tr" if p.get("mode", "train") in ("train", "restore") else "te"                    # env_communication.py:25-29
    pl = p.get(f"{pref}pl")
    if pl is None:
        raise ValueError("Loss probability is not applied (params['trpl'/'tepl'])")
    if channel is None:                                                                         # :35-43
        channel = "FC" if pl == 0 else ("FL" if pl == 1 else "IID")
        if not (0 <= pl <= 1):
            raise ValueError(f"invalid Ploss value: pl={pl}")
    c.channel = L.CHANNELS[channel]
    c.ploss, c.pgb, c.pbg = float(pl), float(p.get("Pgb", 0.0196)), float(p.get("Pbg", 0.282))
    # GE variants (env_communication.py:21,54-60,106-157): GE_INIT 1 good / 0 bad / else random; loss_apply 0 = one
    # state transition per env step shared by all hops, 1 (default) = one per GCN hop
    gi = p.get("GE_INIT", 1)
    la = p.get("loss_apply", 1)
    c.ge_flags = (0 if (la is None or la) else 1) | ((0 if gi in (1, None) else (1 if gi == 0 else 2)) << 1)
    c.rcom = int(p.get(f"{pref}Rcom", 9))
    c.obst_hard = int(p.get("obstComplex", "Easy") == "Hard")
    c.add_clock = int(p.get("add_clock") or 0)
    c.rng_mode, c.env_id_offset, c.seed = rng_mode, int(env_id_offset), int(seed)
    c.capture_reward = abs(p.get("capture_reward", 10 if pp else 2))
    c.step_cost = -abs(p.get("step_cost", 0.1 if pp else 0.0))
    c.move_cost = -abs(p.get("rm", 0))
    c.penalty = -abs(p.get("penalty", 0 if pp else 1))
    c.lazy_penalty = -abs(p.get("lazy_penalty", 1))
    c.revisit_penalty = -abs(p.get("revisit_penalty", 0.5))
    c.final_reward = 100.0                                                                      # coverage.py:92
    return c, channel, pl, bool(p.get("calc_diameter"))


# ---- per-env comm conditions (cm_env_set_conditions): pure numpy, no GPU ----------------------------------------------------
COND_KEYS = ("Rcom", "pl", "Pgb", "Pbg")
# cm_env_cond, record for record (include/commarl.h)
COND_DTYPE = np.dtype([("rcom", "<i4"), ("ploss", "<f4"), ("pgb", "<f4"), ("pbg", "<f4"), ("rng_id", "<i4"), ("reserved", "<i4", (3,))])


def conditions_channel(conditions, channel=None):
    """The channel kind of a batch built with `conditions`: the explicit one; else IID if any condition has 0 < pl < 1; else
    None - make_cfg derives it from params as it does without conditions."""
    if channel is not None:
        return channel
    for c in conditions:
        pl = c.get("pl")
        if pl is not None and 0 < pl < 1:
            return "IID"
    return None


def condition_table(scenario, params, conditions, condition_of, rng_ids=None, *, channel=None, env_id_offset=0):
    """The [B] table cm_env_set_conditions takes (structured array, COND_DTYPE): env b gets conditions[condition_of[b]] and the
    Philox env id rng_ids[b] (default env_id_offset + b: the id it has without a table).  A condition is a dict with optional keys
    Rcom, pl, Pgb, Pbg (the runners' --teRcom / --tepl / --Pgb / --Pbg); a missing key takes the value make_cfg takes from
    params.  The channel kind is one per batch (conditions_channel): ValueError for a pl given when it is not IID and for Pgb /
    Pbg given when it is not GE - the env step would not read them - as for an index outside the list, an unknown key, a
    negative Rcom and a probability outside [0, 1]."""
    conditions = [dict(c) for c in conditions]
    if not conditions:
        raise ValueError("condition_table: at least one condition")
    cond_of = np.asarray(condition_of)
    if cond_of.ndim != 1 or cond_of.size == 0 or not np.issubdtype(cond_of.dtype, np.integer):
        raise ValueError("condition_table: condition_of is an int array [B], B >= 1")
    B = cond_of.shape[0]
    if cond_of.min() < 0 or cond_of.max() >= len(conditions):
        raise ValueError(f"condition_table: condition_of names a condition outside 0..{len(conditions) - 1}")
    cfg, kind, _, _ = make_cfg(scenario, params, B, env_id_offset=env_id_offset, channel=conditions_channel(conditions, channel))
    rows = np.zeros(len(conditions), COND_DTYPE)
    for k, c in enumerate(conditions):
        extra = set(c) - set(COND_KEYS)
        if extra:
            raise ValueError(f"condition {k}: unknown keys {sorted(extra)} (a condition has {COND_KEYS})")
        if "pl" in c and kind != "IID":
            raise ValueError(f"condition {k}: pl is given but the batch's channel is {kind}, not IID: the env step would ignore it")
        if ("Pgb" in c or "Pbg" in c) and kind != "GE":
            raise ValueError(f"condition {k}: Pgb / Pbg are given but the batch's channel is {kind}, not GE: the env step would ignore them")
        rcom = c.get("Rcom", cfg.rcom)
        if int(rcom) != rcom or rcom < 0:
            raise ValueError(f"condition {k}: Rcom must be a non-negative integer, got {rcom}")
        vals = dict(pl=c.get("pl", cfg.ploss), Pgb=c.get("Pgb", cfg.pgb), Pbg=c.get("Pbg", cfg.pbg))
        for name, v in vals.items():
            if not 0 <= v <= 1:
                raise ValueError(f"condition {k}: {name}={v} is outside [0, 1]")
        rows[k]["rcom"], rows[k]["ploss"], rows[k]["pgb"], rows[k]["pbg"] = int(rcom), vals["pl"], vals["Pgb"], vals["Pbg"]
    ids = int(env_id_offset) + np.arange(B, dtype=np.int64) if rng_ids is None else np.asarray(rng_ids)
    if ids.shape != (B,) or not np.issubdtype(ids.dtype, np.integer):
        raise ValueError(f"condition_table: rng_ids is an int array [{B}]")
    if ids.min() < -2 ** 31 or ids.max() >= 2 ** 31:
        raise ValueError("condition_table: rng_ids are 32-bit Philox env ids")
    table = rows[cond_of]
    table["rng_id"] = ids
    return np.ascontiguousarray(table)


def graph_diameter(dist_adj, out=None):
    """Hop diameter of every graph of a contiguous f32 CUDA tensor [..., N, N] (cm_graph_diameter: an edge where either
    direction is non-zero, the diagonal ignored, 0 for a disconnected graph - get_graph's calc_diameter branch,
    env_communication.py:235-241) -> int32 [...].  One launch on the current stream; `out` receives the values when given."""
    assert dist_adj.is_cuda and dist_adj.dtype == torch.float32 and dist_adj.dim() >= 2 and dist_adj.shape[-1] == dist_adj.shape[-2]
    assert dist_adj.is_contiguous(), "cm_graph_diameter reads [S,N,N] through the raw pointer"
    lead, N = dist_adj.shape[:-2], dist_adj.shape[-1]
    if out is None:
        out = torch.empty(lead, dtype=torch.int32, device=dist_adj.device)
    assert out.dtype == torch.int32 and out.shape == lead and out.device == dist_adj.device and out.is_contiguous()
    L.run("cm_graph_diameter", out.numel(), N, L.ptr(dist_adj), L.ptr(out), device=dist_adj.device)
    return out


def comm_stats(dist_adj, channels, n_hops, out=None):
    """Link delivery and L-hop reach of every graph (cm_comm_stats, include/commarl.h): contiguous f32 CUDA tensors dist_adj
    [..., N, N] and channels [..., L, N, N] with the same leading shape, either None = all ones (not both: the team size comes
    from the tensors) -> int32 [..., 4]: in_range, delivered (summed over the n_hops hops), reach, range_reach.  An entry is set
    when it is != 0, the diagonals are ignored.  One launch on the current stream; `out` receives the values when given."""
    ref = dist_adj if dist_adj is not None else channels
    assert ref is not None, "comm_stats: dist_adj and channels cannot both be None"
    n_hops = int(n_hops)
    for t, tail in ((dist_adj, 2), (channels, 3)):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.dim() >= tail and t.shape[-1] == t.shape[-2])
        assert t is None or t.is_contiguous(), "cm_comm_stats reads the blocks through the raw pointer"
    N = ref.shape[-1]
    lead = dist_adj.shape[:-2] if dist_adj is not None else channels.shape[:-3]
    if channels is not None:
        assert channels.shape[-3] == n_hops and channels.shape[-1] == N and channels.shape[:-3] == lead
        assert channels.device == ref.device
    if out is None:
        out = torch.empty(*lead, L.COMM_COLS, dtype=torch.int32, device=ref.device)
    assert out.dtype == torch.int32 and out.shape == (*lead, L.COMM_COLS) and out.device == ref.device and out.is_contiguous()
    S = out.numel() // L.COMM_COLS
    L.run("cm_comm_stats", S, N, n_hops, L.ptr(dist_adj), N * N, L.ptr(channels), n_hops * N * N, L.ptr(out), device=ref.device)
    return out


def attn_stats(attn, dist_adj, channels, n_hops, out=None):
    """What a Comm-DP policy's attention does on every graph (cm_attn_stats, include/commarl.h): contiguous f32 CUDA tensors attn
    [..., N, N] (row i = agent i's softmax weights, as the forward records them), dist_adj [..., N, N] and channels [..., L, N, N]
    with the same leading shape, either mask None = all ones -> float64 [..., 6]: self, entropy, range_mass, kept_mass, eff_self,
    eff_entropy, each summed over the graph's N rows (the last three also over the n_hops hops).  A mask entry is set when it is
    != 0 and the diagonals count as recorded.  One launch on the current stream; `out` receives the values when given."""
    n_hops = int(n_hops)
    for t, tail in ((attn, 2), (dist_adj, 2), (channels, 3)):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.dim() >= tail and t.shape[-1] == t.shape[-2])
        assert t is None or t.is_contiguous(), "cm_attn_stats reads the blocks through the raw pointer"
    assert attn is not None, "attn_stats: attn is required"
    lead, N = attn.shape[:-2], attn.shape[-1]
    if dist_adj is not None:
        assert dist_adj.shape == attn.shape and dist_adj.device == attn.device
    if channels is not None:
        assert channels.shape == (*lead, n_hops, N, N) and channels.device == attn.device
    if out is None:
        out = torch.empty(*lead, L.ATTN_COLS, dtype=torch.float64, device=attn.device)
    assert out.dtype == torch.float64 and out.shape == (*lead, L.ATTN_COLS) and out.device == attn.device and out.is_contiguous()
    S = out.numel() // L.ATTN_COLS
    L.run("cm_attn_stats", S, N, n_hops, L.ptr(attn), N * N, L.ptr(dist_adj), N * N, L.ptr(channels), n_hops * N * N, L.ptr(out),
          device=attn.device)
    return out


def listen_stats(probs, mute=None, lossless=None, out=None):
    """Whether the messages changed the action distributions, per graph (cm_listen_stats, include/commarl.h): contiguous f32 CUDA
    tensors probs [..., N, A] (what the policy acted on) and mute / lossless of the same shape (what it gives under the identity
    channel / the all-ones channel), either None = identical to probs -> float64 [..., 6]: mute_kl, mute_tv, mute_flip, loss_kl,
    loss_tv, loss_flip, each summed over the graph's N agents; a None counterfactual's three columns are exact 0.  One launch on
    the current stream; `out` receives the values when given."""
    assert probs is not None, "listen_stats: probs is required"
    for t in (probs, mute, lossless):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.dim() >= 2 and t.shape == probs.shape and t.device == probs.device)
        assert t is None or t.is_contiguous(), "cm_listen_stats reads the blocks through the raw pointer"
    lead, (N, A) = probs.shape[:-2], probs.shape[-2:]
    if out is None:
        out = torch.empty(*lead, L.LISTEN_COLS, dtype=torch.float64, device=probs.device)
    assert out.dtype == torch.float64 and out.shape == (*lead, L.LISTEN_COLS) and out.device == probs.device and out.is_contiguous()
    S = out.numel() // L.LISTEN_COLS
    L.run("cm_listen_stats", S, N, A, L.ptr(probs), N * A, L.ptr(mute), N * A, L.ptr(lossless), N * A, L.ptr(out), device=probs.device)
    return out


def value_stats(rewards, path_len, values, mute=None, lossless=None, discount=0.99, out=None):
    """How well a critic's values explain the returns, per recorded step (cm_value_stats, include/commarl.h): contiguous CUDA
    tensors rewards [T, B] (float64), path_len [T, B] (int32: > 0 where an episode ended) and values [T, B] (float32), and
    mute / lossless of values' shape and type (the critic's values under the identity channel / the all-ones channel), either
    None = identical to values -> float64 [T, B, 6]: value, ret (the return-to-go discounted by `discount` within the env's
    first episode, no bootstrap), sq_err, ret_sq, msg_value = value - mute, loss_value = lossless - value; rows behind the first
    episode's end are exact zeros and a None counterfactual's column is exact 0.  One launch on the current stream; `out`
    receives the values when given."""
    assert rewards is not None and path_len is not None and values is not None, "value_stats: rewards, path_len and values are required"
    assert rewards.is_cuda and rewards.dim() == 2 and rewards.dtype == torch.float64
    assert path_len.dtype == torch.int32 and path_len.shape == rewards.shape and path_len.device == rewards.device
    for t in (values, mute, lossless):
        assert t is None or (t.dtype == torch.float32 and t.shape == rewards.shape and t.device == rewards.device)
    for t in (rewards, path_len, values, mute, lossless):
        assert t is None or t.is_contiguous(), "cm_value_stats reads the arrays through the raw pointer"
    T, B = rewards.shape
    if out is None:
        out = torch.empty(T, B, L.VALUE_COLS, dtype=torch.float64, device=rewards.device)
    assert out.dtype == torch.float64 and out.shape == (T, B, L.VALUE_COLS) and out.device == rewards.device and out.is_contiguous()
    L.run("cm_value_stats", T, B, L.ptr(rewards), L.ptr(path_len), L.ptr(values), L.ptr(mute), L.ptr(lossless), float(discount),
          L.ptr(out), device=rewards.device)
    return out


BOOT_KINDS = {"columns": L.BOOT_COLUMNS, "comm": L.BOOT_COMM, "value": L.BOOT_VALUE}   # bootstrap's kind= -> cm_boot_quantiles' kind


def boot_keys(kind, cols):
    """How many keys cm_boot_quantiles forms from rows of `cols` columns: the columns themselves (4, 6 or 9), the comm family's 5
    (its 4 columns and delivery), the value family's 7 (VALUE_KEYS from its 6 columns).  ValueError for any other pair."""
    if kind not in BOOT_KINDS or cols not in {"columns": (4, 6, 9), "comm": (4,), "value": (6,)}[kind]:
        raise ValueError(f"bootstrap: kind={kind!r} does not take rows of {cols} columns (columns: 4, 6 or 9; comm: 4; value: 6)")
    return {"columns": cols, "comm": 5, "value": 7}[kind]


def boot_ranks(level, n_boot, who="bootstrap", name="level"):
    """The order statistics of a two-sided interval at `level` from n_boot resamples -> (lo_rank, hi_rank) with
    lo_rank = min(floor((1 - level) / 2 * n_boot), (n_boot - 1) // 2) and hi_rank = n_boot - 1 - lo_rank.  ValueError (naming
    `name` / n_boot) unless 0 < level < 1 and 2 <= n_boot <= 4096."""
    if isinstance(level, bool) or not isinstance(level, (int, float)) or not 0 < level < 1:      # (a NaN fails the comparison too)
        raise ValueError(f"{who}: {name}= must be a confidence level with 0 < {name} < 1, not {level!r}")
    if isinstance(n_boot, bool) or not isinstance(n_boot, (int, np.integer)) or not 2 <= n_boot <= L.BOOT_MAX_R:
        raise ValueError(f"{who}: n_boot= must be an integer in 2..{L.BOOT_MAX_R}, not {n_boot!r}")
    lo = min(math.floor((1 - level) / 2 * n_boot), (int(n_boot) - 1) // 2)
    return lo, int(n_boot) - 1 - lo


def boot_seed_words(seed, who="bootstrap", name="seed"):
    """A bootstrap seed 0 .. 2^64 - 1 -> (lo, hi), the two Philox key words; ValueError naming `name` for anything else."""
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 1 << 64:
        raise ValueError(f"{who}: {name}= must be an integer in 0..2^64-1, not {seed!r}")
    return int(seed) & 0xFFFFFFFF, int(seed) >> 32


def boot_means(table, n_boot, seed=0, out=None):
    """The resampled means of every cell of a contiguous float64 CUDA tensor table [cells, n, cols] (cols 4, 6 or 9; row e of a cell
    one episode) -> float64 [cells, n_boot, cols] (cm_boot_means, include/commarl.h): resample r draws n rows with replacement from
    the Philox stream of (seed, r) - the same rows for every cell, column and table.  One launch on the current stream."""
    assert table.is_cuda and table.dtype == torch.float64 and table.dim() == 3
    assert table.is_contiguous(), "cm_boot_means reads the table through the raw pointer"
    cells, n, cols = table.shape
    lo, hi = boot_seed_words(seed)
    if out is None:
        out = torch.empty(cells, int(n_boot), cols, dtype=torch.float64, device=table.device)
    assert out.dtype == torch.float64 and out.shape == (cells, int(n_boot), cols) and out.device == table.device and out.is_contiguous()
    L.run("cm_boot_means", cells, n, cols, L.ptr(table), int(n_boot), lo, hi, L.ptr(out), device=table.device)
    return out


def boot_quantiles(means, lo_rank, hi_rank, kind="columns", ref_cell=None, out=None):
    """boot_means' tensor [cells, n_boot, cols] -> float64 [cells, keys, 4] (cm_boot_quantiles): per cell and key (boot_keys) the
    order statistics lo_rank and hi_rank of the key's resampled values, their standard deviation (ddof 1) and the share above
    zero (ties half) - with ref_cell (an int32 CUDA tensor [cells], entries in 0 .. cells-1) of the values minus those of cell
    ref_cell[g] in the same resample.  One launch on the current stream."""
    assert means.is_cuda and means.dtype == torch.float64 and means.dim() == 3
    assert means.is_contiguous(), "cm_boot_quantiles reads the means through the raw pointer"
    cells, R, cols = means.shape
    keys = boot_keys(kind, cols)
    if ref_cell is not None:
        assert ref_cell.dtype == torch.int32 and ref_cell.shape == (cells,) and ref_cell.device == means.device and ref_cell.is_contiguous()
    if out is None:
        out = torch.empty(cells, keys, L.BOOT_OUT, dtype=torch.float64, device=means.device)
    assert out.dtype == torch.float64 and out.shape == (cells, keys, L.BOOT_OUT) and out.device == means.device and out.is_contiguous()
    L.run("cm_boot_quantiles", BOOT_KINDS[kind], cells, R, cols, L.ptr(means), L.ptr(ref_cell), int(lo_rank), int(hi_rank), L.ptr(out),
          device=means.device)
    return out


def bootstrap(table, level, n_boot=2000, seed=0, kind="columns", ref_cell=None):
    """Bootstrap intervals of the means of per-episode tables of your own (cm_boot_means + cm_boot_quantiles, include/commarl.h):
    table a contiguous float64 CUDA tensor [cells, n, cols], row e of a cell one episode -> float64 [cells, keys, 4] on the
    device: per cell and key the interval (lo, hi) at confidence `level` - order statistics of n_boot resampled means, not
    interpolated (boot_ranks) - the bootstrap standard error se, and p_gt, the share of resamples above zero (ties half).
    kind: "columns" - the keys are the 4, 6 or 9 columns; "comm" - evaluate.COMM_KEYS from the 4 comm columns; "value" -
    evaluate.VALUE_KEYS from the 6 value columns, each key formed per resample from the resampled means as the host forms it from
    the means.  Resample r picks the same rows in every cell (and in every call with the same `seed` and n): with ref_cell (a
    sequence of `cells` ints in 0 .. cells-1) everything is of the PAIRED difference of cell g and cell ref_cell[g] - meaningful
    only when row e of both cells is the same scenario (evaluate.sweep_layout(paired=True)); a cell referred to itself holds exact
    zeros and p_gt 0.5.  ValueError for a level outside (0, 1), n_boot outside 2..4096, a seed outside 0..2^64-1, a kind that does
    not take the table's columns or a ref_cell entry out of range.  Two launches on the current stream."""
    lo_rank, hi_rank = boot_ranks(level, n_boot)
    boot_seed_words(seed)
    assert table.dim() == 3
    boot_keys(kind, table.shape[2])
    ref = None
    if ref_cell is not None:
        ref_host = np.asarray(ref_cell.cpu() if isinstance(ref_cell, torch.Tensor) else ref_cell, dtype=np.int64)
        if ref_host.shape != (table.shape[0],) or ref_host.min() < 0 or ref_host.max() >= table.shape[0]:
            raise ValueError(f"bootstrap: ref_cell= must hold one cell index in 0..{table.shape[0] - 1} per cell")
        ref = torch.as_tensor(ref_host, dtype=torch.int32).to(table.device)
    return boot_quantiles(boot_means(table, n_boot, seed), lo_rank, hi_rank, kind, ref)


class GridEnvBatch:
    """B envs stepped by one kernel launch.  All tensors are torch CUDA tensors."""

    def __init__(self, scenario, params, n_envs=1, *, device="cuda:0", seed=None, env_id_offset=0, rng_mode="philox",
                 max_steps=None, max_path_length=None, channel=None, conditions=None, condition_of=None, rng_ids=None,
                 fused_conditions=False):
        """conditions: a list of C comm conditions (condition_table) - env b steps under conditions[condition_of[b]] (default:
        C contiguous blocks of B / C envs) and draws with the Philox env id rng_ids[b] (default: its own, env_id_offset + b).
        Without an explicit `channel` the kind is IID if any condition has 0 < pl < 1, else what params give.  Such a batch
        records every env's dist_adj (adj_const is off) and steps in two launches; set_conditions() replaces the values later.
        fused_conditions: fuse_conditions() at construction - teams of 4 then roll out in one launch per step / chunk."""
        assert scenario in ("pp", "co")
        self.scenario, self.params = scenario, dict(params)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.CommarlError("GridEnvBatch runs on the MI355X only (device must be cuda:k); there is no CPU path")
        seed = int(params.get("seed", 1) if seed is None else seed)
        mode = L.RNG_TAPE if rng_mode == "tape" else L.RNG_PHILOX
        if conditions is not None:
            conditions = [dict(c) for c in conditions]
            channel = conditions_channel(conditions, channel)
        self.cfg, self.channelType, self.pl, calc_diameter = make_cfg(scenario, params, n_envs, seed=seed, env_id_offset=env_id_offset,
                                                       rng_mode=mode, max_steps=max_steps,
                                                       max_path_length=max_path_length, channel=channel)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(L.lib().cm_env_create(C.byref(self.cfg), C.byref(self._h)), "cm_env_create")
        c = self.cfg
        self.B, self.N, self.M, self.Lh = c.n_envs, c.n_agents, c.n_preys, c.n_hops
        self.conditions = self.condition_of = self.rng_ids = None
        self.fused_conditions = False
        if fused_conditions:
            self.fuse_conditions()
        if conditions is not None:                          # before the const-ness queries: the first table turns adj_const off
            if condition_of is None:
                if self.B % len(conditions):
                    raise ValueError(f"{self.B} envs do not split evenly between {len(conditions)} conditions: pass condition_of=")
                condition_of = np.repeat(np.arange(len(conditions)), self.B // len(conditions))
            self._upload_conditions(conditions, condition_of, rng_ids)
        self.S = c.grid if scenario == "pp" else c.grid + 2
        self.d = L.lib().cm_env_obs_dim(self._h)
        self.n_empty_cells = L.lib().cm_env_n_empty_cells(self._h)
        self.adj_const = bool(L.lib().cm_env_adj_is_const(self._h))
        self.ch_const = bool(L.lib().cm_env_channels_are_const(self._h))
        # params['calc_diameter'] on a range graph: engines and wrappers derive the hop diameter from dist_adj (Rcom == 0 keeps N)
        self.calc_diameter = calc_diameter and not self.adj_const
        dev, B, N, M = self.device, self.B, self.N, max(self.M, 1)
        f32, i32, u8 = torch.float32, torch.int32, torch.uint8
        self.obs = torch.zeros(B, N, self.d, dtype=f32, device=dev)
        self.reward = torch.zeros(B, dtype=f32, device=dev)
        self.reward64 = torch.zeros(B, dtype=torch.float64, device=dev)
        self.done = torch.zeros(B, dtype=u8, device=dev)
        self.details = torch.zeros(B, 6, dtype=i32, device=dev)
        self.dist_adj = torch.ones(B, N, N, dtype=f32, device=dev)
        self.channels = torch.ones(B, self.Lh, N, N, dtype=f32, device=dev)
        self.prey_alive = torch.ones(B, M, dtype=u8, device=dev)
        self.success_t = torch.zeros(B, dtype=i32, device=dev)
        L.run("cm_env_fill_constants", self._h, L.ptr(self.dist_adj), L.ptr(self.channels), device=dev)
        self._keep = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                L.destroy_env(h)                        # deferred while a hipGraph capture is open
            except Exception:
                pass
            self._h = None

    # ---- per-env comm conditions ---------------------------------------------------------
    def _upload_conditions(self, conditions, condition_of, rng_ids):
        table = condition_table(self.scenario, self.params, conditions, condition_of, rng_ids, channel=self.channelType,
                                env_id_offset=self.cfg.env_id_offset)
        if table.shape[0] != self.B:
            raise ValueError(f"condition_of has {table.shape[0]} entries for {self.B} envs")
        L.run("cm_env_set_conditions", self._h, table.ctypes.data, device=self.device)
        self.conditions = [dict(c) for c in conditions]
        self.condition_of = np.asarray(condition_of).astype(np.int64)
        self.rng_ids = table["rng_id"].astype(np.int64)

    def set_conditions(self, conditions, condition_of=None, rng_ids=None):
        """New values for a batch built with conditions= (a copy ordered on the current stream into the table the kernels read:
        captured graphs stay valid and replay with the new values - how a curriculum changes conditions between epochs).
        condition_of / rng_ids None keep the current assignment.  The channel kind is the batch's and does not change."""
        if self.conditions is None:
            raise L.CommarlError("set_conditions: this batch was built without conditions= (its buffers and launch form are "
                                 "those of a uniform batch)")
        self._upload_conditions(list(conditions), self.condition_of if condition_of is None else condition_of,
                                self.rng_ids if rng_ids is None else rng_ids)

    def fuse_conditions(self, on=True):
        """Let the fused rollout entry points run this batch's conditions (cm_env_fuse_conditions): Predator-Prey teams of 4 on the
        wave-owned kernel then step in one launch (csrc/cm_rollout_wc.hip), bit for bit what the two launches give; every other
        shape keeps the two launches.  No effect on a batch without conditions.  A RolloutEngine asks the fused forms once and
        remembers the answer: call this before the engine's first step."""
        with torch.cuda.device(self.device):
            L.check(L.lib().cm_env_fuse_conditions(self._h, int(bool(on))), "cm_env_fuse_conditions")
        self.fused_conditions = bool(on)

    # ---- raw device-side API -------------------------------------------------------------
    def _out(self, over=None):
        o = dict(obs=self.obs, reward=self.reward, reward_f64=self.reward64, done=self.done, details=self.details,
                 dist_adj=None if self.adj_const else self.dist_adj,
                 channels=None if self.ch_const else self.channels,
                 prey_alive=self.prey_alive if self.M else None, success=self.success_t, path_len=None)
        if over:
            o.update(over)
        return L.StepOut(*[L.ptr(o[k]) for k in ("obs", "reward", "reward_f64", "done", "details", "dist_adj",
                                                 "channels", "prey_alive", "success", "path_len")])

    def _tape(self, tape):
        if not tape:
            return None
        dev = self.device

        def up(a, dt):
            return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev).contiguous()
        prey, spawn = up(tape.get("prey"), torch.uint8), up(tape.get("spawn"), torch.int32)
        iid, ge = up(tape.get("iid_u"), torch.float32), up(tape.get("ge_u"), torch.float32)
        gi = up(tape.get("ge_init_u"), torch.float32)
        self._keep = (prey, spawn, iid, ge, gi)
        return L.RngTape(L.ptr(prey), L.ptr(spawn), 0 if spawn is None else spawn.shape[1], 0, L.ptr(iid), L.ptr(ge),
                         L.ptr(gi))

    def reset_all(self, tape=None, out=None):
        t = self._tape(tape)
        so = self._out(out)
        L.run("cm_env_reset", self._h, C.byref(t) if t else None, C.byref(so), device=self.device)

    def step_device(self, actions, tape=None, out=None):
        """actions: int32 CUDA tensor [B,N].  Asynchronous; results land in self.* (or `out` overrides)."""
        assert actions.dtype == torch.int32 and actions.shape == (self.B, self.N) and actions.is_cuda
        t = self._tape(tape)
        so = self._out(out)
        L.run("cm_env_step", self._h, L.ptr(actions), C.byref(t) if t else None, C.byref(so), device=self.device)

    def check_status(self):
        with torch.cuda.device(self.device):
            L.check(L.lib().cm_env_status(self._h), "cm_env_status")

    def get_state(self):
        B, N, M, S = self.B, self.N, max(self.M, 1), self.S
        st = dict(agent_pos=np.zeros((B, N, 2), np.int32), prey_pos=np.zeros((B, M, 2), np.int32),
                  prey_alive=np.zeros((B, M), np.uint8),
                  visited=np.zeros((B, S) if S <= 32 else (B, S, (S + 31) // 32), np.uint32),   # row bitmasks: 2 words from map 40 on
                  step_count=np.zeros(B, np.int32), total_capture=np.zeros(B, np.int32),
                  success=np.zeros(B, np.int32), ge_state=np.zeros((B, N, N), np.uint8),
                  rng_step=np.zeros(B, np.uint32))
        if self.M == 0:
            st["prey_pos"], st["prey_alive"] = st["prey_pos"][:, :0], st["prey_alive"][:, :0]
        cs = L.EnvState(*[st[k].ctypes.data if st[k].size else None for k in (
            "agent_pos", "prey_pos", "prey_alive", "visited", "step_count", "total_capture", "success", "ge_state",
            "rng_step")])
        with torch.cuda.device(self.device):
            L.check(L.lib().cm_env_get_state(self._h, C.byref(cs)), "cm_env_get_state")
        return st

    # ---- dormant fault / delay helpers of the reference (custom_implement/env_communication.py:270-301) ----
    @property
    def agent_condition(self):
        """[B,N] uint8: PP agent_condition (predator_prey.py:258): 0 = the agent's moves are not applied."""
        out = np.zeros((self.B, self.N), np.uint8)
        with torch.cuda.device(self.device):
            L.check(L.lib().cm_env_agent_condition(self._h, None, out.ctypes.data), "cm_env_agent_condition")
        return out

    @agent_condition.setter
    def agent_condition(self, cond):
        c = np.ascontiguousarray(np.broadcast_to(np.asarray(cond, np.uint8), (self.B, self.N)))
        with torch.cuda.device(self.device):
            L.check(L.lib().cm_env_agent_condition(self._h, c.ctypes.data, None), "cm_env_agent_condition")

    def apply_agent_fault(self, kind, p, r=0.0, fault_step=0, tape_u=None):
        """kind 'iid': iid_fault(n_agents, p_fault=p) (:290-292); kind 'GE': GE_fault(condition, p, r) (:294-301, one draw
        per group as written).  tape_u: the uniforms (numpy, [B,N] / [B,2]) in tape mode, else Philox site 9 at fault_step."""
        mode = {"iid": 1, "GE": 2}[kind]
        keep = None if tape_u is None else torch.as_tensor(np.ascontiguousarray(tape_u, np.float32)).to(self.device)
        with torch.cuda.device(self.device):
            L.run("cm_env_agent_fault", self._h, mode, float(p), float(r), L.ptr(keep), int(fault_step) & 0xFFFFFFFF)
            torch.cuda.current_stream().synchronize()

    def comm_delays(self, dist_adj, link_loss, delay_th=None, old_delays=None):
        """delays_init(adjacency, link_loss, delay_th) when old_delays is None, else calc_delays(adjacency, link_loss,
        old_delays) (:271-286).  CUDA tensors [B,N,N] / [B,L,N,N] / [B,N,N] int32 -> delays [B,L,N,N] int32."""
        Lh = link_loss.shape[1]
        out = torch.empty(self.B, Lh, self.N, self.N, dtype=torch.int32, device=self.device)
        L.run("cm_comm_delays", self.B, Lh, self.N, L.cptr(dist_adj), L.cptr(link_loss), L.cptr(old_delays), int(delay_th or 0),
              int(old_delays is None), L.ptr(out), device=self.device)
        return out

    def set_state(self, **arrays):
        if "agent_cond" in arrays:
            self.agent_condition = arrays.pop("agent_cond")
            if not arrays:
                return
        keep = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
        cs = L.EnvState(*[keep[k].ctypes.data if k in keep and keep[k].size else None for k in (
            "agent_pos", "prey_pos", "prey_alive", "visited", "step_count", "total_capture", "success", "ge_state",
            "rng_step")])
        with torch.cuda.device(self.device):
            L.check(L.lib().cm_env_set_state(self._h, C.byref(cs)), "cm_env_set_state")


class _WrapperBase:
    """Attribute surface the sampler / runner touch (SURVEY.md §8b 'Env object')."""
    _scenario = None

    def __init__(self, centralized, other_agent_visible=False, *args, n_envs=1, device="cuda:0", seed=None,
                 env_id_offset=0, rng_mode="philox", max_steps=None, channel=None, conditions=None, condition_of=None,
                 rng_ids=None, fused_conditions=False, **kwargs):
        params = kwargs["params"]
        self.centralized = centralized
        self._agent_visible = other_agent_visible
        self.batch = GridEnvBatch(self._scenario, params, n_envs, device=device, seed=seed, env_id_offset=env_id_offset,
                                  rng_mode=rng_mode, max_steps=max_steps, channel=channel, conditions=conditions,
                                  condition_of=condition_of, rng_ids=rng_ids, fused_conditions=fused_conditions)
        b = self.batch
        self.n_envs, self.n_agents = b.B, b.N
        self.n_preys = b.M
        self.maps = int(params["grid_size"])
        self.Rsen = int(params["Rsen"])
        self.GCNHops = self.L = b.Lh
        self.curriculum_learning = params.get("curriculum_learning")
        self.channelType, self.pl = b.channelType, b.pl
        self.pconn = 1 - self.pl
        rc = b.cfg.rcom
        self.Rcom = 0 if rc + 1 >= self.maps else rc                               # env_communication.py:71-72
        self.Rcom_th = np.float32(math.sqrt(2.0) * self.Rcom)                       # cdist([0,0],[R,R]) (:73-75)
        self.loss_apply = params.get("loss_apply")
        self.mode = params.get("mode")
        self.epoch = None
        self.total_n_epi = self.epoch_n_epi = 0
        self.positions_record = {"agent": [], "target": []}
        self.pickleable = False            # state lives in HBM; snapshots go through get_state()
        self.n_action = 5
        self.action_space = _Discrete(5)
        d = b.d
        low = np.zeros(d, np.float32)
        if self._scenario == "co":
            low[: d - 2 - int(b.cfg.add_clock)] = -1.0                              # coverage.py:117-118
        self.observation_space = _Box(np.tile(low, b.N) if centralized else low,
                                      np.ones(d * b.N if centralized else d, np.float32))
        self.spec = EnvSpec(self.observation_space, self.action_space)
        self.ave_trput = b.n_empty_cells if self._scenario == "co" else 0           # coverage.py:232
        if self._scenario == "pp":
            self.bound_return = self.n_preys * abs(params.get("capture_reward", 10))   # predator_prey.py:72
        else:
            n, ne = b.N, b.n_empty_cells                                            # coverage.py:214-219
            self.bound_return = b.cfg.capture_reward * ne / n - abs(b.cfg.step_cost) * ne / n + b.cfg.final_reward
        self._diameter = b.N if self._full_graph else 0                             # get_graph :219-223,234
        self._single = (b.B == 1)

    # -- per-env comm conditions (GridEnvBatch(conditions=...)): Rcom / pl above stay the values params give --
    @property
    def _full_graph(self):
        """Every env fully connected by the Rcom rule: without conditions only (with them each env's graph is recorded)."""
        return self.Rcom == 0 and self.batch.conditions is None

    @property
    def conditions(self):
        return self.batch.conditions

    @property
    def condition_of(self):
        return self.batch.condition_of

    def set_conditions(self, conditions, condition_of=None, rng_ids=None):
        self.batch.set_conditions(conditions, condition_of, rng_ids)

    def fuse_conditions(self, on=True):
        self.batch.fuse_conditions(on)

    # -- env attributes the sampler reads each step (sampler.py:123-131) --
    @property
    def dist_adj(self):
        a = self.batch.dist_adj.cpu().numpy()
        if self._full_graph:
            a = a.astype(np.float64)                                                # np.ones(...) f64 (:220)
        return a[0] if self._single else a

    @property
    def channels(self):
        c = self.batch.channels.cpu().numpy()
        return c[0] if self._single else c

    @property
    def ave_deg(self):
        if self._full_graph:
            return self.n_agents
        v = self.batch.dist_adj.sum(-1).mean(-1).cpu().numpy()                      # :232
        return v[0] if self._single else v

    @property
    def diameter(self):
        """get_graph's third value for the current graph: N with Rcom == 0, else 0 - or, with params['calc_diameter'], the
        hop diameter (0 when disconnected; int for one env, int32 [B] otherwise)."""
        if not self.batch.calc_diameter:
            return self._diameter
        v = graph_diameter(self.batch.dist_adj).cpu().numpy()
        return int(v[0]) if self._single else v

    @property
    def success(self):
        s = self.batch.success_t.cpu().numpy()
        return int(s[0]) if self._single else s

    @property
    def agent_pos(self):
        p = self.batch.get_state()["agent_pos"]
        if self._single:
            return {i: [int(p[0, i, 0]), int(p[0, i, 1])] for i in range(self.n_agents)}
        return p

    @property
    def agent_condition(self):
        """predator_prey.py:74: ones unless a fault model was applied (GridEnvBatch.apply_agent_fault)."""
        c = self.batch.agent_condition
        return c[0].astype(np.float64) if self.batch.B == 1 else c

    @agent_condition.setter
    def agent_condition(self, cond):
        self.batch.agent_condition = cond

    def get_avail_actions(self):
        """All ones (predatorprey_wrapper.py:46-51)."""
        if not self.centralized:
            return [[1] * 5 for _ in range(self.n_agents)]
        a = np.ones(self.n_agents * 5, dtype=np.int64)
        return a if self._single else np.tile(a, (self.n_envs, 1))

    def seed(self, n):
        return [n, n + 1]

    def close(self):
        pass

    def _obs_np(self):
        o = self.batch.obs.cpu().numpy().astype(np.float64)
        o = o.reshape(self.n_envs, -1) if self.centralized else o
        return o[0] if self._single else o

    def reset(self, epoch=-1):
        """Resets ALL B envs (VecEnvExecutor.reset, vec_env_executor.py:47-54)."""
        self.epoch = epoch
        self.batch.reset_all()
        self.total_n_epi += self.n_envs
        self.epoch_n_epi += self.n_envs
        return self._obs_np()

    def _details(self, det):
        n = float(self.n_agents)
        if self._scenario == "pp":                                                  # predator_prey.py:440-448
            return dict(capture_cnt=int(det[0]), step_cnt=1, move_cnt=det[1] / n, penalty_cnt=int(det[2]),
                        variable=det[4] / n, vars2=0)
        return dict(capture_cnt=det[0] / n, step_cnt=1, move_cnt=det[1] / n, penalty_cnt=det[2] / n,   # coverage.py:308-315
                    variable=det[4] / n, vars2=det[3] / n)

    def step(self, actions):
        """actions: [N] (single env) or [B,N].  Envs that finish are auto-reset and return the
        reset observation, exactly as VecEnvExecutor.step does (vec_env_executor.py:36-43)."""
        a = torch.as_tensor(np.asarray(actions), dtype=torch.int32).reshape(self.n_envs, self.n_agents)
        self.batch.step_device(a.to(self.batch.device))
        self.batch.check_status()
        rew = self.batch.reward64.cpu().numpy()
        done = self.batch.done.cpu().numpy().astype(bool)
        det = self.batch.details.cpu().numpy()
        info = {}
        if self._scenario == "pp":
            info["prey_alive"] = self.batch.prey_alive.cpu().numpy().astype(bool)
        if self._single:
            d = self._details(det[0])
            d["reward"] = float(rew[0])
            if "prey_alive" in info:
                info["prey_alive"] = info["prey_alive"][0]
            return self._obs_np(), (float(rew[0]), d), bool(done[0]), info
        ds = [dict(self._details(det[b]), reward=float(rew[b])) for b in range(self.n_envs)]
        return self._obs_np(), (rew, ds), done, info


class PredatorPreyWrapper(_WrapperBase):
    """envs/predatorprey_wrapper.py:23 - same ctor (centralized, other_agent_visible, params=...)."""
    _scenario = "pp"


class CoverageWrapper(_WrapperBase):
    """envs/coverage_wrapper.py:16."""
    _scenario = "co"

"""ctypes binding of libnfsp (include/nfsp.h).

The product path is this library: every Env / Agent / buffer operation of the package
ends in one of these entry points.  There is no CPU fallback -- if the library or a
GPU is missing, ``lib()`` raises.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NFSP_LIB", os.path.join(HERE, "libnfsp.so"))

OK, EINVAL, EHIP, ENOMEM = 0, -1, -2, -3
GAME_LEDUC = 0
GAME_KUHN = 1     # the Kuhn swap-in (include/nfsp.h NFSP_GAME_KUHN)
ACT_RELU, ACT_SOFTMAX, ACT_LINEAR = 0, 1, 2
QUIRK_TERMINAL_BOOTSTRAP, QUIRK_ROW0_TARGET, QUIRK_ALIAS_RL = 1, 2, 4
QUIRKS_REFERENCE = 7
# textbook-NFSP extensions (include/nfsp.h NFSP_EXT_*; not the reference's algorithm)
EXT_SL_ONEHOT, EXT_RESERVOIR, EXT_LINEAR_Q, EXT_EPS_CONST, EXT_SAMPLE_AR = 8, 16, 32, 64, 128
TEXTBOOK = EXT_SL_ONEHOT | EXT_RESERVOIR | EXT_LINEAR_Q | EXT_EPS_CONST | EXT_SAMPLE_AR
EXT_MSE_Q = 256
TEXTBOOK_MSE = TEXTBOOK | EXT_MSE_Q
TEXTBOOK_MSE_DECAY = TEXTBOOK_MSE & ~EXT_EPS_CONST      # epsilon / iteration, as the reference

NP = 30 * 64 + 64 + 64 * 3 + 3      # floats of a packed net: W1 | b1 | W2 | b2 (include/nfsp.h)
NET_AR, NET_BR, NET_TARGET = 0, 1, 2
# the hidden widths the fits off the engine are built for (nfsp_net_params); the engine's is 64
FIT_WIDTHS = (16, 32, 64, 128)


def net_params(hidden: int) -> int:
    """floats of a packed net of that width: 34 H + 3 (nfsp_net_params' rule, without the library)"""
    if hidden not in FIT_WIDTHS:
        raise ValueError(f"hidden is {hidden}: the widths built are {FIT_WIDTHS}")
    return 34 * hidden + 3


P = C.c_void_p
I32, I64, U32, U64, F32, F64 = C.c_int, C.c_int64, C.c_uint, C.c_uint64, C.c_float, C.c_double


class Records(C.Structure):
    """``nfsp_records``: device column pointers of an M_RL / M_SL table."""
    _fields_ = [("s", P), ("a", P), ("r", P), ("s2", P), ("t", P), ("cap", I64)]


class EngineCfg(C.Structure):
    """``nfsp_engine_cfg``"""
    _fields_ = [("n_lanes", C.c_int32), ("hidden", C.c_int32), ("rl_capacity", I64),
                ("sl_capacity", I64), ("batch", C.c_int32), ("inserts_per_update", C.c_int32),
                ("target_every", C.c_int32), ("epochs", C.c_int32), ("fit_batch", C.c_int32),
                ("quirks", C.c_uint32), ("eta", F32), ("lr_br", F32), ("lr_ar", F32),
                ("gamma", F64), ("epsilon", F64), ("seed", U64), ("slices", C.c_int32),
                ("slice_lag", C.c_int32), ("sched", C.c_uint32)]


class GroupSched(C.Structure):
    """``nfsp_group_sched``: how a group schedules its BR rounds and slices (no result changes)"""
    _fields_ = [("br_cap", C.c_int32), ("br_pace", C.c_int32), ("br_streams", C.c_int32),
                ("serial", C.c_int32), ("br_persist", C.c_int32)]


class EngineStats(C.Structure):
    """``nfsp_engine_stats``"""
    _fields_ = [("hands", I64), ("rollouts", I64), ("rl_total", I64 * 2), ("sl_total", I64 * 2),
                ("rl_size", I64 * 2), ("sl_size", I64 * 2), ("last_rl", I64 * 2),
                ("last_sl", I64 * 2), ("br_updates", I64 * 2), ("ar_updates", I64 * 2),
                ("iteration", I64 * 2), ("target_syncs", I64 * 2), ("actions", (I64 * 3) * 2),
                ("reward", F64 * 2), ("epsilon", F64 * 2), ("temp", F64 * 2), ("lr_br", F64 * 2),
                ("exploitability", F64 * 2)]

    def to_dict(self):
        out = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            if isinstance(v, (int, float)):
                out[name] = v
            elif name == "actions":
                out[name] = [list(v[0]), list(v[1])]
            else:
                out[name] = list(v)
        return out


class StateInfo(C.Structure):
    """``nfsp_state_info``: what nfsp_state_check reads from a state blob's header"""
    _fields_ = [("version", C.c_int32), ("kind", C.c_int32), ("replicas", C.c_int32),
                ("n_sections", C.c_int32), ("slices", C.c_int32), ("slice_lag", C.c_int32),
                ("sched", C.c_uint32), ("group_flags", C.c_uint32), ("total_bytes", I64),
                ("payload_offset", I64), ("payload_bytes", I64), ("digest", U64 * 2)]


class TreeNode(C.Structure):
    """``nfsp_tree_node``: a node of the evaluator's public tree (nfsp_tree_export)"""
    _fields_ = [("kind", C.c_int8), ("p", C.c_int8), ("via", C.c_int8), ("nchild", C.c_int8),
                ("parent", C.c_int32), ("child", C.c_int32 * 3), ("row", C.c_int32)]


class PolicySpec(C.Structure):
    """``nfsp_policy``: a policy kind and its device pointer (a packed net or a table)"""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("dev", P)]


class XfpCfg(C.Structure):
    """``nfsp_xfp_cfg``: one fictitious-play run's eta and weighting (XFP_WEIGHT_*)"""
    _fields_ = [("eta", C.c_double), ("weight", C.c_int32), ("reserved", C.c_int32)]


class MccfrCfg(C.Structure):
    """``nfsp_mccfr_cfg``: one external-sampling MCCFR run's seed and walkers per half-iteration"""
    _fields_ = [("seed", C.c_uint64), ("walkers", C.c_int32), ("reserved", C.c_int32)]


class MccfrOsCfg(C.Structure):
    """``nfsp_mccfr_os_cfg``: one outcome-sampling MCCFR run's seed, walkers per half-iteration and
    exploration rate"""
    _fields_ = [("seed", C.c_uint64), ("walkers", C.c_int32), ("reserved", C.c_int32), ("epsilon", C.c_double)]


class MccfrVrCfg(C.Structure):
    """``nfsp_mccfr_vr_cfg``: one baseline-corrected outcome-sampling run's seed, walkers per
    half-iteration and exploration rate"""
    _fields_ = [("seed", C.c_uint64), ("walkers", C.c_int32), ("reserved", C.c_int32), ("epsilon", C.c_double)]


class MccfrXCfg(C.Structure):
    """``nfsp_mccfr_x_cfg``: one run of any sampling kind (the handle's) with its regret rule
    (``MCCFR_REGRET_*``) and the average ``nfsp_mccfr_average`` returns (``MCCFR_AVG_*``)"""
    _fields_ = [("seed", C.c_uint64), ("walkers", C.c_int32), ("sampling", C.c_int32), ("epsilon", C.c_double),
                ("regret", C.c_int32), ("average", C.c_int32)]


class MccfrNetCfg(C.Structure):
    """``nfsp_mccfr_net_cfg``: ``nfsp_mccfr_x_cfg``'s fields, then what the run's two regret nets are
    fitted with: the target (``MCCFR_NET_TARGET_*``), the steps per fit, the loss (``FIT_MSE`` /
    ``FIT_HUBER``), the learning rate and the momentum"""
    _fields_ = [("seed", C.c_uint64), ("walkers", C.c_int32), ("sampling", C.c_int32), ("epsilon", C.c_double),
                ("regret", C.c_int32), ("average", C.c_int32), ("target", C.c_int32), ("fit_steps", C.c_int32),
                ("loss", C.c_int32), ("lr", F32), ("momentum", F32), ("reserved", C.c_int32)]


class MemSegment(C.Structure):
    """``nfsp_mem_segment``: n packed records (SlRec 16 B / RlRec 32 B) at a device address"""
    _fields_ = [("dev_recs", P), ("n", I64)]


class MemtabInfo(C.Structure):
    """``nfsp_memtab_info``: what one table call read"""
    _fields_ = [("records", I64), ("matched", I64), ("unmatched", I64), ("clamped", I64)]

    def to_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class TdArgs(C.Structure):
    """``nfsp_td_args``: the target net, gamma and quirks a TD table is counted with"""
    _fields_ = [("dev_target_w", P), ("gamma", F64), ("quirks", C.c_uint32), ("reserved", C.c_uint32)]


class FitJob(C.Structure):
    """``nfsp_fit_job``: one net fitted to one seat's rows of a table (nfsp_fit_tables)"""
    _fields_ = [("dev_w", P), ("dev_v", P), ("dev_target", P), ("dev_weight", P), ("dev_mask", P),
                ("seat", C.c_int32), ("head", C.c_int32), ("loss", C.c_int32), ("lr", F32), ("momentum", F32)]


PP = C.POINTER(P)
# name -> (restype, argtypes); must list every symbol include/nfsp.h declares
SIGNATURES = {
    "nfsp_last_error": (C.c_char_p, []),
    "nfsp_version": (I32, []),
    "nfsp_device_count": (I32, [C.POINTER(I32)]),
    "nfsp_create": (I32, [C.POINTER(P), I32, U64, I32, I32]),
    "nfsp_destroy": (I32, [P]),
    "nfsp_set_stream": (I32, [P, P]),
    "nfsp_synchronize": (I32, [P]),
    "nfsp_num_envs": (I32, [P]),
    "nfsp_env_set_deal": (I32, [P, P]),
    "nfsp_env_reset": (I32, [P, P]),
    "nfsp_env_set_deal_mode": (I32, [P, I32, U64]),
    "nfsp_deal_mt": (I32, [I32, U64, I64, P]),
    "nfsp_env_get_state": (I32, [P, I32, P, P, P, P, P, P]),
    "nfsp_env_step": (I32, [P, P, I32, P, P]),
    "nfsp_env_round": (I32, [P, P]),
    "nfsp_env_do_action": (I32, [P, P, I32, P, P, P]),
    "nfsp_env_round_status": (I32, [P, P]),
    "nfsp_env_export": (I32, [P, P]),
    "nfsp_mlp_forward": (I32, [P, P, I32, I32, P, P, I64]),
    "nfsp_mlp_fit": (I32, [P, P, I32, I32, P, P, I32, P, I32, I32, F32]),
    "nfsp_br_targets": (I32, [P, P, I32, P, P, P, P, P, I32, F64, U32, P, P]),
    "nfsp_buf_insert": (I32, [P, C.POINTER(Records), C.POINTER(Records), P, I64]),
    "nfsp_buf_sample": (I32, [P, C.POINTER(Records), P, I64, C.POINTER(Records)]),
    "nfsp_engine_default_cfg": (I32, [C.POINTER(EngineCfg)]),
    "nfsp_engine_create": (I32, [P, C.POINTER(EngineCfg), C.POINTER(P)]),
    "nfsp_engine_destroy": (I32, [P]),
    "nfsp_engine_weights": (I32, [P, I32, I32, PP]),
    "nfsp_rollout": (I32, [P]),
    "nfsp_rollout_with": (I32, [P, P, P]),
    "nfsp_engine_update": (I32, [P]),
    "nfsp_engine_step": (I32, [P]),
    "nfsp_engine_get_stats": (I32, [P, C.POINTER(EngineStats)]),
    "nfsp_engine_memories": (I32, [P, I32, C.POINTER(Records), C.POINTER(I64), C.POINTER(Records),
                                   PP, PP, PP]),
    "nfsp_engine_last_update": (I32, [P, I32, I32, PP, PP]),
    "nfsp_engine_lane_counts": (I32, [P, PP]),
    "nfsp_exploitability": (I32, [P, P, P, I32, P]),
    "nfsp_exploitability_batch": (I32, [P, P, P, I32, I32, P]),
    "nfsp_tree_size": (I32, [I32] + [C.POINTER(C.c_int32)] * 4),
    "nfsp_tree_export": (I32, [I32, P, P, P, P, P, P, P]),
    "nfsp_evaluate_batch": (I32, [P, C.POINTER(PolicySpec), C.POINTER(PolicySpec), I32, P]),
    "nfsp_policy_table": (I32, [P, C.POINTER(PolicySpec), P]),
    "nfsp_cfr_create": (I32, [P, C.POINTER(P)]),
    "nfsp_cfr_run": (I32, [P, I64]),
    "nfsp_cfr_iterations": (I32, [P, C.POINTER(I64)]),
    "nfsp_cfr_average": (I32, [P, C.POINTER(P)]),
    "nfsp_cfr_state": (I32, [P, P, P]),
    "nfsp_cfr_destroy": (I32, [P]),
    "nfsp_best_response_table": (I32, [P, C.POINTER(PolicySpec), C.POINTER(PolicySpec), P, P, P]),
    "nfsp_xfp_create": (I32, [P, C.POINTER(XfpCfg), I32, C.POINTER(P)]),
    "nfsp_xfp_run": (I32, [P, I64, P]),
    "nfsp_xfp_iterations": (I32, [P, C.POINTER(I64)]),
    "nfsp_xfp_average": (I32, [P, I32, C.POINTER(P)]),
    "nfsp_xfp_state": (I32, [P, I32, P, P, C.POINTER(F64)]),
    "nfsp_xfp_destroy": (I32, [P]),
    "nfsp_mccfr_cfgs_check": (I32, [I32, C.POINTER(MccfrCfg), I32, I64]),
    "nfsp_mccfr_create": (I32, [P, C.POINTER(MccfrCfg), I32, C.POINTER(P)]),
    "nfsp_mccfr_run": (I32, [P, I64]),
    "nfsp_mccfr_iterations": (I32, [P, C.POINTER(I64)]),
    "nfsp_mccfr_counts": (I32, [P, I32, C.POINTER(I64)]),
    "nfsp_mccfr_average": (I32, [P, I32, C.POINTER(P)]),
    "nfsp_mccfr_state": (I32, [P, I32, P, P]),
    "nfsp_mccfr_destroy": (I32, [P]),
    "nfsp_mccfr_os_cfgs_check": (I32, [I32, C.POINTER(MccfrOsCfg), I32, I64]),
    "nfsp_mccfr_os_create": (I32, [P, C.POINTER(MccfrOsCfg), I32, C.POINTER(P)]),
    "nfsp_mccfr_sampling": (I32, [P, C.POINTER(I32)]),
    "nfsp_mccfr_vr_cfgs_check": (I32, [I32, C.POINTER(MccfrVrCfg), I32, I64]),
    "nfsp_mccfr_vr_create": (I32, [P, C.POINTER(MccfrVrCfg), I32, C.POINTER(P)]),
    "nfsp_mccfr_baseline": (I32, [P, I32, P, P]),
    "nfsp_mccfr_set_baseline": (I32, [P, I32, P, P]),
    "nfsp_mccfr_x_cfgs_check": (I32, [I32, C.POINTER(MccfrXCfg), I32, I64]),
    "nfsp_mccfr_x_create": (I32, [P, C.POINTER(MccfrXCfg), I32, C.POINTER(P)]),
    "nfsp_mccfr_rule": (I32, [P, I32, C.POINTER(I32)]),
    "nfsp_mccfr_average_of": (I32, [P, I32, I32, C.POINTER(P)]),
    "nfsp_mccfr_weighted": (I32, [P, I32, P]),
    "nfsp_mccfr_net_cfgs_check": (I32, [I32, C.POINTER(MccfrNetCfg), I32, I64]),
    "nfsp_mccfr_net_create": (I32, [P, C.POINTER(MccfrNetCfg), I32, C.POINTER(P), C.POINTER(P)]),
    "nfsp_mccfr_net_tables": (I32, [P, I32, C.POINTER(P), C.POINTER(P), C.POINTER(P)]),
    "nfsp_mccfr_net_weights": (I32, [P, I32, I32, C.POINTER(P), C.POINTER(P)]),
    "nfsp_mccfr_net_loss": (I32, [P, I32, C.POINTER(F64)]),
    "nfsp_mccfr_net_create_h": (I32, [P, I32, C.POINTER(MccfrNetCfg), I32, C.POINTER(P), C.POINTER(P)]),
    "nfsp_mccfr_net_hidden": (I32, [P, C.POINTER(I32)]),
    "nfsp_mccfr_set_timing": (I32, [P, I32]),
    "nfsp_mccfr_get_timings": (I32, [P, C.POINTER(F64), C.POINTER(I64)]),
    "nfsp_engine_set_loss_log": (I32, [P, I32]),
    "nfsp_engine_losses": (I32, [P, P]),
    "nfsp_engine_set_timing": (I32, [P, I32]),
    "nfsp_engine_get_timings": (I32, [P, C.POINTER(F64), C.POINTER(I64)]),
    "nfsp_engine_set_update_limit": (I32, [P, I64]),
    "nfsp_engine_snapshot": (I32, [P, I32, PP, P]),
    "nfsp_group_create": (I32, [P, C.POINTER(EngineCfg), I32, U32, C.POINTER(P)]),
    "nfsp_group_create_v": (I32, [P, C.POINTER(EngineCfg), I32, U32, C.POINTER(P)]),
    "nfsp_group_cfgs_check": (I32, [C.POINTER(EngineCfg), I32, U32]),
    "nfsp_group_replica_cfg": (I32, [P, I32, C.POINTER(EngineCfg)]),
    "nfsp_group_destroy": (I32, [P]),
    "nfsp_group_engine": (I32, [P, I32, C.POINTER(P)]),
    "nfsp_group_step": (I32, [P]),
    "nfsp_group_average_ar": (I32, [P]),
    "nfsp_group_set_timing": (I32, [P, I32]),
    "nfsp_group_get_timings": (I32, [P, C.POINTER(F64), C.POINTER(I64)]),
    "nfsp_group_rounds": (I32, [P, C.POINTER(I64)]),
    "nfsp_group_check": (I32, [P]),
    "nfsp_group_set_trace": (I32, [P, I32]),
    "nfsp_group_trace": (I32, [P, C.POINTER(I32), I64, C.POINTER(I64)]),
    "nfsp_group_set_exchange": (I32, [P, U32, I32, F32]),
    "nfsp_group_default_sched": (I32, [C.POINTER(GroupSched)]),
    "nfsp_group_set_sched": (I32, [P, C.POINTER(GroupSched)]),
    "nfsp_group_get_sched": (I32, [P, C.POINTER(GroupSched)]),
    "nfsp_engine_set_exchange": (I32, [P, I32, F32, P, P, P]),
    "nfsp_engine_exchanges": (I32, [P, C.POINTER(I64)]),
    "nfsp_rccl_ready": (I32, [I32]),
    "nfsp_rccl_unique_id": (I32, [P]),
    "nfsp_rccl_comm_create": (I32, [P, I32, I32, I32, C.POINTER(P)]),
    "nfsp_rccl_comm_destroy": (I32, [P]),
    "nfsp_engine_state_bytes": (I32, [P, C.POINTER(I64)]),
    "nfsp_engine_save_state": (I32, [P, P, I64, C.POINTER(I64)]),
    "nfsp_engine_load_state": (I32, [P, P, I64]),
    "nfsp_engine_state_digest": (I32, [P, C.POINTER(U64)]),
    "nfsp_engine_state_digest_timed": (I32, [P, C.POINTER(U64), C.POINTER(F64), C.POINTER(I64)]),
    "nfsp_group_state_bytes": (I32, [P, C.POINTER(I64)]),
    "nfsp_group_save_state": (I32, [P, P, I64, C.POINTER(I64)]),
    "nfsp_group_load_state": (I32, [P, P, I64]),
    "nfsp_state_check": (I32, [P, I64, C.POINTER(StateInfo)]),
    "nfsp_state_cfg": (I32, [P, I64, I32, C.POINTER(EngineCfg), C.POINTER(C.c_int32)]),
    "nfsp_state_digest": (I32, [P, I64, C.POINTER(U64)]),
    "nfsp_memtab_lookup": (I32, [I32, I32, C.c_uint32]),
    "nfsp_memtab_fix": (I64, [F32]),
    "nfsp_memory_table": (I32, [P, I32, I32, I32, C.POINTER(MemSegment), I32, P, C.POINTER(MemtabInfo)]),
    "nfsp_engine_memory_table": (I32, [P, I32, P, C.POINTER(MemtabInfo)]),
    "nfsp_group_memory_tables": (I32, [P, I32, P, C.POINTER(MemtabInfo)]),
    "nfsp_memtab_last_ms": (I32, [C.POINTER(F64)]),
    "nfsp_td_table": (I32, [P, I32, I32, C.POINTER(MemSegment), I32, C.POINTER(TdArgs), P, C.POINTER(MemtabInfo)]),
    "nfsp_engine_td_table": (I32, [P, P, C.POINTER(MemtabInfo)]),
    "nfsp_group_td_tables": (I32, [P, P, C.POINTER(MemtabInfo)]),
    "nfsp_head_tables": (I32, [P, I32, PP, C.POINTER(I32), I32, P]),
    "nfsp_head_tables_h": (I32, [P, I32, I32, PP, C.POINTER(I32), I32, P]),
    # tables that act: a slot's net (agent/agent.py:124-151's predict calls) replaced by a lookup
    "nfsp_engine_set_act_table": (I32, [P, I32, I32, P]),
    "nfsp_engine_get_act_table": (I32, [P, I32, I32, PP, C.POINTER(I64)]),
    "nfsp_group_set_act_table": (I32, [P, I32, I32, I32, P]),
    # tabular NFSP: fitted-Q sweeps over M_RL, and the memory tables as the rows a slot acts on
    "nfsp_tdq_table": (I32, [P, I32, I32, C.POINTER(MemSegment), I32, P, F64, U32, P, C.POINTER(MemtabInfo)]),
    "nfsp_table_rows": (I32, [P, I32, I32, P, P, P, I32, P, P]),
    "nfsp_engine_tabular_q": (I32, [P, I32, P, P, P, C.POINTER(MemtabInfo), C.POINTER(C.c_int32)]),
    "nfsp_group_tabular_q": (I32, [P, I32, P, P, P, C.POINTER(MemtabInfo), C.POINTER(C.c_int32)]),
    # nets fitted to tables: weighted full-batch descent, one workgroup per job
    "nfsp_fit_jobs_check": (I32, [C.POINTER(FitJob), I32, I64]),
    "nfsp_fit_tables": (I32, [P, I32, C.POINTER(FitJob), I32, I64, P]),
    # the same at hidden widths 16, 32, 64, 128
    "nfsp_net_params": (I32, [I32, C.POINTER(I64)]),
    "nfsp_fit_width_check": (I32, [I32, I32, C.POINTER(I64)]),
    "nfsp_fit_tables_h": (I32, [P, I32, I32, C.POINTER(FitJob), I32, I64, P]),
}
# int (*nfsp_exchange_fn)(void* user, float* dev_sum, int64_t n)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, P, P, I64)
GROUP_AVG_AR = 1
XCHG_AR, XCHG_BR = 1, 2
DEAL_PHILOX, DEAL_PY3_MT, DEAL_PY2_MT = 0, 1, 2
GROUP_MAX_REPLICAS = 256
# nfsp_policy kinds (include/nfsp.h NFSP_POL_*) and the CFR+ launch cap (NFSP_CFR_LAUNCH_ITERS)
POL_AR_SOFTMAX, POL_AR_ARGMAX, POL_BR_GREEDY, POL_BR_GREEDY_LINEAR, POL_TABLE = 0, 1, 2, 3, 4
CFR_LAUNCH_ITERS = 1024
# fictitious-play weightings (NFSP_XFP_WEIGHT_*), the launch cap and the most runs of a handle
XFP_WEIGHT_UNIFORM, XFP_WEIGHT_LINEAR = 0, 1
XFP_LAUNCH_ITERS = 1024
XFP_MAX_RUNS = 1024
# external-sampling MCCFR (NFSP_MCCFR_*): the fixed point of R and S, the most runs of a handle, the
# most walkers of a run and the traversals of one workgroup
MCCFR_Q = 1 << 24
MCCFR_MAX_RUNS = 64
MCCFR_MAX_WALKERS = 1 << 22
MCCFR_WG_WALKERS = 1024
MCCFR_OS_EPS_MIN = 0.0625       # outcome sampling's least exploration rate (NFSP_MCCFR_OS_EPS_MIN)
# nfsp_mccfr_x_cfg.regret / .average (NFSP_MCCFR_REGRET_*, NFSP_MCCFR_AVG_*)
MCCFR_REGRET_PLAIN, MCCFR_REGRET_PLUS = 0, 1
MCCFR_AVG_UNIFORM, MCCFR_AVG_LINEAR = 0, 1
# nfsp_mccfr_net_cfg.target (NFSP_MCCFR_NET_TARGET_*), the most steps of a fit and the most iterations timed per run call
MCCFR_NET_TARGET_AVG, MCCFR_NET_TARGET_ROWMAX = 0, 1
MCCFR_NET_MAX_STEPS = 4096
MCCFR_TIMED_ITERS = 4096
# the memories as tables (NFSP_MEM_*, NFSP_MEMTAB_*)
MEM_SL, MEM_RL, MEM_TD, MEM_TDQ = 0, 1, 2, 3
# what nfsp_table_rows makes of a table (NFSP_ROWS_*), and the most sweeps and tables of a call
ROWS_SL_MASS, ROWS_SL_ARGMAX, ROWS_TD_MEAN = 0, 1, 2
TABQ_MAX_SWEEPS = 64
TABLE_ROWS_MAX = 65535
MEMTAB_FIX_SHIFT = 24
MEMTAB_MAX_SEGMENTS = 8
# losses of nfsp_fit_tables (NFSP_FIT_*) and its jobs per launch
FIT_CE, FIT_MSE, FIT_HUBER = 0, 1, 2
FIT_MAX_JOBS = 64

_LIB = None


class NativeError(RuntimeError):
    pass


def load(path: str = LIB_PATH):
    """dlopen libnfsp and bind every signature (no GPU needed)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(path):
        raise NativeError(f"libnfsp not built: {path} is missing (run __graft_entry__.build())")
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def lib():
    """The library, on a machine that has a HIP device; raises otherwise (no fallback)."""
    L = load()
    n = I32(0)
    rc = L.nfsp_device_count(C.byref(n))
    if rc != OK or n.value < 1:
        raise NativeError("libnfsp needs a HIP device (none visible): "
                          + L.nfsp_last_error().decode())
    return L


def check(rc: int, what: str = ""):
    if rc != OK:
        raise NativeError(f"{what} failed ({rc}): {load().nfsp_last_error().decode()}")


def ptr(t) -> P:
    """Device pointer of a torch tensor (or None -> NULL)."""
    return None if t is None else P(t.data_ptr())


def stream_handle():
    import torch
    return P(torch.cuda.current_stream().cuda_stream)


def wrap_device(addr, numel, dtype, device, owner=None):
    """Zero-copy torch view of device memory owned by libnfsp.  ``owner`` (the engine) is
    referenced by the view's array-interface object, which torch keeps alive with the tensor:
    the engine -- and so the memory -- outlives every view of it."""
    import torch
    if numel == 0:
        return torch.empty(0, dtype=dtype, device=device)

    class _Holder:
        pass
    h = _Holder()
    h.owner = owner
    esize = torch.empty(0, dtype=dtype).element_size()
    h.__cuda_array_interface__ = {
        "shape": (int(numel),), "typestr": torch.empty(0, dtype=dtype).numpy().dtype.str,
        "data": (int(addr), False), "version": 2, "strides": (esize,)}
    return torch.as_tensor(h, device=device)


class Handle:
    """Owner of a library handle ``h``: ``close()``, and the collector, give it to ``_destroy``."""

    def close(self):
        if getattr(self, "h", None):
            self._destroy()
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context(Handle):
    """Owns one ``nfsp_ctx`` (n envs on the current device), bound to torch's stream."""

    def __init__(self, n_envs: int, seed: int = 1234, device: int | None = None, game: int = GAME_LEDUC):
        import torch
        L = lib()
        self.L = L
        dev = torch.cuda.current_device() if device is None else device
        h = P()
        check(L.nfsp_create(C.byref(h), int(n_envs), int(seed) & (2**64 - 1), int(game), dev),
              "nfsp_create")
        self.h = h
        self.n = int(n_envs)
        self.game = int(game)
        self.set_stream()

    def set_stream(self):
        """Rebind the ctx -- and every engine, group and solver on it -- to torch's current stream
        (``nfsp_set_stream``).  Nothing orders the new stream after the one it leaves: the caller does."""
        check(self.L.nfsp_set_stream(self.h, stream_handle()), "nfsp_set_stream")

    def call(self, name, *args):
        check(getattr(self.L, name)(self.h, *args), name)

    def _destroy(self):
        self.L.nfsp_destroy(self.h)

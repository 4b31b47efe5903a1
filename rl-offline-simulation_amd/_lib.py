"""ctypes binding of the C ABI in include/offsim.h (csrc/liboffsim_hip.so).

There is no CPU fallback: if the shared library is missing or no HIP device is visible, the product
path raises.  torch is used only for device memory, streams and torch.distributed.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# OFFSIM_LIB: another build of the same sources (A/B timing of kernel variants, the -DOFFSIM_ROWS_PROF / -DSHUF_FAULT_INJECT builds)
LIB_PATH = os.environ.get("OFFSIM_LIB") or os.path.join(_HERE, "csrc", "liboffsim_hip.so")

OK = 0
EINVAL, EHIP, EUNSUPPORTED = -1, -2, -3
F32, F64, F16 = 0, 1, 2
REJECT_DEFAULT, REJECT_NEVER = 0, 1
STREAM_PCG64, STREAM_PHILOX = 0, 1
STREAMS_A, STREAMS_B, STREAMS_C = 0, 1, 2
PROB_F64, PROB_F32 = 0, 1
ST_OK, ST_EXHAUSTED, ST_NO_INIT, ST_KEYERROR, ST_INACTIVE, ST_PROTOCOL = 0, 1, 2, 3, 4, 5

_vp, _i32, _i64, _u8 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint8


class Table(C.Structure):
    """struct offsim_table"""
    _fields_ = [("N", _i64), ("n_slots", _i32), ("nA", _i32), ("plog_dtype", _i32), ("r_dtype", _i32),
                ("seg_off", _vp), ("p_log", _vp), ("a", _vp), ("r", _vp), ("z_next", _vp), ("done", _vp),
                ("orig_idx", _vp), ("N0", _i64), ("init_slot", _vp), ("init_orig", _vp), ("max_seg", _i64), ("min_seg", _i64)]


class Rollouts(C.Structure):
    """struct offsim_rollouts"""
    _fields_ = [("R", _i32), ("rng", _vp), ("cursor", _vp), ("init_cursor", _vp), ("cur_slot", _vp),
                ("perm", _vp), ("perm_stride", _i64), ("init_perm", _vp), ("init_stride", _i64), ("rng_kind", _i32)]


class EvalMCOut(C.Structure):
    """struct offsim_evalmc_out"""
    _fields_ = [("sum_g", _vp), ("n_ep", _vp), ("steps", _vp), ("cand", _vp), ("n_len", _vp), ("status", _vp),
                ("ep_g", _vp), ("ep_len", _vp), ("ep_cap", _i64), ("trace_row", _vp), ("trace_pop", _vp),
                ("trace_cap", _i64), ("dbg", _vp)]


class Streams(C.Structure):
    """struct offsim_streams"""
    _fields_ = [("dig", _vp), ("dig_stride", _i64), ("loc", _vp), ("loc_stride", _i64), ("format", _i32)]


class Column(C.Structure):
    """struct offsim_column"""
    _fields_ = [("src", _vp), ("dst", _vp), ("row_bytes", _i64), ("zero_if_not_ok", _i32), ("reserved", _i32)]


class TD(C.Structure):
    """struct offsim_td"""
    _fields_ = [("mode", _i32), ("alpha", C.c_double), ("q", _vp), ("td_err", _vp), ("td_cap", _i64), ("behaviour", _i32), ("epsilon", C.c_double),
                ("alpha_ep", _vp), ("epsilon_ep", _vp), ("n_sched", _i64), ("q_snap", _vp), ("snap_cap", _i64), ("snap_stride", _i64),
                ("tie_mt", _vp), ("beh_arg", _vp)]


class TDPop(C.Structure):
    """struct offsim_td_pop"""
    _fields_ = [("mode", _i32), ("alpha", _vp), ("epsilon", _vp), ("gamma", _vp), ("gamma_pow", _vp), ("n_gamma_pow", _i64), ("behaviour", _vp),
                ("behaviour_host", C.POINTER(_i32)), ("alpha_ep", _vp), ("epsilon_ep", _vp), ("n_sched", _i64), ("pi", _vp), ("pi_stride", _i64),
                ("q", _vp), ("td_err", _vp), ("td_cap", _i64), ("q_snap", _vp), ("snap_cap", _i64), ("snap_stride", _i64), ("tie_mt", _vp),
                ("beh_arg", _vp)]


ACT_IDENTITY, ACT_TANH, ACT_RELU, ACT_LEAKY_RELU = 0, 1, 2, 3
POLICY_MLP_MAX_LAYERS, POLICY_MLP_MAX_IN, POLICY_MLP_MAX_HIDDEN, POLICY_MLP_MAX_ACTIONS = 4, 128, 256, 16


class MLPLayer(C.Structure):
    """struct offsim_mlp_layer"""
    _fields_ = [("W", _vp), ("b", _vp), ("in", _i32), ("out", _i32)]


COLLECT_MLP, COLLECT_ROWS, COLLECT_TABULAR = 0, 1, 2
COLLECT_MLP_MAX_FLOATS = 16384
COLLECT_SERVED, COLLECT_TERMINATED, COLLECT_TRUNCATED, COLLECT_RESET, COLLECT_ALIVE = 1, 2, 4, 8, 16


class CollectPolicy(C.Structure):
    """struct offsim_collect_policy"""
    _fields_ = [("form", _i32), ("n_layers", _i32), ("layers_host", C.POINTER(MLPLayer)), ("activation", _i32), ("slope", C.c_float),
                ("x_dtype", _i32), ("dO", _i32), ("x_start", _vp), ("x_next", _vp), ("x_init", _vp), ("p_next", _vp), ("p_init", _vp),
                ("pi", _vp)]


class CollectState(C.Structure):
    """struct offsim_collect_state"""
    _fields_ = [("ep_t", _vp), ("obs_row", _vp), ("alive", _vp), ("obs", _vp), ("obs_next", _vp), ("obs_init", _vp), ("obs_bytes", _i64)]


class CollectOut(C.Structure):
    """struct offsim_collect_out"""
    _fields_ = [("row", _vp), ("flags", _vp), ("obs", _vp), ("probs", _vp), ("status", _vp)]


VALUE_MLP, VALUE_ROWS = 0, 1
PPO_BOOT_REFERENCE, PPO_BOOT_SPINUP = 0, 1
EPLEN_REFERENCE, EPLEN_STEPS = 0, 1
PPO_LOG_STATS = 10


def ppo_work_doubles(E):
    """include/offsim.h: OFFSIM_PPO_WORK_DOUBLES(E)"""
    return 3 * ((E + 255) // 256)


class CollectValue(C.Structure):
    """struct offsim_collect_value"""
    _fields_ = [("form", _i32), ("n_layers", _i32), ("layers_host", C.POINTER(MLPLayer)), ("activation", _i32), ("slope", C.c_float),
                ("x_dtype", _i32), ("dO", _i32), ("x_start", _vp), ("x_next", _vp), ("x_init", _vp), ("v_next", _vp), ("v_init", _vp)]


class CollectPPOOut(C.Structure):
    """struct offsim_collect_ppo_out"""
    _fields_ = [("value", _vp), ("logp", _vp), ("final_value", _vp), ("v_trunc", _vp)]


ENV_GRID, ENV_GRID_COORDS, ENV_CARTPOLE = 0, 1, 2


class Env(C.Structure):
    """struct offsim_env"""
    _fields_ = [("kind", _i32), ("R", _i32), ("num_cells", _i32), ("num_steps", _i32), ("goal_x", _i32), ("goal_y", _i32), ("rng_env", _vp),
                ("rng_act", _vp), ("state", _vp), ("step_count", _vp), ("ep_t", _vp)]


class EnvOut(C.Structure):
    """struct offsim_env_out"""
    _fields_ = [("obs", _vp), ("next_obs", _vp), ("state", _vp), ("next_state", _vp), ("probs", _vp), ("action", _vp), ("reward", _vp),
                ("flags", _vp), ("ep_step", _vp), ("status", _vp)]


class EnvEval(C.Structure):
    """struct offsim_env_eval"""
    _fields_ = [("kind", _i32), ("S", _i32), ("num_cells", _i32), ("num_steps", _i32), ("goal_x", _i32), ("goal_y", _i32), ("rng_env", _vp),
                ("rng_act", _vp)]


class EnvEvalOut(C.Structure):
    """struct offsim_env_eval_out"""
    _fields_ = [("Gs", _vp), ("lengths", _vp), ("ended", _vp), ("n_ep", _vp), ("steps", _vp), ("status", _vp), ("value", _vp), ("trace_cap", _i64),
                ("trace_action", _vp), ("trace_state", _vp), ("trace_next_state", _vp)]


LATENT_BOX, LATENT_MLP = 0, 1


class LatentEncoder(C.Structure):
    """struct offsim_latent_encoder"""
    _fields_ = [("kind", _i32), ("nS", _i32), ("dO", _i32), ("H", _i32), ("nZ", _i32), ("W1", _vp), ("b1", _vp), ("W2", _vp), ("b2", _vp)]


class LatentRun(C.Structure):
    """struct offsim_latent_run"""
    _fields_ = [("reseed", _i32), ("max_episode_steps", _i32), ("rec_max", _i32), ("tie_reseed_episode", _i32), ("episode0", _i64),
                ("rng_act_end", _vp), ("rng_env_end", _vp), ("trace_cap", _i64), ("trace_z", _vp), ("trace_z_next", _vp), ("trace_reward", _vp),
                ("trace_done", _vp), ("trace_state", _vp), ("trace_next_state", _vp)]


GRID_PLAIN, GRID_NOISE, GRID_COUNTER = 0, 1, 2


class GridEnv(C.Structure):
    """struct offsim_grid_env"""
    _fields_ = [("kind", _i32), ("num_cells", _i32), ("num_steps", _i32), ("goal_x", _i32), ("goal_y", _i32), ("factor", _i32)]


class EnvRollouts(C.Structure):
    """struct offsim_env_rollouts"""
    _fields_ = [("R", _i32), ("rng_kind", _i32), ("rng", _vp)]


PPO_ACTOR, PPO_CRITIC = 0, 1
PPO_MAX_BLOCKS = 256


def ppo_update_work_doubles(P):
    """include/offsim.h: OFFSIM_PPO_UPDATE_WORK_DOUBLES(P)"""
    return PPO_MAX_BLOCKS * 8 + 8 + PPO_MAX_BLOCKS * ((P + 1) // 2)


class PPONet(C.Structure):
    """struct offsim_ppo_net"""
    _fields_ = [("n_layers", _i32), ("activation", _i32), ("layers_host", C.POINTER(MLPLayer)), ("slope", C.c_float), ("reserved", _i32)]


class PPOBatchC(C.Structure):
    """struct offsim_ppo_batch"""
    _fields_ = [("obs", _vp), ("x_dtype", _i32), ("dO", _i32), ("act", _vp), ("adv", _vp), ("logp", _vp), ("ret", _vp), ("valid", _vp),
                ("M", _i64)]


class PPOAdam(C.Structure):
    """struct offsim_ppo_adam"""
    _fields_ = [("m", _vp), ("v", _vp), ("t", _vp), ("lr", C.c_double)]


class PPOAdamPop(C.Structure):
    """struct offsim_ppo_adam_pop"""
    _fields_ = [("m", _vp), ("v", _vp), ("t", _vp), ("lr", C.POINTER(C.c_double))]


def ppo_update_work_doubles_nb(P, nb):
    """include/offsim.h: OFFSIM_PPO_UPDATE_WORK_DOUBLES_NB(P, NB)"""
    return nb * 8 + 8 + nb * ((P + 1) // 2)


HOMER_MAX_BLOCKS, HOMER_MAX_FLOATS = 128, 20480


def homer_params(dO, nA, nZ, H):
    """the number of trainable parameters of the HOMER model: offsim_homer_grad's P"""
    return dO * H + H + H * nZ + nZ + (2 * nZ + nA) * H + H + 2 * H + 2


def homer_work_doubles(P):
    """include/offsim.h: OFFSIM_HOMER_WORK_DOUBLES(P)"""
    return HOMER_MAX_BLOCKS * 2 + 8 + (P + 255) // 256 + (P + 1) // 2 + HOMER_MAX_BLOCKS * ((P + 1) // 2)


class HomerNet(C.Structure):
    """struct offsim_homer_net"""
    _fields_ = [("enc_W1", _vp), ("enc_b1", _vp), ("enc_W2", _vp), ("enc_b2", _vp), ("cls_W1", _vp), ("cls_b1", _vp), ("cls_W2", _vp),
                ("cls_b2", _vp), ("dO", _i32), ("nA", _i32), ("nZ", _i32), ("H", _i32), ("slope", C.c_float), ("reserved", _i32)]


class HomerBatch(C.Structure):
    """struct offsim_homer_batch"""
    _fields_ = [("obs", _vp), ("next_obs", _vp), ("x_dtype", _i32), ("reserved", _i32), ("act", _vp), ("n_rows", _i64), ("idx_real", _vp),
                ("idx_impo", _vp), ("noise", _vp), ("M", _i64)]


class HomerAdam(C.Structure):
    """struct offsim_homer_adam"""
    _fields_ = [("m", _vp), ("v", _vp), ("t", _vp), ("lr", C.c_double), ("weight_decay", C.c_double)]


def homer_work_doubles_nb(P, nb):
    """include/offsim.h: OFFSIM_HOMER_WORK_DOUBLES_NB(P, NB)"""
    return nb * 2 + 8 + (P + 255) // 256 + (P + 1) // 2 + nb * ((P + 1) // 2)


class HomerBatchPop(C.Structure):
    """struct offsim_homer_batch_pop"""
    _fields_ = [("obs", _vp), ("next_obs", _vp), ("x_dtype", _i32), ("reserved", _i32), ("act", _vp), ("n_rows", _i64), ("idx_real", _vp),
                ("idx_impo", _vp), ("noise", _vp), ("M", _i64), ("idx_stride", _i64)]


class HomerAdamPop(C.Structure):
    """struct offsim_homer_adam_pop"""
    _fields_ = [("m", _vp), ("v", _vp), ("t", _vp), ("lr", _vp), ("weight_decay", _vp), ("max_grad_norm", _vp)]


MAILBOX_MAX_ACTIONS = 24
SERVER_CMD_STEP, SERVER_CMD_POP_ONE, SERVER_CMD_EXIT, SERVER_CMD_RESET = 1, 2, 3, 4
SERVER_STARTING, SERVER_RUNNING, SERVER_EXITED = 1, 2, 3
SERVER_GONE = 1  # offsim_step_server_call: the server ended before it saw the request
SERVER_ANSWER_SECONDS = 10.0  # include/offsim.h: OFFSIM_SERVER_ANSWER_SECONDS


class StepMailbox(C.Structure):
    """struct offsim_step_mailbox (host-coherent pinned memory shared with the resident step server)"""
    _fields_ = [("seq_in", C.c_uint32), ("cmd", C.c_uint32), ("reject_mode", _i32), ("reserved0", C.c_uint32), ("p_head", C.c_double * 5),
                ("reserved1", C.c_uint32), ("seq_in2", C.c_uint32), ("p_tail", C.c_double * (MAILBOX_MAX_ACTIONS - 5)),
                ("reserved2", C.c_uint32 * 2), ("seq_out", C.c_uint32), ("row", _i32), ("status", _i32), ("popped", C.c_uint32),
                ("state", C.c_uint32), ("reserved3", C.c_uint32 * 3)]


TD_QLEARN, TD_EXPSARSA = 1, 2
BEHAVIOUR_FIXED, BEHAVIOUR_EPS_GREEDY, BEHAVIOUR_SOFT_GREEDY = 0, 1, 2
EXO_RESEED_NONE, EXO_RESEED_EPISODE = 0, 1


class ReplayLog(C.Structure):
    """struct offsim_replay_log"""
    _fields_ = [("N", _i64), ("nS", _i32), ("nA", _i32), ("s", _vp), ("a", _vp), ("r", _vp), ("s_next", _vp), ("done", _vp)]


class Replay(C.Structure):
    """struct offsim_replay"""
    _fields_ = [("mode", _i32), ("order", _vp), ("M", _i64), ("passes", _i64), ("alpha", _vp), ("gamma", _vp), ("alpha_ep", _vp), ("n_sched", _i64),
                ("pi", _vp), ("pi_stride", _i64), ("q", _vp), ("td_err", _vp), ("td_cap", _i64), ("q_snap", _vp), ("snap_cap", _i64),
                ("snap_stride", _i64), ("n_ep", _vp), ("steps", _vp), ("status", _vp)]


class ExoOut(C.Structure):
    """struct offsim_exo_out"""
    _fields_ = [("trace_row_x", _vp), ("last", _vp)]


# name -> (restype, argtypes): exactly the entry points include/offsim.h declares
SIGNATURES = {
    "offsim_last_error": (C.c_char_p, []),
    "offsim_version": (C.c_int, []),
    "offsim_device_count": (C.c_int, []),
    "offsim_group_scratch_bytes": (_i64, [_i64, _i32]),
    "offsim_group_by_state": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "offsim_gather_rows": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "offsim_seed_streams": (C.c_int, [_vp, _i32, _vp, _vp]),
    "offsim_pcg_jump_probe": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp]),
    "offsim_shuffle_queues": (C.c_int, [C.POINTER(Table), _vp, _i32, _vp, _vp, _vp]),
    "offsim_env_reset": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), _vp, _vp, _vp]),
    "offsim_env_set_state": (C.c_int, [C.POINTER(Rollouts), _vp, _vp, _vp]),
    "offsim_vector_gather": (C.c_int, [_vp, _vp, _vp, C.c_int32, _vp, C.c_int32, _vp, _vp]),
    "offsim_vector_step": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), _vp, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    "offsim_step_batch": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "offsim_eval_mc": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), _vp, _i32, _i32, C.c_double, _vp, _i64, _i64,
                                 C.POINTER(EvalMCOut), _vp]),
    "offsim_step_exo": (C.c_int, [C.POINTER(Table), C.POINTER(Table), C.POINTER(Rollouts), C.POINTER(Rollouts), _vp, _i32,
                                  _vp, _vp, _vp, _vp, _vp]),
    "offsim_eval_td": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), _vp, _i32, C.c_double, _vp, _i64, _i64,
                                 C.POINTER(EvalMCOut), C.POINTER(TD), _vp]),
    "offsim_eval_td_pop": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), _i32, _i32, C.POINTER(TDPop), _i32, _i64, C.POINTER(EvalMCOut), _vp]),
    "offsim_td_curves": (C.c_int, [_vp, _vp, _i32, _i32, _i64, _vp, _vp, _vp, _vp]),
    "offsim_eval_mc_exo": (C.c_int, [C.POINTER(Table), C.POINTER(Table), C.POINTER(Rollouts), C.POINTER(Rollouts), _vp, _vp, _i32, _i32, _i32,
                                     C.c_uint64, C.c_double, _vp, _i64, _i64, C.POINTER(EvalMCOut), C.POINTER(ExoOut), C.POINTER(TD), _vp]),
    "offsim_eval_td_exo_pop": (C.c_int, [C.POINTER(Table), C.POINTER(Table), C.POINTER(Rollouts), C.POINTER(Rollouts), _i32, _i32, C.POINTER(TDPop), _vp,
                                         _i32, _i32, C.c_uint64, _i64, C.POINTER(EvalMCOut), C.POINTER(ExoOut), _vp]),
    "offsim_eval_queue": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), _i32, _vp, C.c_double, _vp, _i64, _i64, C.POINTER(EvalMCOut),
                                    C.POINTER(TD), _i32, _i64, _vp, _vp]),
    "offsim_eval_queue_pop": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), _i32, _i32, _i32, C.POINTER(TDPop), _i64, C.POINTER(EvalMCOut), _i32,
                                        _i64, _vp, _vp]),
    "offsim_eval_queue_rows_policy": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), _i32, _vp, _vp, _i32, C.c_double, _vp, _i64, _i64,
                                                C.POINTER(EvalMCOut), _vp, _vp, _vp]),
    "offsim_eval_queue_rows_policy_pop": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), _i32, _vp, _vp, _i32, _i32, _i32, C.c_double, _vp, _i64,
                                                    _i64, C.POINTER(EvalMCOut), _vp, _vp, _vp]),
    "offsim_eval_env": (C.c_int, [C.POINTER(GridEnv), C.POINTER(EnvRollouts), _vp, C.c_double, _vp, _i64, _i64, C.POINTER(EvalMCOut), C.POINTER(TD),
                                  _i32, _i64, _vp]),
    "offsim_eval_env_pop": (C.c_int, [C.POINTER(GridEnv), C.POINTER(EnvRollouts), _i32, _i32, C.POINTER(TDPop), _vp, C.c_double, _vp, _i64, _i64,
                                      C.POINTER(EvalMCOut), _i32, _i64, _vp]),
    "offsim_compile_policy": (C.c_int, [C.POINTER(Table), _vp, _vp, _vp]),
    "offsim_eval_mc_keys_kernel": (C.c_char_p, [_i32, _i32]),
    "offsim_compile_digests": (C.c_int, [C.POINTER(Table), _vp, _i32, _vp, _vp]),
    "offsim_shuffle_queues_keys": (C.c_int, [C.POINTER(Table), _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    "offsim_shuffle_queues_keys_ws": (C.c_int, [C.POINTER(Table), _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "offsim_shuffle_workspace_bytes": (_i64, [C.POINTER(Table), _i32]),
    "offsim_shuffle_queues_ws": (C.c_int, [C.POINTER(Table), _vp, _i32, _vp, _vp, _vp, _i64, _vp]),
    "offsim_eval_mc_streams": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), C.POINTER(Streams), _vp, C.c_double, _vp, _i64, _i64,
                                         C.POINTER(EvalMCOut), _vp]),
    "offsim_eval_mc_keys": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), _vp, C.c_double, _vp, _i64, _i64,
                                      C.POINTER(EvalMCOut), _vp]),
    "offsim_selftest_lds_atomic_order": (C.c_int, [_vp, _vp]),
    "offsim_lds_order_ok": (C.c_int, []),
    "offsim_host_alloc": (C.c_int, [_i64, C.POINTER(_vp)]),
    "offsim_host_free": (C.c_int, [_vp]),
    "offsim_step_server_start": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), _vp, _i32, C.c_uint32, _vp]),
    "offsim_step_server_call": (C.c_int, [_vp, _vp, _i32, _i32, C.c_uint32, _i32, C.c_uint64, _vp]),
    "offsim_async_faults": (C.c_int, []),
    "offsim_encode_box": (C.c_int, [_vp, _i64, _vp, _vp]),
    "offsim_encode_mlp": (C.c_int, [_vp, _i32, _i64, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "offsim_encode_mlp_pop": (C.c_int, [_vp, _i32, _i64, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "offsim_latent_counts": (C.c_int, [_vp, _i32, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    "offsim_eval_mc_rows_policy": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), _vp, _vp, _i32, _i32, C.c_double, _vp, _i64, _i64,
                                             C.POINTER(EvalMCOut), _vp, _vp]),
    "offsim_eval_mc_rows_policy_pop": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), _vp, _vp, _i32, _i32, _i32, _i32, C.c_double, _vp, _i64,
                                                 _i64, C.POINTER(EvalMCOut), _vp, _vp]),
    "offsim_policy_mlp": (C.c_int, [_vp, _i32, _i64, _i32, _vp, _i64, C.POINTER(MLPLayer), _i32, _i32, C.c_float, _vp, _vp]),
    "offsim_policy_mlp_pop": (C.c_int, [_vp, _i32, _i64, _i32, _vp, _i64, C.POINTER(MLPLayer), _i32, _i32, C.c_float, _i32, _vp, _vp]),
    "offsim_vector_collect": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), C.POINTER(CollectPolicy), _i32, _i32, _i64, _i32,
                                        C.POINTER(CollectState), C.POINTER(CollectOut), _vp]),
    "offsim_value_mlp": (C.c_int, [_vp, _i32, _i64, _i32, _vp, _i64, C.POINTER(MLPLayer), _i32, _i32, C.c_float, _vp, _vp]),
    "offsim_vector_collect_ppo": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), C.POINTER(CollectPolicy), C.POINTER(CollectValue), _i32, _i32,
                                            _i64, _i32, C.POINTER(CollectState), C.POINTER(CollectOut), C.POINTER(CollectPPOOut), _vp]),
    "offsim_ppo_advantages": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, C.c_double, C.c_double, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "offsim_ppo_update_work_doubles": (_i64, [C.POINTER(PPONet)]),
    "offsim_ppo_grad": (C.c_int, [C.POINTER(PPONet), _i32, C.POINTER(PPOBatchC), C.c_double, _vp, _vp, _vp, _vp]),
    "offsim_ppo_update": (C.c_int, [C.POINTER(PPONet), _i32, C.POINTER(PPOBatchC), C.c_double, C.c_double, _i32, C.POINTER(PPOAdam), _vp, _vp,
                                    _vp, _vp]),
    "offsim_vector_collect_ppo_pop": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), C.POINTER(CollectPolicy), C.POINTER(CollectValue), _i32, _i32,
                                                _i32, _i32, _i64, _i32, C.POINTER(CollectState), C.POINTER(CollectOut), C.POINTER(CollectPPOOut), _vp]),
    "offsim_queue_collect": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), _i32, C.POINTER(CollectPolicy), _i64, _i32, C.POINTER(CollectState),
                                       C.POINTER(CollectOut), _vp, _vp]),
    "offsim_queue_collect_ppo": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), _i32, C.POINTER(CollectPolicy), C.POINTER(CollectValue), _i64, _i32,
                                           C.POINTER(CollectState), C.POINTER(CollectOut), _vp, C.POINTER(CollectPPOOut), _vp]),
    "offsim_queue_collect_ppo_pop": (C.c_int, [C.POINTER(Table), C.POINTER(Rollouts), _i32, C.POINTER(CollectPolicy), C.POINTER(CollectValue), _i32,
                                               _i32, _i64, _i32, C.POINTER(CollectState), C.POINTER(CollectOut), _vp, C.POINTER(CollectPPOOut), _vp]),
    "offsim_env_collect_reset": (C.c_int, [C.POINTER(Env), _vp, _vp]),
    "offsim_env_collect": (C.c_int, [C.POINTER(Env), C.POINTER(CollectPolicy), _i64, _i32, C.POINTER(EnvOut), _vp]),
    "offsim_env_collect_ppo": (C.c_int, [C.POINTER(Env), C.POINTER(CollectPolicy), C.POINTER(CollectValue), _i64, _i32, C.POINTER(EnvOut),
                                         C.POINTER(CollectPPOOut), _vp]),
    "offsim_env_collect_ppo_pop": (C.c_int, [C.POINTER(Env), C.POINTER(CollectPolicy), C.POINTER(CollectValue), _i32, _i32, _i64, _i32,
                                             C.POINTER(EnvOut), C.POINTER(CollectPPOOut), _vp]),
    "offsim_eval_env_obs": (C.c_int, [C.POINTER(EnvEval), C.POINTER(CollectPolicy), _i32, _i64, _i32, _vp, _i64, C.POINTER(EnvEvalOut), _vp]),
    "offsim_eval_env_latent": (C.c_int, [C.POINTER(EnvEval), C.POINTER(LatentEncoder), _vp, C.c_double, _vp, _i64, _i64, C.POINTER(EvalMCOut),
                                         C.POINTER(TD), C.POINTER(LatentRun), _vp]),
    "offsim_eval_env_latent_pop": (C.c_int, [C.POINTER(EnvEval), C.POINTER(LatentEncoder), _i32, _i32, C.POINTER(TDPop), _vp, C.c_double, _vp, _i64,
                                             _i64, C.POINTER(EvalMCOut), C.POINTER(LatentRun), _vp]),
    "offsim_ppo_advantages_pop": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i64, C.c_double, C.c_double, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "offsim_ppo_epoch_log": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "offsim_ppo_epoch_log_pop": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "offsim_ppo_update_work_doubles_pop":(_i64, [C.POINTER(PPONet), _i32, _i64]),
    "offsim_ppo_grad_pop": (C.c_int, [C.POINTER(PPONet), _i32, C.POINTER(PPOBatchC), _i32, _i32, C.POINTER(C.c_double), _vp, _vp, _vp, _vp]),
    "offsim_ppo_update_pop": (C.c_int, [C.POINTER(PPONet), _i32, C.POINTER(PPOBatchC), _i32, _i32, C.POINTER(C.c_double), C.POINTER(C.c_double), _i32,
                                        C.POINTER(PPOAdamPop), _vp, _vp, _vp, _vp]),
    "offsim_homer_work_doubles": (_i64, [C.POINTER(HomerNet)]),
    "offsim_homer_grad": (C.c_int, [C.POINTER(HomerNet), C.POINTER(HomerBatch), C.c_double, _i32, _vp, _vp, _vp, _vp]),
    "offsim_homer_step": (C.c_int, [C.POINTER(HomerNet), C.POINTER(HomerBatch), C.c_double, C.c_double, C.POINTER(HomerAdam), _vp, _vp, _vp]),
    "offsim_homer_work_doubles_pop": (_i64, [C.POINTER(HomerNet), _i32, _i64]),
    "offsim_homer_grad_pop": (C.c_int, [C.POINTER(HomerNet), C.POINTER(HomerBatchPop), _i32, C.c_double, _i32, _vp, _vp, _vp, _vp, _vp]),
    "offsim_homer_step_pop": (C.c_int, [C.POINTER(HomerNet), C.POINTER(HomerBatchPop), _i32, C.c_double, C.POINTER(HomerAdamPop), _vp, _vp, _vp,
                                        _vp]),
    "offsim_replay_lpw": (_i32, [_i32, _i32, _i32]),
    "offsim_replay_td": (C.c_int, [C.POINTER(ReplayLog), _i32, _i32, C.POINTER(Replay), _vp]),
}

_lib = None


class OffsimError(RuntimeError):
    pass


def load():
    """dlopen the HIP library and bind every symbol; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OffsimError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(or rl-offline-simulation_amd/csrc/build.sh).  There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def check(rc):
    if rc != OK:
        raise OffsimError(f"offsim error {rc}: {load().offsim_last_error().decode()}")


FAULT_SHUFFLE, FAULT_SCAN = 1, 2


def check_async_faults():
    """Raise if a kernel gave up a bounded inter-wavefront wait since the last check (include/offsim.h: offsim_async_faults).
    Call with the stream synchronised -- the host-facing drivers do, after they have copied their results back."""
    v = load().offsim_async_faults()
    if v < 0:
        check(v)
    if v:
        what = [n for b, n in ((FAULT_SHUFFLE, "sampler reset (shuffle ring protocol)"), (FAULT_SCAN, "scan (chain / helper hand-off)")) if v & b]
        raise OffsimError("a kernel gave up a bounded wait instead of hanging: " + ", ".join(what) + "; the results of that call are invalid")


_LDS_ORDER = {}


def lds_order_ok(device=None):
    """include/offsim.h: offsim_lds_order_ok for `device` (default: the current one) -- whether the LDS of this part serves the
    same-address lanes of one ds_add_rtn_u32 / ds_wrxchg_rtn_b32 in lane order, which the row-packed scan and the chunked shuffle rely
    on.  One short self-test per device and process, cached (here and in the library); a device without the property gets one warning
    and the host mirror routes it to the window kernel on permutations and the in-place shuffle (same results, slower)."""
    import torch
    idx = torch.cuda.current_device() if device is None else torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    if idx not in _LDS_ORDER:
        with torch.cuda.device(idx):
            v = load().offsim_lds_order_ok()
        if v < 0:
            check(v)
        _LDS_ORDER[idx] = bool(v)
        if not v:
            import warnings
            warnings.warn(f"offsim: cuda:{idx} does not apply same-address LDS lanes in lane order (offsim_lds_order_ok = 0): the row-packed "
                          "scan and the chunked shuffle are off for this device -- window kernel on permutations, in-place shuffle",
                          RuntimeWarning, stacklevel=2)
    return _LDS_ORDER[idx]


def require_device():
    """Fail loudly when the HIP path cannot run (no GPU visible to torch)."""
    import torch
    if not torch.cuda.is_available():
        raise OffsimError("no HIP device visible: the PSRS engine runs only on the GPU (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    # the LDS lane-order guard runs its one-time self-test here, at table construction -- never inside a launch path, whose stream may
    # be capturing (include/offsim.h, offsim_lds_order_ok)
    lds_order_ok(dev)
    return dev


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    """device pointer of a contiguous torch tensor (None -> NULL)"""
    if t is None:
        return None
    assert t.is_contiguous(), "offsim needs contiguous tensors"
    return t.data_ptr()

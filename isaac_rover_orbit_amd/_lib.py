"""ctypes loader of the C-ABI HIP library ``librover_hip.so`` (declared in ``include/rover_hip.h``).

The product path has NO CPU fallback: if the library is missing or a call fails, a ``RoverHipError`` is raised.
"""
from __future__ import annotations

import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "librover_hip.so")

NUM_REW, NUM_TERM, NUM_BODIES, LOG_WORDS, STATE_WORDS = 7, 4, 13, 16, 72

# state word offsets (include/rover_hip.h)
POS, QUAT, LINVEL, ANGVEL = 0, 3, 7, 10
BOGIE_Q, STEER_Q, WHEEL_Q, BOGIE_QD, STEER_QD, WHEEL_QD = 13, 16, 20, 26, 29, 33
TARGET_W, HEADING_CMD_W, ENV_ORIGIN, ACTION, PREV_ACTION, TIME_LEFT, EP_LEN = 39, 42, 43, 46, 48, 50, 51
CMD_B, HEADING_CMD_B, EP_SUM, METRIC_POS, METRIC_HEAD, LAMBDA_N, RESET_COUNT = 52, 55, 56, 63, 64, 65, 71

EXPORTS = [
    "rover_default_config", "rover_create", "rover_destroy", "rover_set_terrain", "rover_set_terrain_q16", "rover_workspace_bytes", "rover_bind",
    "rover_reset", "rover_reset_with_draws", "rover_set_seed", "rover_get_counter", "rover_set_counter", "rover_step", "rover_profile_step",
    "rover_profile_event_overhead", "rover_mdp_terms", "rover_ackermann", "rover_height_scan", "rover_physics", "rover_model_constants",
    "rover_state_words", "rover_config_bytes", "rover_last_error", "rover_version", "rover_set_markers", "rover_kernel_names",
    "rover_set_log_deferred", "rover_flush_log", "rover_step_begin", "rover_step_finish", "rover_set_obs_streaming",
    "rover_terrain_rasterize", "rover_terrain_surface", "rover_terrain_rock_mask", "rover_terrain_scratch_bytes",   # rover_terrain.h
    "rover_set_terrain_lookup",
    "rover_policy_default_desc", "rover_policy_packed_floats", "rover_policy_pack", "rover_policy_forward",  # rover_policy.h
    "rover_policy_forward_pair", "rover_lift_policy_desc",
    "rover_lift_default_config", "rover_lift_config_bytes", "rover_lift_state_words", "rover_lift_create", "rover_lift_destroy",
    "rover_lift_workspace_bytes", "rover_lift_bind", "rover_lift_reset", "rover_lift_step", "rover_lift_terms",   # rover_lift.h
    "rover_lift_model_constants", "rover_lift_set_seed", "rover_lift_profile_step", "rover_lift_kernel_name",
    "rover_lift_set_log_deferred", "rover_lift_flush_log",
    "rover_camera_default_config", "rover_camera_config_bytes", "rover_camera_workspace_bytes", "rover_camera_prepare",  # rover_camera.h
    "rover_camera_render",
    "rover_viewer_default_config", "rover_viewer_config_bytes", "rover_viewer_workspace_bytes", "rover_viewer_prepare",  # rover_viewer.h
    "rover_viewer_render",
    "rover_ppo_default_hparams", "rover_ppo_hparams_bytes", "rover_ppo_state_bytes", "rover_ppo_param_floats",  # rover_train.h
    "rover_ppo_workspace_bytes", "rover_ppo_minibatch", "rover_ppo_apply", "rover_ppo_gae", "rover_ppo_kl_schedule",
    "rover_policy_unpack",
    "rover_lift_ppo_default_hparams", "rover_lift_ppo_hparams_bytes", "rover_lift_ppo_state_bytes",  # rover_lift_train.h
    "rover_lift_ppo_param_floats", "rover_lift_ppo_workspace_bytes", "rover_lift_ppo_scaler_doubles", "rover_lift_ppo_standardize",
    "rover_lift_ppo_minibatch", "rover_lift_ppo_apply", "rover_lift_ppo_kl_schedule",
    "rover_trpo_default_hparams", "rover_trpo_hparams_bytes", "rover_trpo_state_bytes", "rover_trpo_param_floats",  # rover_trpo.h
    "rover_trpo_workspace_bytes", "rover_trpo_policy_grad", "rover_trpo_fvp", "rover_trpo_policy_step", "rover_trpo_value_minibatch",
    "rover_trpo_value_apply",
    "rover_td3_default_hparams", "rover_td3_hparams_bytes", "rover_td3_state_bytes", "rover_td3_critic_desc",  # rover_td3.h
    "rover_td3_critic_pack", "rover_td3_param_floats", "rover_td3_workspace_bytes", "rover_td3_critic_step", "rover_td3_actor_step",
    "rover_td3_polyak",
    "rover_rollout_default_hparams", "rover_rollout_hparams_bytes", "rover_rollout_act", "rover_rollout_record",  # rover_rollout.h
    "rover_lift_rollout_default_hparams", "rover_lift_rollout_hparams_bytes", "rover_lift_rollout_act",  # rover_lift_rollout.h
    "rover_lift_rollout_record",
    "rover_td3_collect_default_hparams", "rover_td3_collect_hparams_bytes", "rover_td3_collect_act",  # rover_td3_collect.h
    "rover_td3_collect_record",
    "rover_td3_explore_default_hparams", "rover_td3_explore_hparams_bytes", "rover_td3_explore_act",  # rover_td3_explore.h
    "rover_td3_smooth_draw",
    "rover_trace_stream_bytes", "rover_trace_stage_pitch", "rover_trace_stage_bytes", "rover_trace_state_bytes",  # rover_trace.h
    "rover_trace_init", "rover_trace_append", "rover_trace_commit_all", "rover_trace_gather", "rover_trace_drained",
    "rover_sac_default_hparams", "rover_sac_hparams_bytes", "rover_sac_state_bytes", "rover_sac_param_floats",  # rover_sac.h
    "rover_sac_workspace_bytes", "rover_sac_critic_step", "rover_sac_policy_step", "rover_sac_polyak",
    "rover_sac_collect_default_hparams", "rover_sac_collect_hparams_bytes", "rover_sac_collect_act",  # rover_sac_collect.h
    "rover_sac_collect_record",
    "rover_scaler_default_hparams", "rover_scaler_hparams_bytes", "rover_scaler_doubles", "rover_scaler_workspace_bytes",  # rover_scaler.h
    "rover_scaler_train", "rover_scaler_apply", "rover_scaler_train_gated",
    "rover_ppo_epoch_bytes", "rover_ppo_minibatch_gated", "rover_ppo_apply_gated", "rover_ppo_epoch_end",  # rover_train_gate.h
    "rover_rollout_record_shaped",  # rover_rollout.h
    "rover_tracker_state_bytes", "rover_tracker_workspace_bytes", "rover_tracker_snapshot_words", "rover_tracker_init",  # rover_tracker.h
    "rover_tracker_step", "rover_tracker_track", "rover_tracker_snapshot",
    "rover_offpolicy_stage_resolve", "rover_offpolicy_stage_rows",  # rover_offpolicy_scaled.h
    "rover_lift_viewer_default_config", "rover_lift_viewer_config_bytes", "rover_lift_viewer_workspace_bytes",  # rover_lift_viewer.h
    "rover_lift_viewer_constants", "rover_lift_viewer_env_origins", "rover_lift_viewer_render",
    "rover_dagger_default_hparams", "rover_dagger_hparams_bytes", "rover_dagger_state_bytes", "rover_dagger_param_floats",  # rover_dagger.h
    "rover_dagger_workspace_bytes", "rover_dagger_rows", "rover_dagger_act", "rover_dagger_record", "rover_dagger_update",
    "rover_dagger_conv_stem_floats", "rover_dagger_conv_param_floats", "rover_dagger_conv_stem_offset",  # rover_dagger_conv.h
    "rover_dagger_conv_chunk_rows", "rover_dagger_conv_workspace_bytes", "rover_dagger_conv_rows", "rover_dagger_conv_update",
    "rover_obs_post_segment_bytes", "rover_obs_post_apply",  # rover_obs_post.h
    "rover_depth_sensor_cfg_bytes", "rover_depth_sensor_apply",  # rover_depth_sensor.h
    "rover_elevation_cfg_bytes", "rover_elevation_step", "rover_elevation_scan",  # rover_elevation.h
    "rover_elevation_fill_cfg_bytes", "rover_elevation_fill",  # rover_elevation_fill.h
    "rover_elevation_traverse_cfg_bytes", "rover_elevation_traverse",  # rover_elevation_traverse.h
    "rover_lidar_config_bytes", "rover_lidar_workspace_bytes", "rover_lidar_prepare", "rover_lidar_cast",  # rover_lidar.h
]
POLICY_MAX_LAYERS = 8
ACT_NONE, ACT_LEAKY_RELU, ACT_TANH, ACT_ELU = 0, 1, 2, 3


class PolicyLayer(C.Structure):
    """Mirror of ``struct rover_policy_layer``."""
    _fields_ = [("K", C.c_int32), ("N", C.c_int32), ("act", C.c_int32), ("split_k", C.c_int32),
                ("w_off", C.c_uint32), ("b_off", C.c_uint32)]


class PolicyDesc(C.Structure):
    """Mirror of ``struct rover_policy_desc``."""
    _fields_ = [("obs_dim", C.c_int32), ("prop_dim", C.c_int32), ("enc_offset", C.c_int32), ("enc_dim", C.c_int32),
                ("n_enc", C.c_int32), ("n_mlp", C.c_int32), ("leaky_slope", C.c_float),
                ("layers", PolicyLayer * POLICY_MAX_LAYERS)]


class PpoHparams(C.Structure):
    """Mirror of ``struct rover_ppo_hparams`` (include/rover_train.h)."""
    _fields_ = [("gamma", C.c_float), ("lam", C.c_float), ("clip_ratio", C.c_float), ("value_clip", C.c_float),
                ("value_loss_scale", C.c_float), ("log_std_min", C.c_float), ("log_std_max", C.c_float),
                ("max_grad_norm", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("kl_threshold", C.c_float), ("lr_factor", C.c_float), ("lr_min", C.c_float), ("lr_max", C.c_float)]


class PpoState(C.Structure):
    """Mirror of ``struct rover_ppo_state`` (include/rover_train.h; it lives in device memory)."""
    _fields_ = [("lr", C.c_double), ("step", C.c_int32), ("grad_norm", C.c_float), ("clip_coef", C.c_float),
                ("step_size", C.c_float), ("bc2_sqrt", C.c_float), ("reserved", C.c_float)]


class PpoEpoch(C.Structure):
    """Mirror of ``struct rover_ppo_epoch`` (include/rover_train_gate.h; it lives in device memory)."""
    _fields_ = [("stop", C.c_int32), ("recorded", C.c_int32), ("epochs", C.c_int32), ("stopped_epochs", C.c_int32),
                ("stop_minibatch", C.c_int32), ("stop_kl", C.c_float), ("reserved", C.c_int32 * 2)]


class LiftPpoHparams(C.Structure):
    """Mirror of ``struct rover_lift_ppo_hparams`` (include/rover_lift_train.h)."""
    _fields_ = [("gamma", C.c_float), ("lam", C.c_float), ("clip_ratio", C.c_float), ("value_clip", C.c_float),
                ("value_loss_scale", C.c_float), ("log_std_min", C.c_float), ("log_std_max", C.c_float),
                ("max_grad_norm", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("kl_threshold", C.c_float), ("lr_factor", C.c_float), ("lr_min", C.c_float), ("lr_max", C.c_float),
                ("kl_early_stop", C.c_float), ("reward_scale", C.c_float), ("scaler_eps", C.c_float), ("scaler_clip", C.c_float)]


class LiftPpoState(C.Structure):
    """Mirror of ``struct rover_lift_ppo_state`` (include/rover_lift_train.h; it lives in device memory)."""
    _fields_ = [("lr", C.c_double), ("step", C.c_int32), ("grad_norm", C.c_float), ("clip_coef", C.c_float),
                ("step_size", C.c_float), ("bc2_sqrt", C.c_float), ("stop", C.c_int32), ("recorded", C.c_int32),
                ("epochs", C.c_int32), ("stopped_epochs", C.c_int32), ("reserved", C.c_int32)]


class TrpoHparams(C.Structure):
    """Mirror of ``struct rover_trpo_hparams`` (include/rover_trpo.h)."""
    _fields_ = [("gamma", C.c_float), ("lam", C.c_float), ("value_loss_scale", C.c_float), ("log_std_min", C.c_float),
                ("log_std_max", C.c_float), ("max_grad_norm", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("value_lr", C.c_float), ("damping", C.c_float), ("max_kl", C.c_float), ("cg_tol", C.c_float),
                ("accept_ratio", C.c_float), ("step_fraction", C.c_float), ("cg_steps", C.c_int32), ("max_backtrack", C.c_int32)]


class TrpoState(C.Structure):
    """Mirror of ``struct rover_trpo_state`` (include/rover_trpo.h; it lives in device memory)."""
    _fields_ = [("cg_done", C.c_int32), ("ls_done", C.c_int32), ("accepted", C.c_int32), ("cg_iters", C.c_int32),
                ("trials", C.c_int32), ("value_step", C.c_int32), ("value_batches", C.c_int32), ("reserved0", C.c_int32),
                ("loss_old", C.c_float), ("loss_new", C.c_float), ("rr_old", C.c_float), ("rr", C.c_float), ("cg_alpha", C.c_float),
                ("cg_beta", C.c_float), ("xhx", C.c_float), ("step", C.c_float), ("expected", C.c_float), ("kl", C.c_float),
                ("value_loss_sum", C.c_float), ("grad_norm", C.c_float), ("clip_coef", C.c_float), ("step_size", C.c_float),
                ("bc2_sqrt", C.c_float), ("reserved1", C.c_float)]


class Td3Hparams(C.Structure):
    """Mirror of ``struct rover_td3_hparams`` (include/rover_td3.h)."""
    _fields_ = [("gamma", C.c_float), ("polyak", C.c_float), ("actor_lr", C.c_float), ("critic_lr", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("eps", C.c_float), ("noise_clip", C.c_float), ("act_min", C.c_float), ("act_max", C.c_float)]


class Td3State(C.Structure):
    """Mirror of ``struct rover_td3_state`` (include/rover_td3.h; it lives in device memory)."""
    _fields_ = [("critic_step", C.c_int32), ("actor_step", C.c_int32), ("critic_updates", C.c_int32), ("bad_index", C.c_int32),
                ("critic_loss", C.c_float), ("policy_loss", C.c_float), ("q1_mean", C.c_float), ("q2_mean", C.c_float),
                ("y_mean", C.c_float), ("critic_step_size", C.c_float), ("critic_bc2_sqrt", C.c_float), ("actor_step_size", C.c_float),
                ("actor_bc2_sqrt", C.c_float), ("reserved", C.c_float * 3)]


class RolloutHparams(C.Structure):
    """Mirror of ``struct rover_rollout_hparams`` (include/rover_rollout.h)."""
    _fields_ = [("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("env_id_offset", C.c_int32), ("clip_actions", C.c_int32),
                ("action_low", C.c_float), ("action_high", C.c_float), ("log_std_min", C.c_float), ("log_std_max", C.c_float)]


class LiftRolloutHparams(C.Structure):
    """Mirror of ``struct rover_lift_rollout_hparams`` (include/rover_lift_rollout.h)."""
    _fields_ = [("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("env_id_offset", C.c_int32), ("clip_actions", C.c_int32),
                ("action_low", C.c_float), ("action_high", C.c_float), ("log_std_min", C.c_float), ("log_std_max", C.c_float),
                ("scaler_eps", C.c_float), ("scaler_clip", C.c_float), ("reward_scale", C.c_float)]


class Td3CollectHparams(C.Structure):
    """Mirror of ``struct rover_td3_collect_hparams`` (include/rover_td3_collect.h)."""
    _fields_ = [("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("env_id_offset", C.c_int32), ("explore", C.c_int32),
                ("noise_std", C.c_float), ("noise_scale", C.c_float), ("action_low", C.c_float), ("action_high", C.c_float)]


TD3_EXPLORE_OFF, TD3_EXPLORE_GAUSSIAN, TD3_EXPLORE_OU, TD3_EXPLORE_RANDOM = 0, 1, 2, 3


class Td3ExploreHparams(C.Structure):
    """Mirror of ``struct rover_td3_explore_hparams`` (include/rover_td3_explore.h)."""
    _fields_ = [("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("env_id_offset", C.c_int32), ("mode", C.c_int32),
                ("noise_std", C.c_float), ("noise_scale", C.c_float), ("ou_theta", C.c_float), ("ou_sigma", C.c_float),
                ("ou_base_scale", C.c_float), ("action_low", C.c_float), ("action_high", C.c_float)]


class TraceStream(C.Structure):
    """Mirror of ``struct rover_trace_stream`` (include/rover_trace.h)."""
    _fields_ = [("src", C.c_void_p), ("src_pitch", C.c_int64), ("stage", C.c_void_p), ("stage_pitch", C.c_int64),
                ("out", C.c_void_p), ("out_pitch", C.c_int64), ("row_bytes", C.c_int32), ("flags", C.c_int32)]


class SacHparams(C.Structure):
    """Mirror of ``struct rover_sac_hparams`` (include/rover_sac.h)."""
    _fields_ = [("gamma", C.c_float), ("polyak", C.c_float), ("actor_lr", C.c_float), ("critic_lr", C.c_float),
                ("entropy_lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("target_entropy", C.c_float), ("learn_entropy", C.c_int32)]


class SacState(C.Structure):
    """Mirror of ``struct rover_sac_state`` (include/rover_sac.h; it lives in device memory)."""
    _fields_ = [("critic_step", C.c_int32), ("actor_step", C.c_int32), ("entropy_step", C.c_int32), ("bad_index", C.c_int32),
                ("critic_loss", C.c_float), ("policy_loss", C.c_float), ("entropy_loss", C.c_float), ("q1_mean", C.c_float),
                ("q2_mean", C.c_float), ("y_mean", C.c_float), ("logp_mean", C.c_float), ("alpha", C.c_float),
                ("critic_step_size", C.c_float), ("critic_bc2_sqrt", C.c_float), ("actor_step_size", C.c_float),
                ("actor_bc2_sqrt", C.c_float), ("entropy_step_size", C.c_float), ("entropy_bc2_sqrt", C.c_float),
                ("reserved", C.c_float * 2)]


SAC_COLLECT_SAMPLE, SAC_COLLECT_MEAN, SAC_COLLECT_RANDOM = 0, 1, 2


class SacCollectHparams(C.Structure):
    """Mirror of ``struct rover_sac_collect_hparams`` (include/rover_sac_collect.h)."""
    _fields_ = [("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("env_id_offset", C.c_int32), ("mode", C.c_int32)]


class DaggerHparams(C.Structure):
    """Mirror of ``struct rover_dagger_hparams`` (include/rover_dagger.h)."""
    _fields_ = [("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("env_id_offset", C.c_int32), ("depth_clip", C.c_float),
                ("depth_scale", C.c_float), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("grad_norm_clip", C.c_float)]


class DaggerState(C.Structure):
    """Mirror of ``struct rover_dagger_state`` (include/rover_dagger.h; it lives in device memory)."""
    _fields_ = [("steps", C.c_int32), ("bad_index", C.c_int32), ("loss", C.c_float), ("grad_norm", C.c_float),
                ("clip_coef", C.c_float), ("step_size", C.c_float), ("bc2_sqrt", C.c_float), ("reserved", C.c_float)]


SCALER_MAX_WIDTH, SCALER_CHUNK_ROWS = 1024, 64
SCALER_INVERSE, SCALER_SANITISE = 1, 2


class ScalerHparams(C.Structure):
    """Mirror of ``struct rover_scaler_hparams`` (include/rover_scaler.h)."""
    _fields_ = [("eps", C.c_float), ("clip", C.c_float)]


def scaler_doubles(width: int) -> int:
    """Mirror of ``rover_scaler_doubles``: mean[width], var[width], count."""
    return 2 * width + 1 if 1 <= width <= SCALER_MAX_WIDTH else 0


def scaler_workspace_bytes(width: int, max_rows: int) -> int:
    """Mirror of ``rover_scaler_workspace_bytes``: the batch mean and one float64 sum per column and chunk of 64 rows."""
    if not 1 <= width <= SCALER_MAX_WIDTH or max_rows < 2:
        return 0
    return 8 * width * (1 + (max_rows + SCALER_CHUNK_ROWS - 1) // SCALER_CHUNK_ROWS)


OBS_POST_MAX_SEGMENTS, OBS_POST_MAX_WIDTH = 8, 262144
OBS_POST_NONE, OBS_POST_UNIFORM, OBS_POST_GAUSSIAN, OBS_POST_CONSTANT = 0, 1, 2, 3
# Word 3 of the Philox counter of the post-processing draws: the HIGH HALF names the stream ("OP": observation rows, "OD": depth
# images, "OL": lidar frames), the low half carries the column quad.  td3_explore.TAGS is the table of the streams named by their
# upper 24 bits; the first two are checked against it by tests/test_obs_post.py, the lidar's by tests/test_lidar.py.
OBS_POST_STREAM_ROW = 0x4F500000
OBS_POST_STREAM_DEPTH = 0x4F440000
OBS_POST_STREAM_LIDAR = 0x4F4C0000     # "OL": lidar frames (ROVER_LIDAR_STREAM_NOISE, include/rover_lidar.h)


class ObsPostSegment(C.Structure):
    """Mirror of ``struct rover_obs_post_segment`` (include/rover_obs_post.h)."""
    _fields_ = [("col_lo", C.c_int32), ("col_hi", C.c_int32), ("noise", C.c_int32), ("a", C.c_float), ("b", C.c_float),
                ("has_clip", C.c_int32), ("clip_lo", C.c_float), ("clip_hi", C.c_float), ("scale", C.c_float)]


DEPTH_SENSOR_MAX_PIXELS = 16384
# the depth sensor model's two streams (include/rover_depth_sensor.h), named like the two above by the high half of word 3
DEPTH_SENSOR_STREAM_NORMAL = 0x444E0000
DEPTH_SENSOR_STREAM_DROPOUT = 0x44550000


class DepthSensorCfg(C.Structure):
    """Mirror of ``struct rover_depth_sensor_cfg`` (include/rover_depth_sensor.h)."""
    _fields_ = [("range_min", C.c_float), ("range_max", C.c_float), ("sigma0", C.c_float), ("sigma1", C.c_float),
                ("sigma2", C.c_float), ("p_drop", C.c_float), ("p_edge", C.c_float), ("edge_rel", C.c_float),
                ("edge_at_invalid", C.c_int32), ("disparity_step", C.c_float), ("fb", C.c_float), ("inv_step", C.c_float),
                ("invalid_value", C.c_float)]


ELEVATION_MIN_GRID, ELEVATION_MAX_GRID, ELEVATION_MAX_PIXELS, ELEVATION_MAX_RAYS = 8, 128, 16384, 4096


class ElevationCfg(C.Structure):
    """Mirror of ``struct rover_elevation_cfg`` (include/rover_elevation.h)."""
    _fields_ = [("cell", C.c_float), ("inv_cell", C.c_float), ("grid", C.c_int32), ("range_min", C.c_float),
                ("range_max", C.c_float), ("alpha", C.c_float), ("mount_pos", C.c_float * 3), ("height_offset", C.c_float),
                ("unknown_value", C.c_float)]


ELEVATION_FILL_MAX_ITERATIONS = 254


class ElevationFillCfg(C.Structure):
    """Mirror of ``struct rover_elevation_fill_cfg`` (include/rover_elevation_fill.h)."""
    _fields_ = [("iterations", C.c_int32)]


ELEVATION_TRAVERSE_MAX_RADIUS = 4


class ElevationTraverseCfg(C.Structure):
    """Mirror of ``struct rover_elevation_traverse_cfg`` (include/rover_elevation_traverse.h)."""
    _fields_ = [("radius", C.c_int32), ("min_support", C.c_int32), ("slope_crit", C.c_float), ("step_crit", C.c_float),
                ("rough_crit", C.c_float), ("w_slope", C.c_float), ("w_step", C.c_float), ("w_rough", C.c_float),
                ("unknown_cost", C.c_float)]


class LidarConfig(C.Structure):
    """Mirror of ``struct rover_lidar_config`` (include/rover_lidar.h)."""
    _fields_ = [("rays", C.c_int32), ("mount_pos", C.c_float * 3), ("near_clip", C.c_float), ("far_clip", C.c_float),
                ("attach_yaw_only", C.c_int32)]


class RoverHipError(RuntimeError):
    pass


LIFT_NUM_REW, LIFT_OBS, LIFT_ACT, LIFT_STATE_WORDS, LIFT_LOG_WORDS = 6, 36, 8, 64, 16
# lift state word offsets (include/rover_lift.h)
LIFT_Q, LIFT_QD, LIFT_OBJ_POS, LIFT_OBJ_QUAT, LIFT_OBJ_LIN, LIFT_OBJ_ANG, LIFT_CMD = 0, 9, 18, 21, 25, 28, 31
LIFT_TIME_LEFT, LIFT_EP_LEN, LIFT_ACTION, LIFT_PREV_ACTION, LIFT_EP_SUM, LIFT_RESET_COUNT, LIFT_CMD_COUNT = 38, 39, 40, 48, 56, 62, 63


class LiftConfig(C.Structure):
    """Mirror of ``struct lift_config`` (include/rover_lift.h)."""
    _fields_ = [
        ("sim_dt", C.c_float), ("decimation", C.c_int32), ("max_episode_length", C.c_int32), ("max_episode_length_s", C.c_float),
        ("action_scale", C.c_float), ("finger_open", C.c_float), ("finger_close", C.c_float),
        ("rew_weight", C.c_float * LIFT_NUM_REW),
        ("reach_std", C.c_float), ("goal_std", C.c_float), ("goal_fine_std", C.c_float), ("minimal_height", C.c_float),
        ("drop_height", C.c_float), ("cmd_lo", C.c_float * 3), ("cmd_hi", C.c_float * 3), ("cmd_resample_time", C.c_float),
        ("obj_init", C.c_float * 3), ("obj_range_lo", C.c_float * 3), ("obj_range_hi", C.c_float * 3), ("ee_offset_z", C.c_float),
        ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("solver_iterations", C.c_int32), ("mu_table", C.c_float),
        ("mu_pad", C.c_float),
    ]


class RoverConfig(C.Structure):
    """Mirror of ``struct rover_config``."""
    _fields_ = [
        ("scale_lin", C.c_float), ("scale_ang", C.c_float), ("offset_lin", C.c_float), ("offset_ang", C.c_float),
        ("wheel_radius", C.c_float), ("d_fr", C.c_float), ("d_mw", C.c_float), ("wheelbase", C.c_float),
        ("sim_dt", C.c_float), ("decimation", C.c_int32), ("max_episode_length", C.c_int32),
        ("max_episode_length_s", C.c_float),
        ("success_threshold", C.c_float), ("far_threshold", C.c_float), ("target_distance", C.c_float),
        ("heading_lo", C.c_float), ("heading_hi", C.c_float), ("resample_time", C.c_float),
        ("rew_weight", C.c_float * NUM_REW),
        ("obs_scale_distance", C.c_float), ("obs_scale_heading", C.c_float),
        ("scan_resolution", C.c_float), ("scan_size_x", C.c_float), ("scan_size_y", C.c_float),
        ("scan_height_offset", C.c_float), ("scan_nx", C.c_int32), ("scan_ny", C.c_int32),
        ("reset_z_offset", C.c_float), ("reset_mode", C.c_int32), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32),
        ("friction_mu", C.c_float), ("solver_iterations", C.c_int32), ("max_target_tries", C.c_int32),
        ("step_mapping", C.c_int32), ("spawn_draw", C.c_int32), ("counter_lo", C.c_uint32), ("counter_hi", C.c_uint32),
        ("scan_surface", C.c_int32), ("mass_model", C.c_int32),
        ("rew_success_threshold", C.c_float), ("rew_far_threshold", C.c_float),
    ]


class CameraConfig(C.Structure):
    """Mirror of ``struct rover_camera_config`` (include/rover_camera.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("focal_length", C.c_float), ("horizontal_aperture", C.c_float),
                ("vertical_aperture", C.c_float), ("mount_pos", C.c_float * 3), ("mount_quat", C.c_float * 4),
                ("near_clip", C.c_float), ("far_clip", C.c_float)]


VIEWER_ORIGIN_WORLD, VIEWER_ORIGIN_ENV = 0, 1
VIEWER_MAX_SIZE = 8192


class ViewerConfig(C.Structure):
    """Mirror of ``struct rover_viewer_config`` (include/rover_viewer.h)."""
    _fields_ = [("eye", C.c_float * 3), ("lookat", C.c_float * 3), ("origin_type", C.c_int32), ("env_index", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32), ("focal_length", C.c_float), ("horizontal_aperture", C.c_float),
                ("near_clip", C.c_float), ("far_clip", C.c_float), ("draw_targets", C.c_int32)]


class LiftViewerConfig(C.Structure):
    """Mirror of ``struct rover_lift_viewer_config`` (include/rover_lift_viewer.h)."""
    _fields_ = ViewerConfig._fields_ + [("env_spacing", C.c_float), ("ee_offset_z", C.c_float)]


_lib = None


def _hip_runtimes() -> set:
    out = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    out.add(line.split()[-1])
    except OSError:
        pass
    return out


# (rover_X_bytes entry, Python mirror of struct rover_X): load() refuses a library whose sizes differ
_MIRRORS = [("rover_config_bytes", RoverConfig), ("rover_lift_config_bytes", LiftConfig), ("rover_camera_config_bytes", CameraConfig),
            ("rover_viewer_config_bytes", ViewerConfig), ("rover_ppo_hparams_bytes", PpoHparams), ("rover_ppo_state_bytes", PpoState),
            ("rover_ppo_epoch_bytes", PpoEpoch), ("rover_lift_ppo_hparams_bytes", LiftPpoHparams),
            ("rover_lift_ppo_state_bytes", LiftPpoState), ("rover_trpo_hparams_bytes", TrpoHparams),
            ("rover_trpo_state_bytes", TrpoState), ("rover_td3_hparams_bytes", Td3Hparams), ("rover_td3_state_bytes", Td3State),
            ("rover_rollout_hparams_bytes", RolloutHparams), ("rover_lift_rollout_hparams_bytes", LiftRolloutHparams),
            ("rover_td3_collect_hparams_bytes", Td3CollectHparams), ("rover_td3_explore_hparams_bytes", Td3ExploreHparams),
            ("rover_sac_hparams_bytes", SacHparams), ("rover_sac_state_bytes", SacState),
            ("rover_sac_collect_hparams_bytes", SacCollectHparams), ("rover_scaler_hparams_bytes", ScalerHparams),
            ("rover_trace_stream_bytes", TraceStream), ("rover_lift_viewer_config_bytes", LiftViewerConfig),
            ("rover_dagger_hparams_bytes", DaggerHparams), ("rover_dagger_state_bytes", DaggerState),
            ("rover_obs_post_segment_bytes", ObsPostSegment), ("rover_depth_sensor_cfg_bytes", DepthSensorCfg),
            ("rover_elevation_cfg_bytes", ElevationCfg), ("rover_elevation_fill_cfg_bytes", ElevationFillCfg),
            ("rover_elevation_traverse_cfg_bytes", ElevationTraverseCfg),
            ("rover_lidar_config_bytes", LidarConfig)]


def load():
    """Load ``librover_hip.so`` (built in-tree by ``__graft_entry__.build()`` / ``isaac_rover_orbit_amd.build``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RoverHipError(
            f"{LIB_PATH} not found: build it with `python -m isaac_rover_orbit_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the rover hot path.")
    # torch-ROCm bundles its own libamdhip64.so.7; device pointers and streams are only meaningful inside ONE HIP runtime,
    # so torch must be loaded first: the dynamic linker then binds librover_hip.so to the runtime torch already mapped.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    runtimes = _hip_runtimes()
    if len(runtimes) > 1:
        raise RoverHipError(f"two HIP runtimes are mapped into this process ({sorted(runtimes)}): import torch before "
                            "loading librover_hip.so")
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    lib.rover_default_config.argtypes = [C.POINTER(RoverConfig)]
    lib.rover_create.argtypes = [C.POINTER(RoverConfig), i32, i32, i32, C.POINTER(vp)]
    lib.rover_destroy.argtypes = [vp]
    lib.rover_set_terrain.argtypes = [vp, vp, vp, vp, i32, i32, f32, f32, f32, vp, i32]
    lib.rover_set_terrain_q16.argtypes = [vp, vp, f32]
    lib.rover_workspace_bytes.argtypes = [vp]
    lib.rover_workspace_bytes.restype = C.c_size_t
    lib.rover_bind.argtypes = [vp, vp, vp, C.c_size_t]
    lib.rover_reset.argtypes = [vp, vp, vp]
    lib.rover_reset_with_draws.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    lib.rover_set_seed.argtypes = [vp, C.c_uint32, C.c_uint32]
    lib.rover_get_counter.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.rover_set_counter.argtypes = [vp, C.c_uint64]
    lib.rover_profile_event_overhead.argtypes = [vp, vp, i32, C.POINTER(C.c_float)]
    lib.rover_set_markers.argtypes = [vp, i32]
    lib.rover_set_log_deferred.argtypes = [vp, i32]
    lib.rover_flush_log.argtypes = [vp, vp, vp]
    lib.rover_set_obs_streaming.argtypes = [vp, i32]
    lib.rover_step_begin.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.rover_step_finish.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.rover_kernel_names.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_size_t]
    lib.rover_mdp_terms.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.rover_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.rover_profile_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.rover_ackermann.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    lib.rover_height_scan.argtypes = [vp, vp, vp]
    lib.rover_physics.argtypes = [vp, vp, vp, i32, vp, vp]
    lib.rover_model_constants.argtypes = [vp, i32]
    lib.rover_terrain_rasterize.argtypes = [vp, vp, i32, vp, i32, i32, vp]
    lib.rover_terrain_surface.argtypes = [vp, vp, i32, vp, i32, i32, C.c_double, C.c_double, C.c_double, vp]
    lib.rover_set_terrain_lookup.argtypes = [vp, vp]
    lib.rover_terrain_rock_mask.argtypes = [vp, i32, i32, C.c_double, vp, vp, vp, vp]
    lib.rover_terrain_scratch_bytes.argtypes = [i32, i32]
    lib.rover_terrain_scratch_bytes.restype = C.c_size_t
    lib.rover_policy_default_desc.argtypes = [C.POINTER(PolicyDesc), i32, i32]
    lib.rover_policy_packed_floats.argtypes = [C.POINTER(PolicyDesc)]
    lib.rover_policy_packed_floats.restype = C.c_size_t
    lib.rover_policy_pack.argtypes = [C.POINTER(PolicyDesc), C.POINTER(vp), C.POINTER(vp), vp]
    lib.rover_policy_forward.argtypes = [C.POINTER(PolicyDesc), vp, i32, vp, i32, vp, vp]
    lib.rover_policy_forward_pair.argtypes = [C.POINTER(PolicyDesc), vp, C.POINTER(PolicyDesc), vp, i32, vp, i32, vp, vp, vp]
    lib.rover_lift_default_config.argtypes = [C.POINTER(LiftConfig)]
    lib.rover_lift_config_bytes.restype = C.c_size_t
    lib.rover_lift_create.argtypes = [C.POINTER(LiftConfig), i32, i32, i32, C.POINTER(vp)]
    lib.rover_lift_destroy.argtypes = [vp]
    lib.rover_lift_workspace_bytes.argtypes = [vp]
    lib.rover_lift_workspace_bytes.restype = C.c_size_t
    lib.rover_lift_bind.argtypes = [vp, vp, vp, C.c_size_t]
    lib.rover_lift_reset.argtypes = [vp, vp, vp]
    lib.rover_lift_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    lib.rover_lift_model_constants.argtypes = [vp, i32]
    lib.rover_lift_set_seed.argtypes = [vp, C.c_uint32, C.c_uint32]
    lib.rover_lift_profile_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.rover_lift_set_log_deferred.argtypes = [vp, C.c_int32]
    lib.rover_lift_flush_log.argtypes = [vp, vp, vp]
    lib.rover_lift_kernel_name.argtypes = [vp, C.c_char_p, C.c_size_t]
    lib.rover_lift_debug_set_lanes.argtypes = [vp, i32]
    lib.rover_lift_terms.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.rover_camera_default_config.argtypes = [C.POINTER(CameraConfig)]
    lib.rover_camera_config_bytes.restype = C.c_size_t
    lib.rover_camera_workspace_bytes.argtypes = [vp, C.POINTER(CameraConfig)]
    lib.rover_camera_workspace_bytes.restype = C.c_size_t
    lib.rover_camera_prepare.argtypes = [vp, C.POINTER(CameraConfig), vp, C.c_size_t, vp]
    lib.rover_camera_render.argtypes = [vp, C.POINTER(CameraConfig), vp, vp, vp]
    lib.rover_viewer_default_config.argtypes = [C.POINTER(ViewerConfig)]
    lib.rover_viewer_config_bytes.restype = C.c_size_t
    lib.rover_viewer_workspace_bytes.argtypes = [vp, C.POINTER(ViewerConfig)]
    lib.rover_viewer_workspace_bytes.restype = C.c_size_t
    lib.rover_viewer_prepare.argtypes = [vp, C.POINTER(ViewerConfig), vp, C.c_size_t, vp]
    lib.rover_viewer_render.argtypes = [vp, C.POINTER(ViewerConfig), vp, vp, vp, vp, vp]
    lib.rover_lift_viewer_default_config.argtypes = [C.POINTER(LiftViewerConfig)]
    lib.rover_lift_viewer_config_bytes.restype = C.c_size_t
    lib.rover_lift_viewer_workspace_bytes.argtypes = [i32, C.POINTER(LiftViewerConfig)]
    lib.rover_lift_viewer_workspace_bytes.restype = C.c_size_t
    lib.rover_lift_viewer_constants.argtypes = [vp, i32]
    lib.rover_lift_viewer_env_origins.argtypes = [i32, f32, vp]
    lib.rover_lift_viewer_render.argtypes = [vp, i32, C.POINTER(LiftViewerConfig), vp, C.c_size_t, vp, vp, vp, vp]
    lib.rover_ppo_default_hparams.argtypes = [C.POINTER(PpoHparams)]
    lib.rover_ppo_hparams_bytes.restype = C.c_size_t
    lib.rover_ppo_state_bytes.restype = C.c_size_t
    lib.rover_ppo_param_floats.argtypes = [C.POINTER(PolicyDesc), C.POINTER(PolicyDesc)]
    lib.rover_ppo_param_floats.restype = C.c_size_t
    lib.rover_ppo_workspace_bytes.argtypes = [i32]
    lib.rover_ppo_workspace_bytes.restype = C.c_size_t
    lib.rover_ppo_minibatch.argtypes = [C.POINTER(PolicyDesc), C.POINTER(PolicyDesc), C.POINTER(PpoHparams), vp, vp, vp, vp, vp, vp,
                                        vp, vp, i32, vp, C.c_size_t, vp, vp, vp, vp, vp]
    lib.rover_ppo_apply.argtypes = [C.POINTER(PolicyDesc), C.POINTER(PolicyDesc), C.POINTER(PpoHparams), vp, vp, vp, vp, vp, vp, vp,
                                    i32, vp, C.c_size_t, vp]
    lib.rover_ppo_gae.argtypes = [C.POINTER(PpoHparams), vp, vp, vp, vp, i32, i32, vp, vp, vp]
    lib.rover_ppo_kl_schedule.argtypes = [C.POINTER(PpoHparams), vp, i32, vp, vp, vp]
    lib.rover_policy_unpack.argtypes = [C.POINTER(PolicyDesc), vp, C.POINTER(vp), C.POINTER(vp)]
    lib.rover_ppo_epoch_bytes.restype = C.c_size_t
    lib.rover_ppo_minibatch_gated.argtypes = [C.POINTER(PolicyDesc), C.POINTER(PolicyDesc), C.POINTER(PpoHparams), vp, vp, vp, vp, vp,
                                              vp, vp, vp, i32, vp, C.c_size_t, vp, vp, vp, vp, f32, vp, vp]
    lib.rover_ppo_apply_gated.argtypes = [C.POINTER(PolicyDesc), C.POINTER(PolicyDesc), C.POINTER(PpoHparams), vp, vp, vp, vp, vp, vp,
                                          vp, i32, vp, C.c_size_t, vp, vp]
    lib.rover_ppo_epoch_end.argtypes = [C.POINTER(PpoHparams), vp, i32, vp, vp, i32, vp, vp]
    lib.rover_lift_policy_desc.argtypes = [C.POINTER(PolicyDesc), i32]
    lib.rover_lift_ppo_default_hparams.argtypes = [C.POINTER(LiftPpoHparams)]
    lib.rover_lift_ppo_hparams_bytes.restype = C.c_size_t
    lib.rover_lift_ppo_state_bytes.restype = C.c_size_t
    lib.rover_lift_ppo_param_floats.argtypes = [C.POINTER(PolicyDesc), C.POINTER(PolicyDesc)]
    lib.rover_lift_ppo_param_floats.restype = C.c_size_t
    lib.rover_lift_ppo_workspace_bytes.argtypes = [i32]
    lib.rover_lift_ppo_workspace_bytes.restype = C.c_size_t
    lib.rover_lift_ppo_scaler_doubles.argtypes = [i32]
    lib.rover_lift_ppo_scaler_doubles.restype = C.c_size_t
    lib.rover_lift_ppo_standardize.argtypes = [C.POINTER(LiftPpoHparams), vp, i32, vp, i32, i32, i32, vp, vp, C.c_size_t, vp]
    lib.rover_lift_ppo_minibatch.argtypes = [C.POINTER(PolicyDesc), C.POINTER(PolicyDesc), C.POINTER(LiftPpoHparams), vp, vp, vp, vp,
                                             vp, vp, vp, vp, vp, i32, i32, vp, vp, C.c_size_t, vp, vp, vp, vp, vp]
    lib.rover_lift_ppo_apply.argtypes = [C.POINTER(PolicyDesc), C.POINTER(PolicyDesc), C.POINTER(LiftPpoHparams), vp, vp, vp, vp, vp,
                                         vp, vp, i32, vp, C.c_size_t, vp]
    lib.rover_lift_ppo_kl_schedule.argtypes = [C.POINTER(LiftPpoHparams), vp, i32, vp, vp, vp]
    lib.rover_trpo_default_hparams.argtypes = [C.POINTER(TrpoHparams)]
    lib.rover_trpo_hparams_bytes.restype = C.c_size_t
    lib.rover_trpo_state_bytes.restype = C.c_size_t
    lib.rover_trpo_param_floats.argtypes = [C.POINTER(PolicyDesc), C.POINTER(PolicyDesc)]
    lib.rover_trpo_param_floats.restype = C.c_size_t
    lib.rover_trpo_workspace_bytes.argtypes = [i32, i32]
    lib.rover_trpo_workspace_bytes.restype = C.c_size_t
    pd, th = C.POINTER(PolicyDesc), C.POINTER(TrpoHparams)
    lib.rover_trpo_policy_grad.argtypes = [pd, pd, th, vp, vp, vp, vp, vp, i32, vp, C.c_size_t, vp, vp, vp]
    lib.rover_trpo_fvp.argtypes = [pd, pd, th, vp, vp, i32, vp, C.c_size_t, vp, vp, vp]
    lib.rover_trpo_policy_step.argtypes = [pd, pd, th, vp, vp, vp, vp, vp, i32, vp, C.c_size_t, vp, vp, i32, vp, vp, vp]
    lib.rover_trpo_value_minibatch.argtypes = [pd, pd, th, vp, vp, vp, vp, i32, i32, vp, C.c_size_t, vp, vp, vp]
    lib.rover_trpo_value_apply.argtypes = [pd, pd, th, vp, vp, vp, vp, vp, vp, i32, vp, C.c_size_t, vp]
    tdh = C.POINTER(Td3Hparams)
    lib.rover_td3_default_hparams.argtypes = [tdh]
    lib.rover_td3_hparams_bytes.restype = C.c_size_t
    lib.rover_td3_state_bytes.restype = C.c_size_t
    lib.rover_td3_critic_desc.argtypes = [pd]
    lib.rover_td3_critic_pack.argtypes = [pd, C.POINTER(vp), C.POINTER(vp), vp]
    lib.rover_td3_param_floats.argtypes = [pd, pd]
    lib.rover_td3_param_floats.restype = C.c_size_t
    lib.rover_td3_workspace_bytes.argtypes = [i32]
    lib.rover_td3_workspace_bytes.restype = C.c_size_t
    lib.rover_td3_critic_step.argtypes = [pd, pd, tdh, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, C.c_int64, vp, vp,
                                          C.c_size_t, vp, vp, vp]
    lib.rover_td3_actor_step.argtypes = [pd, pd, tdh, vp, vp, vp, vp, vp, i32, i32, vp, vp, i32, C.c_int64, vp, C.c_size_t, vp, vp, i32,
                                         vp, vp]
    lib.rover_td3_polyak.argtypes = [tdh, vp, vp, C.c_size_t, vp]
    lib.rover_rollout_default_hparams.argtypes = [C.POINTER(RolloutHparams)]
    lib.rover_rollout_hparams_bytes.restype = C.c_size_t
    lib.rover_rollout_act.argtypes = [pd, vp, pd, vp, i32, C.POINTER(RolloutHparams), C.c_uint64, vp, i32, vp, vp, vp, vp, vp, vp, vp,
                                      vp, vp]
    lib.rover_rollout_record.argtypes = [vp, vp, vp, i32, vp, vp, vp]
    lib.rover_rollout_record_shaped.argtypes = [vp, vp, vp, vp, i32, f32, f32, i32, vp, vp, vp]
    lib.rover_lift_rollout_default_hparams.argtypes = [C.POINTER(LiftRolloutHparams)]
    lib.rover_lift_rollout_hparams_bytes.restype = C.c_size_t
    lib.rover_lift_rollout_act.argtypes = [pd, vp, pd, vp, i32, C.POINTER(LiftRolloutHparams), C.c_uint64, vp, i32, vp, vp, vp, vp, vp,
                                           vp, vp, vp, vp, vp, vp]
    lib.rover_lift_rollout_record.argtypes = [vp, vp, vp, i32, f32, vp, vp, vp, vp, vp, vp]
    tch = C.POINTER(Td3CollectHparams)
    lib.rover_td3_collect_default_hparams.argtypes = [tch]
    lib.rover_td3_collect_hparams_bytes.restype = C.c_size_t
    lib.rover_td3_collect_act.argtypes = [pd, vp, i32, tch, C.c_uint64, vp, i32, vp, vp, vp, vp, vp]
    lib.rover_td3_collect_record.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, i32, C.c_int64, tch, C.c_uint64, vp]
    teh = C.POINTER(Td3ExploreHparams)
    lib.rover_td3_explore_default_hparams.argtypes = [teh]
    lib.rover_td3_explore_hparams_bytes.restype = C.c_size_t
    lib.rover_td3_explore_act.argtypes = [pd, vp, i32, teh, C.c_uint64, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.rover_td3_smooth_draw.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, f32, vp, i32, i32, vp]
    trs = C.POINTER(TraceStream)
    for name in ("rover_trace_stream_bytes", "rover_trace_stage_pitch", "rover_trace_stage_bytes", "rover_trace_state_bytes"):
        getattr(lib, name).restype = C.c_size_t
    lib.rover_trace_stage_pitch.argtypes = [i32]
    lib.rover_trace_stage_bytes.argtypes = [i32, i32, i32]
    lib.rover_trace_state_bytes.argtypes = [i32, i32]
    lib.rover_trace_init.argtypes = [vp, i32, i32, vp]
    lib.rover_trace_append.argtypes = [trs, i32, vp, i32, i32, i32, i32, vp, vp]
    lib.rover_trace_commit_all.argtypes = [vp, i32, i32, i32, vp]
    lib.rover_trace_gather.argtypes = [trs, i32, vp, i32, i32, i32, i32, i32, vp]
    lib.rover_trace_drained.argtypes = [vp, i32, vp]
    sah = C.POINTER(SacHparams)
    lib.rover_sac_default_hparams.argtypes = [sah]
    lib.rover_sac_hparams_bytes.restype = C.c_size_t
    lib.rover_sac_state_bytes.restype = C.c_size_t
    lib.rover_sac_param_floats.argtypes = [pd, pd]
    lib.rover_sac_param_floats.restype = C.c_size_t
    lib.rover_sac_workspace_bytes.argtypes = [i32]
    lib.rover_sac_workspace_bytes.restype = C.c_size_t
    lib.rover_sac_critic_step.argtypes = [pd, pd, sah, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, C.c_int64, vp, vp,
                                          C.c_size_t, vp, vp, vp]
    lib.rover_sac_policy_step.argtypes = [pd, pd, sah, vp, vp, vp, vp, vp, i32, i32, vp, vp, i32, C.c_int64, vp, vp, C.c_size_t, vp, vp,
                                          i32, vp, vp, vp, vp]
    lib.rover_sac_polyak.argtypes = [pd, pd, sah, vp, vp, vp]
    sch = C.POINTER(SacCollectHparams)
    lib.rover_sac_collect_default_hparams.argtypes = [sch]
    lib.rover_sac_collect_hparams_bytes.restype = C.c_size_t
    lib.rover_sac_collect_act.argtypes = [pd, vp, i32, vp, sch, C.c_uint64, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.rover_sac_collect_record.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, i32, C.c_int64, vp, sch, C.c_uint64, vp]
    slh = C.POINTER(ScalerHparams)
    lib.rover_scaler_default_hparams.argtypes = [slh]
    lib.rover_scaler_hparams_bytes.restype = C.c_size_t
    lib.rover_scaler_doubles.argtypes = [i32]
    lib.rover_scaler_doubles.restype = C.c_size_t
    lib.rover_scaler_workspace_bytes.argtypes = [i32, i32]
    lib.rover_scaler_workspace_bytes.restype = C.c_size_t
    lib.rover_scaler_train.argtypes = [slh, vp, i32, vp, vp, i32, vp, C.c_size_t, vp]
    lib.rover_scaler_apply.argtypes = [slh, vp, i32, vp, vp, i32, i32, vp, vp, vp]
    lib.rover_scaler_train_gated.argtypes = [slh, vp, i32, vp, vp, i32, vp, C.c_size_t, vp, vp]
    lib.rover_tracker_state_bytes.argtypes = [i32, i32]
    lib.rover_tracker_state_bytes.restype = C.c_size_t
    lib.rover_tracker_workspace_bytes.argtypes = [i32]
    lib.rover_tracker_workspace_bytes.restype = C.c_size_t
    lib.rover_tracker_snapshot_words.argtypes = [i32]
    lib.rover_tracker_snapshot_words.restype = C.c_size_t
    lib.rover_tracker_init.argtypes = [vp, i32, i32, vp]
    lib.rover_tracker_step.argtypes = [vp, i32, i32, vp, vp, vp, i32, vp, C.c_size_t, vp]
    lib.rover_tracker_track.argtypes = [vp, i32, i32, i32, vp, i32, vp]
    lib.rover_tracker_snapshot.argtypes = [vp, i32, i32, vp, i32, vp]
    lib.rover_offpolicy_stage_resolve.argtypes = [vp, i32, C.c_int64, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.rover_offpolicy_stage_rows.argtypes = [slh, vp, i32, vp, C.c_int64, vp, i32, vp, vp, vp]
    dgh = C.POINTER(DaggerHparams)
    lib.rover_dagger_default_hparams.argtypes = [dgh]
    lib.rover_dagger_hparams_bytes.restype = C.c_size_t
    lib.rover_dagger_state_bytes.restype = C.c_size_t
    lib.rover_dagger_param_floats.argtypes = [pd]
    lib.rover_dagger_param_floats.restype = C.c_size_t
    lib.rover_dagger_workspace_bytes.argtypes = [i32]
    lib.rover_dagger_workspace_bytes.restype = C.c_size_t
    lib.rover_dagger_rows.argtypes = [dgh, vp, vp, i32, vp, vp, vp]
    lib.rover_dagger_act.argtypes = [pd, vp, i32, pd, vp, i32, dgh, C.c_uint64, f32, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.rover_dagger_record.argtypes = [dgh, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, i32, C.c_int64, C.c_uint64, vp]
    lib.rover_dagger_update.argtypes = [pd, dgh, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, C.c_int64, vp, C.c_size_t, vp, vp, i32, vp,
                                        vp]
    lib.rover_dagger_conv_stem_floats.restype = C.c_size_t
    lib.rover_dagger_conv_param_floats.argtypes = [pd]
    lib.rover_dagger_conv_param_floats.restype = C.c_size_t
    lib.rover_dagger_conv_stem_offset.argtypes = [pd]
    lib.rover_dagger_conv_stem_offset.restype = C.c_size_t
    lib.rover_dagger_conv_chunk_rows.restype = i32
    lib.rover_dagger_conv_workspace_bytes.argtypes = [i32]
    lib.rover_dagger_conv_workspace_bytes.restype = C.c_size_t
    lib.rover_dagger_conv_rows.argtypes = [dgh, vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, i32, C.c_int64,
                                           C.c_uint64, vp]
    lib.rover_dagger_conv_update.argtypes = [pd, dgh, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, i32, C.c_int64, vp,
                                             C.c_size_t, vp, vp, i32, vp, vp, vp, vp]
    lib.rover_obs_post_segment_bytes.restype = C.c_size_t
    lib.rover_obs_post_apply.argtypes = [C.POINTER(ObsPostSegment), i32, vp, i32, C.c_int64, i32, C.c_uint64, C.c_uint64, C.c_uint64,
                                         C.c_uint32, vp]
    lib.rover_depth_sensor_cfg_bytes.restype = C.c_size_t
    lib.rover_depth_sensor_apply.argtypes = [C.POINTER(DepthSensorCfg), vp, vp, i32, i32, C.c_int64, i32, C.c_uint64, C.c_uint64,
                                             C.c_uint64, vp, vp]
    lib.rover_elevation_cfg_bytes.restype = C.c_size_t
    lib.rover_elevation_step.argtypes = [C.POINTER(ElevationCfg), vp, C.c_int64, i32, i32, vp, vp, vp, C.c_int64, C.c_int64, vp, vp,
                                         vp, vp, vp, i32, vp, i32, vp, C.c_int64, vp, vp, i32, vp]
    lib.rover_elevation_scan.argtypes = [C.POINTER(ElevationCfg), vp, vp, C.c_int64, C.c_int64, vp, vp, vp, i32, vp, i32, vp,
                                         C.c_int64, vp, vp, i32, vp]
    lib.rover_elevation_fill_cfg_bytes.restype = C.c_size_t
    lib.rover_elevation_fill.argtypes = [C.POINTER(ElevationCfg), C.POINTER(ElevationFillCfg), vp, vp, C.c_int64, C.c_int64, vp, vp,
                                         vp, i32, vp, i32, vp, C.c_int64, vp, vp, vp, vp, i32, vp]
    lib.rover_elevation_traverse_cfg_bytes.restype = C.c_size_t
    lib.rover_elevation_traverse.argtypes = [C.POINTER(ElevationCfg), C.POINTER(ElevationTraverseCfg), vp, vp, C.c_int64, C.c_int64,
                                             vp, vp, vp, i32, vp, i32, vp, C.c_int64, vp, vp, vp, vp, vp, vp, i32, vp]
    lib.rover_lidar_config_bytes.restype = C.c_size_t
    lib.rover_lidar_workspace_bytes.argtypes = [vp]
    lib.rover_lidar_workspace_bytes.restype = C.c_size_t
    lib.rover_lidar_prepare.argtypes = [vp, vp, C.c_size_t, vp]
    lib.rover_lidar_cast.argtypes = [vp, C.POINTER(LidarConfig), vp, vp, vp, C.c_int64, vp, vp]
    lib.rover_last_error.restype = C.c_char_p
    lib.rover_version.restype = C.c_char_p
    for name in EXPORTS:
        fn = getattr(lib, name)
        if fn.restype is C.c_int:
            fn.restype = C.c_int
    lib.rover_config_bytes.restype = C.c_size_t
    for entry, mirror in _MIRRORS:              # rover_X_bytes() of the library against sizeof of the Python mirror of struct rover_X
        if getattr(lib, entry)() != C.sizeof(mirror):
            raise RoverHipError(f"struct {entry[:-len('_bytes')]} of librover_hip.so does not match the Python mirror")
    if lib.rover_lift_state_words() != LIFT_STATE_WORDS:
        raise RoverHipError("lift state layout of librover_hip.so does not match the Python mirror")
    if lib.rover_state_words() != STATE_WORDS:
        raise RoverHipError("librover_hip.so state layout does not match the Python binding")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().rover_last_error().decode("utf-8", "replace")
        raise RoverHipError(f"{what} failed (code {rc}): {msg}")


def default_camera_config() -> CameraConfig:
    cfg = CameraConfig()
    check(load().rover_camera_default_config(C.byref(cfg)), "rover_camera_default_config")
    return cfg


def default_viewer_config() -> ViewerConfig:
    cfg = ViewerConfig()
    check(load().rover_viewer_default_config(C.byref(cfg)), "rover_viewer_default_config")
    return cfg


def default_config() -> RoverConfig:
    cfg = RoverConfig()
    check(load().rover_default_config(C.byref(cfg)), "rover_default_config")
    return cfg

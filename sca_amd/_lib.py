"""ctypes binding of libsca_hip.so (include/sca_hip.h).  No fallback: if the library is missing the import of
anything that needs it raises."""
import ctypes as C
import os

import numpy as np

from . import build as _build

K = 16
ACTION_DIM = 7
DIAG_DIM = 5

dp = C.POINTER(C.c_double)
fp = C.POINTER(C.c_float)
ip = C.POINTER(C.c_int32)
bp = C.POINTER(C.c_uint8)


class Params(C.Structure):
    _fields_ = [('neighbor_dist', C.c_double), ('time_step', C.c_double), ('time_horizon', C.c_double),
                ('max_speed', C.c_double), ('max_heading_change', C.c_double), ('near_goal_threshold', C.c_double),
                ('max_neighbors', C.c_int32), ('struct_bytes', C.c_int32), ('dt_nominal', C.c_double)]


class HostState(C.Structure):
    """sca_host_state: pointers into the library's page-locked state block (sca_host_state_get), rows of agent i at index i"""
    _fields_ = [('struct_bytes', C.c_int32), ('n', C.c_int32), ('pos', dp), ('vel', fp), ('heading', dp), ('flags', bp), ('total_dist', dp),
                ('step_num', ip), ('vpref', dp), ('vpref_mode', bp), ('action', fp)]


HOST_IN_STATE, HOST_IN_VPREF = 1, 2                               # SCA_HOST_IN_*


class SceneSummary(C.Structure):
    """sca_scene_summary: what k_scene_harvest writes for a scene in the step it finishes in (64 bytes)"""
    _fields_ = [('fresh', C.c_int32), ('steps', C.c_int32), ('batch_step', C.c_int32), ('arrived', C.c_int32), ('collided', C.c_int32),
                ('timed_out', C.c_int32), ('successful_num', C.c_int32), ('reserved0', C.c_int32), ('all_step_num', C.c_int64),
                ('all_distance', C.c_double), ('reserved1', C.c_int64 * 2)]


SUMMARY_DTYPE = np.dtype([('fresh', np.int32), ('steps', np.int32), ('batch_step', np.int32), ('arrived', np.int32), ('collided', np.int32),
                          ('timed_out', np.int32), ('successful_num', np.int32), ('reserved0', np.int32), ('all_step_num', np.int64),
                          ('all_distance', np.float64), ('reserved1', np.int64, (2,))])


class SceneHarvest(C.Structure):
    """sca_scene_harvest: pointers into the library's page-locked harvest block (sca_scene_harvest_get)"""
    _fields_ = [('struct_bytes', C.c_int32), ('nscenes', C.c_int32), ('n', C.c_int32), ('reserved', C.c_int32), ('counters', ip),
                ('summary', C.POINTER(SceneSummary)), ('pos', dp), ('vel', fp), ('heading', dp), ('flags', bp), ('total_dist', dp), ('step_num', ip)]


class RestartAttrs(C.Structure):
    """sca_restart_attrs: the attributes a restarted scene's episode brings (sca_restart_scenes_attrs); a NULL array = the context's value"""
    _fields_ = [('struct_bytes', C.c_int32), ('reserved', C.c_int32), ('neighbor_dist', dp), ('max_neighbors', ip), ('time_step', dp),
                ('time_horizon', dp), ('max_speed', dp), ('max_heading_change', dp), ('dt_nominal', dp), ('turning_radius', dp), ('pitch_lo', dp),
                ('pitch_hi', dp)]


class SceneCheckpointInfo(C.Structure):
    """struct sca_scene_checkpoint_info: the header of a scene checkpoint (sca_scene_checkpoint_info)"""
    _fields_ = [('struct_bytes', C.c_int32), ('reserved', C.c_int32), ('format', C.c_int32), ('lib_version', C.c_int32), ('size', C.c_int32),
                ('trk_words', C.c_int32), ('record_bytes', C.c_int32), ('has_tracker', C.c_int32), ('has_paths', C.c_int32), ('steps', C.c_int32),
                ('live', C.c_int32), ('prev', C.c_int32), ('total_bytes', C.c_int64), ('checksum', C.c_uint64)]


class ContextCheckpointShape(C.Structure):
    """sca_context_checkpoint_shape: what a context checkpoint's layout depends on (sca_context_checkpoint_layout)"""
    _fields_ = [('struct_bytes', C.c_int32), ('n', C.c_int32), ('trk_words', C.c_int32), ('list_form', C.c_int32), ('W', C.c_int32), ('M', C.c_int32),
                ('R', C.c_int32), ('has_gate', C.c_int32), ('has_clearance', C.c_int32)]


class ContextCheckpointInfo(C.Structure):
    """struct sca_context_checkpoint_info: the header of a context checkpoint (sca_context_checkpoint_info)"""
    _fields_ = [('struct_bytes', C.c_int32), ('reserved', C.c_int32), ('format', C.c_int32), ('lib_version', C.c_int32), ('n', C.c_int32),
                ('trk_words', C.c_int32), ('record_bytes', C.c_int32), ('has_tracker', C.c_int32), ('list_form', C.c_int32), ('W', C.c_int32),
                ('M', C.c_int32), ('R', C.c_int32), ('has_gate', C.c_int32), ('has_clearance', C.c_int32), ('clear_step', C.c_int32),
                ('state_fresh', C.c_int32), ('updates', C.c_int64), ('total_bytes', C.c_int64), ('checksum', C.c_uint64),
                ('occupied', C.c_int32), ('reserved1', C.c_int32)]


class SceneClearance(C.Structure):
    """sca_scene_clearance: an agent row's closest approach so far (sca_get_scene_clearance), 32 bytes"""
    _fields_ = [('agent_clear', C.c_double), ('obs_clear', C.c_double), ('agent_partner', C.c_int32), ('agent_step', C.c_int32),
                ('obs_partner', C.c_int32), ('obs_step', C.c_int32)]


CLEARANCE_DTYPE = np.dtype([('agent_clear', np.float64), ('obs_clear', np.float64), ('agent_partner', np.int32), ('agent_step', np.int32),
                            ('obs_partner', np.int32), ('obs_step', np.int32)])


class FinishedRow(C.Structure):
    """sca_finished_row: a row that carries at-goal / collision / timeout (sca_get_finished), 48 bytes"""
    _fields_ = [('id', C.c_int32), ('flags', C.c_uint32), ('step_num', C.c_int32), ('reserved', C.c_int32), ('total_dist', C.c_double),
                ('pos', C.c_double * 3)]


FINISHED_DTYPE = np.dtype([('id', np.int32), ('flags', np.uint32), ('step_num', np.int32), ('reserved', np.int32), ('total_dist', np.float64),
                           ('pos', np.float64, (3,))])


class Mission(C.Structure):
    """sca_mission: one entry of a row's mission table (sca_set_missions), 128 bytes"""
    _fields_ = [('pos', C.c_double * 3), ('heading', C.c_double * 3), ('goal', C.c_double * 3), ('goal_heading', C.c_double * 3),
                ('pref_speed', C.c_double), ('max_run_dist', C.c_double), ('vel', C.c_float * 3), ('next_ok', C.c_int8), ('next_fail', C.c_int8),
                ('zaxis', C.c_uint8), ('flags', C.c_uint8)]


MISSION_DTYPE = np.dtype([('pos', np.float64, (3,)), ('heading', np.float64, (3,)), ('goal', np.float64, (3,)), ('goal_heading', np.float64, (3,)),
                          ('pref_speed', np.float64), ('max_run_dist', np.float64), ('vel', np.float32, (3,)), ('next_ok', np.int8),
                          ('next_fail', np.int8), ('zaxis', np.uint8), ('flags', np.uint8)])


class MissionResult(C.Structure):
    """sca_mission_result: one ending of a row that has a table (sca_get_mission_results), 96 bytes"""
    _fields_ = [('id', C.c_int32), ('entry', C.c_int32), ('flags', C.c_uint32), ('step_num', C.c_int32), ('total_dist', C.c_double),
                ('pos', C.c_double * 3), ('update', C.c_int64), ('next', C.c_int32), ('reserved', C.c_int32), ('clear', SceneClearance)]


MISSION_RESULT_DTYPE = np.dtype([('id', np.int32), ('entry', np.int32), ('flags', np.uint32), ('step_num', np.int32), ('total_dist', np.float64),
                                 ('pos', np.float64, (3,)), ('update', np.int64), ('next', np.int32), ('reserved', np.int32), ('clear', CLEARANCE_DTYPE)])


class MissionTotals(C.Structure):
    """sca_mission_totals: the counters since sca_set_missions (sca_get_mission_totals), 64 bytes"""
    _fields_ = [(k, C.c_uint64) for k in ('updates', 'agent_steps', 'arrived', 'collided', 'timed_out', 'taken', 'stopped', 'reserved')]


class MissionGateTotals(C.Structure):
    """sca_mission_gate_totals: the gate's counters (sca_get_mission_gate_totals), 64 bytes"""
    _fields_ = [(k, C.c_uint64) for k in ('offered', 'admitted', 'blocked_agent', 'blocked_obstacle', 'blocked_entry', 'over_cap', 'dropped', 'reserved')]


CHECKPOINT_SECTIONS = 14                                         # sca_scene_checkpoint_layout's offsets
CONTEXT_CHECKPOINT_SECTIONS = 26                                 # sca_context_checkpoint_layout's offsets (SCA_CONTEXT_CHECKPOINT_SECTIONS)


# name -> (restype, argtypes); this table is also what tests/test_abi.py checks against include/sca_hip.h
SIGNATURES = {
    'sca_default_params': (None, [C.c_void_p]),                   # (version-100 form: 56 bytes)
    'sca_default_params_v2': (None, [C.POINTER(Params), C.c_int32]),
    'sca_version': (C.c_int, []),
    'sca_create': (C.c_int, [C.POINTER(Params), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    'sca_destroy': (None, [C.c_void_p]),
    'sca_last_error': (C.c_char_p, [C.c_void_p]),
    'sca_set_obstacles': (C.c_int, [C.c_void_p, C.c_int, dp, dp]),
    'sca_set_agents': (C.c_int, [C.c_void_p, C.c_int, dp, dp, dp, bp, bp, dp]),
    'sca_set_agent_params': (C.c_int, [C.c_void_p, C.c_int, dp, ip, dp, dp, dp, dp, dp]),
    'sca_set_state': (C.c_int, [C.c_void_p, dp, fp, dp, bp, dp, ip]),
    'sca_get_state': (C.c_int, [C.c_void_p, dp, fp, dp, bp, dp, ip]),
    'sca_set_kd_perm': (C.c_int, [C.c_void_p, ip]),
    'sca_get_kd_perm': (C.c_int, [C.c_void_p, ip]),
    'sca_get_kd_tree': (C.c_int, [C.c_void_p, dp]),
    'sca_set_vpref': (C.c_int, [C.c_void_p, dp, bp]),
    'sca_set_paths': (C.c_int, [C.c_void_p, C.c_int, ip, dp]),
    'sca_get_path_state': (C.c_int, [C.c_void_p, ip, dp]),
    'sca_get_path_slot_lists': (C.c_int, [C.c_void_p, ip, dp]),
    'sca_get_vpref_mode': (C.c_int, [C.c_void_p, bp]),
    'sca_set_scenes': (C.c_int, [C.c_void_p, C.c_int, ip]),
    'sca_get_scene_state': (C.c_int, [C.c_void_p, ip, ip]),
    'sca_set_scene_obstacles': (C.c_int, [C.c_void_p, C.c_int, ip, dp, dp]),
    'sca_restart_scenes': (C.c_int, [C.c_void_p, C.c_int, ip, dp, fp, dp, dp, dp, dp, bp, bp, dp, dp]),
    'sca_restart_scenes_sized': (C.c_int, [C.c_void_p, C.c_int, ip, ip, dp, fp, dp, dp, dp, dp, bp, bp, dp, dp]),
    'sca_get_scene_sizes': (C.c_int, [C.c_void_p, ip]),
    'sca_set_scene_obstacle_slots': (C.c_int, [C.c_void_p, C.c_int, ip, ip, dp, dp]),
    'sca_get_scene_obstacle_counts': (C.c_int, [C.c_void_p, ip, ip]),
    'sca_restart_scenes_obstacles': (C.c_int, [C.c_void_p, C.c_int, ip, ip, ip, dp, dp, dp, fp, dp, dp, dp, dp, bp, bp, dp, dp]),
    'sca_restart_scenes_attrs': (C.c_int, [C.c_void_p, C.c_int, ip, ip, ip, dp, dp, C.POINTER(RestartAttrs), dp, fp, dp, dp, dp, dp, bp, bp, dp, dp]),
    'sca_restart_scenes_paths': (C.c_int, [C.c_void_p, C.c_int, ip, ip, ip, dp, dp, C.POINTER(RestartAttrs), ip, dp, dp, fp, dp, dp, dp, dp, bp, bp, dp, dp]),
    'sca_set_path_slots': (C.c_int, [C.c_void_p, C.c_int, C.c_int, ip, dp]),
    'sca_get_path_slots': (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    'sca_scene_history_enable': (C.c_int, [C.c_void_p, C.c_int]),
    'sca_scene_history_rows': (C.c_int, [C.c_void_p, ip, ip]),
    'sca_get_scene_history': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, fp]),
    'sca_scene_harvest_layout': (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'sca_scene_harvest_enable': (C.c_int, [C.c_void_p, C.c_int]),
    'sca_scene_harvest_get': (C.c_int, [C.c_void_p, C.POINTER(SceneHarvest), C.c_int32]),
    'sca_scene_harvest_collect': (C.c_int, [C.c_void_p, ip, C.POINTER(C.c_int32)]),
    'sca_scene_checkpoint_layout': (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'sca_scene_checkpoint_info': (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(SceneCheckpointInfo), C.c_int32]),
    'sca_scene_checkpoint_bytes': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]),
    'sca_save_scenes': (C.c_int, [C.c_void_p, C.c_int, ip, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    'sca_load_scenes': (C.c_int, [C.c_void_p, C.c_int, ip, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    'sca_context_checkpoint_layout': (C.c_int, [C.POINTER(ContextCheckpointShape), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'sca_context_checkpoint_info': (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(ContextCheckpointInfo), C.c_int32]),
    'sca_context_checkpoint_bytes': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    'sca_save_context': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'sca_load_context': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'sca_context_checkpoint_bytes_opt': (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_int64)]),
    'sca_save_context_opt': (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64]),
    'sca_load_context_opt': (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64]),
    'sca_scene_clearance_enable': (C.c_int, [C.c_void_p, C.c_int]),
    'sca_get_scene_clearance': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(SceneClearance), C.c_int32]),
    'sca_clearance_enable': (C.c_int, [C.c_void_p, C.c_int]),
    'sca_get_clearance': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(SceneClearance), C.c_int32]),
    'sca_respawn_agents': (C.c_int, [C.c_void_p, C.c_int, ip, dp, fp, dp, dp, dp, dp, bp, dp, dp, ip, dp]),
    'sca_get_finished': (C.c_int, [C.c_void_p, C.POINTER(FinishedRow), C.c_int, C.POINTER(C.c_int), C.c_int32]),
    'sca_retire_agents': (C.c_int, [C.c_void_p, C.c_int, ip]),
    'sca_get_vacant': (C.c_int, [C.c_void_p, ip, C.c_int, C.POINTER(C.c_int)]),
    'sca_get_population': (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    'sca_probe_clearance': (C.c_int, [C.c_void_p, C.c_int, dp, dp, ip, C.POINTER(SceneClearance), C.c_int32]),
    'sca_respawn_agents_gated': (C.c_int, [C.c_void_p, C.c_int, ip, dp, fp, dp, dp, dp, dp, bp, dp, dp, ip, dp, C.c_double, ip, C.POINTER(SceneClearance), ip]),
    'sca_respawn_agents_attrs': (C.c_int, [C.c_void_p, C.c_int, ip, bp, C.POINTER(RestartAttrs), dp, fp, dp, dp, dp, dp, bp, dp, dp, ip, dp]),
    'sca_respawn_agents_gated_attrs': (C.c_int, [C.c_void_p, C.c_int, ip, bp, C.POINTER(RestartAttrs), dp, fp, dp, dp, dp, dp, bp, dp, dp, ip, dp, C.c_double, ip,
                                                 C.POINTER(SceneClearance), ip]),
    'sca_set_missions': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Mission), ip, ip]),
    'sca_set_missions_paths': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Mission), ip, ip, ip, dp]),
    'sca_get_mission_paths': (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    'sca_get_mission_results': (C.c_int, [C.c_void_p, C.POINTER(MissionResult), C.c_int, C.POINTER(C.c_int), C.c_int32]),
    'sca_get_mission_totals': (C.c_int, [C.c_void_p, C.POINTER(MissionTotals), C.c_int32]),
    'sca_get_mission_state': (C.c_int, [C.c_void_p, C.c_int, C.c_int, ip, ip]),
    'sca_set_mission_gate': (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int32]),
    'sca_get_mission_gate_state': (C.c_int, [C.c_void_p, C.c_int, C.c_int, ip, ip, ip]),
    'sca_get_mission_gate_totals': (C.c_int, [C.c_void_p, C.POINTER(MissionGateTotals), C.c_int32]),
    'sca_set_path_state': (C.c_int, [C.c_void_p, ip, dp]),
    'sca_policy_pass': (C.c_int, [C.c_void_p, C.c_int]),
    'sca_get_actions': (C.c_int, [C.c_void_p, fp]),
    'sca_get_neighbors': (C.c_int, [C.c_void_p, ip, ip, bp, dp, bp]),
    'sca_get_nbr0': (C.c_int, [C.c_void_p, dp]),
    'sca_get_diag': (C.c_int, [C.c_void_p, ip, ip, dp]),
    'sca_env_update': (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    'sca_run_steps': (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    'sca_env_step': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    'sca_host_state_layout': (C.c_int, [C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'sca_host_state_get': (C.c_int, [C.c_void_p, C.POINTER(HostState), C.c_int32]),
    'sca_step_host': (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_int)]),
    'sca_synchronize': (C.c_int, [C.c_void_p]),
    'sca_active_count': (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    'sca_set_shard': (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    'sca_public_records': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    'sca_bind_public_records': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    'sca_step_begin': (C.c_int, [C.c_void_p, C.c_int]),
    'sca_step_end': (C.c_int, [C.c_void_p]),
    'sca_set_stream': (C.c_int, [C.c_void_p, C.c_void_p]),
    'sca_use_own_stream': (C.c_int, [C.c_void_p]),
    'sca_comm_probe': (C.c_int, []),
    'sca_comm_unique_id': (C.c_int, [C.c_void_p]),
    'sca_comm_init': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'sca_comm_destroy': (C.c_int, [C.c_void_p]),
    'sca_partition_init': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, dp, C.c_int, C.c_int]),
    'sca_partition_disable': (C.c_int, [C.c_void_p]),
    'sca_partition_message_bytes': (C.c_int64, [C.c_void_p]),
    'sca_partition_pack': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'sca_partition_unpack': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'sca_partition_commit': (C.c_int, [C.c_void_p]),
    'sca_partition_counts': (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'sca_partition_owned': (C.c_int, [C.c_void_p, ip, C.POINTER(C.c_int)]),
    'sca_last_kernel_ms': (C.c_int, [C.c_void_p, fp, fp, fp]),
    'sca_last_exchange_ms': (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    'sca_last_kd_build_ms': (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    'sca_auto_stats': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    'sca_last_replan_ms': (C.c_int, [C.c_void_p, fp]),
    'sca_last_pass_forms': (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    'sca_set_shard_emulation': (C.c_int, [C.c_void_p, C.c_int]),
    'sca_set_profiling': (C.c_int, [C.c_void_p, C.c_int]),
    'sca_agent_steps': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    'sca_selftest_l3norm': (C.c_int, [C.c_void_p, C.c_int, dp, dp, dp, dp]),
    'sca_selftest_libm': (C.c_int, [C.c_void_p, C.c_int, C.c_int, dp, dp, dp]),
    'sca_selftest_libm_host': (C.c_int, [C.c_int, C.c_int, dp, dp, dp]),
    'sca_history_enable': (C.c_int, [C.c_void_p, C.c_int]),
    'sca_history_rows': (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'sca_get_history': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, fp]),
    'sca_tracker_create': (C.c_void_p, [C.c_int, dp, dp, dp, bp, C.c_double, C.c_double, C.c_double, C.c_double]),
    'sca_tracker_set_neighbor_dist': (C.c_int, [C.c_void_p, dp]),
    'sca_tracker_set_agent_params': (C.c_int, [C.c_void_p, dp, dp, dp]),
    'sca_tracker_destroy': (None, [C.c_void_p]),
    'sca_tracker_vpref': (C.c_int, [C.c_void_p, dp, fp, dp, bp, dp, dp, C.c_int]),
    'sca_tracker_replans': (C.c_int, [C.c_void_p, ip]),
    'sca_tracker_debug': (C.c_int, [C.c_void_p, C.c_int, dp]),
    'sca_device_tracker_debug': (C.c_int, [C.c_void_p, C.c_int, dp]),
    'sca_device_tracker_enable': (C.c_int, [C.c_void_p, dp, C.c_double, C.c_double, C.c_double, C.c_int]),
    'sca_device_tracker_disable': (C.c_int, [C.c_void_p]),
    'sca_device_tracker_set_agent_params': (C.c_int, [C.c_void_p, C.c_int, dp, dp, dp]),
    'sca_device_tracker_vpref': (C.c_int, [C.c_void_p, dp, dp]),
    'sca_device_tracker_replans': (C.c_int, [C.c_void_p, ip]),
    'sca_selftest_dubins_words': (C.c_int, [C.c_int, dp, dp, dp, C.POINTER(C.c_int64)]),
    'sca_selftest_plan3d_lean': (C.c_int, [C.c_int, dp, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'sca_libm_check': (C.c_int, [C.POINTER(C.c_int64)]),
    'sca_dubins_plan': (C.c_int, [dp, dp, C.c_double, C.c_double, C.c_double, dp, C.c_char_p, ip, dp, C.c_int]),
    'sca_candidate_table': (C.c_int, [C.c_int, dp, dp]),
    'sca_kd_build_host': (C.c_int, [C.c_int, dp, ip, dp]),
}

_LIB = None


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64.so (same SONAME as /opt/rocm's): whichever of the two a
    process loads first is the one everybody gets.  With torch first that is torch's, and libsca_hip.so runs on it (bench.py, the
    multi-GPU steppers); with libsca_hip.so first it would be /opt/rocm's, and a later `import torch` finds no GPU
    (torch.cuda.is_available() == False, measured).  So when a torch installation is present but not imported yet, its runtime is loaded
    here, before the library: either import order then works.  SCA_OWN_HIP_RUNTIME=1 skips this (the system's runtime, no torch later)."""
    import importlib.util
    import sys
    if os.environ.get('SCA_OWN_HIP_RUNTIME') or 'torch' in sys.modules:
        return None
    try:
        spec = importlib.util.find_spec('torch')
    except (ImportError, ValueError):
        return None
    if spec is None or not spec.origin:
        return None
    cand = os.path.join(os.path.dirname(spec.origin), 'lib', 'libamdhip64.so')
    if not os.path.exists(cand):
        return None
    try:
        return C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except OSError:
        return None


def lib():
    """Loads sca_amd/lib/libsca_hip.so.  Raises if it has not been built (python -m sca_amd.build)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(_build.LIB):
            raise RuntimeError(f'{_build.LIB} is missing: build it with `python -m sca_amd.build` '
                               '(there is no CPU fallback)')
        _share_torch_hip_runtime()
        L = C.CDLL(_build.LIB)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def as_d(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if shape is None else a.reshape(shape)

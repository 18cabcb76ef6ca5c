"""ctypes mirror of include/tde_abi.h (field for field) plus helpers to fill the structs from numpy arrays
(host pointers, for the CPU oracle used by the tests) or torch tensors (device pointers, for libtde_hip.so).

PyTorch is plumbing here: it owns device memory and the HIP stream; nothing in the C-ABI mentions torch.
"""
import ctypes as C

import numpy as np

TDE_ABI_VERSION = 14
TDE_MAX_AGENTS = 128

F_NPC = 1 << 0
F_REPLAY = 1 << 1
F_OFFROAD = 1 << 2
F_REWARD = 1 << 3
F_AUTORESET = 1 << 4
F_EGO_ONLY_ATTRS = 1 << 5
F_TRAFFIC_LIGHTS = 1 << 6
F_NPC_FIRST_STEP = 1 << 7
F_ALL = F_NPC | F_REPLAY | F_OFFROAD | F_REWARD | F_AUTORESET | F_NPC_FIRST_STEP    # (TDE_F_ALL: the reference's NPC timing)

CELL_EMPTY, CELL_MIXED, CELL_FULL = 0, 1, 2

_p = C.c_void_p


class TdeConfig(C.Structure):
    _fields_ = [
        ("waypoint_bonus", C.c_double),
        ("heading_penalty", C.c_double),
        ("distance_bonus", C.c_double),
        ("distance_cutoff", C.c_double),
        ("reach_radius", C.c_double),
        ("seed", C.c_uint64),
        ("dt", C.c_float),
        ("offroad_threshold", C.c_float),
        ("npc_k_steer", C.c_float),
        ("npc_k_speed", C.c_float),
        ("npc_gap_s0", C.c_float),
        ("npc_cone_k", C.c_float),
        ("npc_lane_half", C.c_float),
        ("npc_reach", C.c_float),
        ("npc_max_accel", C.c_float),
        ("npc_max_steer", C.c_float),
        ("max_steps", C.c_int32),
        ("terminated_at_infraction", C.c_int32),
        ("flags", C.c_uint32),
        ("npc_cone_range", C.c_float),
        ("env_base", C.c_uint32),
        ("offroad_threshold_squared", C.c_int32),
    ]


class TdeMap(C.Structure):
    _fields_ = [
        ("ox", C.c_float), ("oy", C.c_float), ("cell", C.c_float), ("inv_cell", C.c_float),
        ("nx", C.c_int32), ("ny", C.c_int32), ("cell_base", C.c_int32), ("tri_base", C.c_int32),
        ("n_tri", C.c_int32), ("stop_base", C.c_int32), ("n_stop", C.c_int32), ("phase_base", C.c_int32),
        ("n_phase", C.c_int32), ("cycle_steps", C.c_int32), ("row_shift", C.c_int32), ("cls2_base", C.c_int32),
        ("rec_base", C.c_int32), ("coarse_base", C.c_int32), ("near_base", C.c_int32), ("_pad0", C.c_int32),
    ]


class TdeGrid(C.Structure):
    """tde_grid: what tde_grid_build returns for one map (host arrays owned by the library)"""
    _fields_ = [
        ("ox", C.c_float), ("oy", C.c_float), ("cell", C.c_float), ("nx", C.c_int32), ("ny", C.c_int32),
        ("n_lists", C.c_int64), ("n_records", C.c_int64),
        ("cell_class", C.POINTER(C.c_uint8)), ("cell_count", C.POINTER(C.c_uint8)),
        ("cell_first", C.POINTER(C.c_uint32)), ("cell_sub", C.POINTER(C.c_uint32)), ("rec_tri", C.POINTER(C.c_int32)),
        ("tile_near", C.POINTER(C.c_uint32)), ("rec_len", C.POINTER(C.c_int32)), ("n_near_lists", C.c_int64),
    ]


MAP_DTYPE = np.dtype([("ox", "f4"), ("oy", "f4"), ("cell", "f4"), ("inv_cell", "f4"), ("nx", "i4"), ("ny", "i4"),
                      ("cell_base", "i4"), ("tri_base", "i4"), ("n_tri", "i4"), ("stop_base", "i4"), ("n_stop", "i4"),
                      ("phase_base", "i4"), ("n_phase", "i4"), ("cycle_steps", "i4"), ("row_shift", "i4"), ("cls2_base", "i4"),
                      ("rec_base", "i4"), ("coarse_base", "i4"), ("near_base", "i4"), ("_pad0", "i4")])
STOPLINE_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("c", "f4"), ("s", "f4"), ("hl", "f4"), ("hw", "f4"),
                           ("light", "i4"), ("_pad0", "i4")])
PHASE_DTYPE = np.dtype([("end_step", "i4"), ("red_mask", "u4")])
assert MAP_DTYPE.itemsize == C.sizeof(TdeMap) == 80 and STOPLINE_DTYPE.itemsize == 32 and PHASE_DTYPE.itemsize == 8

SPAWN_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("psi", "f4"), ("v", "f4"), ("len", "f4"), ("wid", "f4"),
                        ("lr", "f4"), ("vdes", "f4"), ("route", "i4"), ("route_wp", "i4"), ("route_n", "i4"),
                        ("replay", "i4"), ("replay_len", "i4"), ("present", "i4"), ("tgx0", "f4"), ("tgy0", "f4")])
SCN_DTYPE = np.dtype([("map", "i4"), ("wp_n", "i4"), ("start_heading", "f4"), ("_pad0", "i4")])
assert SPAWN_DTYPE.itemsize == 64 and SCN_DTYPE.itemsize == 16

WORLD_PTRS = ["maps", "tri", "cell_word", "cell_tri", "cell_cls2", "cell_sub", "cell_coarse", "tile_near", "scn", "wp_xy", "spawn", "route_xy", "replay_states",
              "stoplines", "phases", "start_psi", "first_gap"]
WORLD_INTS = ["n_maps", "n_scn", "NW", "A", "n_routes", "RW", "n_replay", "RT", "hints", "NH"]
WORLD_LARGE_GRID = 1 << 0


class TdeWorld(C.Structure):
    _fields_ = [(n, _p) for n in WORLD_PTRS] + [(n, C.c_int32) for n in WORLD_INTS]


STATE_AGENT_F32 = ["x", "y", "psi", "v", "len", "wid", "lr", "vdes"]
STATE_AGENT_I32 = ["route_wp"]
STATE_AGENT_U8 = ["present", "collided", "offroad"]
STATE_ENV_I32 = ["scn", "steps", "target_idx", "reached", "episode"]
STATE_PTRS = (STATE_AGENT_F32 + STATE_AGENT_I32 + STATE_AGENT_U8 + STATE_ENV_I32 +
              ["action", "reward", "terminated", "truncated", "tl_violation", "info", "info_reached", "done_bits", "obs",
               "ep_return", "ep_final", "ep_final_len", "slot_cache", "env_cache", "act_cache", "magnitudes", "slot_route"])


class TdeState(C.Structure):
    # (slot_route is the struct's last member, behind the sizes)
    _fields_ = [(n, _p) for n in STATE_PTRS if n != "slot_route"] + [("B", C.c_int32), ("A", C.c_int32), ("slot_route", _p)]


class TdeRollout(C.Structure):
    _fields_ = [("actions", _p), ("reward", _p), ("done", _p), ("K", C.c_int32), ("ldb", C.c_int32)]


class TdeRender(C.Structure):
    _fields_ = [("out", _p), ("H", C.c_int32), ("W", C.c_int32), ("fov", C.c_float), ("n_stack", C.c_int32),
                ("layers", _p), ("phase", C.c_int32), ("flags", C.c_int32), ("fresh", _p), ("only", _p)]


class TdeSceneView(C.Structure):
    """tde_scene_view (tde_hip.h): camera pose of one tde_render_scene view"""
    _fields_ = [("env", C.c_int32), ("x", C.c_float), ("y", C.c_float), ("psi", C.c_float)]


class TdeNearField(C.Structure):
    """tde_near_field (tde_abi.h): the candidate table of tde_near_field_spawn"""
    _fields_ = [("cand", _p), ("nbr", _p), ("nbr_n", _p), ("fixed", _p), ("n_cand", _p), ("S", C.c_int32), ("A", C.c_int32),
                ("NC", C.c_int32), ("K", C.c_int32), ("radius", C.c_float), ("clear_ego", C.c_float), ("count", C.c_int32),
                ("density", C.c_int32)]


NF_MAX_CAND, NF_MAX_NBR, NF_TAG = 1024, 32, 0x4E46
# tde_nf_cand: x, y, psi, c, s, len, wid, lr, vdes, then the route words (route id + 1 or 0, first waypoint, length: zero without routes)
NF_CAND_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("psi", "f4"), ("c", "f4"), ("s", "f4"), ("len", "f4"), ("wid", "f4"),
                          ("lr", "f4"), ("vdes", "f4"), ("route", "u4"), ("route_wp", "u4"), ("route_n", "u4")])
CACHE_ID_BITS = 20          # TDE_CACHE_ID_BITS: route ids below 2^20 - 1, lengths below 4096 (tde_slot_cache.route, tde_state.slot_route)
assert NF_CAND_DTYPE.itemsize == 48

class TdeVectorObs(C.Structure):
    """struct tde_vector_obs (tde_abi.h): the parameters of tde_vector_obs"""
    _fields_ = [("ray_dir", _p), ("k_nbr", C.c_int32), ("n_rays", C.c_int32), ("nbr_radius", C.c_float), ("ray_range", C.c_float),
                ("ray_step", C.c_float), ("_pad0", C.c_int32)]


VO_MAX_NBR, VO_MAX_RAYS, VO_MAX_SAMPLES = 16, 64, 1024
VO_EGO, VO_NBR, VO_RAY = 10, 9, 3

class TdePlanner(C.Structure):
    """tde_planner (tde_abi.h): the parameters of tde_plan_action, the lattice tables inline"""
    _fields_ = [("accel", C.c_float * 64), ("steer", C.c_float * 64), ("n_a", C.c_int32), ("n_s", C.c_int32), ("horizon", C.c_int32),
                ("v_target", C.c_float), ("margin", C.c_float), ("w_progress", C.c_float), ("w_speed", C.c_float), ("w_steer", C.c_float)]


PLAN_MAX_CAND, PLAN_MAX_H = 64, 32
PLAN_FAIL_UNIT, PLAN_RUN_MAX, PLAN_RUN_BIAS = 2048.0, 1024.0, 512.0
PLAN_DIAG_DTYPE = np.dtype([("winner", "i4"), ("fail_step", "i4"), ("cost", "f4"), ("n_safe", "i4")])
assert PLAN_DIAG_DTYPE.itemsize == 16


class TdePlanSet(C.Structure):
    """tde_plan_set (tde_abi.h): the sequences tde_score_plans judges; seq is a device address"""
    _fields_ = [("seq", C.c_void_p), ("N", C.c_int32), ("K", C.c_int32), ("knot_len", C.c_int32), ("tail", C.c_int32)]


PLAN_MAX_SET, PLAN_MAX_TAIL = 1024, 64
FORECAST_MAX_T = PLAN_MAX_H + PLAN_MAX_TAIL      # TDE_FORECAST_MAX_T: steps of tde_forecast_agents / tde_forecast_scene / tde_score_plans_forecast
PLAN_SCENE_MAX_LANES = 2**31 - 256                # TDE_PLAN_SCENE_MAX_LANES (tde_hip.h): B * N * A of tde_score_plans_scene
PLAN_BOX_ACCEL, PLAN_BOX_STEER = 1.0, 0.3

class TdeEpisodeRecord(C.Structure):
    """tde_episode_record (tde_abi.h): one finished episode of an evaluation, 48 bytes"""
    _fields_ = [("ret", C.c_double), ("psi_sum", C.c_double), ("speed_sum", C.c_double), ("length", C.c_int32), ("reached", C.c_int32),
                ("scn", C.c_int32), ("bits", C.c_uint8), ("_pad0", C.c_uint8 * 3), ("_pad1", C.c_int32 * 2)]


EPISODE_RECORD_DTYPE = np.dtype([("ret", "f8"), ("psi_sum", "f8"), ("speed_sum", "f8"), ("length", "i4"), ("reached", "i4"), ("scn", "i4"),
                                 ("bits", "u1"), ("_pad0", "u1", (3,)), ("_pad1", "i4", (2,))])
assert EPISODE_RECORD_DTYPE.itemsize == C.sizeof(TdeEpisodeRecord) == 48


class TdeEval(C.Structure):
    """tde_eval (tde_abi.h): the schedule and the results of tde_eval_advance; device addresses"""
    _fields_ = [("plan", _p), ("round", _p), ("active", _p), ("acc", _p), ("results", _p), ("R", C.c_int32), ("_pad0", C.c_int32)]


class TdeReplay(C.Structure):
    """tde_replay (include/tde_replay.h): the ring of a replay buffer; device addresses"""
    _fields_ = [("C", C.c_int32), ("B", C.c_int32), ("n_stack", C.c_int32), ("plane", C.c_int32), ("D", C.c_int32), ("frames", _p),
                ("action", _p), ("reward", _p), ("done", _p), ("age", _p)]


TDE_REPLAY_VERSION = 1
REPLAY_CUT, REPLAY_TAG = 0x80, 0x5250
REPLAY_MAX_STACK, REPLAY_MAX_PLANE = 8, 4096
TDE_ONPOLICY_VERSION = 1         # include/tde_onpolicy.h


class TdeTerminal(C.Structure):
    """tde_terminal (include/tde_terminal.h): the pool of terminal frames beside a replay ring; device addresses"""
    _fields_ = [("M", C.c_int32), ("pool", _p), ("ref", _p)]


TDE_TERMINAL_VERSION = 1         # include/tde_terminal.h
TERMINAL_HAS = 0x40              # in the done byte a terminal sample returns: next_observations is the terminal observation
TDE_NSTEP_VERSION = 1            # include/tde_nstep.h
NSTEP_MAX = 64                   # the longest look-ahead of an n-step sample


class TdePriority(C.Structure):
    """tde_priority (include/tde_priority.h): the integer priorities beside a replay ring; device addresses"""
    _fields_ = [("leaf", _p), ("sums", _p), ("qmax", _p)]


TDE_PRIORITY_VERSION = 1         # include/tde_priority.h
PRIORITY_ONE, PRIORITY_QMAX, PRIORITY_TAG = 1 << 16, 1 << 28, 0x5052      # q of priority 1.0, the largest q, the draws' Philox tag
TDE_SEQUENCE_VERSION = 1         # include/tde_sequence.h
SEQUENCE_MAX = 256               # the longest window of a sequence sample


class TdeSnapshotFrames(C.Structure):
    """tde_snapshot_frames (include/tde_snapshot.h): the frame-stack ring of the rows tde_state_copy moves; device addresses"""
    _fields_ = [("src_layers", _p), ("dst_layers", _p), ("src_obs", _p), ("dst_obs", _p), ("n_stack", C.c_int32), ("plane", C.c_int32),
                ("src_phase", C.c_int32), ("dst_phase", C.c_int32)]


class TdeAgentTrack(C.Structure):
    """tde_agent_track (include/tde_agents.h): what tde_agent_obs saw of a pair, 32 bytes; tde_agent_outcomes reads it"""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("psi", C.c_float), ("v", C.c_float), ("route_wp", C.c_int32), ("episode", C.c_int32),
                ("steps", C.c_int32), ("present", C.c_uint32)]


TDE_SNAPSHOT_VERSION = 1         # include/tde_snapshot.h
TDE_DRIVEN_VERSION = 1           # include/tde_driven.h
TDE_AGENTS_VERSION = 1           # include/tde_agents.h
AG_VALID, AG_COLLIDED, AG_OFFROAD, AG_REACHED, AG_ENDED = 1, 2, 4, 8, 16     # TDE_AG_*: the flag bits of tde_agent_outcomes
SNAPSHOT_OUTPUTS, SNAPSHOT_CHECK, SNAPSHOT_MAX_STACK = 1 << 0, 1 << 1, 8
# the group of every tde_state array under tde_state_copy (the header's list): copied always, copied with SNAPSHOT_OUTPUTS, invalidated
SNAPSHOT_COPIED = (STATE_AGENT_F32 + STATE_AGENT_I32 + STATE_AGENT_U8 + ["slot_route"] + STATE_ENV_I32 + ["action", "obs", "ep_return"])
SNAPSHOT_OUTPUT_ARRAYS = ["reward", "terminated", "truncated", "tl_violation", "done_bits", "info", "info_reached", "ep_final",
                          "ep_final_len", "magnitudes"]
SNAPSHOT_INVALIDATED = ["slot_cache", "env_cache", "act_cache"]

LAYER_BLANK = 5
LAYER_STOP_RED, LAYER_STOP_GO = 6, 7
RENDER_LEFT_HANDED, RENDER_PLAIN_EGO = 1 << 0, 1 << 1
# palette of the layer codes 0..7 (tde_abi.h TDE_RGB_*): background, road, waypoint, NPC, ego, blank, stop red, stop go
PALETTE = ((255, 255, 255), (128, 128, 128), (44, 160, 44), (31, 119, 180), (214, 39, 40), (0, 0, 0), (255, 0, 0),
           (0, 255, 0))


def ptr_of(a):
    """Raw address of a contiguous numpy array or torch tensor (None -> NULL)."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"], "arrays handed to the C-ABI must be contiguous"
        return a.ctypes.data
    # torch tensor
    assert a.is_contiguous(), "tensors handed to the C-ABI must be contiguous"
    return a.data_ptr()


def default_config(**over):
    """tde_config with the reference's defaults (EnvConfig, gym_env.py:34-54) and the NPC controller's."""
    cfg = TdeConfig()
    cfg.waypoint_bonus = 100.0
    cfg.heading_penalty = 25.0
    cfg.distance_bonus = 1.0
    cfg.distance_cutoff = 0.5
    cfg.reach_radius = 3.0
    cfg.seed = 0
    cfg.dt = 0.1
    cfg.offroad_threshold = 0.5
    cfg.npc_k_steer = 1.2
    cfg.npc_k_speed = 3.0
    cfg.npc_gap_s0 = 3.0
    cfg.npc_cone_k = 0.5
    cfg.npc_cone_range = 25.0
    cfg.npc_lane_half = 1.75
    cfg.npc_reach = 3.0
    cfg.npc_max_accel = 3.0
    cfg.npc_max_steer = 0.3
    cfg.max_steps = 200
    cfg.terminated_at_infraction = 1
    cfg.flags = F_ALL
    cfg.env_base = 0
    cfg.offroad_threshold_squared = 0
    for k, v in over.items():
        if not hasattr(cfg, k):
            raise AttributeError(f"tde_config has no field {k!r}")
        setattr(cfg, k, v)
    return cfg


WORLD_DTYPES = {
    "maps": MAP_DTYPE, "tri": np.float32, "cell_word": np.uint32, "cell_tri": np.float32, "cell_cls2": np.uint32, "cell_sub": np.uint32, "cell_coarse": np.uint8, "tile_near": np.uint32, "scn": SCN_DTYPE,
    "wp_xy": np.float64, "spawn": SPAWN_DTYPE, "route_xy": np.float32, "replay_states": np.float32,
    "stoplines": STOPLINE_DTYPE, "phases": PHASE_DTYPE, "start_psi": np.float32,
    "first_gap": np.uint32,        # tde_first_gap [S][A] as pairs of words (gap bits, key): scratch the kernels fill, zeros at upload
}

STATE_DTYPES = {**{n: np.float32 for n in STATE_AGENT_F32}, **{n: np.int32 for n in STATE_AGENT_I32},
                **{n: np.uint8 for n in STATE_AGENT_U8}, **{n: np.int32 for n in STATE_ENV_I32},
                "action": np.float32, "reward": np.float32, "terminated": np.uint8, "truncated": np.uint8,
                "tl_violation": np.uint8,
                "info": np.float64, "info_reached": np.int32, "done_bits": np.uint8, "obs": np.float32,
                "ep_return": np.float64, "ep_final": np.float64, "ep_final_len": np.int32,
                "slot_cache": np.int32, "env_cache": np.int32, "act_cache": np.int32, "magnitudes": np.float32,
                "slot_route": np.int32}     # (uint32 words held as int32: torch has no arithmetic on uint32; view them as uint32)          # opaque 32-byte records (tde_slot_cache / tde_env_cache)


def state_shapes(B, A):
    sh = {n: (B * A,) for n in STATE_AGENT_F32 + STATE_AGENT_I32 + STATE_AGENT_U8}
    sh.update({n: (B,) for n in STATE_ENV_I32})
    sh.update({"action": (B, 2), "reward": (B,), "terminated": (B,), "truncated": (B,), "tl_violation": (B,),
               "info": (B, 4),
               "info_reached": (B,), "done_bits": (B,), "obs": (B, 8), "ep_return": (B,), "ep_final": (B,),
               "ep_final_len": (B,), "slot_cache": (B * A, 8), "env_cache": (B, 8), "act_cache": (B * (A + 1), 2),
               "magnitudes": (B, 4), "slot_route": (B * A,)})
    return sh


def fill_world_struct(arrays, ints):
    w = TdeWorld()
    for n in WORLD_PTRS:
        setattr(w, n, ptr_of(arrays[n]))
    for n in WORLD_INTS:
        setattr(w, n, int(ints[n]))
    return w


def fill_state_struct(arrays, B, A):
    s = TdeState()
    for n in STATE_PTRS:
        setattr(s, n, ptr_of(arrays.get(n)))
    s.B, s.A = int(B), int(A)
    return s

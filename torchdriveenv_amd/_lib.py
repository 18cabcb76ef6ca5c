"""Loader of libtde_hip.so (the C-ABI of include/tde_hip.h).  Fails loudly: there is no CPU or eager fallback."""
import ctypes as C
import os

from . import _abi

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TDE_HIP_LIB") or os.path.join(_PKG, "libtde_hip.so")   # override: A/B builds only

# every symbol include/tde_hip.h declares
SYMBOLS = ["tde_abi_version", "tde_last_error", "tde_kernel_override", "tde_kinematics_step", "tde_compute_collision",
           "tde_compute_offroad", "tde_kin_collide_step", "tde_waypoint_reward", "tde_env_reset", "tde_env_step",
           "tde_env_rollout", "tde_render_ego", "tde_render_scene", "tde_env_reset_render", "tde_env_step_render", "tde_state_obs", "tde_ego_infractions", "tde_env_post_step", "tde_first_gaps", "tde_near_field_spawn", "tde_vector_obs", "tde_plan_action", "tde_score_plans", "tde_forecast_agents", "tde_score_plans_forecast", "tde_forecast_scene", "tde_score_plans_scene", "tde_env_reset_to", "tde_eval_advance", "tde_grid_build", "tde_grid_free"]
# every symbol include/tde_replay.h declares (an additive header with a version of its own: TDE_REPLAY_VERSION)
REPLAY_SYMBOLS = ["tde_replay_version", "tde_replay_begin", "tde_replay_push", "tde_replay_sample", "tde_replay_pack"]
# every symbol include/tde_onpolicy.h declares (additive over the replay header: TDE_ONPOLICY_VERSION)
ONPOLICY_SYMBOLS = ["tde_onpolicy_version", "tde_gae", "tde_onpolicy_gather"]
# every symbol include/tde_terminal.h declares (additive over the replay header: TDE_TERMINAL_VERSION)
TERMINAL_SYMBOLS = ["tde_terminal_version", "tde_terminal_stash", "tde_terminal_push", "tde_terminal_sample"]
# every symbol include/tde_nstep.h declares (additive over the terminal header: TDE_NSTEP_VERSION)
NSTEP_SYMBOLS = ["tde_nstep_version", "tde_nstep_sample"]
# every symbol include/tde_priority.h declares (additive over the replay header: TDE_PRIORITY_VERSION)
PRIORITY_SYMBOLS = ["tde_priority_version", "tde_priority_words", "tde_priority_reset", "tde_priority_push", "tde_priority_update",
                    "tde_priority_sample"]
# every symbol include/tde_sequence.h declares (additive over the terminal header: TDE_SEQUENCE_VERSION)
SEQUENCE_SYMBOLS = ["tde_sequence_version", "tde_sequence_sample"]
# every symbol include/tde_snapshot.h declares (additive over tde_hip.h: TDE_SNAPSHOT_VERSION)
SNAPSHOT_SYMBOLS = ["tde_snapshot_version", "tde_state_copy"]

_lib = None


class TdeError(RuntimeError):
    pass


def load():
    """dlopen the in-tree library.  `torch` is imported first so that its bundled HIP runtime (libamdhip64.so.7) is
    the one already mapped when the loader resolves our NEEDED entry: one HIP runtime per process, so torch's
    device pointers and streams are valid in our launches."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TdeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950).  There is no fallback path.")
    import torch  # noqa: F401  (side effect: maps torch/lib/libamdhip64.so)

    L = C.CDLL(LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    if missing:
        raise TdeError(f"{LIB_PATH} lacks symbols {missing}: stale build?")
    if L.tde_abi_version() != _abi.TDE_ABI_VERSION:
        raise TdeError(f"ABI mismatch: library {L.tde_abi_version()} vs python {_abi.TDE_ABI_VERSION}")
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    cfgp, wp, sp = C.POINTER(_abi.TdeConfig), C.POINTER(_abi.TdeWorld), C.POINTER(_abi.TdeState)
    L.tde_last_error.restype = C.c_char_p
    L.tde_kinematics_step.argtypes = [i64] + [vp] * 7 + [f32, vp]
    L.tde_compute_collision.argtypes = [i32, i32] + [vp] * 7 + [vp]
    L.tde_compute_offroad.argtypes = [i32, i32] + [vp] * 6 + [wp, vp, f32, vp, vp]
    L.tde_kin_collide_step.argtypes = [i32, i32] + [vp] * 9 + [f32, vp, vp]
    L.tde_waypoint_reward.argtypes = [cfgp, i32] + [vp] * 13 + [i32] + [vp] * 9 + [vp]
    L.tde_env_reset.argtypes = [cfgp, wp, sp, vp, vp]
    L.tde_env_step.argtypes = [cfgp, wp, sp, vp]
    L.tde_env_rollout.argtypes = [cfgp, wp, sp, C.POINTER(_abi.TdeRollout), vp]
    L.tde_render_ego.argtypes = [cfgp, wp, sp, C.POINTER(_abi.TdeRender), vp]
    L.tde_render_scene.argtypes = [cfgp, wp, sp, vp, i32, i32, i32, f32, i32, vp, vp]
    L.tde_env_step_render.argtypes = [cfgp, wp, sp, C.POINTER(_abi.TdeRender), C.POINTER(vp), i32]
    L.tde_env_reset_render.argtypes = [cfgp, wp, sp, vp, C.POINTER(_abi.TdeRender), vp]
    L.tde_state_obs.argtypes = [wp, sp, vp, vp]
    L.tde_ego_infractions.argtypes = [cfgp, wp, sp, vp, vp]
    L.tde_env_post_step.argtypes = [cfgp, wp, sp, vp, vp]
    L.tde_first_gaps.argtypes = [cfgp, wp, vp]
    L.tde_near_field_spawn.argtypes = [cfgp, wp, sp, C.POINTER(_abi.TdeNearField), vp, vp]
    L.tde_vector_obs.argtypes = [cfgp, wp, sp, C.POINTER(_abi.TdeVectorObs), vp, vp, vp]
    L.tde_plan_action.argtypes = [cfgp, wp, sp, C.POINTER(_abi.TdePlanner), vp, vp, vp, vp]
    L.tde_score_plans.argtypes = [cfgp, wp, sp, C.POINTER(_abi.TdePlanner), C.POINTER(_abi.TdePlanSet), vp, vp, vp, vp, vp, vp]
    L.tde_forecast_agents.argtypes = [cfgp, wp, sp, i32, vp, vp, vp]
    L.tde_forecast_scene.argtypes = [cfgp, wp, sp, i32, vp, vp, vp, vp]
    L.tde_score_plans_forecast.argtypes = [cfgp, wp, sp, C.POINTER(_abi.TdePlanner), C.POINTER(_abi.TdePlanSet), vp, vp, vp, vp, vp, vp, i32, vp]
    L.tde_score_plans_scene.argtypes = [cfgp, wp, sp, C.POINTER(_abi.TdePlanner), C.POINTER(_abi.TdePlanSet), vp, vp, vp, vp, vp, vp]
    L.tde_env_reset_to.argtypes = [cfgp, wp, sp, vp, vp, vp]
    L.tde_eval_advance.argtypes = [cfgp, wp, sp, C.POINTER(_abi.TdeEval), vp]
    L.tde_kernel_override.argtypes = [C.c_int, C.c_int]
    L.tde_grid_build.argtypes = [vp, i32, f32, f32, f32, f32, i32, C.POINTER(C.POINTER(_abi.TdeGrid))]
    L.tde_grid_free.argtypes = [C.POINTER(_abi.TdeGrid)]
    L.tde_grid_free.restype = None
    for s in SYMBOLS:
        if s not in ("tde_last_error", "tde_grid_free"):
            getattr(L, s).restype = C.c_int
    missing = [s for s in REPLAY_SYMBOLS if not hasattr(L, s)]
    if missing:
        raise TdeError(f"{LIB_PATH} lacks symbols {missing}: stale build?")
    if L.tde_replay_version() != _abi.TDE_REPLAY_VERSION:
        raise TdeError(f"replay version mismatch: library {L.tde_replay_version()} vs python {_abi.TDE_REPLAY_VERSION}")
    rpp, u64 = C.POINTER(_abi.TdeReplay), C.c_uint64
    L.tde_replay_version.argtypes = []
    L.tde_replay_begin.argtypes = [rpp, i32, vp, i64, vp, vp]
    L.tde_replay_push.argtypes = [rpp, i32, vp, vp, vp, vp, i64, vp]
    L.tde_replay_sample.argtypes = [rpp, i32, i32, i32, vp, u64, u64] + [vp] * 6 + [vp]
    L.tde_replay_pack.argtypes = [rpp, vp, i64, vp, i64, vp]
    for s in REPLAY_SYMBOLS:
        getattr(L, s).restype = C.c_int
    missing = [s for s in ONPOLICY_SYMBOLS if not hasattr(L, s)]
    if missing:
        raise TdeError(f"{LIB_PATH} lacks symbols {missing}: stale build?")
    if L.tde_onpolicy_version() != _abi.TDE_ONPOLICY_VERSION:
        raise TdeError(f"on-policy version mismatch: library {L.tde_onpolicy_version()} vs python {_abi.TDE_ONPOLICY_VERSION}")
    L.tde_onpolicy_version.argtypes = []
    L.tde_gae.argtypes = [rpp, i32, i32, i32, vp, vp, f32, f32, vp, vp, vp]
    L.tde_onpolicy_gather.argtypes = [rpp, i32, i32, i32, i32] + [vp] * 5 + [vp] * 6 + [vp]
    for s in ONPOLICY_SYMBOLS:
        getattr(L, s).restype = C.c_int
    missing = [s for s in TERMINAL_SYMBOLS if not hasattr(L, s)]
    if missing:
        raise TdeError(f"{LIB_PATH} lacks symbols {missing}: stale build?")
    if L.tde_terminal_version() != _abi.TDE_TERMINAL_VERSION:
        raise TdeError(f"terminal version mismatch: library {L.tde_terminal_version()} vs python {_abi.TDE_TERMINAL_VERSION}")
    tmp = C.POINTER(_abi.TdeTerminal)
    L.tde_terminal_version.argtypes = []
    L.tde_terminal_stash.argtypes = [i32, i32, vp, vp, i64, vp, vp]
    L.tde_terminal_push.argtypes = [rpp, tmp, i32, vp, vp, i64, vp]
    L.tde_terminal_sample.argtypes = [rpp, tmp, i32, i32, i32, vp, u64, u64] + [vp] * 6 + [vp]
    for s in TERMINAL_SYMBOLS:
        getattr(L, s).restype = C.c_int
    missing = [s for s in NSTEP_SYMBOLS if not hasattr(L, s)]
    if missing:
        raise TdeError(f"{LIB_PATH} lacks symbols {missing}: stale build?")
    if L.tde_nstep_version() != _abi.TDE_NSTEP_VERSION:
        raise TdeError(f"n-step version mismatch: library {L.tde_nstep_version()} vs python {_abi.TDE_NSTEP_VERSION}")
    L.tde_nstep_version.argtypes = []
    L.tde_nstep_sample.argtypes = [rpp, tmp, i32, i32, i32, vp, u64, u64, i32, f32] + [vp] * 8 + [vp]
    for s in NSTEP_SYMBOLS:
        getattr(L, s).restype = C.c_int
    missing = [s for s in PRIORITY_SYMBOLS if not hasattr(L, s)]
    if missing:
        raise TdeError(f"{LIB_PATH} lacks symbols {missing}: stale build?")
    if L.tde_priority_version() != _abi.TDE_PRIORITY_VERSION:
        raise TdeError(f"priority version mismatch: library {L.tde_priority_version()} vs python {_abi.TDE_PRIORITY_VERSION}")
    prp = C.POINTER(_abi.TdePriority)
    L.tde_priority_version.argtypes = []
    L.tde_priority_words.argtypes = [i32, i32]
    L.tde_priority_reset.argtypes = [prp, rpp, vp]
    L.tde_priority_push.argtypes = [prp, rpp, i32, i32, i32, vp]
    L.tde_priority_update.argtypes = [prp, rpp, i32, i32, i32, vp, vp, vp]
    L.tde_priority_sample.argtypes = [prp, rpp, i32, i32, i32, u64, u64, vp, vp, vp]
    for s in PRIORITY_SYMBOLS:
        getattr(L, s).restype = C.c_int64 if s == "tde_priority_words" else C.c_int
    missing = [s for s in SEQUENCE_SYMBOLS if not hasattr(L, s)]
    if missing:
        raise TdeError(f"{LIB_PATH} lacks symbols {missing}: stale build?")
    if L.tde_sequence_version() != _abi.TDE_SEQUENCE_VERSION:
        raise TdeError(f"sequence version mismatch: library {L.tde_sequence_version()} vs python {_abi.TDE_SEQUENCE_VERSION}")
    L.tde_sequence_version.argtypes = []
    L.tde_sequence_sample.argtypes = [rpp, tmp, i32, i32, i32, vp, u64, u64, i32] + [vp] * 6 + [vp]
    for s in SEQUENCE_SYMBOLS:
        getattr(L, s).restype = C.c_int
    missing = [s for s in SNAPSHOT_SYMBOLS if not hasattr(L, s)]
    if missing:
        raise TdeError(f"{LIB_PATH} lacks symbols {missing}: stale build?")
    if L.tde_snapshot_version() != _abi.TDE_SNAPSHOT_VERSION:
        raise TdeError(f"snapshot version mismatch: library {L.tde_snapshot_version()} vs python {_abi.TDE_SNAPSHOT_VERSION}")
    L.tde_snapshot_version.argtypes = []
    L.tde_state_copy.argtypes = [sp, sp, i32, vp, vp, C.POINTER(_abi.TdeSnapshotFrames), C.c_uint32, vp]
    for s in SNAPSHOT_SYMBOLS:
        getattr(L, s).restype = C.c_int
    _lib = L
    return L


def check(rc, what=""):
    if rc != 0:
        msg = load().tde_last_error().decode() or f"error {rc}"
        raise TdeError(f"{what}: {msg}" if what else msg)


TEAMS = {None: 0, "auto": 0, "solo": 1, "duo": 2, "trio": 3}


def kernel_override(rollout=None, step=None):
    """force a kernel form of tde_env_rollout ("solo" | "duo" | "trio") / tde_env_step ("solo" | "trio"); None = the
    library's own choice (tde_hip.h: tde_kernel_override).  Process-wide; tests and A/B scripts only."""
    check(load().tde_kernel_override(TEAMS[rollout], TEAMS[step]), "tde_kernel_override")


def current_stream(device):
    import torch

    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)

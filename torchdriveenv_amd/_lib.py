"""Loader of libtde_hip.so (the C-ABI of include/tde_hip.h).  Fails loudly: there is no CPU or eager fallback."""
import collections
import ctypes as C
import os

from . import _abi

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TDE_HIP_LIB") or os.path.join(_PKG, "libtde_hip.so")   # override: A/B builds only

vp, i32, i64, u32, u64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_float
cfgp, wp, sp = C.POINTER(_abi.TdeConfig), C.POINTER(_abi.TdeWorld), C.POINTER(_abi.TdeState)
plp, psp = C.POINTER(_abi.TdePlanner), C.POINTER(_abi.TdePlanSet)
rpp, tmp, prp = C.POINTER(_abi.TdeReplay), C.POINTER(_abi.TdeTerminal), C.POINTER(_abi.TdePriority)

# One record per header of the C ABI: the core first, then the additive headers in the order they were added.  load(), build.DEPS and
# tests/test_abi_families_cpu.py are driven by this table (adding a family: INTEGRATION.md, "Adding a family").
#   name     as the error messages say it
#   header   under include/
#   unit     under csrc/ (None: the core's units are whatever else build.UNITS lists)
#   version  the header's #define and the constant of _abi, one name for both; the first symbol returns it
#   symbols  (name, argtypes) or (name, argtypes, restype): the version symbol, then the entry points in header order; restype is c_int
#            unless stated
Family = collections.namedtuple("Family", "name header unit version symbols")
FAMILIES = [
    Family("core", "tde_hip.h", None, "TDE_ABI_VERSION", [
        ("tde_abi_version", []),
        ("tde_last_error", [], C.c_char_p),
        ("tde_kernel_override", [C.c_int, C.c_int]),
        ("tde_kinematics_step", [i64] + [vp] * 7 + [f32, vp]),
        ("tde_compute_collision", [i32, i32] + [vp] * 7 + [vp]),
        ("tde_compute_offroad", [i32, i32] + [vp] * 6 + [wp, vp, f32, vp, vp]),
        ("tde_kin_collide_step", [i32, i32] + [vp] * 9 + [f32, vp, vp]),
        ("tde_waypoint_reward", [cfgp, i32] + [vp] * 13 + [i32] + [vp] * 9 + [vp]),
        ("tde_env_reset", [cfgp, wp, sp, vp, vp]),
        ("tde_env_step", [cfgp, wp, sp, vp]),
        ("tde_env_rollout", [cfgp, wp, sp, C.POINTER(_abi.TdeRollout), vp]),
        ("tde_render_ego", [cfgp, wp, sp, C.POINTER(_abi.TdeRender), vp]),
        ("tde_render_scene", [cfgp, wp, sp, vp, i32, i32, i32, f32, i32, vp, vp]),
        ("tde_env_reset_render", [cfgp, wp, sp, vp, C.POINTER(_abi.TdeRender), vp]),
        ("tde_env_step_render", [cfgp, wp, sp, C.POINTER(_abi.TdeRender), C.POINTER(vp), i32]),
        ("tde_state_obs", [wp, sp, vp, vp]),
        ("tde_ego_infractions", [cfgp, wp, sp, vp, vp]),
        ("tde_env_post_step", [cfgp, wp, sp, vp, vp]),
        ("tde_first_gaps", [cfgp, wp, vp]),
        ("tde_near_field_spawn", [cfgp, wp, sp, C.POINTER(_abi.TdeNearField), vp, vp]),
        ("tde_vector_obs", [cfgp, wp, sp, C.POINTER(_abi.TdeVectorObs), vp, vp, vp]),
        ("tde_plan_action", [cfgp, wp, sp, plp, vp, vp, vp, vp]),
        ("tde_score_plans", [cfgp, wp, sp, plp, psp] + [vp] * 6),
        ("tde_forecast_agents", [cfgp, wp, sp, i32, vp, vp, vp]),
        ("tde_score_plans_forecast", [cfgp, wp, sp, plp, psp] + [vp] * 6 + [i32, vp]),
        ("tde_forecast_scene", [cfgp, wp, sp, i32, vp, vp, vp, vp]),
        ("tde_score_plans_scene", [cfgp, wp, sp, plp, psp] + [vp] * 6),
        ("tde_env_reset_to", [cfgp, wp, sp, vp, vp, vp]),
        ("tde_eval_advance", [cfgp, wp, sp, C.POINTER(_abi.TdeEval), vp]),
        ("tde_grid_build", [vp, i32, f32, f32, f32, f32, i32, C.POINTER(C.POINTER(_abi.TdeGrid))]),
        ("tde_grid_free", [C.POINTER(_abi.TdeGrid)], None)]),
    Family("replay", "tde_replay.h", "tde_replay.hip", "TDE_REPLAY_VERSION", [
        ("tde_replay_version", []),
        ("tde_replay_begin", [rpp, i32, vp, i64, vp, vp]),
        ("tde_replay_push", [rpp, i32, vp, vp, vp, vp, i64, vp]),
        ("tde_replay_sample", [rpp, i32, i32, i32, vp, u64, u64] + [vp] * 6 + [vp]),
        ("tde_replay_pack", [rpp, vp, i64, vp, i64, vp])]),
    Family("on-policy", "tde_onpolicy.h", "tde_onpolicy.hip", "TDE_ONPOLICY_VERSION", [
        ("tde_onpolicy_version", []),
        ("tde_gae", [rpp, i32, i32, i32, vp, vp, f32, f32, vp, vp, vp]),
        ("tde_onpolicy_gather", [rpp, i32, i32, i32, i32] + [vp] * 5 + [vp] * 6 + [vp])]),
    Family("terminal", "tde_terminal.h", "tde_terminal.hip", "TDE_TERMINAL_VERSION", [
        ("tde_terminal_version", []),
        ("tde_terminal_stash", [i32, i32, vp, vp, i64, vp, vp]),
        ("tde_terminal_push", [rpp, tmp, i32, vp, vp, i64, vp]),
        ("tde_terminal_sample", [rpp, tmp, i32, i32, i32, vp, u64, u64] + [vp] * 6 + [vp])]),
    Family("n-step", "tde_nstep.h", "tde_nstep.hip", "TDE_NSTEP_VERSION", [
        ("tde_nstep_version", []),
        ("tde_nstep_sample", [rpp, tmp, i32, i32, i32, vp, u64, u64, i32, f32] + [vp] * 8 + [vp])]),
    Family("priority", "tde_priority.h", "tde_priority.hip", "TDE_PRIORITY_VERSION", [
        ("tde_priority_version", []),
        ("tde_priority_words", [i32, i32], i64),
        ("tde_priority_reset", [prp, rpp, vp]),
        ("tde_priority_push", [prp, rpp, i32, i32, i32, vp]),
        ("tde_priority_update", [prp, rpp, i32, i32, i32, vp, vp, vp]),
        ("tde_priority_sample", [prp, rpp, i32, i32, i32, u64, u64, vp, vp, vp])]),
    Family("sequence", "tde_sequence.h", "tde_sequence.hip", "TDE_SEQUENCE_VERSION", [
        ("tde_sequence_version", []),
        ("tde_sequence_sample", [rpp, tmp, i32, i32, i32, vp, u64, u64, i32] + [vp] * 6 + [vp])]),
    Family("snapshot", "tde_snapshot.h", "tde_snapshot.hip", "TDE_SNAPSHOT_VERSION", [
        ("tde_snapshot_version", []),
        ("tde_state_copy", [sp, sp, i32, vp, vp, C.POINTER(_abi.TdeSnapshotFrames), u32, vp])]),
]

# Families added since tests/test_abi_families_cpu.py pinned FAMILIES to its eight names: the same records under the same rules, walked
# by load() and build.DEPS behind FAMILIES, each held to the rules by its own test file ("Adding a family").
ADDED_FAMILIES = [
    Family("driven", "tde_driven.h", "tde_step_driven.hip", "TDE_DRIVEN_VERSION", [
        ("tde_driven_version", []),
        ("tde_env_step_driven", [cfgp, wp, sp, vp, vp, vp])]),
]

# Families added since tests/test_driven_cpu.py pinned ADDED_FAMILIES to its one name: the list the NEXT family appends to.  No test
# pins its length or its names - each family's own test file asserts that its record is in it and that no symbol occurs twice over
# the three lists - and load(), symbols() and build.DEPS walk it right behind the other two, under the same rules.
LATER_FAMILIES = [
    Family("agents", "tde_agents.h", "tde_agents.hip", "TDE_AGENTS_VERSION", [
        ("tde_agents_version", []),
        ("tde_agent_obs", [cfgp, wp, sp, C.POINTER(_abi.TdeVectorObs), vp, i32, vp, vp, vp]),
        ("tde_agent_outcomes", [cfgp, wp, sp, vp, i32, vp, vp, vp, vp])]),
]


def families():
    """every family, in the order load() checks them"""
    return FAMILIES + ADDED_FAMILIES + LATER_FAMILIES


def symbols(name):
    """the symbols of family `name`, as FAMILIES / ADDED_FAMILIES / LATER_FAMILIES list them"""
    return [s[0] for f in families() if f.name == name for s in f.symbols]


SYMBOLS = symbols("core")        # every symbol include/tde_hip.h declares

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
    for fam in families():
        missing = [s[0] for s in fam.symbols if not hasattr(L, s[0])]
        if missing:
            raise TdeError(f"{LIB_PATH} lacks symbols {missing}: stale build?")
        got, want = getattr(L, fam.symbols[0][0])(), getattr(_abi, fam.version)
        if got != want:
            what = "ABI mismatch" if fam.name == "core" else f"{fam.name} version mismatch"
            raise TdeError(f"{what}: library {got} vs python {want}")
        for name, argtypes, *restype in fam.symbols:
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, restype[0] if restype else C.c_int
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

"""ops.CtypesHandle against the C++ extension's EnvHandle, without a GPU and without loading the extension: the pybind11 bindings of
csrc/tde_torch_ext.cpp are read as text.  BatchedWaypointEnv and ops.FrameStack launch through either handle with one call per site,
so a method of one that the other lacks, or that takes its arguments in another order, is a launch that works under one binding only."""
import inspect
import os
import re

from torchdriveenv_amd import ops
from torchdriveenv_amd.config import Planner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "torchdriveenv_amd", "csrc", "tde_torch_ext.cpp")

# EnvHandle methods with no CtypesHandle counterpart.  step_render: it takes raw hipStream_t values for its sub-batches, the env never
# calls it, and its ctypes form is ops.env_step_render, which takes torch.cuda.Stream objects
ONLY_IN_EXTENSION = {"step_render"}


def _env_handle_defs():
    """name -> [(argument, has a default)] of every .def("name", &EnvHandle::name, py::arg(...), ...) of the EnvHandle class; where a
    .def names no argument, the parameters of the method's C++ declaration"""
    text = open(SRC).read()
    start = text.index('py::class_<EnvHandle>(m, "EnvHandle")')
    block = text[start:text.index(";", start)]
    defs = {}
    for piece in block.split(".def(")[1:]:
        m = re.match(r'"(\w+)",\s*&EnvHandle::(\w+)', piece)
        if m is None:
            continue                                                 # (the constructor: py::init)
        assert m.group(1) == m.group(2), piece
        args = [(a, bool(eq)) for a, eq in re.findall(r'py::arg\("(\w+)"\)(\s*=)?', piece)]
        if not args:
            decl = re.search(r"\bvoid\s+%s\(([^)]*)\)" % m.group(1), text).group(1)
            args = [(re.search(r"(\w+)\s*$", p).group(1), False) for p in decl.split(",") if p.strip()]
        defs[m.group(1)] = args
    return defs


def _public_methods(cls):
    return {n: f for n, f in vars(cls).items() if inspect.isfunction(f) and not n.startswith("_")}


def test_the_extension_source_is_read_as_expected():
    """the parser sees what a reader of the file sees: a few entries spelled out, the default of score_plans' forecast included"""
    defs = _env_handle_defs()
    assert len(defs) == 18 and ONLY_IN_EXTENSION <= set(defs)
    assert defs["step"] == [("action", False), ("flags", False)]
    assert defs["state_obs"] == [("out", False)]                      # (.def names no argument: from the declaration)
    assert defs["reset_render"][:3] == [("mask", False), ("flags", False), ("out", False)] and defs["reset_render"][-1] == ("rflags", False)
    assert defs["score_plans"][-2:] == [("flags", False), ("forecast", True)] and len(defs["score_plans"]) == 16
    assert [a for a, _ in defs["near_field_spawn"]] == ["nf", "mask", "flags"]


def test_ctypes_handle_has_every_env_handle_method_with_the_same_positional_arguments():
    defs = _env_handle_defs()
    methods = _public_methods(ops.CtypesHandle)
    for name, args in defs.items():
        if name in ONLY_IN_EXTENSION:
            assert name not in methods, name
            continue
        assert name in methods, f"ops.CtypesHandle lacks EnvHandle.{name}"
        params = list(inspect.signature(methods[name]).parameters.values())
        assert params[0].name == "self" and all(p.kind is p.POSITIONAL_OR_KEYWORD for p in params), name
        assert [p.name for p in params[1:]] == [a for a, _ in args], name
        assert [p.default is not p.empty for p in params[1:]] == [d for _, d in args], name


def test_ctypes_handle_has_no_method_of_its_own():
    assert set(_public_methods(ops.CtypesHandle)) == set(_env_handle_defs()) - ONLY_IN_EXTENSION


def test_the_handles_planner_is_planner_struct_and_is_made_once():
    """the tde_planner the handle builds from EnvHandle.plan_action's flattened arguments == ops.planner_struct of the same Planner,
    byte for byte; the plan-set judges' has the scalars and an empty lattice; one struct per argument tuple"""
    pl = Planner(horizon=17, v_target=7.5, margin=0.3, w_progress=1.5, w_speed=0.25, w_steer=0.125)
    scalars = (int(pl.horizon), float(pl.v_target), float(pl.margin), float(pl.w_progress), float(pl.w_speed), float(pl.w_steer))
    tables = (tuple(float(v) for v in pl.accelerations), tuple(float(v) for v in pl.steerings))
    h = ops.CtypesHandle(None, None, None)
    t = h._planner(*scalars, *tables)
    assert bytes(t) == bytes(ops.planner_struct(pl))
    assert h._planner(*scalars, *tables) is t
    s = h._planner(*scalars, (), ())
    assert s is not t and h._planner(*scalars, (), ()) is s
    assert (s.n_a, s.n_s, s.horizon) == (0, 0, 17) and not any(s.accel) and not any(s.steer)
    assert [getattr(s, n) for n in ("v_target", "margin", "w_progress", "w_speed", "w_steer")] == [getattr(t, n) for n in
                                                                                                 ("v_target", "margin", "w_progress", "w_speed", "w_steer")]

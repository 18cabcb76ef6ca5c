"""CPU checks of every family of the C ABI, driven by the one table that states them (torchdriveenv_amd/_lib.py: FAMILIES): each public
header alone and beside the others, as C and as C++; header, table, _abi and the built library against each other and against the one
literal pin below; the loader's stale-build and version refusals, family by family; and the three lists of translation units (the
table's, build.UNITS, and the #include list of the single-unit form csrc/tde_kernels.hip) against each other.  What is a family's own
(struct layouts, constants, refusals of its entry points) is in tests/test_<family>_cpu.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from torchdriveenv_amd import _abi, _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "torchdriveenv_amd", "csrc")
COMPILERS = [("gcc", "c"), ("g++", "cpp")]
each_family = pytest.mark.parametrize("fam", _lib.FAMILIES, ids=[f.name for f in _lib.FAMILIES])
each_compiler = pytest.mark.parametrize("cc,ext", COMPILERS, ids=["c", "cxx"])

# THE pin: family -> (version, {symbol: number of arguments}), symbols in the loader's order.  A change of the ABI edits this table on purpose.
PINS = {
    "core": (14, {"tde_abi_version": 0, "tde_last_error": 0, "tde_kernel_override": 2, "tde_kinematics_step": 10, "tde_compute_collision": 10,
                  "tde_compute_offroad": 13, "tde_kin_collide_step": 14, "tde_waypoint_reward": 26, "tde_env_reset": 5, "tde_env_step": 4,
                  "tde_env_rollout": 5, "tde_render_ego": 5, "tde_render_scene": 11, "tde_env_reset_render": 6, "tde_env_step_render": 6,
                  "tde_state_obs": 4, "tde_ego_infractions": 5, "tde_env_post_step": 5, "tde_first_gaps": 3, "tde_near_field_spawn": 6,
                  "tde_vector_obs": 7, "tde_plan_action": 8, "tde_score_plans": 11, "tde_forecast_agents": 7, "tde_score_plans_forecast": 13,
                  "tde_forecast_scene": 8, "tde_score_plans_scene": 11, "tde_env_reset_to": 6, "tde_eval_advance": 5, "tde_grid_build": 8,
                  "tde_grid_free": 1}),
    "replay": (1, {"tde_replay_version": 0, "tde_replay_begin": 6, "tde_replay_push": 8, "tde_replay_sample": 14, "tde_replay_pack": 6}),
    "on-policy": (1, {"tde_onpolicy_version": 0, "tde_gae": 11, "tde_onpolicy_gather": 17}),
    "terminal": (1, {"tde_terminal_version": 0, "tde_terminal_stash": 7, "tde_terminal_push": 7, "tde_terminal_sample": 15}),
    "n-step": (1, {"tde_nstep_version": 0, "tde_nstep_sample": 19}),
    "priority": (1, {"tde_priority_version": 0, "tde_priority_words": 2, "tde_priority_reset": 3, "tde_priority_push": 6,
                     "tde_priority_update": 8, "tde_priority_sample": 10}),
    "sequence": (1, {"tde_sequence_version": 0, "tde_sequence_sample": 16}),
    "snapshot": (1, {"tde_snapshot_version": 0, "tde_state_copy": 8}),
}
# every symbol returns int but these
RESTYPES = {"tde_last_error": C.c_char_p, "tde_grid_free": None, "tde_priority_words": C.c_int64}
# the project headers each header includes itself
BUILDS_ON = {"core": ["tde_abi.h"], "replay": ["tde_abi.h"], "on-policy": ["tde_replay.h"], "terminal": ["tde_replay.h"],
             "n-step": ["tde_terminal.h"], "priority": ["tde_replay.h"], "sequence": ["tde_terminal.h"], "snapshot": ["tde_hip.h"]}


def c_status(tmp_path, headers, expr, cc="gcc", ext="c", decls=""):
    """compile (-Wall -Werror) and run `<the headers> int main(void){<decls> return (<expr>) != 0;}`: the program's exit status"""
    src, exe = tmp_path / f"prog.{ext}", str(tmp_path / f"prog_{ext}")
    src.write_text("".join(f'#include "{h}"\n' for h in headers) + f"int main(void){{{decls} return ({expr}) != 0;}}\n")
    subprocess.run([cc, "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", exe], check=True)
    return subprocess.run([exe]).returncode


def includes(header):
    return re.findall(r'^#include "(tde_\w+\.h)"', open(os.path.join(INCLUDE, header)).read(), re.M)


def reach(header):
    """the header and every project header it brings, directly or not"""
    got = {header}
    for h in includes(header):
        got |= reach(h)
    return got


def pinned(fams):
    """a C expression that is 0 only if the version macro of every family of `fams` has its pinned value"""
    return " | ".join(f"({f.version} - {PINS[f.name][0]})" for f in fams)


def test_the_pin_names_the_families_of_the_table_in_its_order():
    names = [f.name for f in _lib.FAMILIES]
    assert names == list(PINS) == list(BUILDS_ON) == ["core", "replay", "on-policy", "terminal", "n-step", "priority", "sequence", "snapshot"]
    assert _lib.SYMBOLS == _lib.symbols("core") == list(PINS["core"][1]) and len(_lib.SYMBOLS) == 31
    assert not any(n.endswith("_SYMBOLS") for n in vars(_lib))         # one spelling: _lib.symbols(name)


@each_compiler
@each_family
def test_header_compiles_alone(tmp_path, fam, cc, ext):
    """it brings what it builds on (their version macros are defined), and declares each of its symbols as a function"""
    brought = [f for f in _lib.FAMILIES if f.header in reach(fam.header)]
    syms = _lib.symbols(fam.name)
    functions = " + ".join(f"sizeof(&{s})" for s in syms) + f" != {len(syms)} * sizeof(void (*)(void))"
    assert fam in brought and c_status(tmp_path, [fam.header], f"{pinned(brought)} | ({functions})", cc, ext) == 0


@each_compiler
def test_headers_compile_beside_each_other_in_table_order_and_in_reverse(tmp_path, cc, ext):
    headers = [f.header for f in _lib.FAMILIES]
    for order in (headers, headers[::-1]):
        assert c_status(tmp_path, order, pinned(_lib.FAMILIES), cc, ext) == 0


@each_compiler
@each_family
def test_header_compiles_ahead_of_all_the_others(tmp_path, fam, cc, ext):
    order = [fam.header] + [f.header for f in _lib.FAMILIES if f is not fam]
    assert c_status(tmp_path, order, pinned(_lib.FAMILIES), cc, ext) == 0


@each_family
def test_header_includes_what_it_builds_on(fam):
    assert includes(fam.header) == BUILDS_ON[fam.name]


@each_family
def test_declared_symbols_match_the_table(fam):
    """the table lists the version symbol first and then the entry points in the header's order (the additive headers declare their
    version symbol last)"""
    text = open(os.path.join(INCLUDE, fam.header)).read()
    declared = re.findall(r"TDE_API\s+[\w\s\*]+?\b(tde_\w+)\s*\(", text)
    table = _lib.symbols(fam.name)
    assert table == list(PINS[fam.name][1]) and len(set(table)) == len(table)
    assert table[0].endswith("_version") and [s for s in declared if s.endswith("_version")] == table[:1]
    assert [s for s in declared if s != table[0]] == table[1:]
    assert len(re.findall(r"^TDE_API\s", text, re.M)) == len(table)     # nothing the pattern failed to read


def test_symbol_sets_of_any_two_families_are_disjoint():
    every = [s for f in _lib.FAMILIES for s in _lib.symbols(f.name)]
    assert len(set(every)) == len(every) == sum(len(p[1]) for p in PINS.values())


@each_family
def test_header_abi_library_and_pin_agree(fam):
    version, nargs = PINS[fam.name]
    defines = [int(v) for h in sorted(reach(fam.header))
               for v in re.findall(rf"^#define {fam.version} (\d+)\b", open(os.path.join(INCLUDE, h)).read(), re.M)]
    L = _lib.load()
    assert defines == [version] and getattr(_abi, fam.version) == version == getattr(L, list(nargs)[0])()
    assert all(hasattr(L, s) for s in nargs)
    assert [len(getattr(L, s).argtypes) for s in nargs] == list(nargs.values())
    assert [getattr(L, s).restype for s in nargs] == [RESTYPES.get(s, C.c_int) for s in nargs]


@each_family
def test_unit_and_header_are_what_the_build_depends_on(fam):
    assert all(os.path.exists(d) for d in build.DEPS)
    deps = [os.path.normpath(d) for d in build.DEPS]
    assert os.path.join(INCLUDE, fam.header) in deps and os.path.join(INCLUDE, "tde_abi.h") in deps
    units = [f.unit for f in _lib.FAMILIES if f.unit]
    if fam.unit:
        assert fam.unit in build.UNITS and units.count(fam.unit) == 1 and os.path.join(CSRC, fam.unit) in deps
    else:                                                               # the core: whatever else build.UNITS lists
        assert fam is _lib.FAMILIES[0] and "tde_api.hip" in set(build.UNITS) - set(units)


def _patched(monkeypatch, fam, **change):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "FAMILIES", [f._replace(**change) if f is fam else f for f in _lib.FAMILIES])


@each_family
def test_a_library_without_a_symbol_of_the_family_is_a_stale_build(monkeypatch, fam):
    absent = f"{fam.symbols[0][0][:-len('version')]}not_there"          # tde_replay_not_there
    _patched(monkeypatch, fam, symbols=fam.symbols + [(absent, [])])
    with pytest.raises(_lib.TdeError) as err:
        _lib.load()
    assert str(err.value) == f"{_lib.LIB_PATH} lacks symbols ['{absent}']: stale build?"
    monkeypatch.undo()
    _lib.load()


@each_family
def test_a_library_of_another_version_is_refused_by_its_family(monkeypatch, fam):
    version = PINS[fam.name][0]
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_abi, fam.version, version + 1)
    with pytest.raises(_lib.TdeError) as err:
        _lib.load()
    what = "ABI mismatch" if fam.name == "core" else f"{fam.name} version mismatch"
    assert str(err.value) == f"{what}: library {version} vs python {version + 1}"
    monkeypatch.undo()
    _lib.load()


def test_the_first_family_at_fault_is_the_one_reported(monkeypatch):
    """the loader checks family by family, symbols before version: of two faults the earlier family's is raised"""
    replay, snapshot = _lib.FAMILIES[1], _lib.FAMILIES[-1]
    _patched(monkeypatch, snapshot, symbols=snapshot.symbols + [("tde_snapshot_not_there", [])])
    monkeypatch.setattr(_abi, replay.version, 2)
    with pytest.raises(_lib.TdeError, match=r"^replay version mismatch: library 1 vs python 2$"):
        _lib.load()
    monkeypatch.undo()
    _lib.load()


def test_the_single_unit_form_includes_every_unit_of_the_build():
    text = open(os.path.join(CSRC, "tde_kernels.hip")).read()
    included = re.findall(r'^#include "(tde_\w+\.hip)"', text, re.M)
    assert set(included) == set(build.UNITS) and len(included) == len(build.UNITS) == len(set(build.UNITS))
    assert all(os.path.exists(os.path.join(CSRC, u)) for u in build.UNITS)


def test_the_single_unit_form_passes_a_host_syntax_pass():
    """the units' anonymous namespaces merge in csrc/tde_kernels.hip: two host helpers of one name in two units fail here, in seconds,
    not in the minutes-long build of a variant"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "--offload-host-only", "-I", INCLUDE, "-I", CSRC,
                        "-x", "hip", os.path.join(CSRC, "tde_kernels.hip")], capture_output=True, text=True)
    assert r.returncode == 0 and "error" not in r.stderr, r.stderr

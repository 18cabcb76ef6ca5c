"""The CPU conditions of the config zoo (tests/config_zoo.py), on the oracle alone: what has to hold before the GPU tests of
tests/test_gpu_config_zoo.py mean anything.  Every run is the GPU test's own at 16 slots: the junction world, 64 envs, the entry's
actions and its T.

Liveness: a constant the oracle's run cannot see is a constant a kernel may ignore, so for every field an entry changes, putting that
one field back to its default changes the run - the per-step rewards, the done bits or the state after the last step, by bits.
Events: the runs keep what the kernel matrix demands of its groups (finished episodes, ego collisions or offroad, red-light
violations) and what each entry is there for.  Plumbing: to_tde_config delivers the fields EnvConfig / SimulatorConfig can express."""
import numpy as np
import pytest

from tests import config_zoo as Z
from torchdriveenv_amd import _abi
from torchdriveenv_amd.config import EnvConfig, SimulatorConfig, to_tde_config

A, B = 16, 64
_runs = {}


def _run(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _runs:
        _runs[key] = Z.Run(Z.config(name, A, **kw), Z.world(name, A), B, Z.actions(name, B, A))
    return _runs[key]


def test_the_zoo_is_what_the_gpu_tests_assume():
    assert Z.batch(A, 256) == B and Z.batch(128, 256) == 48 and Z.batch(128, 8) == 16
    for name in Z.NAMES:
        cfg, over = Z.config(name, A), Z.overrides(name)
        stored = {f: getattr(_abi.default_config(**{f: v}), f) for f, v in over.items()}       # (the float fields round to float32)
        assert over and all(getattr(cfg, f) == v for f, v in stored.items()), name
        assert all(v != Z.default_of(f) for f, v in stored.items()), name          # an entry lists only what it changes
        assert cfg.flags == _abi.F_ALL | _abi.F_TRAFFIC_LIGHTS and cfg.max_steps == 20 and Z.steps(name) <= 60
        # assert_state_equal's one tolerance (info[2] within 8e-15) is an ulp of the cosine times the penalty: it holds up to 25
        assert 0.0 <= cfg.heading_penalty <= 25.0, name
        assert Z.world(name, A).threshold == pytest.approx(Z.threshold(name))
    assert Z.threshold("thin_edge") == pytest.approx(0.2) and Z.threshold("thick_edge") == pytest.approx(1.25)
    a = Z.actions("degenerate", B, A)
    zero = a == 0
    assert (zero & np.signbit(a)).any() and (zero & ~np.signbit(a)).any()             # both signed zeros, in both columns
    assert zero[..., 0].any() and zero[..., 1].any()
    # the fields no GPU test moved before: every one of them is moved by some entry
    moved = {f for n in Z.NAMES for f in Z.fields(n)}
    assert moved >= {"dt", "reach_radius", "waypoint_bonus", "heading_penalty", "distance_bonus", "distance_cutoff", "offroad_threshold",
                     "offroad_threshold_squared", "npc_k_steer", "npc_k_speed", "npc_gap_s0", "npc_cone_k", "npc_cone_range",
                     "npc_lane_half", "npc_reach", "npc_max_accel", "npc_max_steer", "seed"}
    # the collapsed values: each alive in some entry
    zeros = {f for n in Z.NAMES for f, v in Z.overrides(n).items() if v == 0}
    assert zeros >= {"npc_max_steer", "npc_k_steer", "npc_gap_s0", "npc_cone_range", "npc_lane_half", "npc_cone_k"}


@pytest.mark.parametrize("name,field", [(n, f) for n in Z.NAMES for f in Z.fields(n)], ids=lambda v: str(v))
def test_every_changed_field_is_live(name, field):
    """the entry's run against the run with `field` alone back at its default: they differ"""
    assert not _run(name).same(_run(name, **{field: Z.default_of(field)})), \
        f"{name}: the oracle's run cannot tell {field} = {Z.overrides(name)[field]!r} from its default"


def test_wide_seed_is_not_its_low_word():
    """a kernel that keyed Philox with the low word of the seed alone would give the reset of seed & 0xFFFFFFFF"""
    seed = Z.overrides("wide_seed")["seed"]
    assert seed >> 32 and seed & 0xFFFFFFFF
    wide, low = _run("wide_seed").reset, _run("wide_seed", seed=seed & 0xFFFFFFFF).reset
    assert not np.array_equal(wide["scn"], low["scn"])
    assert not np.array_equal(wide["x"].view(np.uint32), low["x"].view(np.uint32))
    assert not np.array_equal(wide["v"].view(np.uint32), low["v"].view(np.uint32))


@pytest.mark.parametrize("name", Z.NAMES)
def test_the_runs_hold_the_events(name):
    r = _run(name)
    counts = dict(ended=r.n_ended(), hit=r.n_hit(), offroad=r.n_offroad(), red=r.n_red(), reach_steps=r.n_reach_steps(),
                  routes_finished=r.n_routes_finished())
    # what the kernel matrix demands of a lit group
    assert counts["ended"] > 0 and counts["hit"] > 0 and counts["red"] > 0, (name, counts)
    if name in ("slow_wide", "fast_narrow"):
        assert counts["reach_steps"] > 0, (name, counts)
    if name == "slow_wide":
        assert counts["routes_finished"] > 0, (name, counts)
    if name in ("thin_edge", "thick_edge"):
        assert counts["offroad"] > 0, (name, counts)


def test_the_edges_move_the_offroad_judgement():
    """both edge runs really happened: with the same seed and actions, some env is offroad under the 0.2 m threshold at a step at which
    it is not under 0.5 m, and some env is offroad under 0.5 m at a step at which it is not under 1.25 m.  (Up to an env's first
    infraction the two runs of a pair are the same trajectory: the threshold only judges.)"""
    thin, thin_d = _run("thin_edge"), _run("thin_edge", offroad_threshold=0.5)
    thick, thick_d = _run("thick_edge"), _run("thick_edge", offroad_threshold=0.5, offroad_threshold_squared=0)
    off = lambda r: (r.done & 4) != 0                                                # noqa: E731
    assert (off(thin) & ~off(thin_d)).any()
    assert (off(thick_d) & ~off(thick)).any()
    first = lambda m: np.where(m.any(0), m.argmax(0), len(m))                        # noqa: E731: an env's first offroad step
    assert (first(off(thin)) <= first(off(thin_d))).all() and (first(off(thick_d)) <= first(off(thick))).all()


def test_to_tde_config_delivers_the_entries():
    """every field an entry changes that EnvConfig / SimulatorConfig can express arrives unchanged.  dt and reach_radius are not
    exposed there (the reference fixes them: 10 Hz, 3 m), so slow_wide and fast_narrow go to the kernels through _abi.default_config
    only - which is how every GPU test of the zoo passes its config."""
    env_fields = ("waypoint_bonus", "heading_penalty", "distance_bonus", "distance_cutoff")
    sim_fields = ("offroad_threshold", "offroad_threshold_squared", "npc_k_steer", "npc_k_speed", "npc_gap_s0", "npc_cone_k",
                  "npc_cone_range", "npc_lane_half", "npc_reach", "npc_max_accel", "npc_max_steer")
    hidden = ("dt", "reach_radius")
    assert not any(hasattr(EnvConfig(), f) or hasattr(SimulatorConfig(), f) for f in hidden)
    for name in Z.NAMES:
        over = Z.overrides(name)
        seed = over.pop("seed", 5)
        assert set(over) <= set(env_fields + sim_fields + hidden), name
        sim = SimulatorConfig(**{f: (bool(v) if f == "offroad_threshold_squared" else v) for f, v in over.items() if f in sim_fields})
        env = EnvConfig(simulator=sim, max_environment_steps=20, **{f: v for f, v in over.items() if f in env_fields})
        got = to_tde_config(env, seed, Z.FLAGS)
        want = Z.config(name, A, seed=seed, **{f: Z.default_of(f) for f in hidden if f in over})
        for f, _ in _abi.TdeConfig._fields_:
            assert getattr(got, f) == getattr(want, f), (name, f, getattr(got, f), getattr(want, f))

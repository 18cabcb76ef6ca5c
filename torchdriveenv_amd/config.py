"""Config / data carriers with the reference's field names and defaults (ref gym_env.py:34-68).

`EnvConfig.simulator` held a torchdrivesim `TorchDriveConfig` in the reference (gym_env.py:46-49); here it is this
package's own `SimulatorConfig` with the fields the step path uses."""
from dataclasses import dataclass, field
from typing import Dict, List, Optional


@dataclass
class RendererConfig:
    left_handed_coordinates: bool = True      # ref gym_env.py:46
    highlight_ego_vehicle: bool = True        # ref gym_env.py:47
    res: int = 64                             # observation space (3,64,64), ref gym_env.py:95
    fov: float = 35.0                         # metres across the image (torchdrivesim default)


@dataclass
class SimulatorConfig:
    renderer: RendererConfig = field(default_factory=RendererConfig)
    collision_metric: str = "nograd"          # CollisionMetric.nograd, ref gym_env.py:48
    left_handed_coordinates: bool = True      # ref gym_env.py:49
    offroad_threshold: float = 0.5            # TorchDriveConfig default (not overridden by the env)
    # how the threshold meets the point-to-mesh distance (torchdrivesim internals are not in the reference repository):
    # False: distance > threshold; True: SQUARED distance > threshold (pytorch3d-style point_mesh distance)
    offroad_threshold_squared: bool = False
    # heuristic NPC controller (stands where the IAI call was, ref gym_env.py:285-294)
    npc_k_steer: float = 1.2
    npc_k_speed: float = 3.0
    npc_gap_s0: float = 3.0
    npc_cone_k: float = 0.5
    npc_cone_range: float = 25.0
    npc_lane_half: float = 1.75
    npc_reach: float = 3.0
    npc_max_accel: float = 3.0
    npc_max_steer: float = 0.3
    # the NPC controller acts from the FIRST step of an episode, as the reference's NPCs do (ref gym_env.py:285-294: IAIWrapper
    # predicts from step one) -> TDE_F_NPC_FIRST_STEP.  False: the NPCs coast through step one (the rule of rounds 4 / 5, slightly
    # cheaper: a re-spawn then leaves nothing to recompute)
    npc_first_step: bool = True


@dataclass
class EnvConfig:
    ego_only: bool = False
    max_environment_steps: int = 200
    frame_stack: int = 3
    waypoint_bonus: float = 100.
    heading_penalty: float = 25.
    distance_bonus: float = 1.
    distance_cutoff: float = 0.5
    use_background_traffic: bool = True
    terminated_at_infraction: bool = True
    seed: Optional[int] = None
    simulator: SimulatorConfig = field(default_factory=SimulatorConfig)
    render_mode: Optional[str] = "rgb_array"
    video_filename: Optional[str] = "rendered_video.mp4"
    video_res: Optional[int] = 1024
    video_fov: Optional[float] = 500
    device: Optional[str] = None


@dataclass
class Scenario:
    agent_states: List[List[float]] = None
    agent_attributes: List[List[float]] = None
    recurrent_states: List[List[float]] = None


@dataclass
class WaypointSuite:
    locations: List[str] = None
    waypoint_suite: List[List[List[float]]] = None
    car_sequence_suite: List[Optional[Dict[int, List[List[float]]]]] = None
    scenarios: List[Optional[Scenario]] = None


def validate(cfg: EnvConfig):
    """Reject what this path does not implement instead of silently ignoring it (the reference accepts these through
    TorchDriveConfig, ref gym_env.py:46-49, 75-80, 295-297)."""
    sim = cfg.simulator
    if str(getattr(sim.collision_metric, "name", sim.collision_metric)) != "nograd":
        raise NotImplementedError(f"collision_metric={sim.collision_metric!r}: only CollisionMetric.nograd (the reference's "
                                  "setting, gym_env.py:48) is implemented: strict OBB overlap")
    if cfg.render_mode == "video":
        raise NotImplementedError("render_mode='video' (BirdviewRecordingWrapper, gym_env.py:295-297) is not part of the "
                                  "step path; use render_mode='rgb_array' and record the frames render() returns")
    if cfg.render_mode not in (None, "rgb_array"):
        raise NotImplementedError                                   # ref gym_env.py:79-80
    if sim.left_handed_coordinates != sim.renderer.left_handed_coordinates:
        raise NotImplementedError("simulator.left_handed_coordinates and renderer.left_handed_coordinates differ: the "
                                  "reference sets both (gym_env.py:46-49); here the flag mirrors the birdview's lateral axis "
                                  "(the kinematic model is built with its default handedness, gym_env.py:245)")
    if sim.npc_cone_k < 0:
        raise ValueError("simulator.npc_cone_k must be >= 0")
    if sim.offroad_threshold <= 0:
        raise ValueError("simulator.offroad_threshold must be > 0")
    if not sim.npc_max_steer >= 0:
        raise ValueError("simulator.npc_max_steer must be >= 0")
    if not 1e-3 <= sim.npc_max_accel <= 1e3:
        raise ValueError("simulator.npc_max_accel must be in [1e-3, 1e3] m/s^2 (tde_env_* reject anything else)")


def render_flags(cfg: EnvConfig):
    """tde_render.flags of this config (RendererConfig, ref gym_env.py:46-47)"""
    from . import _abi

    r = cfg.simulator.renderer
    return ((_abi.RENDER_LEFT_HANDED if r.left_handed_coordinates else 0) |
            (0 if r.highlight_ego_vehicle else _abi.RENDER_PLAIN_EGO))


def to_tde_config(cfg: EnvConfig, seed: int, flags: int):
    """EnvConfig -> the C-ABI's tde_config"""
    from . import _abi

    validate(cfg)
    sim = cfg.simulator
    return _abi.default_config(
        waypoint_bonus=float(cfg.waypoint_bonus), heading_penalty=float(cfg.heading_penalty),
        distance_bonus=float(cfg.distance_bonus), distance_cutoff=float(cfg.distance_cutoff), seed=int(seed),
        max_steps=int(cfg.max_environment_steps), terminated_at_infraction=int(bool(cfg.terminated_at_infraction)),
        offroad_threshold=float(sim.offroad_threshold), npc_k_steer=sim.npc_k_steer, npc_k_speed=sim.npc_k_speed,
        npc_gap_s0=sim.npc_gap_s0, npc_cone_k=sim.npc_cone_k, npc_cone_range=sim.npc_cone_range,
        npc_lane_half=sim.npc_lane_half, npc_reach=sim.npc_reach, npc_max_accel=sim.npc_max_accel,
        npc_max_steer=sim.npc_max_steer, flags=flags,
        offroad_threshold_squared=int(bool(sim.offroad_threshold_squared)))


@dataclass
class NearField:
    """Near-field traffic around the ego at every reset: the local stand-in for the reference's iai_conditional_initialize
    (ref gym_env.py:232-238, iai.py:6-60), which tops the scene up to max(95 - n, agent_density) agents within INITIALIZE_FOV = 120 m
    of the ego.  Candidate poses are tabled once per scenario (world.build_near_field); tde_near_field_spawn draws from them per
    episode.  Not a field of EnvConfig, which mirrors the reference's class name for name: pass it as `near_field=`.

      radius     the spawn radius around the ego [m] (INITIALIZE_FOV)
      count      the agent count the scene is topped up to (95)
      density    the lower bound of the agents to add (agent_density); None: the background file's when `background=` is given,
                 else 0
      pitch      spacing of the candidate poses along polylines / on the lattice [m]
      margin     minimum gap between a candidate and any other agent's box [m]
      clear_ego  minimum centre distance of a candidate from the ego [m]
      speed      (low, high) range of the candidates' desired speeds [m/s]; the spawn speed is a uniform fraction of it
      candidates optional hook (location, scenario_index) -> array [n, 3] of (x, y, psi), e.g. lane centrelines; with `routes` it may
                 return (array [n, 3], routes) instead, routes[i] = the polyline [k, 2] candidate i drives along (or None)
      routes     True: every candidate gets a route ahead of its pose (world.build_near_field) and the spawned agents drive: they
                 keep their desired speed, follow the lane, queue, yield and stop at red lines like the scenario's routed NPCs, and
                 stop at the end of their route.  False (default): no routes - a spawned agent holds its heading and brakes to a
                 standstill; every table, launch and result as without the field
      route_pitch  spacing of a route's waypoints [m]; None: `pitch`
      route_points the most waypoints a route has"""
    radius: float = 120.0
    count: int = 95
    density: Optional[int] = None
    pitch: float = 6.0
    margin: float = 0.5
    clear_ego: float = 10.0
    speed: tuple = (5.0, 12.0)
    candidates: Optional[object] = None
    routes: bool = False
    route_pitch: Optional[float] = None
    route_points: int = 32


def check_near_field(nf, cfg: Optional[EnvConfig] = None):
    """validate a NearField (and its combination with `cfg`); returns it (a dict is accepted as NearField(**dict))"""
    if isinstance(nf, dict):
        nf = NearField(**nf)
    if not isinstance(nf, NearField):
        raise TypeError("near_field must be a NearField (or a dict of its fields)")
    if cfg is not None and cfg.ego_only:
        raise ValueError("near_field with ego_only=True: the reference spawns no traffic in ego-only mode (gym_env.py:192-198)")
    if not (nf.radius > 0 and nf.pitch > 0 and nf.margin > 0 and nf.clear_ego >= 0) or not all(
            map(lambda v: v == v and abs(v) != float("inf"), (nf.radius, nf.pitch, nf.margin, nf.clear_ego))):
        raise ValueError("near_field: radius, pitch and margin must be finite and > 0, clear_ego finite and >= 0")
    if int(nf.count) < 0 or (nf.density is not None and int(nf.density) < 0):
        raise ValueError("near_field: count and density must be >= 0")
    lo, hi = (float(v) for v in nf.speed)
    if not (0 <= lo <= hi) or hi == float("inf"):
        raise ValueError("near_field.speed must be a finite range (low, high) with 0 <= low <= high")
    if nf.route_pitch is not None and not (nf.route_pitch > 0 and nf.route_pitch != float("inf")):
        raise ValueError("near_field.route_pitch must be finite and > 0 (or None: pitch)")
    if int(nf.route_points) != nf.route_points or not 2 <= int(nf.route_points) < 4096:
        raise ValueError("near_field.route_points must be an integer in [2, 4096)")
    if nf.candidates is not None and not callable(nf.candidates):
        raise ValueError("near_field.candidates must be a callable (location, scenario_index) -> array [n, 3] of (x, y, psi)")
    return nf


@dataclass
class VectorObs:
    """The vector observation of BatchedWaypointEnv(obs_mode="vector") (tde_vector_obs, include/tde_hip.h): per env a float32 row of
    dim = 10 + 9 * k_neighbours + 3 * n_rays values - the ego block (v, length, width, the offsets of the current and the next target
    waypoint in the ego frame, targets left (at most 2), steps / max_steps, map-has-lights), the k_neighbours nearest other agents
    within neighbour_radius (valid, forward, left, cos / sin of the relative heading, relative velocity forward / left, length,
    width) and, per ray, the distances to the road edge, to another car and to a red stop line.  Positions are (forward, left) in
    the ego frame.  No reference counterpart.

      k_neighbours      neighbour entries per row, 0 .. 16
      n_rays            rays per row, 0 .. 64, spread evenly counter-clockwise from straight ahead
      ray_range         ray length [m]
      ray_step          spacing of the road-edge samples along a ray [m]; ray_range / ray_step must be an integer <= 1024
      neighbour_radius  agents farther than this from the ego are not neighbours [m]"""
    k_neighbours: int = 8
    n_rays: int = 32
    ray_range: float = 50.0
    ray_step: float = 0.5
    neighbour_radius: float = 50.0

    @property
    def dim(self):
        return 10 + 9 * int(self.k_neighbours) + 3 * int(self.n_rays)

    def ray_directions(self):
        """float32 [n_rays, 2]: unit vectors (forward, left) of the rays, ray k at angle 2 pi k / n_rays"""
        import numpy as np

        a = 2.0 * np.pi * np.arange(int(self.n_rays), dtype=np.float64) / max(1, int(self.n_rays))
        return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], -1).astype(np.float32).reshape(int(self.n_rays), 2))

    def slices(self):
        """name -> slice of a row: ego fields, the neighbour block (reshape row[s] to [k_neighbours, 9]), the ray block (reshape to
        [n_rays, 3]) and its three channels (strided slices, one value per ray)"""
        k, n = int(self.k_neighbours), int(self.n_rays)
        r0 = 10 + 9 * k
        return {"v": slice(0, 1), "length": slice(1, 2), "width": slice(2, 3), "target": slice(3, 5), "next_target": slice(5, 7),
                "targets_left": slice(7, 8), "progress": slice(8, 9), "has_lights": slice(9, 10), "ego": slice(0, 10),
                "neighbours": slice(10, r0), "rays": slice(r0, r0 + 3 * n), "road": slice(r0, r0 + 3 * n, 3),
                "car": slice(r0 + 1, r0 + 3 * n, 3), "red_line": slice(r0 + 2, r0 + 3 * n, 3)}


def check_vector_obs(vo):
    """validate a VectorObs (tde_vector_obs rejects the same); returns it (a dict is accepted as VectorObs(**dict))"""
    import numpy as np

    if isinstance(vo, dict):
        vo = VectorObs(**vo)
    if not isinstance(vo, VectorObs):
        raise TypeError("vector_obs must be a VectorObs (or a dict of its fields)")
    if not (0 <= int(vo.k_neighbours) <= 16) or not (0 <= int(vo.n_rays) <= 64):
        raise ValueError("vector_obs: k_neighbours must be in [0, 16] and n_rays in [0, 64]")
    vals = [np.float32(v) for v in (vo.neighbour_radius, vo.ray_range, vo.ray_step)]
    if not all(np.isfinite(v) and v > 0 for v in vals):
        raise ValueError("vector_obs: neighbour_radius, ray_range and ray_step must be finite and > 0")
    q = np.float32(vals[1] / vals[2])
    if not (1 <= q <= 1024) or q != np.rint(q):
        raise ValueError("vector_obs: ray_range / ray_step must be an integer in [1, 1024]")
    return vo


def observation_layout(cfg: EnvConfig, obs_mode="birdview", frame_stack=1, vector_obs=None):
    """(shape, torch dtype) of ONE env's observation - the single statement of it, and of which obs_mode / frame_stack / vector_obs
    combinations exist: (3 * frame_stack, res, res) uint8 for "birdview", (8,) float32 for "state", (VectorObs.dim,) float32 for
    "vector" (vector_obs None: VectorObs()).  Pure: no device is touched."""
    import torch

    if obs_mode not in ("birdview", "state", "vector"):
        raise ValueError("obs_mode must be 'birdview', 'state' or 'vector'")
    if obs_mode == "vector" and int(frame_stack) > 1:
        raise ValueError("obs_mode='vector' has no frame stack: frame_stack must be 1")
    if vector_obs is not None and obs_mode != "vector":
        raise ValueError("vector_obs= needs obs_mode='vector'")
    if obs_mode == "birdview":
        res = int(cfg.simulator.renderer.res)
        return (3 * max(1, int(frame_stack)), res, res), torch.uint8
    if obs_mode == "state":
        return (8,), torch.float32
    return (check_vector_obs(vector_obs if vector_obs is not None else VectorObs()).dim,), torch.float32


PLANNER_PREDICT = ("constant", "route", "queue")


@dataclass
class Planner:
    """The sampling planner of BatchedWaypointEnv.plan_actions() (tde_plan_action, include/tde_hip.h): every pair of an acceleration
    and a steering value is rolled forward `horizon` steps through the step's own kinematics; a candidate that leaves the road,
    overlaps the predicted box of another agent (constant velocity, inflated by `margin`) or crosses a red stop line fails at that
    step; the cheapest candidate wins, any earlier failure costing more than any later one.  No reference counterpart.

      accelerations  candidate accelerations, each in [-1, 1] (the action box); must contain 0 exactly
      steerings      candidate steering values, each in [-0.3, 0.3]; must contain 0 exactly; len(accelerations) * len(steerings) <= 64
      horizon        steps rolled forward, 1 .. 32
      v_target       speed tracked while a target waypoint exists [m/s] (a finished route plans a stop)
      margin         inflation of the other agents' half extents [m]
      w_progress, w_speed, w_steer   cost weights: per metre gained towards the target waypoint, per (m/s)^2 of speed error summed over
                     the steps, per rad^2 of steering
      predict        how plan_actions() predicts the other agents: "constant" (default; tde_plan_action as it is: each slides along
                     its heading at its speed) or "route": tde_forecast_agents once per call - the environment's own rules for an agent
                     with an empty cone: replay records, route following, braking for red lines and at the route's end - and the lattice
                     judged as one-knot sequences through tde_score_plans_forecast (with PlanRefine's tail and rounds when one is given,
                     every round on the same forecast).  EXPERIMENTAL and opt-in: the forecast is exact for an agent that meets
                     nobody (tests/test_gpu_forecast.py) but ignores queues and yielding, and it does not pay yet: on the junction
                     world with lights (512 envs x 400 steps) collision-ended episodes rise from 117 to 244 of ~1040 (with a 40-step
                     tail from 95 to 159) while red-light ends fall from 37 to 9 and offroad ends from 18 to 6
                     (profiles/forecast_behaviour.txt); or "queue": tde_forecast_scene once per call with
                     the ego coasting - the same rules with the controller's leader sweep kept, so an NPC that queues behind another
                     car or behind the ego is forecast where the step will put it (bit for bit while the ego does coast:
                     tests/test_gpu_forecast_scene.py) - and then "route"'s path exactly.  EXPERIMENTAL and opt-in as well.
                     In the same setting (junction world with lights, 512 envs x 400 steps, seed 7; episodes / infraction ends /
                     offroad / collision / red light / waypoints per episode):
                       constant          1035 / 172 / 18 / 117 / 37 / 4.472      constant + tail 40   1032 / 121 / 7 /  95 / 21 / 4.032
                       route             1062 / 258 /  6 / 244 /  9 / 4.427      route + tail 40      1044 / 166 / 2 / 159 /  6 / 4.090
                       queue             1028 /  31 /  5 /  18 /  9 / 4.621      queue + tail 40      1026 /  23 / 3 /  15 /  6 / 4.129
                     so collisions do fall, against "route" and against "constant" - one seed of one world, and NPCs that would
                     react to the ego's chosen action are still forecast against a coasting ego; no test asserts a ranking.  It
                     costs 5 - 6 % per step(plan_actions()) over "route" at 8192 x 16
                     (profiles/forecast_scene_behaviour.txt, profiles/forecast_scene_kernel_stats.txt)"""
    accelerations: tuple = (-1.0, -0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75, 1.0)
    steerings: tuple = (-0.3, -0.2, -0.1, 0.0, 0.1, 0.2, 0.3)
    horizon: int = 32
    v_target: float = 4.0
    margin: float = 0.3
    w_progress: float = 1.0
    w_speed: float = 0.2
    w_steer: float = 1.0
    predict: str = "constant"

    @property
    def n_candidates(self):
        return len(self.accelerations) * len(self.steerings)

    def tables(self):
        """(float32 [n_a], float32 [n_s]): the lattice; candidate i = ia * n_s + is"""
        import numpy as np

        return np.asarray(self.accelerations, np.float32).reshape(-1), np.asarray(self.steerings, np.float32).reshape(-1)

    def candidate(self, i):
        """(acceleration, steering) of candidate i as float32"""
        a, s = self.tables()
        return a[int(i) // len(s)], s[int(i) % len(s)]


@dataclass
class PlanRefine:
    """Refinement of BatchedWaypointEnv.plan_actions() on top of tde_score_plans (include/tde_hip.h): the lattice's candidates
    become `knots`-knot sequences judged with a brake tail, and the winner is refined knot by knot.
      round 0        the n_a * n_s lattice candidates as constant sequences, each judged over the horizon and then braked for up to
                     `tail` steps (a candidate that cannot be stopped safely loses to any that can) -> winner w
      round r >= 1   knots * n_a * n_s sequences: w with knot k replaced by clamp(w_k + (acceleration_i, steering_j) * shrink^r) into
                     the action box (float32; shrink^r by repeated float32 multiplication); the round's winner becomes w.  The
                     lattice holds 0, so w is among them and the winning cost never rises.
      rounds         refinement rounds after round 0, 0 .. 8
      knots          knots per sequence, 1 .. horizon; knot k holds ceil(horizon / knots) steps
      tail           brake-tail steps, 0 .. 64
      shrink         scale of the lattice offsets per round, in (0, 1]
    EXPERIMENTAL with rounds > 0: measured on the junction world (profiles/plan_refine_behaviour.txt) the tail alone (rounds=0) ends
    fewer episodes by an infraction than the plain planner (121 against 172 of ~1030), but the default two refinement rounds end
    more (261), every cause up.  A likely reason, not yet measured: a two-knot plan that is safe only if its second half is carried
    out leaves less slack against other agents that do not keep their velocity.  PlanRefine(rounds=0) is the setting that pays today."""
    rounds: int = 2
    knots: int = 2
    tail: int = 40
    shrink: float = 0.5


def check_plan_refine(pr, planner=None):
    """validate a PlanRefine (a dict is accepted as PlanRefine(**dict)) against the Planner it refines; returns it"""
    import numpy as np

    if isinstance(pr, dict):
        pr = PlanRefine(**pr)
    if not isinstance(pr, PlanRefine):
        raise TypeError("plan_refine must be a PlanRefine (or a dict of its fields)")
    if int(pr.rounds) != pr.rounds or not (0 <= int(pr.rounds) <= 8):
        raise ValueError("plan_refine: rounds must be an integer in [0, 8]")
    H = int(planner.horizon) if planner is not None else 32
    if int(pr.knots) != pr.knots or not (1 <= int(pr.knots) <= H):
        raise ValueError("plan_refine: knots must be an integer in [1, horizon]")
    if int(pr.tail) != pr.tail or not (0 <= int(pr.tail) <= 64):
        raise ValueError("plan_refine: tail must be an integer in [0, 64]")
    s = np.float32(pr.shrink)
    if not (np.isfinite(s) and 0 < s <= 1):
        raise ValueError("plan_refine: shrink must lie in (0, 1]")
    if planner is not None and int(pr.rounds) > 0 and int(pr.knots) * planner.n_candidates > 1024:
        raise ValueError("plan_refine: knots * candidates must be at most 1024")
    return pr


@dataclass
class PlanReact:
    """plan_actions() with every lattice candidate judged in a scene that reacts to it (tde_score_plans_scene, include/tde_hip.h):
    the candidates are one-knot sequences; for each of them the other agents run the controller - leader sweep included - against
    the ego that takes THAT candidate, where Planner(predict="queue") forecasts them once against a coasting ego.  A follower then
    brakes for a candidate that brakes, and an NPC yields - or does not - to a candidate that pulls out in front of it.
      tail           brake-tail steps after the horizon, 0 .. 64 (PlanRefine's tail; there are no refinement rounds here)
    Needs Planner(predict="constant") (the scene replaces the prediction) and excludes plan_refine.
    EXPERIMENTAL and opt-in: on the junction world with lights (512 envs x 400 steps, seed 7) collision-ended episodes fall from 18 to
    14 against predict="queue" (with the 40-step tail from 15 to 12) but infraction ends as a whole do not move (31 -> 32, 23 -> 21),
    at 6.4 (4.6) times the time per step(plan_actions()) at 8192 x 16: it does not clearly pay as a planner setting
    (profiles/plan_scene_behaviour.txt, profiles/plan_scene_kernel_stats.txt).  The primitive behind it -
    score_plans(react=True), an exact look-ahead of the environment - stands on its exactness tests."""
    tail: int = 40


def check_plan_react(pr, planner=None, plan_refine=None):
    """validate a PlanReact (a dict is accepted as PlanReact(**dict)) against the Planner and PlanRefine it comes with; returns it"""
    if isinstance(pr, dict):
        pr = PlanReact(**pr)
    if not isinstance(pr, PlanReact):
        raise TypeError("plan_react must be a PlanReact (or a dict of its fields)")
    if isinstance(pr.tail, bool) or int(pr.tail) != pr.tail or not (0 <= int(pr.tail) <= 64):
        raise ValueError("plan_react: tail must be an integer in [0, 64]")
    if plan_refine is not None:
        raise ValueError("plan_react with plan_refine: the scene judge has no refinement rounds (choose one)")
    if planner is not None and planner.predict != "constant":
        raise ValueError(f"plan_react needs Planner(predict='constant'): the scene replaces the prediction, got {planner.predict!r}")
    return pr


def check_planner(pl):
    """validate a Planner (tde_plan_action rejects the same); returns it (a dict is accepted as Planner(**dict))"""
    import numpy as np

    if isinstance(pl, dict):
        pl = Planner(**pl)
    if not isinstance(pl, Planner):
        raise TypeError("planner must be a Planner (or a dict of its fields)")
    a, s = pl.tables()
    if len(a) < 1 or len(s) < 1 or len(a) * len(s) > 64:
        raise ValueError("planner: accelerations and steerings must be non-empty with at most 64 candidates in all")
    if not (np.isfinite(a).all() and (np.abs(a) <= np.float32(1.0)).all()):
        raise ValueError("planner: accelerations must lie in [-1, 1]")
    if not (np.isfinite(s).all() and (np.abs(s) <= np.float32(0.3)).all()):
        raise ValueError("planner: steerings must lie in [-0.3, 0.3]")
    if not (a == 0).any() or not (s == 0).any():
        raise ValueError("planner: accelerations and steerings must each contain 0 exactly")
    if int(pl.horizon) != pl.horizon or not (1 <= int(pl.horizon) <= 32):
        raise ValueError("planner: horizon must be an integer in [1, 32]")
    vals = [np.float32(v) for v in (pl.v_target, pl.margin, pl.w_progress, pl.w_speed, pl.w_steer)]
    if not all(np.isfinite(v) and v >= 0 for v in vals):
        raise ValueError("planner: v_target, margin and the weights must be finite and >= 0")
    if pl.predict not in PLANNER_PREDICT:
        raise ValueError(f"planner: predict must be one of {PLANNER_PREDICT}, got {pl.predict!r}")
    return pl


@dataclass
class Prioritized:
    """env.replay_buffer(..., prioritized=Prioritized()): prioritized experience replay (Schaul et al.; include/tde_priority.h).  A
    transition is drawn with probability proportional to its priority p = (|td_error| + eps) ** alpha, kept on the device as an integer
    (16.16 fixed point, so every sum is exact), and new transitions enter with the largest priority seen.
      alpha   how much the TD error decides, in [0, 1]: 0 is the uniform draw over valid_pairs()
      beta    the exponent of the importance weights sample_prioritized() returns, in [0, 1] (its own `beta` argument overrides it: a
              learner anneals it to 1)
      eps     added to |td_error|, > 0: no transition becomes undrawable"""
    alpha: float = 0.6
    beta: float = 0.4
    eps: float = 1e-6


def check_prioritized(pz):
    """validate a Prioritized (a dict is accepted as Prioritized(**dict)); returns it"""
    if isinstance(pz, dict):
        pz = Prioritized(**pz)
    if not isinstance(pz, Prioritized):
        raise TypeError("prioritized must be a Prioritized (or a dict of its fields)")
    if not 0.0 <= float(pz.alpha) <= 1.0:
        raise ValueError(f"prioritized: alpha must be in [0, 1], got {pz.alpha}")
    if not 0.0 <= float(pz.beta) <= 1.0:
        raise ValueError(f"prioritized: beta must be in [0, 1], got {pz.beta}")
    if not 0.0 < float(pz.eps) < float("inf"):
        raise ValueError(f"prioritized: eps must be finite and > 0, got {pz.eps}")
    return pz

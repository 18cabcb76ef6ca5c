"""The config zoo: named sets of tde_config overrides, each leaving the defaults in a direction chosen to break one assumption of the
step / rollout kernels, of the controller's leader sweep or of the host-side keys, and what the tests that cross the kernel matrix
with them share: the config, world, batch and actions of an (entry, A), and a plain oracle run that records what the CPU conditions
count.  A plain helper module: tests/test_config_zoo_cpu.py proves on the oracle alone that every changed field is live and that the
runs hold the events the kernel matrix demands; tests/test_gpu_config_zoo.py then runs the kernels.  Nothing in the package imports
it."""
import numpy as np

from oracle import oracle
from tests import kernel_matrix as km
from torchdriveenv_amd import _abi
from torchdriveenv_amd.state import EnvState
from torchdriveenv_amd.world import effective_offroad_distance

FLAGS = _abi.F_ALL | _abi.F_TRAFFIC_LIGHTS
MAX_STEPS = 20
SLOTS = (4, 16, 64, 128)

# name -> (overrides of _abi.default_config, T: the steps of a run - the smallest multiple of 10 at which the CPU conditions hold, 30
# at least: episodes are 20 steps long, so every env is re-spawned once or more, as in the kernel matrix).
# Values that differ from the first proposal (each reason is a CPU condition of tests/test_config_zoo_cpu.py):
#   slow_wide.reach_radius 6 -> 64: an episode is at most 20 steps of 0.05 s, an ego starts at 10 m/s at most, and the routes have seven
#       or more waypoints 13 - 15 m apart: no route can be finished inside a 6 m radius.  Within 64 m the waypoints are reached one
#       per step and the shortest routes are finished before the episode is truncated (at 48 m none is).
#   slow_wide.T = 40: at 30 steps npc_cone_k = 1 gives the bits of 0.5.
#   fast_narrow.npc_cone_k 0 -> 4: with a cone that does not open the cone predicate implies the lane predicate, so no value of
#       npc_cone_range can be seen; a cone 5 m long shows only when it opens wide (up to 2 it still gives the default's bits).
#       npc_cone_k = 0 is kept, alive, in thin_edge, where npc_cone_range has its default.
#   degenerate.npc_max_steer 0 -> 0.0625: with the clamp at zero no NPC steers, so no value of npc_k_steer can be seen (a steering
#       angle of +0 or -0 leaves the bicycle's bits alone), and without turning NPCs nothing enters a cone: npc_cone_range = 0 gives
#       the bits of 25.  npc_max_steer = 0 is kept, alive, in thick_edge, where npc_k_steer has its default.
ZOO = {
    "slow_wide": (dict(dt=0.05, npc_max_accel=1.0, npc_gap_s0=6.0, npc_lane_half=2.5, npc_cone_k=1.0, npc_cone_range=60.0,
                       npc_reach=5.0, npc_k_steer=2.5, npc_k_speed=1.0, npc_max_steer=0.15, reach_radius=64.0, distance_cutoff=0.05,
                       waypoint_bonus=7.5, heading_penalty=12.5, distance_bonus=0.125), 40),
    "fast_narrow": (dict(dt=0.2, npc_max_accel=8.0, npc_gap_s0=0.5, npc_lane_half=0.9, npc_cone_k=4.0, npc_cone_range=5.0,
                         npc_reach=1.0, npc_k_steer=0.5, npc_k_speed=6.0, npc_max_steer=0.5, reach_radius=1.5, distance_cutoff=2.0,
                         waypoint_bonus=1000.0, heading_penalty=3.125, distance_bonus=3.0), 30),
    "degenerate": (dict(npc_max_steer=0.0625, npc_k_steer=0.0, npc_gap_s0=0.0, npc_cone_range=0.0, npc_lane_half=0.0), 30),
    "thin_edge": (dict(offroad_threshold=0.2, npc_cone_k=0.0), 30),
    "thick_edge": (dict(offroad_threshold=1.5625, offroad_threshold_squared=1, npc_max_steer=0.0), 30),     # (1.25 m)
    "wide_seed": (dict(seed=0x9E3779B97F4A7C15), 30),
}
NAMES = tuple(ZOO)
_worlds = {}


def overrides(name):
    return dict(ZOO[name][0])


def fields(name):
    """the tde_config fields entry `name` changes"""
    return tuple(ZOO[name][0])


def steps(name):
    return ZOO[name][1]


def default_of(field):
    return getattr(_abi.default_config(), field)


def config(name, A, **kw):
    """the tde_config of (entry, A): the defaults, the flags and episode length of every zoo run, a seed of its own, the entry's
    overrides (name None: the defaults), then `kw`"""
    base = dict(seed=2000 + 16 * A + (NAMES.index(name) if name else 7), flags=FLAGS, max_steps=MAX_STEPS)
    if name:
        base.update(ZOO[name][0])
    base.update(kw)
    return _abi.default_config(**base)


def threshold(name):
    """the offroad distance in metres entry `name` asks for: what its worlds' grid index is built for"""
    o = ZOO[name][0] if name else {}
    return effective_offroad_distance(o.get("offroad_threshold", 0.5), bool(o.get("offroad_threshold_squared", 0)))


def world(name, A, kind=None):
    """the kernel matrix's world of A slots (tests/test_gpu_kernel_matrix.py: the junction maps up to 64 slots, the crowded town at 128;
    kind="town": the town at any A), stop lines lengthened along the lane in the same way, its grid index built for the entry's
    offroad distance.  One host world per (kind, A, distance)."""
    from torchdriveenv_amd.synth import synthetic_town, synthetic_world

    kind = kind or ("town" if A == 128 else "junctions")
    thr = threshold(name)
    key = (kind, A, thr)
    if key not in _worlds:
        if kind == "town":
            w = synthetic_town(n_scn=4, A=A, n_streets=4, spacing=100.0, ext=160.0, min_gap=3.4, n_signals=4, threshold=thr)
            assert w.ints["hints"] & _abi.WORLD_LARGE_GRID
            w.arrays["stoplines"]["hl"][:] = 25.0
        else:
            w = synthetic_world(n_scn=8, A=A, seed=A, n_maps=2, threshold=thr)
            assert not w.ints["hints"] & _abi.WORLD_LARGE_GRID
            w.arrays["stoplines"]["hl"][:] = 60.0
        assert w.has_lights
        _worlds[key] = w
    return _worlds[key]


def batch(A, cu):
    return km._small_B(A)(cu)


def actions(name, B, A, T=None):
    """float32 [T, B, 2]: the kernel matrix's actions (half the egos drive on steadily, half swerve).  Under `degenerate` every
    third env's steering is a signed zero (+0 and -0 in turn) and every fifth env's acceleration is one, on alternate steps."""
    from tests.test_gpu_kernel_matrix import _actions

    T = steps(name) if T is None else T
    a = _actions(B, seed=A + 7, T=T)
    if name == "degenerate":
        sign = np.where((np.arange(T)[:, None] + np.arange(B)[None, :]) % 2 == 0, np.float32(0.0), np.float32(-0.0))
        a[:, ::3, 1] = sign[:, ::3]
        a[::2, ::5, 0] = sign[::2, ::5]
        assert np.signbit(a[..., 1]).any() and (a[..., 1] == 0).any()
    return a


class Run:
    """the oracle on the whole batch for T steps: per step the reward, the done bits, the waypoints reached so far (get_info's
    count), the scenario the step was made in; the state after the reset and after the last step"""

    def __init__(self, cfg, world, B, acts):
        T, A = len(acts), world.A
        hs = EnvState(B, A)
        oracle.env_reset(cfg, world, hs)
        self.reset = hs.host()
        self.reward, self.done = np.zeros((T, B), np.float32), np.zeros((T, B), np.uint8)
        self.reached, self.scn = np.zeros((T, B), np.int32), np.zeros((T, B), np.int32)
        for t in range(T):
            self.scn[t] = hs["scn"]
            hs["action"][...] = acts[t]
            oracle.env_step(cfg, world, hs)
            self.reward[t], self.done[t], self.reached[t] = hs["reward"], hs["done_bits"], hs["info_reached"]
        self.final = hs.host()
        self.wp_n = world.arrays["scn"]["wp_n"][self.scn]

    def same(self, other):
        """bit for bit: the per-step rewards and done bits and the state after the last step"""
        if not (np.array_equal(self.reward.view(np.uint32), other.reward.view(np.uint32)) and np.array_equal(self.done, other.done)):
            return False
        return all(np.array_equal(np.ascontiguousarray(v).view(np.uint8), np.ascontiguousarray(other.final[k]).view(np.uint8))
                   for k, v in self.final.items() if k != "action")

    # what the CPU conditions count (done bits: 1 terminated, 2 truncated, 4 offroad, 8 collided, 16 red light)
    @property
    def ended(self):
        return (self.done & 3) != 0

    def n_ended(self):
        return int(self.ended.sum())

    def n_hit(self):
        return int(((self.done & 12) != 0).sum())

    def n_offroad(self):
        return int(((self.done & 4) != 0).sum())

    def n_red(self):
        return int(((self.done & 16) != 0).sum())

    def n_reach_steps(self):
        """steps at which the ego's count of reached waypoints grew"""
        prev = np.concatenate([np.zeros((1, self.reached.shape[1]), np.int32), self.reached[:-1]], 0)
        prev[np.concatenate([np.zeros((1, self.reached.shape[1]), bool), self.ended[:-1]], 0)] = 0      # (a re-spawn restarts the count)
        return int((self.reached > prev).sum())

    def n_routes_finished(self):
        """episodes that ended with every waypoint reached: the target index (1 + reached: a reset leaves it at 1) at the route's length"""
        return int((self.ended & (1 + self.reached >= self.wp_n)).sum())

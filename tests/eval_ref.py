"""numpy restatement of tde_env_reset_to and tde_eval_advance (include/tde_hip.h) over the oracle's reset and step, the checker of the
evaluation tests: test infrastructure only, nothing in the package imports it.  No new physics is written here.  The oracle has no
forced-scenario reset, and needs none: the scenario draw is (word * n_scn) >> 32, which is 0 in a world of one scenario, and no other
random word depends on it - so "env e starts scenario s" is the oracle's own reset on the world that holds only scenario s (routes,
replays and maps whole: the spawn records keep their ids), with state.scn set to s afterwards."""
import numpy as np

from oracle import oracle
from torchdriveenv_amd import _abi
from torchdriveenv_amd.state import EnvState
from torchdriveenv_amd.world import World

REC = _abi.EPISODE_RECORD_DTYPE
PER_SCENARIO = ("scn", "spawn", "wp_xy", "start_psi", "first_gap")


def single_scenario_world(world, s):
    """the host world that holds only scenario s of `world`: row s of scn, spawn, wp_xy, start_psi and first_gap; routes, replays
    and maps whole"""
    S = world.n_scn
    assert 0 <= s < S
    arrays = {}
    for k, a in world.arrays.items():
        arrays[k] = np.ascontiguousarray(a.reshape(S, -1)[s:s + 1].reshape((-1,) + a.shape[1:]) if k in PER_SCENARIO and a.size >= S
                                         and a.size % S == 0 else a).copy()
    ints = dict(world.ints)
    ints["n_scn"] = 1
    w = World(arrays, ints, world.threshold)
    assert w.arrays["spawn"].size == world.A and w.arrays["wp_xy"].size == world.ints["NW"] * 2
    return w


def singles_of(world):
    return [single_scenario_world(world, s) for s in range(world.n_scn)]


def reset_to(cfg, world, hs, scn=None, mask=None, singles=None):
    """tde_env_reset_to on a host state: envs with scn[e] >= 0 start that scenario, scn[e] < 0 (or scn None) draw it, an id >= n_scn
    leaves its env as it is; mask as tde_env_reset's"""
    B = hs.B
    sel = np.ones(B, bool) if mask is None else np.asarray(mask).reshape(B) != 0
    ids = np.full(B, -1, np.int64) if scn is None else np.asarray(scn, np.int64).reshape(B)
    draw = sel & (ids < 0)
    if draw.any():
        oracle.env_reset(cfg, world, hs, draw.astype(np.uint8))
    singles = singles if singles is not None else singles_of(world)
    for s in sorted(set(ids[sel & (ids >= 0) & (ids < world.n_scn)].tolist())):
        m = sel & (ids == s)
        oracle.env_reset(cfg, singles[s], hs, m.astype(np.uint8))
        hs["scn"][m] = s


def new_eval(plan):
    """the host twin of a tde_eval: plan int32 [R, B]; round, acc and results zero; active where round 0 has an episode"""
    plan = np.ascontiguousarray(plan, np.int32)
    R, B = plan.shape
    return dict(plan=plan, round=np.zeros(B, np.int32), active=(plan[0] >= 0).astype(np.uint8), acc=np.zeros(B, REC),
                results=np.zeros((R, B), REC))


def advance(cfg, world, hs, ev, singles=None):
    """tde_eval_advance on a host state the oracle has just stepped WITHOUT TDE_F_AUTORESET: fold, finish, advance"""
    assert not cfg.flags & _abi.F_AUTORESET
    plan, R = ev["plan"], ev["plan"].shape[0]
    B = hs.B
    respawn = np.full(B, -1, np.int64)
    for e in range(B):
        if not ev["active"][e]:
            continue
        acc = ev["acc"][e]
        acc["ret"] = acc["ret"] + np.float64(hs["reward"][e])
        acc["psi_sum"] = acc["psi_sum"] + hs["info"][e, 0]
        acc["speed_sum"] = acc["speed_sum"] + hs["info"][e, 1]
        if not (hs["terminated"][e] | hs["truncated"][e]):
            continue
        r = int(ev["round"][e])
        nxt = -1
        if 0 <= r < R:
            rec = ev["results"][r, e]
            rec["ret"], rec["psi_sum"], rec["speed_sum"] = acc["ret"], acc["psi_sum"], acc["speed_sum"]
            rec["length"], rec["reached"], rec["scn"], rec["bits"] = hs["steps"][e], hs["info_reached"][e], hs["scn"][e], hs["done_bits"][e]
            ev["acc"][e] = np.zeros((), REC)
            ev["round"][e] = r + 1
            if r + 1 < R:
                nxt = int(plan[r + 1, e])
        if 0 <= nxt < world.n_scn:
            respawn[e] = nxt
        else:
            ev["active"][e] = 0
    if (respawn >= 0).any():
        reset_to(cfg, world, hs, respawn, respawn >= 0, singles)
    return respawn >= 0


def run(cfg, world, B, plan, action_of, max_calls=10_000, singles=None, on_step=None):
    """a whole oracle-driven evaluation: reset_to(plan[0]) (idle envs draw), then step + advance until no env is active.
    action_of(t, hs) -> float32 [B, 2]; on_step(t, hs, ev, respawned) after every advance.  -> (ev, hs, number of steps)"""
    singles = singles if singles is not None else singles_of(world)
    hs = EnvState(B, world.A)
    ev = new_eval(plan)
    reset_to(cfg, world, hs, ev["plan"][0], None, singles)
    t = 0
    while ev["active"].any():
        assert t < max_calls
        hs["action"][...] = action_of(t, hs)
        oracle.env_step(cfg, world, hs)
        re = advance(cfg, world, hs, ev, singles)
        if on_step is not None:
            on_step(t, hs, ev, re)
        t += 1
    return ev, hs, t


def jobs_of(ev, n_jobs):
    """the finished records in job order (job j = episode j // B of env j % B)"""
    return ev["results"].reshape(-1)[:n_jobs]

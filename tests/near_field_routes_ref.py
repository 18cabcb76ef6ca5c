"""Checkers of routed near-field traffic (NearField(routes=True), tde_state.slot_route): test infrastructure only, nothing in the
package imports it.  No new physics is written here.

  * spawn(): the numpy restatement of tde_near_field_spawn WITH the per-slot route words, over tests/near_field_ref.py's.
  * compose(): the specification of the routed step.  The oracle reads a slot's route from its spawn record, as every kernel but the
    routed one does - so "slot a of env e follows route r" is the oracle's own step on a world in which every env is a scenario of its
    own: scenario e = a copy of scenario scn[e] whose records for the slots that carry a route word are patched from the word, the
    state's route_wp and the route table (route, route_wp, route_n, tgx0 / tgy0, present).  The state then says scn[e] = e."""
import numpy as np

from oracle import oracle
from tests import near_field_ref as R
from torchdriveenv_amd import _abi
from torchdriveenv_amd.state import EnvState
from torchdriveenv_amd.world import World

PER_SCENARIO = ("scn", "spawn", "wp_xy", "start_psi", "first_gap")
ID_BITS = _abi.CACHE_ID_BITS
# what a step leaves, bit for bit (the issue's list); `info` gets tests/test_gpu_near_field.py's tolerance on its cosine column
AGENT = ("x", "y", "psi", "v", "route_wp", "present", "collided", "offroad")
ENV = ("reward", "terminated", "truncated", "tl_violation", "done_bits", "steps", "target_idx", "reached")


def words(st):
    return st["slot_route"].view(np.uint32)


def spawn_env(cfg, world, table, st, e):
    """the spawner on env e of the host state `st` (which carries slot_route), in place"""
    A = table.A
    base, s = e * A, int(st["scn"][e])
    sr = words(st)
    sr[base + 1:base + A] = 0
    free = [a for a in range(1, A) if world.arrays["spawn"][s, a]["present"] == 0]
    acc = R.spawn_env(cfg, world, table, st, e)
    for k, i in enumerate(acc):
        cd = table.cand[s, i]
        st["route_wp"][base + free[k]] = int(cd["route_wp"])
        if cd["route"]:
            sr[base + free[k]] = np.uint32(cd["route"]) | (np.uint32(cd["route_n"]) << np.uint32(ID_BITS))
    return acc


def spawn(cfg, world, table, st, mask=None):
    for e in range(len(st["scn"])):
        if mask is None or mask[e]:
            spawn_env(cfg, world, table, st, e)


def compose(world, st, envs=None):
    """the world in which env envs[k] (default: every env) of the host state `st` is scenario k, its route words in the records"""
    S, A = world.n_scn, world.A
    envs = np.arange(len(st["scn"])) if envs is None else np.asarray(envs)
    scn = np.asarray(st["scn"])[envs]
    arrays = {}
    for k, a in world.arrays.items():
        per = k in PER_SCENARIO and a.size >= S and a.size % S == 0
        arrays[k] = np.ascontiguousarray(a.reshape(S, -1)[scn].reshape((-1,) + a.shape[1:])) if per else a
    ints = dict(world.ints)
    ints["n_scn"] = len(envs)
    spawn_rec = arrays["spawn"].reshape(len(envs), A)
    rt = world.arrays["route_xy"].reshape(-1, world.ints["RW"], 2)
    sr = words(st).reshape(-1, A)[envs]
    wp = np.asarray(st["route_wp"]).reshape(-1, A)[envs]
    for k, a in zip(*np.nonzero(sr)):
        rec = spawn_rec[k, a]
        rid, n = int(sr[k, a] & ((1 << ID_BITS) - 1)) - 1, int(sr[k, a] >> ID_BITS)
        rec["route"], rec["route_wp"], rec["route_n"], rec["present"] = rid, wp[k, a], n, 1
        if wp[k, a] < n:
            rec["tgx0"], rec["tgy0"] = rt[rid, wp[k, a]]
    return World(arrays, ints, world.threshold)


def sub_state(host, envs, A):
    """a host EnvState of the envs `envs` of the arrays `host` (an EnvState.host() dict), numbered 0, 1, ..."""
    envs = np.asarray(envs)
    B = len(next(v for k, v in host.items() if k == "scn"))
    hs = EnvState(len(envs), A, with_slot_route="slot_route" in host)
    for k, dst in hs.arrays.items():
        if dst is None or k not in host or k in ("slot_cache", "env_cache", "act_cache"):
            continue
        src = np.asarray(host[k])
        dst[...] = src.reshape((B, -1))[envs].reshape(dst.shape)
    return hs


def oracle_step(cfg, cworld, hs):
    """one oracle step of `hs` on its composed world `cworld` (scenario e = env e), the state's own scenario ids kept"""
    true = hs["scn"].copy()
    hs["scn"][...] = np.arange(len(true))
    oracle.env_step(cfg, cworld, hs)
    hs["scn"][...] = true


def same(h, d, what, envs=None, A=None, keys=AGENT + ENV):
    """host state `h` (envs 0 .. n-1) against the arrays `d` of a device state (its envs `envs`), bit for bit; info as
    tests/test_gpu_near_field.py holds it"""
    n = len(h["scn"])
    envs = np.arange(n) if envs is None else np.asarray(envs)
    B = len(d["scn"])
    for k in keys + ("info",):
        if h[k] is None or k not in d:
            continue
        hv, dv = np.asarray(h[k]).reshape(n, -1), np.asarray(d[k]).reshape(B, -1)[envs]
        if k == "info":
            assert np.array_equal(np.ascontiguousarray(hv[:, [0, 1, 3]]).view(np.uint8), np.ascontiguousarray(dv[:, [0, 1, 3]]).view(np.uint8)), (what, k)
            assert np.allclose(hv[:, 2], dv[:, 2], rtol=0.0, atol=1e-13), (what, k)
            continue
        bad = np.flatnonzero((np.ascontiguousarray(hv).view(np.uint8) != np.ascontiguousarray(dv).view(np.uint8)).reshape(n, -1).any(1))
        assert len(bad) == 0, (what, k, bad[:8])


# ---- worlds of the tests -----------------------------------------------------------------------------------------------------------
def junction_near_field(world, nf, seed=3, trips=1, keep=None):
    """(world, table) of a synth.synthetic_world with near field `nf`: candidates every nf.pitch metres along the routes of the
    scenario's routed NPCs (`trips` staggered passes per route), through world.build_near_field with the tracer of the polylines
    source.  synthetic_world fills every slot, so the records of slots >= `keep` (default A / 4) are made absent first: the free slots
    the spawner fills.  The world's spawn records change in place, and its route table grows when nf.routes."""
    from torchdriveenv_amd.env import _resample_polyline
    from torchdriveenv_amd.world import build_near_field, polyline_ahead

    S = world.n_scn
    rt = world.arrays["route_xy"].reshape(-1, world.ints["RW"], 2)
    gone = world.arrays["spawn"].reshape(S, world.A)[:, max(2, world.A // 4) if keep is None else keep:]
    routes_of = [[(int(r["route"]), int(r["route_n"])) for r in world.arrays["spawn"].reshape(S, world.A)[s, 1:]
                  if r["present"] and r["route"] >= 0 and r["route_n"] >= 2] for s in range(S)]
    gone["present"], gone["route"], gone["replay"], gone["route_n"], gone["replay_len"] = 0, -1, -1, 0, 0
    world._host_struct = None
    rp = float(nf.route_pitch if nf.route_pitch is not None else nf.pitch)
    positions, tracers = [], []
    for s in range(S):
        pls = [rt[r, :n].astype(np.float64) for r, n in routes_of[s]]
        pos, flat = [], []
        for pl in pls:
            for trip in range(trips):
                where = []
                p = _resample_polyline(pl, float(nf.pitch), where)
                if trip:                                             # a second pass, half a pitch further along
                    sh = 0.5 * float(nf.pitch)
                    p = p + sh * np.stack([np.cos(p[:, 2]), np.sin(p[:, 2]), np.zeros(len(p))], -1)
                    where = [(seg, t + sh) for seg, t in where]
                pos.append(p)
                flat += [(pl, seg, t) for seg, t in where]
        positions.append(np.concatenate(pos, 0) if pos else np.zeros((0, 3)))
        tracers.append(lambda i, x, y, psi, flat=flat: polyline_ahead(*flat[i], rp, int(nf.route_points)))
    table = build_near_field(world, positions, nf, seed, 0, tracers if nf.routes else None)
    return world, table


def moving_share(cfg, world, table, B, steps=80, routes=True, seed_episode=0):
    """the composed oracle with zero ego actions: -> (bool [B, A] spawned, float32 [B, A] v after `steps` steps, float [B, A] distance
    travelled).  routes=False: the same spawns with the route words dropped (the control)"""
    A = world.A
    hs = EnvState(B, A, with_slot_route=True)
    hs["episode"][...] = seed_episode
    oracle.env_reset(cfg, world, hs)
    spawn(cfg, world, table, hs)
    if not routes:
        words(hs)[...] = 0
    free = world.arrays["spawn"]["present"][hs["scn"]] == 0
    spawned = (hs["present"].reshape(B, A) != 0) & free
    cw = compose(world, hs)
    x0, y0 = hs["x"].copy(), hs["y"].copy()
    hs["action"][...] = 0.0
    for _ in range(steps):
        oracle_step(cfg, cw, hs)
    dist = np.hypot(hs["x"] - x0, hs["y"] - y0).reshape(B, A)
    return spawned, hs["v"].reshape(B, A).copy(), dist

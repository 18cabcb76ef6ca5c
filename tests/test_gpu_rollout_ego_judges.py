"""The three-role rollout's judges compute the EGO's collision and offroad flags only before a launch's last step (judge C: one
(ego, slot) pair per lane; judge O: one corner of the ego's box per lane) and every slot's flags at the last step.  Forced to the
trio form, each A / world / LIGHTS instantiation is compared bit for bit with the oracle's repeated steps: the reward and done rows of
every step and the final state, for launches of K = 1, 2, 17 and 250 steps from the same hand-edited start.

The start is an oracle reset edited by hand (envs by e % 4): 0 - two NPCs parked on each other off the road; 1, 3 - a parked NPC on
the ego's box, slot 1 + (e // 2) % (A - 1); 2 - the ego turned and shifted towards a road edge.  Before comparing, the oracle run
must show (a) an NPC-NPC overlap at an intermediate step in an env whose ego has none, (b) ego-NPC overlaps at intermediate steps
that cover every slot 1 .. A-1, (c) for every corner, an intermediate step at which that corner alone is off the road (float64
distances, every corner at least 1 cm from the threshold) and (d) an NPC with collided = 1 and one with offroad = 1 in the final
state.  One oracle run of 250 steps serves every K (a launch of K steps is its first K steps).  Episodes end only by
truncation after 1000 steps, so the poses behind every counted event are the state's after the step."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import oracle  # noqa: E402
from tests.witness_util import _mesh_dist  # noqa: E402
from torchdriveenv_amd import _abi, _lib, ops  # noqa: E402
from torchdriveenv_amd.state import EnvState  # noqa: E402
from torchdriveenv_amd.synth import synthetic_town, synthetic_world  # noqa: E402

DEV = "cuda:0"
B = 64
KS = (1, 2, 17, 250)
KMAX = max(KS)
MARGIN = 0.01          # metres: corners this close to the offroad threshold are not counted for (c)
CASES = [(A, kind, lights) for A in (8, 16, 32) for kind in ("junctions", "town") for lights in (False, True)]
_WORLDS = {}


def _world(kind, A):
    if (kind, A) not in _WORLDS:
        if kind == "town":
            w = synthetic_town(n_scn=4, A=A, n_streets=4, spacing=100.0, ext=160.0, min_gap=3.4, n_signals=4)
            assert w.ints["hints"] & _abi.WORLD_LARGE_GRID
        else:
            w = synthetic_world(n_scn=8, A=A, seed=A, n_maps=2)
            assert not w.ints["hints"] & _abi.WORLD_LARGE_GRID
        assert w.has_lights
        _WORLDS[(kind, A)] = w
    return _WORLDS[(kind, A)]


def _config(A, kind, lights):
    # (no replay: a replayed NPC's pose would overwrite the hand edits)
    flags = (_abi.F_ALL & ~_abi.F_REPLAY) | (_abi.F_TRAFFIC_LIGHTS if lights else 0)
    cfg = _abi.default_config(seed=500 + A + 2 * lights + (kind == "town"), flags=flags, distance_cutoff=0.25)
    cfg.terminated_at_infraction = 0
    cfg.max_steps = 1000
    return cfg


def _start(cfg, world, A):
    """an oracle reset, edited by hand (module docstring)"""
    hs = EnvState(B, A)
    oracle.env_reset(cfg, world, hs)
    h = hs.host()
    f = {k: h[k].reshape(B, A) for k in ("x", "y", "psi", "v", "len", "wid", "lr", "vdes", "present")}

    def park(e, j, x, y, psi):
        for k in ("len", "wid", "lr"):
            f[k][e, j] = f[k][e, 0]
        f["x"][e, j], f["y"][e, j], f["psi"][e, j] = x, y, psi
        f["v"][e, j] = f["vdes"][e, j] = 0.0
        f["present"][e, j] = 1

    for e in range(B):
        x, y, psi = float(f["x"][e, 0]), float(f["y"][e, 0]), float(f["psi"][e, 0])
        c, s = np.cos(psi), np.sin(psi)
        if e % 4 == 0:                                   # two NPCs on each other, 40 m to the ego's left: off the road
            px, py = x - 40.0 * s, y + 40.0 * c
            park(e, 1, px, py, psi)
            park(e, 2, px + 1.0 * c, py + 1.0 * s, psi + 0.2)
        elif e % 2 == 1:                                 # a parked NPC on the ego's box, a little ahead
            j = 1 + (e // 2) % (A - 1)
            d = 1.0 + 0.5 * ((e // 4) % 3)
            park(e, j, x + d * c, y + d * s, psi + 0.1 * ((e // 2) % 5 - 2))
        else:                                            # the ego turned towards / away from a road edge and shifted sideways
            k = e // 4
            turn = (0.5 if k % 2 else -0.5) * (1 + (k // 2) % 2)
            side = (2.0 + 1.5 * ((k // 4) % 4)) * (1 if (k // 2) % 2 else -1)
            f["x"][e, 0], f["y"][e, 0], f["psi"][e, 0] = x - side * s, y + side * c, psi + turn
    for k in f:
        h[k] = f[k].reshape(-1)
    return h


def _actions(K, seed):
    rng = np.random.default_rng(seed)
    acc = rng.uniform(-1.0, 1.0, (K, B))
    steer = rng.uniform(-0.3, 0.3, (K, B))
    return np.stack([acc, steer], -1).astype(np.float32)


def _pair_slack(x, y, psi, hl, hw, i, j):
    """float64 separating-axis slack of boxes i and j of every env (< 0: they overlap)"""
    c, s = np.cos(psi), np.sin(psi)
    dx, dy = x[:, j] - x[:, i], y[:, j] - y[:, i]
    ci, si, cj, sj = c[:, i], s[:, i], c[:, j], s[:, j]
    cc, ss = np.abs(ci * cj + si * sj), np.abs(ci * sj - si * cj)
    a0 = np.abs(dx * ci + dy * si) - (hl[:, i] + hl[:, j] * cc + hw[:, j] * ss)
    a1 = np.abs(dy * ci - dx * si) - (hw[:, i] + hl[:, j] * ss + hw[:, j] * cc)
    a2 = np.abs(dx * cj + dy * sj) - (hl[:, j] + hl[:, i] * cc + hw[:, i] * ss)
    a3 = np.abs(dy * cj - dx * sj) - (hw[:, j] + hl[:, i] * ss + hw[:, i] * cc)
    return np.maximum(np.maximum(a0, a1), np.maximum(a2, a3))


def _ego_corner_dist(world, st, A):
    """[B, 4] float64 distance of the ego's corners FL, FR, RR, RL (offroad_issue's order) to its map's mesh.  Only triangles whose
    bounding box comes within hl + hw + 3 m of the ego's centre are searched: a corner farther than 3 m from all of them is off the
    road whichever the true distance is."""
    x, y, psi = (np.asarray(st[k], np.float64).reshape(B, A)[:, 0] for k in ("x", "y", "psi"))
    hl, hw = (0.5 * np.asarray(st[k], np.float64).reshape(B, A)[:, 0] for k in ("len", "wid"))
    c, s = np.cos(psi), np.sin(psi)
    maps = world.arrays["scn"]["map"][np.asarray(st["scn"]).astype(np.int64)]
    mrec, tri = world.arrays["maps"], world.arrays["tri"]
    out = np.full((B, 4), np.inf)
    for e in range(B):
        m = int(maps[e])
        t0, n = int(mrec[m]["tri_base"]), int(mrec[m]["n_tri"])
        T = tri[t0:t0 + n].reshape(-1, 3, 2).astype(np.float64)
        r = hl[e] + hw[e] + 3.0
        near = ((T[:, :, 0].min(1) <= x[e] + r) & (T[:, :, 0].max(1) >= x[e] - r) & (T[:, :, 1].min(1) <= y[e] + r)
                & (T[:, :, 1].max(1) >= y[e] - r))
        if not near.any():
            continue
        for q, (sl, sw) in enumerate(((1, 1), (1, -1), (-1, -1), (-1, 1))):
            px = x[e] + sl * hl[e] * c[e] - sw * hw[e] * s[e]
            py = y[e] + sl * hl[e] * s[e] + sw * hw[e] * c[e]
            out[e, q] = _mesh_dist(np.array([px]), np.array([py]), T[near])[0]
    return out


def oracle_run(cfg, world, A, start, acts, snaps):
    """the oracle's repeated steps from `start`: rewards and done bytes of every step, the state after each step K - 1 for K in
    `snaps`, and the event counts of the steps before the last"""
    hs = EnvState(B, A)
    hs.load(start)
    K = acts.shape[0]
    reward, done = np.zeros((K, B), np.float32), np.zeros((K, B), np.uint8)
    state = {}
    ev = {"npc_npc": 0, "ego_slots": set(), "corner_alone": [0, 0, 0, 0]}
    thr = float(cfg.offroad_threshold)
    for t in range(K):
        hs["action"][...] = acts[t]
        oracle.env_step(cfg, world, hs)
        reward[t], done[t] = hs["reward"], hs["done_bits"]
        if t + 1 in snaps:
            state[t + 1] = hs.host()
        if t == K - 1:
            break
        st = hs.host()
        kept = done[t] & 3 == 0                          # not re-spawned: the state holds this step's poses and flags
        col = st["collided"].reshape(B, A) != 0
        pres = st["present"].reshape(B, A) != 0
        ev["npc_npc"] += int((kept & ~col[:, 0] & col[:, 1:].any(1)).sum())
        x, y, psi = (np.asarray(st[k], np.float64).reshape(B, A) for k in ("x", "y", "psi"))
        hl, hw = (0.5 * np.asarray(st[k], np.float64).reshape(B, A) for k in ("len", "wid"))
        for j in range(1, A):
            hit = kept & pres[:, 0] & pres[:, j] & (_pair_slack(x, y, psi, hl, hw, 0, j) < -MARGIN)
            assert not (hit & ((done[t] & 8) == 0)).any(), "a clear ego overlap without the done byte's collision bit"
            if hit.any():
                ev["ego_slots"].add(j)
        d = _ego_corner_dist(world, st, A)
        clear = kept & pres[:, 0] & (np.abs(d - thr) >= MARGIN).all(1)
        off = d > thr
        for q in range(4):
            alone = clear & off[:, q] & (off.sum(1) == 1)
            assert ((done[t][alone] & 4) != 0).all(), "a corner clearly off the road without the done byte's offroad bit"
            ev["corner_alone"][q] += int(alone.sum())
    return reward, done, state, ev


@pytest.mark.parametrize("A,kind,lights", CASES, ids=[f"A{A}-{k}-{'lights' if L else 'dark'}" for A, k, L in CASES])
def test_trio_rollout_ego_judges_match_the_oracle(A, kind, lights):
    world = _world(kind, A)
    cfg = _config(A, kind, lights)
    start = _start(cfg, world, A)
    acts_h = _actions(KMAX, seed=A + 3 * lights)
    want_r, want_d, want_st, ev = oracle_run(cfg, world, A, start, acts_h, KS)
    final = want_st[KMAX]
    fc, fo = final["collided"].reshape(B, A), final["offroad"].reshape(B, A)
    # non-vacuity: both judge forms meet the events they exist for
    assert ev["npc_npc"] > 0, ev
    assert ev["ego_slots"] == set(range(1, A)), sorted(set(range(1, A)) - ev["ego_slots"])
    assert min(ev["corner_alone"]) > 0, ev["corner_alone"]
    assert fc[:, 1:].any() and fo[:, 1:].any(), (int(fc[:, 1:].sum()), int(fo[:, 1:].sum()))
    dw = world.to_device(DEV)
    for K in KS:
        acts = acts_h[:K]
        d = EnvState(B, A, device=DEV, with_episode=False, with_magnitudes=False)
        d.load(start)
        _lib.kernel_override(rollout="trio")
        try:
            r, dn = ops.env_rollout(cfg, dw, d, torch.from_numpy(acts).to(DEV))
            torch.cuda.synchronize()
        finally:
            _lib.kernel_override()
        r, dn = r.cpu().numpy(), dn.cpu().numpy()
        where = f"A={A} {kind} lights={lights} K={K}"
        for t in range(K):
            assert np.array_equal(r[t].view(np.uint32), want_r[t].view(np.uint32)), f"reward: {where} step {t}"
            assert np.array_equal(dn[t], want_d[t]), f"done bytes: {where} step {t}"
        got = d.host()
        for k in _abi.STATE_AGENT_F32 + _abi.STATE_AGENT_I32 + _abi.STATE_AGENT_U8 + ["scn", "steps", "target_idx", "reached",
                                                                                         "terminated", "truncated", "reward"]:
            if k in got and k in want_st[K]:
                assert np.array_equal(got[k].view(np.uint8), want_st[K][k].view(np.uint8)), f"final {k}: {where}"

"""tde_state_copy on the GPU (include/tde_snapshot.h) and what is built on it (torchdriveenv_amd/snapshot.py: snapshot, restore, fork,
EpisodeRecorder, WaypointVecEnv's recording).  Nothing here has a tolerance: a copy moves bytes, a restored env continues bit for bit,
and a recorded frame is the frame the scene renderer gives live."""
import os

import numpy as np
import pytest
import torch

from tests import snapshot_ref as S
from torchdriveenv_amd import _abi, ops
from torchdriveenv_amd.config import EnvConfig, RendererConfig, SimulatorConfig
from torchdriveenv_amd.env import BatchedWaypointEnv
from torchdriveenv_amd.state import EnvState

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xC3
PAIRS = {1: ([3], [5]), 3: ([4, 0, 2], [1, 6, 3]), 5: ([2, 4, 0, 3, 1], [6, 0, 3, 5, 2])}        # src.B = 5, dst.B = 7, scrambled


@pytest.fixture(scope="module")
def worlds():
    from torchdriveenv_amd.synth import synthetic_world

    made = {}

    def get(A, lights=False):
        if (A, lights) not in made:
            made[A, lights] = synthetic_world(n_scn=8, A=A, lights=lights)
        return made[A, lights]
    return get


def fill_random(st, rng):
    """every array of a device state filled with random bytes (NaN payloads, denormals and all)"""
    for a in st.arrays.values():
        if a is not None:
            nb = a.numel() * a.element_size()
            a.view(-1).view(torch.uint8).copy_(torch.from_numpy(rng.integers(0, 256, nb, dtype=np.uint8)))
    # a few chosen float patterns in x: quiet and signalling NaNs with payloads, -0, inf, a denormal
    pat = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x7F800000, 0x00000001], np.uint32).view(np.float32)
    st["x"][:len(pat)] = torch.from_numpy(pat).to(st["x"].device)[:st["x"].numel()]


def fill_canary(st):
    for a in st.arrays.values():
        if a is not None:
            a.view(-1).view(torch.uint8).fill_(CANARY)


def same_bytes(got, want, what):
    for n in _abi.STATE_PTRS:
        if want.get(n) is None:
            assert got.get(n) is None, n
            continue
        assert np.array_equal(got[n].reshape(-1).view(np.uint8), want[n].reshape(-1).view(np.uint8)), (what, n)


def handles_of(binding, world_dev, states):
    """launch handles of `states` in `binding` (None for ctypes: ops.state_copy's default)"""
    if binding == "ctypes":
        return None
    from torchdriveenv_amd import _ext

    cfg = _abi.default_config()
    return tuple(_ext.env_handle(cfg, world_dev, s) for s in states)


VARIANTS = {
    "full": (dict(with_obs=True, with_slot_route=True), dict(with_obs=True, with_slot_route=True)),
    "src_lean": (dict(with_info=False), dict(with_obs=True, with_slot_route=True)),
    "dst_lean": (dict(with_obs=True), dict(with_info=False, with_cache=False)),
}


# ---- every byte -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binding", ("ctypes", "ext"))
@pytest.mark.parametrize("A", (4, 16, 128))
def test_every_byte_of_every_array(worlds, A, binding):
    rng = np.random.default_rng(A)
    wd = worlds(A).to_device(DEV) if binding == "ext" else None
    for name, (skw, dkw) in VARIANTS.items():
        src, dst = EnvState(5, A, device=DEV, **skw), EnvState(7, A, device=DEV, **dkw)
        fill_random(src, rng)
        h = handles_of(binding, wd, (src, dst))
        src_host = src.host()
        for n, (se, de) in PAIRS.items():
            for outputs in (False, True):
                fill_canary(dst)
                want = S.state_copy(src_host, dst.host(), 5, 7, A, se, de, outputs)
                ops.state_copy(src, dst, se, de, outputs=outputs, check=True, handles=h)
                got = dst.host()
                same_bytes(got, want, (name, n, outputs))
                rest = [r for r in range(7) if r not in de]
                for k, a in got.items():                  # untouched rows keep the canary, every array
                    assert (S.rows(a, 7)[rest] == CANARY).all(), (name, k)
                if dst["act_cache"] is not None:
                    assert got["act_cache"].reshape(7, A + 1, 2)[de[0]].tolist() == [[0, 0]] * A + [[-1, 0]]
                    assert not got["slot_cache"].reshape(7, -1)[de].any() and not got["env_cache"][de].any()
        same_bytes(src.host(), src_host, "the source is read only")


@pytest.mark.parametrize("binding", ("ctypes", "ext"))
@pytest.mark.parametrize("ns,plane", ((1, 4096), (3, 4096), (1, 256), (3, 256)))
def test_frames_land_in_the_slot_of_the_same_age(worlds, ns, plane, binding):
    rng = np.random.default_rng(ns * plane)
    A = 4
    src, dst = EnvState(5, A, device=DEV), EnvState(7, A, device=DEV)
    fill_random(src, rng)
    h = handles_of(binding, worlds(A).to_device(DEV) if binding == "ext" else None, (src, dst))
    sl = torch.from_numpy(rng.integers(0, 256, (5, ns, plane), dtype=np.uint8)).to(DEV)
    so = torch.from_numpy(rng.integers(0, 256, (5, 3 * ns, plane), dtype=np.uint8)).to(DEV)
    se, de = PAIRS[3]
    for sp in range(ns):
        for dp in range(ns):
            for layers, obs in ((True, True), (False, True), (True, False)):
                dl, do = torch.full((7, ns, plane), CANARY, dtype=torch.uint8, device=DEV), torch.full((7, 3 * ns, plane), CANARY, dtype=torch.uint8, device=DEV)
                fr = ops.snapshot_frames(sl if layers else None, dl if layers else None, so if obs else None, do if obs else None, ns, plane, sp, dp)
                ops.state_copy(src, dst, se, de, frames=fr, check=False, handles=h)
                wl, wo = np.full((7, ns, plane), CANARY, np.uint8), np.full((7, 3 * ns, plane), CANARY, np.uint8)
                S.frames_copy(sl.cpu().numpy() if layers else None, wl if layers else None, so.cpu().numpy() if obs else None,
                              wo if obs else None, ns, sp, dp, se, de)
                assert np.array_equal(dl.cpu().numpy(), wl) and np.array_equal(do.cpu().numpy(), wo), (sp, dp, layers, obs)


def test_pairs_out_of_range_are_skipped_without_the_check():
    rng = np.random.default_rng(11)
    A = 16
    src, dst = EnvState(5, A, device=DEV), EnvState(7, A, device=DEV)
    fill_random(src, rng)
    fill_canary(dst)
    sl = torch.from_numpy(rng.integers(0, 256, (5, 3, 256), dtype=np.uint8)).to(DEV)
    dl = torch.full((7, 3, 256), CANARY, dtype=torch.uint8, device=DEV)
    se, de = [0, 5, -1, 2, 1, 2**31 - 1, 3], [1, 2, 3, 7, -2, 0, 4]                   # valid: (0, 1) and (3, 4)
    assert S.valid_pairs(se, de, 5, 7) == [(0, 1), (3, 4)]
    want = S.state_copy(src.host(), dst.host(), 5, 7, A, se, de, True)
    ops.state_copy(src, dst, se, de, frames=ops.snapshot_frames(sl, dl, None, None, 3, 256, 2, 0), outputs=True, check=False)
    got = dst.host()
    same_bytes(got, want, "skip")
    for k, a in got.items():
        assert (S.rows(a, 7)[[0, 2, 3, 5, 6]] == CANARY).all(), k
    wl = np.full((7, 3, 256), CANARY, np.uint8)
    S.frames_copy(sl.cpu().numpy(), wl, None, None, 3, 2, 0, se, de)
    assert np.array_equal(dl.cpu().numpy(), wl) and (wl[[0, 2, 3, 5, 6]] == CANARY).all()
    with pytest.raises(RuntimeError, match="dst_env index is outside"):              # the same call under the check: refused, nothing written
        ops.state_copy(src, dst, [0, 1], [1, 7], check=True)
    with pytest.raises(RuntimeError, match="names a row twice"):
        ops.state_copy(src, dst, [0, 1], [2, 2], check=True)
    same_bytes(dst.host(), got, "a refused call writes nothing")


def test_fork_within_one_state():
    rng = np.random.default_rng(5)
    A = 16
    st = EnvState(6, A, device=DEV, with_obs=True)
    fill_random(st, rng)
    lay = torch.from_numpy(rng.integers(0, 256, (6, 3, 256), dtype=np.uint8)).to(DEV)
    obs = torch.from_numpy(rng.integers(0, 256, (6, 9, 256), dtype=np.uint8)).to(DEV)
    before, lay0, obs0 = st.host(), lay.cpu().numpy(), obs.cpu().numpy()
    want = S.state_copy(before, st.host(), 6, 6, A, [2, 2, 2], [5, 0, 3], True)
    ops.state_copy(st, st, [2, 2, 2], [5, 0, 3], frames=ops.snapshot_frames(lay, lay, obs, obs, 3, 256, 1, 1), outputs=True, check=True)
    got = st.host()
    same_bytes(got, want, "fork")
    for k in _abi.SNAPSHOT_COPIED + _abi.SNAPSHOT_OUTPUT_ARRAYS:
        if k not in got:
            continue                                         # (this state carries no slot_route)
        r, b = S.rows(got[k], 6), S.rows(before[k], 6)
        assert np.array_equal(r[[1, 2, 4]], b[[1, 2, 4]]) and all(np.array_equal(r[d], b[2]) for d in (5, 0, 3)), k
    for k in _abi.SNAPSHOT_INVALIDATED:                      # the source row's caches are left alone
        assert np.array_equal(S.rows(got[k], 6)[[1, 2, 4]], S.rows(before[k], 6)[[1, 2, 4]]), k
    for a, a0 in ((lay.cpu().numpy(), lay0), (obs.cpu().numpy(), obs0)):
        assert np.array_equal(a[[1, 2, 4]], a0[[1, 2, 4]]) and all(np.array_equal(a[d], a0[2]) for d in (5, 0, 3))
    with pytest.raises(RuntimeError, match="overlaps src_env"):
        ops.state_copy(st, st, [2, 2], [5, 2], check=True)


# ---- continuation: the test that cannot pass without the feature ---------------------------------------------------------------------
B = 6


def make_env(world, frame_stack=3, max_steps=6, res=64, **kw):
    cfg = EnvConfig(seed=7, distance_cutoff=0.25, max_environment_steps=max_steps, frame_stack=frame_stack,
                    simulator=SimulatorConfig(renderer=RendererConfig(res=res)))
    return BatchedWaypointEnv(cfg, world, num_envs=B, device=DEV, obs_mode=kw.pop("obs_mode", "birdview"), frame_stack=frame_stack, **kw)


def action_table(n, seed=3):
    rng = np.random.default_rng(seed)
    a = np.stack([rng.uniform(-1, 1, (n, B)), rng.uniform(-0.3, 0.3, (n, B))], -1).astype(np.float32)
    a[:, 0] = np.array([1.0, 0.3], np.float32)               # env 0 drives at the limits: infractions end episodes too
    return torch.from_numpy(a).to(DEV)


def record(env, obs):
    """everything a step leaves, cloned: the state's arrays (caches aside) and the observation"""
    d = {k: v.clone() for k, v in env.state.arrays.items() if v is not None and k not in _abi.SNAPSHOT_INVALIDATED}
    d["_obs"] = obs.clone()
    if env.terminal_frames is not None:
        d["_terminal"] = env.terminal_frames.clone()
    return d


def same_rows(a, b, rows, A, what):
    for k in a:
        x, y = a[k].reshape(B, -1)[rows], b[k].reshape(B, -1)[rows]
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), (what, k)


CONTINUATION = {"A16": dict(A=16), "A128": dict(A=128), "lights": dict(A=16, lights=True), "terminal_obs": dict(A=16, terminal_obs=True),
                "ctypes": dict(A=16, binding="ctypes")}


@pytest.mark.parametrize("case", list(CONTINUATION))
def test_a_restored_env_continues_bit_for_bit_through_respawns(worlds, case):
    kw = dict(CONTINUATION[case])
    world = worlds(kw.pop("A"), kw.pop("lights", False))
    acts = action_table(15)
    env, twin = make_env(world, **kw), make_env(world, **kw)
    for e in (env, twin):
        e.reset()
        for t in range(5):
            e.step(acts[t])
    keep = [1, 4]
    snap = env.snapshot(keep)
    assert snap.envs == keep and snap.B == 2 and snap["slot_cache"] is None and snap.layers is not None
    first = []
    for t in range(5, 14):
        first.append(record(env, env.step(acts[t])[0]))
        twin.step(acts[t])
    assert sum(int(r["done_bits"][keep].bool().sum()) for r in first) >= 2       # the window crosses re-spawns of the kept envs
    assert int(first[-1]["episode"][keep].min()) > int(snap["episode"].min())
    obs = env.restore(snap)
    assert torch.equal(obs[keep], snap.obs.view(2, *obs.shape[1:]))
    others = [0, 2, 3, 5]
    same_rows(record(env, obs), first[-1], others, env.A, "restore leaves the other envs alone")
    for i, t in enumerate(range(5, 14)):
        mixed = acts[t].clone()
        mixed[others] = acts[14][others]                     # the other envs do something else this time round
        got = record(env, env.step(mixed)[0])
        same_rows(got, first[i], keep, env.A, f"{case}: step {t} after the restore")
        if i == 0:
            # the other envs: their next step equals that of an env that ran the same 14 steps and this one, with no restore
            want = record(twin, twin.step(mixed)[0])
            same_rows(got, want, others, env.A, "the others' next step")


def test_a_fork_continues_like_its_source_until_it_respawns(worlds):
    world = worlds(16)
    acts = action_table(12)
    env = make_env(world, max_steps=9)
    env.reset()
    for t in range(3):
        env.step(acts[t])
    before = record(env, env.observer.obs)
    obs = env.fork(2, [5, 0])
    after = record(env, obs)
    same_rows(after, before, [1, 2, 3, 4], env.A, "fork leaves the others alone")
    for d in (5, 0):
        for k in after:
            assert torch.equal(after[k].reshape(B, -1)[d], before[k].reshape(B, -1)[2]), k
    for t in range(3, 12):
        a = acts[t].clone()
        a[[5, 0]] = a[2].clone()
        rec = record(env, env.step(a)[0])
        done = bool(rec["done_bits"][2] & 3)
        for d in (5, 0):                                     # compared up to and including the step that ends the episode
            for k in rec:
                if done and k not in ("reward", "terminated", "truncated", "tl_violation", "done_bits", "info", "info_reached", "ep_final",
                                      "ep_final_len", "magnitudes", "action"):
                    continue                                 # (the re-spawn of that step already draws from the env's own index)
                assert torch.equal(rec[k].reshape(B, -1)[d], rec[k].reshape(B, -1)[2]), (t, k)
        if done:
            assert t > 3
            return
    raise AssertionError("the source env never finished an episode: the window is too short")


# ---- stale caches: why the invalidation exists ----------------------------------------------------------------------------------------
def test_a_restored_row_with_equal_counters_and_other_poses_steps_like_the_oracle(worlds):
    from oracle import oracle

    world = worlds(16)
    A, Bn = 16, 4
    cfg = _abi.default_config(seed=5, distance_cutoff=0.25, max_steps=50)
    dw = world.to_device(DEV)
    live, other = EnvState(Bn, A, device=DEV), EnvState(Bn, A, device=DEV)
    assert live["act_cache"] is not None and live["slot_cache"] is not None
    rng = np.random.default_rng(2)
    acts = torch.from_numpy(np.stack([rng.uniform(-1, 1, (5, Bn)), rng.uniform(-0.3, 0.3, (5, Bn))], -1).astype(np.float32)).to(DEV)
    for st in (live, other):
        ops.env_reset(cfg, dw, st)
        for t in range(3):
            ops.env_step(cfg, dw, st, acts[t])
    # the row to restore: the same counters, other poses (every agent slower and turned)
    other["v"].mul_(0.5)
    other["psi"].add_(0.05)
    other["x"].add_(0.75)
    torch.cuda.synchronize()
    assert torch.equal(live["episode"], other["episode"]) and torch.equal(live["steps"], other["steps"]) and not torch.equal(live["v"], other["v"])

    def oracle_step(host_arrays):
        hs = EnvState(Bn, A)
        hs.load(host_arrays)
        v0 = hs["v"].copy()
        hs["action"][...] = acts[3].cpu().numpy()
        oracle.env_step(cfg, world, hs)
        return hs.host(), hs["v"] - v0

    old, dv_old = oracle_step(live.host())
    rows = [1, 2]
    ops.state_copy(other, live, rows, rows, outputs=True, check=True)
    want, dv_new = oracle_step(live.host())
    npc = np.arange(Bn * A).reshape(Bn, A)[rows, 1:].reshape(-1)
    assert not np.array_equal(dv_old[npc], dv_new[npc])      # the NPC actions of the old poses are not those of the restored ones
    host = live.host()
    assert host["act_cache"].reshape(Bn, A + 1, 2)[rows, A, 0].tolist() == [-1, -1] and host["act_cache"].reshape(Bn, A + 1, 2)[0, A, 0] >= 0
    ops.env_step(cfg, dw, live, acts[3])
    got = live.host()
    for k, w in want.items():
        if k != "action" and k not in _abi.SNAPSHOT_INVALIDATED:
            assert np.array_equal(got[k].reshape(-1).view(np.uint8), w.reshape(-1).view(np.uint8)), k


# ---- the recorder --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,camera", ((64, 64, "map"), (96, 80, "ego")))
def test_recorded_frames_equal_live_frames(worlds, tmp_path, H, W, camera):
    world = worlds(16)
    acts = action_table(6)
    env = make_env(world)
    envs = [4, 0, 3]
    env.reset()
    start = env.snapshot(list(range(B)))
    rec = env.recorder(envs, video_length=7)
    assert rec.capture()
    for t in range(6):
        env.step(acts[t])
        assert rec.capture()
    assert len(rec) == 7 and not rec.capture() and len(rec) == 7
    got = rec.frames(H=H, W=W, fov=120.0, camera=camera, chunk=3)
    assert tuple(got.shape) == (7, 3, 3, H, W)
    # the live frames, in a second pass from the restored snapshot
    env.restore(start)
    live = [env.render_scene(envs, H, W, 120.0, camera).clone()]
    for t in range(6):
        env.step(acts[t])
        live.append(env.render_scene(envs, H, W, 120.0, camera).clone())
    assert torch.equal(got, torch.stack(live))
    assert len({bytes(f.cpu().numpy().tobytes()) for f in got[:, 0]}) > 1          # the frames move
    one = rec.frames(H=H, W=W, fov=120.0, camera=camera, env=1)
    assert torch.equal(one[:, 0], got[:, 1])
    # tiles
    from torchdriveenv_amd.snapshot import tile_frames

    tiled = tile_frames(got).cpu().numpy()
    want = np.zeros((7, 3, 2 * H, 2 * W), np.uint8)
    g = got.cpu().numpy()
    want[:, :, :H, :W], want[:, :, :H, W:], want[:, :, H:, :W] = g[:, 0], g[:, 1], g[:, 2]
    assert np.array_equal(tiled, want)
    # files
    try:
        import cv2  # noqa: F401
        writer = True
    except ImportError:
        try:
            import PIL  # noqa: F401
            writer = True
        except ImportError:
            writer = False
    if not writer:
        with pytest.raises(ImportError, match="needs cv2"):
            rec.save(str(tmp_path / "a.mp4"), env=0, H=H, W=W, fov=120.0, camera=camera)
        return
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for kw in (dict(env=2), dict(tile=True)):
            path = rec.save(str(tmp_path / f"a{len(kw)}{'t' if 'tile' in kw else ''}.mp4"), H=H, W=W, fov=120.0, camera=camera, **kw)
            assert os.path.exists(path) and os.path.getsize(path) > 0
            if path.endswith(".gif"):
                from PIL import Image

                im = Image.open(path)
                assert im.n_frames == 7 and im.size == ((2 * W, 2 * H) if "tile" in kw else (W, H))


def test_vec_env_records_at_the_triggered_step_only(worlds, tmp_path):
    import warnings

    world = worlds(16)
    folder = tmp_path / "videos"
    env = make_env(world, frame_stack=1)
    vec = env.as_vec_env(record_video_trigger=lambda step: step == 2, video_length=3, video_folder=str(folder))
    acts = action_table(8).cpu().numpy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vec.reset()
        for t in range(2):
            vec.step(acts[t])
            assert not folder.exists()
        vec.step(acts[2])
        vec.step(acts[3])                                    # frames of steps 2, 3, 4: the file is written with the third
        made = sorted(os.listdir(folder))
        assert len(made) == 1 and made[0].startswith("rl-video-step-2-to-step-5")
        for t in range(4, 8):
            vec.step(acts[t])
        vec.close()
    assert sorted(os.listdir(folder)) == made and vec.recording.files == [str(folder / made[0])]
    if made[0].endswith(".gif"):
        from PIL import Image

        assert Image.open(folder / made[0]).n_frames == 3
    plain = make_env(world, frame_stack=1).as_vec_env()
    assert plain.recording is None


# ---- side effects ----------------------------------------------------------------------------------------------------------------------
def test_snapshot_and_capture_leave_the_env_untouched(worlds):
    world = worlds(16)
    env = make_env(world)
    acts = action_table(3)
    obs = env.reset()
    for t in range(3):
        obs = env.step(acts[t])[0]
    buf = env.replay_buffer(8)
    draws = buf.draws
    before = {k: v.clone() for k, v in env.state.arrays.items() if v is not None}
    obs0, lay0, phase0 = obs.clone(), env.observer.stack.layers.clone(), env.observer.stack.phase
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    snap = env.snapshot([0, 5, 2])
    rec = env.recorder([1, 3], video_length=4)
    rec.capture()
    assert torch.cuda.memory_allocated() > mem               # they allocate when made - and only then
    for k, v in before.items():                              # every array, the caches included: nothing of the live state moved
        assert torch.equal(v.view(-1).view(torch.uint8), env.state.arrays[k].view(-1).view(torch.uint8)), k
    assert torch.equal(obs0, env.observer.obs) and torch.equal(lay0, env.observer.stack.layers) and env.observer.stack.phase == phase0 and buf.draws == draws
    # and the snapshot holds the rows
    for k in _abi.SNAPSHOT_COPIED + _abi.SNAPSHOT_OUTPUT_ARRAYS:
        if before.get(k) is not None:
            assert torch.equal(snap[k].reshape(3, -1), before[k].reshape(B, -1)[[0, 5, 2]]), k
    assert torch.equal(snap.obs, obs0[[0, 5, 2]])
    ph = phase0
    for age in range(1, 4):                                  # the snapshot's ring stands at phase 0
        assert torch.equal(snap.layers[:, (0 - age) % 3], lay0[[0, 5, 2], (ph - age) % 3])


def test_restore_refuses_a_snapshot_that_does_not_fit(worlds):
    world = worlds(16)
    env = make_env(world)
    env.reset()
    snap = env.snapshot([0, 1])
    with pytest.raises(ValueError, match="holds 2 rows"):
        env.restore(snap, envs=[0])
    with pytest.raises(ValueError, match=r"must be in \[0, 6\)"):
        env.restore(snap, envs=[0, 6])
    with pytest.raises(ValueError, match="names an env twice"):
        env.snapshot([1, 1])
    other = make_env(world, frame_stack=1)
    other.reset()
    with pytest.raises(ValueError, match="do not fit this env"):
        other.restore(snap)
    lean = make_env(world, with_info=False)
    lean.reset()
    with pytest.raises(ValueError, match="'info'"):
        lean.restore(snap)
    with pytest.raises(ValueError, match="src_env"):
        env.fork(1, [2, 1])
    env.restore(snap, envs=[3, 5])                           # another index is fine
    assert torch.equal(env.state["x"].reshape(B, -1)[[3, 5]], snap["x"].reshape(2, -1))

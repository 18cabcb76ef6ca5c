"""Terminal observations on the GPU (include/tde_terminal.h; BatchedWaypointEnv(terminal_obs=True), ReplayBuffer, RolloutBuffer).  Nothing
here has a tolerance: a terminal_obs env must return what its twin without the option returns, bit for bit; the frame it keeps must be
the observation an env without auto-reset shows at that step; and every sample must equal the numpy restatement (tests/terminal_ref.py)
and the step log."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import onpolicy_ref as O
from tests import replay_ref as R
from tests import terminal_ref as T
from torchdriveenv_amd import _abi, _lib, ops
from torchdriveenv_amd.config import EnvConfig, RendererConfig, SimulatorConfig, VectorObs
from torchdriveenv_amd.env import BatchedWaypointEnv

pytestmark = pytest.mark.gpu
B, DEV, CUT, HAS = 5, "cuda:0", _abi.REPLAY_CUT, _abi.TERMINAL_HAS
FIELDS = ("observations", "next_observations", "actions", "rewards", "dones", "indices")
PAL = np.array(_abi.PALETTE, np.uint8)
MODES = [("birdview", 3, {}), ("birdview", 1, {}), ("vector", 1, dict(vector_obs=VectorObs(k_neighbours=2, n_rays=4))), ("state", 1, {})]
MODE_IDS = ["birdview3", "birdview1", "vector", "state"]


@pytest.fixture(scope="module")
def world():
    from torchdriveenv_amd.synth import synthetic_world

    return synthetic_world(n_scn=4, A=4)


def make_env(world, obs_mode="birdview", frame_stack=3, max_steps=5, seed=7, **kw):
    cfg = EnvConfig(seed=seed, distance_cutoff=0.25, max_environment_steps=max_steps, frame_stack=frame_stack,
                    simulator=SimulatorConfig(renderer=RendererConfig(res=64)))
    return BatchedWaypointEnv(cfg, world, num_envs=B, device=DEV, obs_mode=obs_mode, frame_stack=frame_stack, **kw)


def actions(rng):
    """[B, 2] within the action space; envs 0 and 1 steer and accelerate at the limits, so that infractions end episodes too"""
    a = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)
    a[:2] = np.where(rng.uniform(size=(2, 2)) < 0.5, -1.0, 1.0) * np.array([1.0, 0.3])
    return a.astype(np.float32)


def same(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8))


def same_tree(a, b, path=""):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), path
        for k in a:
            same_tree(a[k], b[k], f"{path}/{k}")
    elif torch.is_tensor(a):
        assert same(a, b), path
    else:
        assert a == b, path


# ---- 1. twin equality -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs_mode,frame_stack,kw", MODES, ids=MODE_IDS)
def test_step_equals_the_env_without_the_option(world, obs_mode, frame_stack, kw):
    plain, term = make_env(world, obs_mode, frame_stack, **kw), make_env(world, obs_mode, frame_stack, terminal_obs=True, **kw)
    assert same(plain.reset(), term.reset())
    rng = np.random.default_rng(0)
    n_done = 0
    for k in range(12):
        a = torch.from_numpy(actions(rng)).to(DEV)
        r0, r1 = plain.step(a), term.step(a)
        for x, y in zip(r0[:4], r1[:4]):
            assert same(x, y), k
        i0, i1 = r0[4], r1[4]
        assert sorted(i0.keys()) == sorted(i1.keys())
        for key in i0.keys():
            assert same(torch.as_tensor(i0[key]), torch.as_tensor(i1[key])), (k, key)
        s0, s1 = plain.state_dict(), term.state_dict()
        s1.pop("_terminal_frames")
        assert "done_bits" in s0 and "ep_final" in s0 and "ep_final_len" in s0
        same_tree(s0, s1, f"step {k}")
        n_done += int(((plain.state["done_bits"] & 3) != 0).sum())
    assert n_done >= 2 * B                                  # every env ran out of steps twice
    assert int(term.tde_cfg.flags) == int(plain.tde_cfg.flags) and term.auto_reset
    with pytest.raises(ValueError, match="terminal_obs env"):
        term.rollout(torch.zeros((2, B, 2), device=DEV))


# ---- 2. the stored frame is the terminal frame ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs_mode,frame_stack,kw", MODES, ids=MODE_IDS)
def test_the_stored_frame_is_what_an_env_without_auto_reset_shows(world, obs_mode, frame_stack, kw):
    term = make_env(world, obs_mode, frame_stack, terminal_obs=True, **kw)
    oracle = make_env(world, obs_mode, frame_stack, auto_reset=False, **kw)
    buf = term.replay_buffer(8, seed=1, terminal_per_step=B)
    assert same(term.reset(), oracle.reset())
    buf.begin()
    canary = term.terminal_frames.clone()
    rng = np.random.default_rng(0)
    over = np.zeros(B, bool)
    for k in range(6):
        a = torch.from_numpy(actions(rng)).to(DEV)
        term.step(a)
        buf.push(a)
        want = oracle.step(a)[0].cpu().numpy()
        db = term.state["done_bits"].cpu().numpy()
        first = ((db & 3) != 0) & ~over
        kept = term.terminal_frames.cpu().numpy()
        # the envs that did not finish at this step keep their entry
        assert np.array_equal(kept[(db & 3) == 0], canary.cpu().numpy()[(db & 3) == 0])
        canary = term.terminal_frames.clone()
        if first.any():
            e = np.flatnonzero(first)
            newest = R.layers_of_rgb(want[e][:, -3:].reshape(len(e), 3, -1)) if obs_mode == "birdview" else want[e]
            assert np.array_equal(kept[e].view(np.uint8), np.ascontiguousarray(newest).view(np.uint8)), k
            idx = torch.from_numpy(np.stack([np.full(len(e), (buf.w - 1) % buf.C), e], 1).astype(np.int32))
            s = buf.sample(None, idx=idx)
            assert np.array_equal(s.next_observations.cpu().numpy().view(np.uint8), want[e].view(np.uint8)), k
            assert ((s.dones.cpu().numpy() & HAS) != 0).all()
        over |= first
    assert over.all()


# ---- 3. the buffer against the numpy ring and the step log ---------------------------------------------------------------------------
class Run:
    """a terminal_obs env with a buffer attached, everything step() returned and the terminal frames logged on the host, and the numpy
    ring fed the same frames"""

    def __init__(self, env, capacity, M, seed=3):
        self.env, self.buf = env, env.replay_buffer(capacity, seed=seed, terminal_per_step=M)
        self.rng = np.random.default_rng(seed)
        self.obs, self.act, self.rew, self.db, self.term = [], [], [], [], []
        self.planes = env.obs_mode == "birdview"
        ns = env.frame_stack if self.planes else 1
        M = self.buf.M
        self.ref = T.TerminalRing(capacity, B, M, ns, plane=64 * 64) if self.planes else T.TerminalRing(capacity, B, M, D=env.observation_space.shape[0])
        self.reset()

    def frame(self, obs):
        return R.layers_of_rgb(obs[:, -3:].reshape(B, 3, -1)) if self.planes else obs

    def reset(self, mask=None):
        dmask = None if mask is None else torch.from_numpy(mask).to(DEV)
        obs = self.env.reset(mask=dmask).cpu().numpy().copy()
        self.buf.begin(mask=dmask)
        if mask is None:
            self.obs.append(obs)
        else:
            self.obs[-1] = obs
        self.ref.begin(self.frame(obs), mask)

    def step(self, n=1):
        for _ in range(n):
            a = actions(self.rng)
            ta = torch.from_numpy(a).to(DEV)
            obs, rew, *_ = self.env.step(ta)
            self.buf.push(ta)
            self.obs.append(obs.cpu().numpy().copy())
            self.act.append(a)
            self.rew.append(rew.cpu().numpy().copy())
            self.db.append(self.env.state["done_bits"].cpu().numpy().copy())
            self.term.append(self.env.terminal_frames.cpu().numpy().copy())
            self.ref.push(a, self.rew[-1], self.db[-1], self.frame(self.obs[-1]), self.term[-1])

    def check_all(self, cut=None):
        buf, ref, n_t = self.buf, self.ref, len(self.act)
        assert (buf.first, buf.w, buf.count) == (ref.first, ref.w, ref.count)
        assert np.array_equal(buf.ref.cpu().numpy(), ref.ref)
        pairs = ref.valid_pairs()
        assert np.array_equal(buf.valid_pairs().cpu().numpy(), pairs) and len(pairs)
        s = buf.sample(None, idx=torch.from_numpy(pairs))
        got = {k: getattr(s, k).cpu().numpy() for k in FIELDS}
        want = ref.gather(pairs)
        for k in FIELDS:
            assert np.array_equal(got[k].reshape(want[k].shape).view(np.uint8), want[k].view(np.uint8)), k
        slot, e = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
        t = n_t - 1 - ((buf.w - 1 - slot) % buf.C)
        obs, db, term = np.stack(self.obs), np.stack(self.db), np.stack(self.term)
        cutm = np.zeros(len(t), bool) if cut is None else cut(t, e)
        fin = (db[t, e] & 3) != 0
        has = fin & (ref.ref[slot, e] >= 0)
        assert np.array_equal(got["dones"], db[t, e] | np.where(cutm, CUT, 0).astype(np.uint8) | np.where(has, HAS, 0).astype(np.uint8))
        assert np.array_equal(got["observations"].view(np.uint8), obs[t, e].view(np.uint8))
        ended = fin | cutm
        assert np.array_equal(s.terminal.cpu().numpy(), ended)
        assert np.array_equal(s.bootstrap.cpu().numpy(), ~ended | (has & ((db[t, e] & 3) == 2)))
        nxt = got["next_observations"]
        if self.planes:
            n = int(has.sum())
            assert np.array_equal(nxt[has][:, -3:].reshape(n, 3, 64 * 64), PAL[term[t, e][has]].transpose(0, 2, 1))
            assert np.array_equal(nxt[has][:, :-3], got["observations"][has][:, 3:])
        else:
            assert np.array_equal(nxt[has].view(np.uint8), term[t, e][has].view(np.uint8))
        assert np.array_equal(nxt[~ended].view(np.uint8), obs[t + 1, e][~ended].view(np.uint8))
        assert not nxt[ended & ~has].view(np.uint8).any()
        return got, t, e, has


@pytest.mark.parametrize("M", [B, 2])
def test_samples_against_the_numpy_ring_and_the_log(world, M):
    run = Run(make_env(world, terminal_obs=True), 8, M)
    n_trunc = n_term = n_open = n_over = 0
    at = 0
    for upto in (3, 8, 12, 17, 24, 30):
        run.step(upto - at)
        at = upto
        got, t, e, has = run.check_all()
        d = got["dones"]
        n_trunc += int((has & ((d & 3) == 2)).sum())
        n_term += int((has & ((d & 1) != 0)).sum())
        n_open += int(((d & (3 | CUT)) == 0).sum())
        n_over += int((((d & 3) != 0) & ~has).sum())
    assert run.buf.count == 7 and len(run.act) // 8 == 3    # the ring wrapped three times
    print(f"M = {M}: truncated with frame {n_trunc}, terminated with frame {n_term}, not ended {n_open}, overflowed {n_over}")
    assert n_trunc > 0 and n_term > 0 and n_open > 0
    assert (n_over > 0) == (M < B)


@pytest.mark.parametrize("obs_mode,frame_stack,kw", MODES[1:], ids=MODE_IDS[1:])
def test_samples_in_the_other_modes(world, obs_mode, frame_stack, kw):
    run = Run(make_env(world, obs_mode, frame_stack, terminal_obs=True, **kw), 6, B)
    n_has = 0
    for upto in (2, 15):
        run.step(upto - len(run.act))
        n_has += int(run.check_all()[3].sum())
    assert n_has > 0
    # a checkpoint carries the pool: a reloaded buffer gathers the same bytes
    other = run.env.replay_buffer(6, seed=9, terminal_per_step=B)
    other.load_state_dict(run.buf.state_dict())
    pairs = torch.from_numpy(run.ref.valid_pairs())
    a, b = run.buf.sample(None, idx=pairs), other.sample(None, idx=pairs)
    assert all(same(getattr(a, f), getattr(b, f)) for f in FIELDS)
    env2 = make_env(world, obs_mode, frame_stack, terminal_obs=True, **kw)
    env2.reset()
    env2.load_state_dict(run.env.state_dict())
    assert same(env2.terminal_frames, run.env.terminal_frames)
    with pytest.raises(ValueError, match="with terminal frames, this buffer is without"):
        make_env(world, obs_mode, frame_stack, **kw).replay_buffer(6).load_state_dict(run.buf.state_dict())


# ---- 4. overflow and rank boundaries through the C-ABI alone ---------------------------------------------------------------------------
MASKS = {"none": [], "all": list(range(130)), "last": [129], "wave_edge": [63, 64, 65]}
# more than one workgroup of tde_terminal_stash / tde_terminal_push (256 envs each), B no multiple of 256: the ranks of a workgroup start
# at the number of finished envs in front of it, and "spread" overflows M = 4 exactly at a workgroup's first env
MASKS_WG = {"none": [], "all": list(range(600)), "last": [599], "wg_edge_1": [255, 256, 257], "wg_edge_2": [511, 512, 513],
            "spread": [0, 100, 255, 256, 300, 511, 512, 599]}


def c_abi_case(Bn, M, masks, plane, n_stack, D, sample_envs=None):
    """a ring filled by hand through the C-ABI, one push per done mask, held to the restatement after every push: the masked copy into
    a guarded store, ref, pool, the canaries behind them, then (slot, env) pairs through tde_terminal_sample (sample_envs: of those
    envs; None: of all).  Returns the restatement."""
    Cn = len(masks) + 1
    L = _lib.load()
    rng = np.random.default_rng(plane + n_stack + D + Bn)
    ring = T.TerminalRing(Cn, Bn, M, n_stack, plane=plane, D=D)
    per, dt = (plane, torch.uint8) if plane else (D, torch.float32)
    guard = 64
    frames = torch.zeros((Cn, Bn, per), dtype=dt, device=DEV)
    action, reward = torch.zeros((Cn, Bn, 2), device=DEV), torch.zeros((Cn, Bn), device=DEV)
    done, age = torch.zeros((Cn, Bn), dtype=torch.uint8, device=DEV), torch.zeros((Cn, Bn), dtype=torch.uint8, device=DEV)
    pool_g = torch.full((Cn * M * per + guard,), 7, dtype=dt, device=DEV)
    ref_g = torch.full((Cn * Bn + guard,), -77, dtype=torch.int32, device=DEV)
    pool, ref = pool_g[:Cn * M * per].view(Cn, M, per), ref_g[:Cn * Bn].view(Cn, Bn)
    ring.pool[...] = 7
    ring.ref[...] = -77
    rp = ops.replay_struct(Cn, Bn, n_stack, plane, D, frames, action, reward, done, age)
    tm = ops.terminal_struct(rp, M, pool, ref)

    def rows(lo):
        return rng.integers(0, 8, (Bn, per)).astype(np.uint8) if plane else (rng.standard_normal((Bn, per)) + lo).astype(np.float32)

    f0 = rows(0)
    ops.replay_begin(rp, DEV, 0, torch.from_numpy(f0).to(DEV))
    ring.begin(f0)
    stream = _lib.current_stream(torch.device(DEV))
    for w, (name, envs) in enumerate(masks.items()):
        db = np.zeros(Bn, np.uint8)
        db[envs] = [1 + (k % 3) for k in range(len(envs))]
        db |= (rng.integers(0, 8, Bn) << 2).astype(np.uint8)            # infraction bits alone finish nothing
        a, r, nxt, term = rng.standard_normal((Bn, 2)).astype(np.float32), rng.standard_normal(Bn).astype(np.float32), rows(1), rows(2)
        ta, tr, td = torch.from_numpy(a).to(DEV), torch.from_numpy(r).to(DEV), torch.from_numpy(db).to(DEV)
        tterm = torch.from_numpy(term).to(DEV)
        # the masked copy, into a guarded store
        store_g = torch.full(((Bn + 2) * per,), 9, dtype=dt, device=DEV)
        store = store_g[per:-per].view(Bn, per)
        ops.terminal_stash(DEV, td, tterm, 0, per * tterm.element_size(), store)
        fin = (db & 3) != 0
        sh = store.cpu().numpy()
        assert np.array_equal(sh[fin], term[fin]) and (sh[~fin] == 9).all() and (store_g[:per] == 9).all() and (store_g[-per:] == 9).all(), name
        ops.replay_push(rp, DEV, w, ta, tr, td, torch.from_numpy(nxt).to(DEV))
        assert L.tde_terminal_push(C.byref(rp), C.byref(tm), w, td.data_ptr(), tterm.data_ptr(), per * tterm.element_size(), stream) == 0
        ring.push(a, r, db, nxt, term)
        assert np.array_equal(ref.cpu().numpy(), ring.ref), name
        assert np.array_equal(pool.cpu().numpy().view(np.uint8), ring.pool.view(np.uint8)), name
        assert ring.ref[w].max() == min(len(envs), M) - 1
    # the canaries behind pool and ref
    assert (pool_g[Cn * M * per:] == 7).all() and (ref_g[Cn * Bn:] == -77).all()
    # stored pairs through tde_terminal_sample
    assert (ring.first, ring.w, ring.count) == (0, Cn - 1, Cn - 1)
    pairs = np.array([(s, e) for s in range(Cn - 1) for e in (range(Bn) if sample_envs is None else sample_envs)], np.int32)
    n = len(pairs)
    shape = (n, 3 * n_stack, plane) if plane else (n, D)
    out = {"observations": torch.empty(shape, dtype=dt, device=DEV), "next_observations": torch.empty(shape, dtype=dt, device=DEV),
           "actions": torch.empty((n, 2), device=DEV), "rewards": torch.empty(n, device=DEV),
           "dones": torch.empty(n, dtype=torch.uint8, device=DEV), "indices": torch.empty((n, 2), dtype=torch.int32, device=DEV)}
    ops.terminal_sample(rp, tm, DEV, 0, Cn - 1, n, out, torch.from_numpy(pairs).to(DEV))
    want = ring.gather(pairs)
    for k in FIELDS:
        assert np.array_equal(out[k].cpu().numpy().reshape(want[k].shape).view(np.uint8), want[k].view(np.uint8)), k
    return ring, want["dones"]


@pytest.mark.parametrize("plane,n_stack,D", [(64, 1, 0), (64, 3, 0), (4096, 1, 0), (4096, 3, 0), (0, 1, 5)])
def test_ranks_and_overflow_through_the_c_abi(plane, n_stack, D):
    ring, d = c_abi_case(130, 3, MASKS, plane, n_stack, D)
    assert ring.ref[1].tolist()[:4] == [0, 1, 2, -1] and ring.ref[3, 63:66].tolist() == [0, 1, 2] and ring.ref[2, 129] == 0
    assert ((d & HAS) != 0).sum() == 3 + 1 + 3 and (((d & 3) != 0) & ((d & HAS) == 0)).sum() == 127


@pytest.mark.parametrize("plane,n_stack,D", [(64, 1, 0), (4096, 3, 0), (0, 1, 5)])
def test_ranks_across_workgroups_through_the_c_abi(plane, n_stack, D):
    envs = [0, 1, 2, 3, 4, 100, 254, 255, 256, 257, 258, 300, 510, 511, 512, 513, 514, 598, 599]
    ring, d = c_abi_case(600, 4, MASKS_WG, plane, n_stack, D, sample_envs=envs)
    # conditions on the restatement for these inputs: what a base rank that forgot the workgroups in front would get wrong
    assert ring.ref[1, :5].tolist() == [0, 1, 2, 3, -1] and (ring.ref[1, 4:] == -1).all()
    assert ring.ref[2, 599] == 0 and (ring.ref[2, :599] == -1).all()
    assert ring.ref[3, 255:258].tolist() == [0, 1, 2] and ring.ref[4, 511:514].tolist() == [0, 1, 2]
    assert ring.ref[5, [0, 100, 255, 256, 300, 511, 512, 599]].tolist() == [0, 1, 2, 3, -1, -1, -1, -1]
    assert ((d & HAS) != 0).sum() == 4 + 1 + 3 + 3 + 4 and (((d & 3) != 0) & ((d & HAS) == 0)).sum() == (len(envs) - 4) + 4


# ---- 5. cut plus ended ---------------------------------------------------------------------------------------------------------------
def test_a_reset_right_after_an_ending_keeps_the_frame(world):
    run = Run(make_env(world, terminal_obs=True), 16, B)
    run.step(5)
    fin = (run.db[-1] & 3) != 0
    assert fin.any()                                        # step 5 truncates every env that no infraction ended before
    mask = np.zeros(B, np.uint8)
    mask[np.flatnonzero(fin)[0]] = 1                        # an env that just ended, and - when there is one - an env that did not
    mask[np.flatnonzero(~fin)[:1]] = 1
    run.reset(mask=mask)
    run.step(3)
    got, t, e, has = run.check_all(cut=lambda t, e: (t == 4) & (mask[e] != 0))
    both = (t == 4) & (mask[e] != 0) & fin[e]
    assert both.sum() == 1 and (got["dones"][both] & (CUT | HAS) == (CUT | HAS)).all() and got["next_observations"][both].any()
    only = (t == 4) & (mask[e] != 0) & ~fin[e]
    assert ((got["dones"][only] & (CUT | HAS)) == CUT).all() and not got["next_observations"][only].any()
    rest = (t == 4) & (mask[e] == 0) & fin[e]
    assert rest.sum() == fin.sum() - 1 and ((got["dones"][rest] & (CUT | HAS)) == HAS).all()


# ---- 6. drawn sampling ---------------------------------------------------------------------------------------------------------------
def test_the_draw_is_the_replay_buffers(world):
    run = Run(make_env(world, terminal_obs=True), 8, B)
    run.step(11)
    buf, ref = run.buf, run.ref
    plain_out = {k: torch.empty_like(v) for k, v in buf._buffers(64).items()}
    for k in range(2):
        s = buf.sample(64)
        idx = s.indices.cpu().numpy()
        assert np.array_equal(idx, ref.draw(buf.seed, k, 64))
        ops.replay_sample(buf.struct, DEV, buf.first, buf.count, 64, plain_out, None, buf.seed, k)      # tde_replay_sample, same (seed, draw)
        assert torch.equal(plain_out["indices"], s.indices) and same(plain_out["observations"], s.observations)
        assert torch.equal(plain_out["dones"], s.dones & (0xFF ^ HAS))
        want = ref.gather(idx)
        for f in FIELDS:
            assert np.array_equal(getattr(s, f).cpu().numpy().reshape(want[f].shape).view(np.uint8), want[f].view(np.uint8)), f
    assert buf.draws == 2


# ---- 7. the rollout buffer -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("boot", [True, False])
def test_rollout_buffer_bootstraps_truncated_steps(world, boot):
    n_steps, gamma, lam = 12, 0.99, 0.95
    env = make_env(world, terminal_obs=True)
    plain = make_env(world)
    buf, pbuf = env.rollout_buffer(n_steps, gamma=gamma, gae_lambda=lam, terminal_per_step=B), plain.rollout_buffer(n_steps, gamma=gamma, gae_lambda=lam)
    oracle = make_env(world, auto_reset=False)
    env.reset(), plain.reset(), oracle.reset()
    buf.begin(), pbuf.begin()
    with pytest.raises(ValueError, match="terminal_obs=True"):
        pbuf.terminal_observations()
    rng = np.random.default_rng(5)
    rew, db, val, add = [], [], [], []
    n_boot = 0
    for k in range(n_steps):
        a = torch.from_numpy(actions(rng)).to(DEV)
        v, lp = torch.from_numpy((3 * rng.standard_normal(B)).astype(np.float32)).to(DEV), torch.zeros(B, device=DEV)
        env.step(a), plain.step(a)
        shown = oracle.step(a)[0] if k < 5 else None        # (the oracle's first episode: steps 0 .. 4)
        buf.push(a, v, lp), pbuf.push(a, v, lp)
        d = env.state["done_bits"].cpu().numpy().copy()
        envs, tobs = buf.terminal_observations()
        want = np.flatnonzero((d & 3) == 2)
        assert envs.dtype == torch.int64 and np.array_equal(envs.cpu().numpy(), want)
        assert tobs.shape == (len(want), 9, 64, 64) and tobs.dtype == torch.uint8
        if k == 4:
            assert len(want) and same(tobs, shown[envs])    # exactly what an env without auto-reset shows at that step
        extra = np.zeros(B, np.float32)
        if boot and len(want):
            tv = (rng.standard_normal(len(want)) + 2).astype(np.float32)
            buf.bootstrap(envs, torch.from_numpy(tv).to(DEV))
            extra[want] = np.float32(gamma) * tv
            n_boot += len(want)
        rew.append(env.state["reward"].cpu().numpy().copy()), db.append(d), val.append(v.cpu().numpy()), add.append(extra)
    last = (3 * rng.standard_normal(B)).astype(np.float32)
    buf.finish(torch.from_numpy(last).to(DEV)), pbuf.finish(torch.from_numpy(last).to(DEV))
    adv, ret = O.gae(np.stack(rew) + np.stack(add), np.stack(db), np.stack(val), last, gamma, lam)
    assert np.array_equal(buf.advantages.cpu().numpy().view(np.uint32), adv.view(np.uint32))
    assert np.array_equal(buf.returns.cpu().numpy().view(np.uint32), ret.view(np.uint32))
    if boot:
        assert n_boot >= B and not torch.equal(buf.advantages, pbuf.advantages)
    else:
        assert same(buf.advantages, pbuf.advantages) and same(buf.returns, pbuf.returns)       # today's result
    sd = buf.state_dict()
    assert "pool" in sd["ring"] and "ref" in sd["ring"]
    # the calls above returned 0 .. B envs: one output set served them all, none was cached per size
    assert not buf.ring._out and buf._term_out["next_observations"].shape[0] == B
    assert tobs.untyped_storage().data_ptr() == buf._term_out["next_observations"].untyped_storage().data_ptr()

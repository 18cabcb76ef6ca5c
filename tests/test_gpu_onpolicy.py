"""The rollout buffer on the GPU (include/tde_onpolicy.h, torchdriveenv_amd/onpolicy.py).  Nothing here has a tolerance: advantages and
returns must equal the numpy float32 restatement (tests/onpolicy_ref.py) bit for bit, and a gathered observation must be the one the
env returned at that step, byte for byte."""
import numpy as np
import pytest
import torch

from tests import onpolicy_ref as O
from tests import replay_ref as R
from torchdriveenv_amd import _abi, ops
from torchdriveenv_amd.config import EnvConfig, RendererConfig, SimulatorConfig, VectorObs
from torchdriveenv_amd.env import BatchedWaypointEnv

pytestmark = pytest.mark.gpu
CUT, DEV = _abi.REPLAY_CUT, "cuda:0"
SIDE = ("old_values", "old_log_prob", "advantages", "returns")


@pytest.fixture(scope="module")
def world():
    from torchdriveenv_amd.synth import synthetic_world

    return synthetic_world(n_scn=4, A=4)


def make_env(world, B=5, frame_stack=3, obs_mode="birdview", seed=7, **kw):
    cfg = EnvConfig(seed=seed, distance_cutoff=0.25, max_environment_steps=5, frame_stack=frame_stack,
                    simulator=SimulatorConfig(renderer=RendererConfig(res=64)))
    return BatchedWaypointEnv(cfg, world, num_envs=B, device=DEV, obs_mode=obs_mode, frame_stack=frame_stack, **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


class Run:
    """an env with a rollout buffer attached, everything step() returned and everything pushed logged on the host in time order, and
    the numpy ring fed the same frames"""

    def __init__(self, env, T, gamma=0.99, lam=0.95, seed=3):
        self.env, self.T, self.B, self.gamma, self.lam = env, T, env.num_envs, gamma, lam
        self.buf = env.rollout_buffer(T, gamma=gamma, gae_lambda=lam, seed=seed)
        self.rng = np.random.default_rng(seed)
        self.obs, self.act, self.rew, self.db, self.val, self.logp, self.cut = [], [], [], [], [], [], []
        self.planes = env.obs_mode == "birdview"
        ns = env.frame_stack if self.planes else 1
        assert self.buf.ring.C == T + ns
        self.ref = R.Ring(T + ns, self.B, ns, plane=64 * 64) if self.planes else R.Ring(T + ns, self.B, D=env.observation_space.shape[0])
        self.reset()

    def frame(self, obs):
        return R.layers_of_rgb(obs[:, -3:].reshape(self.B, 3, -1)) if self.planes else obs

    def reset(self, mask=None):
        """mask: numpy uint8 [B] or None"""
        dmask = None if mask is None else torch.from_numpy(mask).to(DEV)
        obs = self.env.reset(mask=dmask).cpu().numpy().copy()
        self.buf.begin(mask=dmask)
        if mask is None:
            self.obs.append(obs)
        else:
            self.obs[-1] = obs                      # the observation of this time, as the env shows it now
            self.cut[-1] = self.cut[-1] | (mask != 0)
        self.ref.begin(self.frame(obs), mask)

    def step(self):
        B = self.B
        a = np.stack([self.rng.uniform(-1, 1, B), self.rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)
        v, lp = (3 * self.rng.standard_normal(B)).astype(np.float32), (-np.abs(self.rng.standard_normal(B))).astype(np.float32)
        ta = torch.from_numpy(a).to(DEV)
        obs, rew, *_ = self.env.step(ta)
        self.buf.push(ta, torch.from_numpy(v).to(DEV), torch.from_numpy(lp).to(DEV))
        self.obs.append(obs.cpu().numpy().copy())
        self.act.append(a)
        self.rew.append(rew.cpu().numpy().copy())
        self.db.append(self.env.state["done_bits"].cpu().numpy().copy())
        self.val.append(v)
        self.logp.append(lp)
        self.cut.append(np.zeros(B, bool))
        self.ref.push(a, self.rew[-1], self.db[-1], self.frame(self.obs[-1]))

    def rollout(self, reset_before=None):
        """T steps and finish(); reset_before = (t, mask): the caller resets the masked envs before step t of this rollout"""
        for t in range(self.T):
            if reset_before is not None and t == reset_before[0]:
                self.reset(mask=reset_before[1])
            self.step()
        assert self.buf.full
        self.last = (3 * self.rng.standard_normal(self.B)).astype(np.float32)
        self.buf.finish(torch.from_numpy(self.last).to(DEV))

    def logged(self):
        """the current rollout in time order, from the log alone: reward, done bits (with the caller's cuts), values, log-probs, actions,
        observations"""
        sl = slice(len(self.act) - self.T, len(self.act))
        done = np.stack(self.db[sl]) | np.where(np.stack(self.cut[sl]), CUT, 0).astype(np.uint8)
        return dict(reward=np.stack(self.rew[sl]), done=done, values=np.stack(self.val[sl]), log_prob=np.stack(self.logp[sl]),
                    action=np.stack(self.act[sl]), obs=np.stack(self.obs[sl.start:sl.stop]))

    def check_gae(self):
        """advantages / returns of the buffer against numpy over the LOGGED rewards and done bits, bit for bit; returns the done bits"""
        buf, log = self.buf, self.logged()
        s = O.slots(self.ref.first, self.ref.count, self.T, self.ref.C)
        assert (buf.ring.first, buf.ring.count) == (self.ref.first, self.ref.count)
        assert np.array_equal(self.ref.done[s], log["done"]) and np.array_equal(bits(self.ref.reward[s]), bits(log["reward"]))
        assert np.array_equal(bits(buf.values.cpu().numpy()), bits(log["values"]))
        for gamma, lam, adv, ret in ((self.gamma, self.lam, buf.advantages, buf.returns),
                                     (1.0, 1.0, torch.full_like(buf.advantages, 7.0), torch.full_like(buf.returns, 7.0))):
            if adv is not buf.advantages:
                ops.gae(buf.ring.struct, buf.dev, buf.ring.first, buf.ring.count, self.T, buf.values, torch.from_numpy(self.last).to(DEV),
                        gamma, lam, adv, ret)
            want_adv, want_ret = O.gae(log["reward"], log["done"], log["values"], self.last, gamma, lam)
            assert np.array_equal(bits(adv.cpu().numpy()), bits(want_adv)), (gamma, lam)
            assert np.array_equal(bits(ret.cpu().numpy()), bits(want_ret)), (gamma, lam)
        return log["done"], s


@pytest.mark.parametrize("T,B,rollouts", [(1, 5, 6), (2, 5, 4), (7, 5, 3), (7, 70, 3)])
def test_gae_equals_the_numpy_restatement_bit_for_bit(world, T, B, rollouts):
    run = Run(make_env(world, B=B), T)
    mask = np.zeros(B, np.uint8)
    mask[[0, 2]] = 1
    seen = dict(wrapped=False, first=False, last=False, cut=False, open=False)
    at = min(T // 2 + 1, T - 1)                 # T = 7: the caller resets envs 0 and 2 before step 4 of the second rollout, so step 3 is cut
    for k in range(rollouts):
        run.rollout(reset_before=(at, mask) if k == 1 and T > 1 else None)
        done, s = run.check_gae()
        ended = (done & (3 | CUT)) != 0
        seen["wrapped"] |= k >= 1 and bool((np.diff(s) < 0).any())
        seen["first"] |= bool(((done[0] & 3) != 0).any())
        seen["last"] |= bool(((done[-1] & 3) != 0).any())
        seen["cut"] |= bool(((done & CUT) != 0).any())
        seen["open"] |= bool((~ended).any())
        if k == 1 and T > 1:
            assert ((done[at - 1] & CUT) != 0).tolist() == (mask != 0).tolist() and ((done & CUT) != 0).sum() == 2
    assert np.any(np.stack(run.val) < 0) and np.any(np.stack(run.val) > 0)
    # conditions on the test's own inputs: none of the cases is vacuous.  Episodes last five steps, so T = 7 meets an episode's end at
    # its step 0 (time 14) and, in the envs the caller reset before time 11, at its last step (time 20)
    assert seen["open"] and (seen["first"] or seen["last"]), seen
    if T == 7:
        assert seen == dict(wrapped=True, first=True, last=True, cut=True, open=True), seen
    if T == 2:
        assert seen["wrapped"] and seen["cut"], seen


def check_get_all(run):
    """get(None): one batch of everything in time order, held to the log and to the replay gather of the same pairs"""
    buf, T, B = run.buf, run.T, run.B
    log = run.logged()
    batches = list(buf.get())
    assert len(batches) == 1
    b = batches[0]
    assert b.indices.dtype == torch.int32 and b.indices.tolist() == list(range(T * B))
    obs = b.observations.cpu().numpy()
    assert obs.dtype == log["obs"].dtype and obs.shape == (T * B,) + log["obs"].shape[2:]
    assert np.array_equal(bits(obs), bits(log["obs"].reshape(obs.shape)))
    assert np.array_equal(bits(b.actions.cpu().numpy()), bits(log["action"].reshape(T * B, 2)))
    assert np.array_equal(bits(b.old_values.cpu().numpy()), bits(log["values"].reshape(-1)))
    assert np.array_equal(bits(b.old_log_prob.cpu().numpy()), bits(log["log_prob"].reshape(-1)))
    want_adv, want_ret = O.gae(log["reward"], log["done"], log["values"], run.last, run.gamma, run.lam)
    assert np.array_equal(bits(b.advantages.cpu().numpy()), bits(want_adv.reshape(-1)))
    assert np.array_equal(bits(b.returns.cpu().numpy()), bits(want_ret.reshape(-1)))
    for name, rows in (("old_values", buf.values), ("old_log_prob", buf.log_probs), ("advantages", buf.advantages), ("returns", buf.returns)):
        assert torch.equal(getattr(b, name).view(torch.int32), rows.reshape(-1)[b.indices.long()].view(torch.int32)), name
    # the same pairs through the replay gather of the owned ring
    s = O.slots(buf.ring.first, buf.ring.count, T, buf.ring.C)
    pairs = np.stack([np.repeat(s, B), np.tile(np.arange(B), T)], 1).astype(np.int32)
    via_ring = buf.ring.sample(None, idx=torch.from_numpy(pairs))
    assert via_ring.observations.shape == b.observations.shape and torch.equal(via_ring.observations, b.observations)
    assert torch.equal(via_ring.actions, b.actions)
    # and the numpy ring
    want = O.gather(run.ref, T, np.arange(T * B), log["values"], log["log_prob"], want_adv, want_ret)
    assert np.array_equal(bits(obs.reshape(want["observations"].shape)), bits(want["observations"]))
    return obs, log


@pytest.mark.parametrize("frame_stack,obs_mode,kw", [(3, "birdview", {}), (1, "birdview", {}),
                                                     (1, "vector", dict(vector_obs=VectorObs(k_neighbours=2, n_rays=4)))])
def test_get_returns_what_the_env_showed(world, frame_stack, obs_mode, kw):
    run = Run(make_env(world, frame_stack=frame_stack, obs_mode=obs_mode, **kw), 4)
    mask = np.array([0, 1, 0, 0, 1], np.uint8)
    reached_back = blanked = 0
    for k in range(3):
        run.rollout(reset_before=(2, mask) if k == 1 else None)
        obs, log = check_get_all(run)
        if frame_stack == 3 and k >= 1:
            first = obs[:run.B]                                         # step 0 of this rollout: older frames are the rollout before's
            reached_back += int(first[:, :6].reshape(run.B, -1).any(1).sum())
            blanked += int((~obs[:, :3].reshape(len(obs), -1).any(1)).sum())
    if frame_stack == 3:
        assert reached_back > 0 and blanked > 0
    assert run.buf.ring.count == 4 + run.ref.n_stack - 1 and len(run.act) == 12


def test_permutation_and_batching(world):
    run = Run(make_env(world), 4)
    run.rollout()
    run.rollout()
    buf, log = run.buf, run.logged()
    adv, ret = buf.advantages.cpu().numpy(), buf.returns.cpu().numpy()

    def one_pass():
        seen = []
        for b in buf.get(7):                                            # (a batch's tensors are reused by the next of its size)
            idx = b.indices.cpu().numpy()
            want = O.gather(run.ref, 4, idx, log["values"], log["log_prob"], adv, ret)
            assert b.observations.shape == (len(idx), 9, 64, 64) and b.actions.shape == (len(idx), 2)
            assert np.array_equal(b.observations.cpu().numpy().reshape(want["observations"].shape), want["observations"])
            assert np.array_equal(bits(b.actions.cpu().numpy()), bits(want["actions"]))
            for name in SIDE:
                assert np.array_equal(bits(getattr(b, name).cpu().numpy()), bits(want[name])), name
            seen.append(idx)
        return seen

    a = one_pass()
    assert [len(x) for x in a] == [7, 7, 6] and sorted(np.concatenate(a).tolist()) == list(range(20)) and buf.calls == 1
    b = one_pass()
    assert sorted(np.concatenate(b).tolist()) == list(range(20)) and not np.array_equal(np.concatenate(a), np.concatenate(b)) and buf.calls == 2
    buf.calls = 0                                                       # the same seed and counter: the same permutation
    assert np.array_equal(np.concatenate(one_pass()), np.concatenate(a))
    other = run.env.rollout_buffer(4, seed=buf.seed + 1)
    other.load_state_dict({**buf.state_dict(), "seed": buf.seed + 1, "calls": 0})
    assert not np.array_equal(torch.cat([x.indices for x in other.get(7)]).cpu().numpy(), np.concatenate(a))
    assert [len(x.indices) for x in buf.get(20)] == [20] and [len(x.indices) for x in buf.get(64)] == [20]
    list(buf.get())
    assert buf.calls == 3                                               # get(None) draws nothing


def test_an_index_outside_the_rollout_gathers_zeros_and_nothing_else_is_written(world):
    run = Run(make_env(world), 4)
    run.rollout()
    run.rollout()
    buf, log = run.buf, run.logged()
    idx = np.array([3, -1, 20, 19, 2 ** 31 - 1, -2 ** 31, 0], np.int32)
    n, per = len(idx), 9 * 64 * 64
    out = buf._buffers(n)
    # guard rows on either side of every output keep their fill
    guarded = torch.full((n + 2, per), 0xA5, dtype=torch.uint8, device=DEV)
    small = {k: torch.full(((n + 2) * v[0].numel() * 4,), 0x25, dtype=torch.uint8, device=DEV).view(torch.float32).view((n + 2,) + tuple(v.shape[1:]))
             for k, v in out.items() if k != "observations"}
    buf._out[n] = {"observations": guarded[1:-1].view(n, 9, 64, 64), **{k: v[1:-1] for k, v in small.items()}}
    r = buf.ring
    got = ops.onpolicy_gather(r.struct, buf.dev, r.first, r.count, 4, torch.from_numpy(idx).to(DEV), buf.values, buf.log_probs, buf.advantages,
                              buf.returns, buf._out[n])
    want = O.gather(run.ref, 4, idx, log["values"], log["log_prob"], buf.advantages.cpu().numpy(), buf.returns.cpu().numpy())
    outside = np.array([False, True, True, False, True, True, False])
    assert (guarded[0] == 0xA5).all() and (guarded[-1] == 0xA5).all()
    obs = got["observations"].cpu().numpy().reshape(n, -1)
    assert np.array_equal(obs, want["observations"].reshape(n, -1)) and not obs[outside].any() and obs[~outside].any(1).all()
    for k, v in small.items():
        assert (v[0].reshape(-1).view(torch.uint8) == 0x25).all() and (v[-1].reshape(-1).view(torch.uint8) == 0x25).all(), k
        g = v[1:-1].cpu().numpy()
        assert np.array_equal(bits(g), bits(want[k])) and not bits(g[outside]).any(), k
    assert np.abs(got["old_values"].cpu().numpy()[~outside]).min() > 0
    # the buffer's own gather: the same bytes
    b = buf.gather(torch.from_numpy(idx).to(DEV))
    assert b.observations.data_ptr() == guarded[1].data_ptr() and np.array_equal(b.observations.cpu().numpy().reshape(n, -1), obs)


def test_state_dict_round_trip(world):
    run = Run(make_env(world), 4)
    run.rollout()
    run.rollout(reset_before=(1, np.array([1, 0, 0, 1, 0], np.uint8)))
    buf = run.buf
    first = next(iter(buf.get(8)))
    sd = buf.state_dict()
    want_all = [t.clone() for t in next(iter(buf.get()))]
    other = run.env.rollout_buffer(4, seed=123)
    assert not other.finished
    other.load_state_dict(sd)
    assert (other.pos, other.finished, other.calls, other.seed) == (4, True, 1, buf.seed)
    got_all = next(iter(other.get()))
    for name, w, g in zip(got_all._fields, want_all, got_all):
        assert w.dtype == g.dtype and torch.equal(w.reshape(-1).view(torch.uint8), g.contiguous().reshape(-1).view(torch.uint8)), name
    # the draw counter travels: the reloaded buffer's next permutation is this buffer's next, not its first
    nxt, onxt = next(iter(buf.get(8))), next(iter(other.get(8)))
    assert torch.equal(nxt.indices, onxt.indices) and not torch.equal(nxt.indices, first.indices)
    with pytest.raises(ValueError, match="values has shape"):
        run.env.rollout_buffer(5).load_state_dict(sd)
    # the next push starts the next rollout
    run.step()
    assert (buf.pos, buf.finished, buf.full) == (1, False, False)
    with pytest.raises(ValueError, match=r"need finish\(\)"):
        buf.get()
